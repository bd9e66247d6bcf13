"""Lattice-free sMBR: the expected frame accuracy of the denominator's path distribution against a reference, differentiable in
the network output (include/pychain_hip.h: pychain_hip_smbr_*; csrc/smbr.hip).

    ref = PosteriorTargets.from_alignment(viterbi_align(y, lengths, num_graphs))
    acc = expected_accuracy(y, lengths, den_graph, ref, leaky_coefficient=1e-5)      # sum_b E_b
    loss = SMBRLoss(den_graph, leaky_coefficient=1e-5, avg=True)(y, lengths, ref)    # -sum_b E_b / sum_b L_b
    total = loss + 0.1 * ChainLoss(den_graph)(y, lengths, num_graphs)                # the usual interpolation with LF-MMI

With `classes` (an integer tensor [D], pdf -> class) the accuracy is by class: a path gets the credit of a frame
where it is on ANY pdf of a class the reference names there - phone-level accuracy (MPFE) with classes = the phone of a pdf, one
silence class with the silence pdfs mapped to one class and the rest to themselves, and a reference from another tree through
PosteriorTargets.to_classes(...) and targets_are_classes=True.

Device tensors run on the HIP kernels, CPU tensors on the library's host twins - never one for the other.  Nothing here
synchronises with the host - but for the first look at a `classes` tensor that lives on a device, which is checked on the host
once -; the calls run on the current stream."""
import torch
import torch.nn as nn

from . import native
from .graph import ChainGraph, ChainGraphBatch
from .loss import PosteriorTargets, _grad_written_in_forward, _recompute, occupancies

__all__ = ["SMBRFunction", "SMBRLoss", "expected_accuracy"]


def _one_graph(den_graph, B):
    """The one probability-domain ChainGraph every sequence of the call shares."""
    if isinstance(den_graph, ChainGraphBatch):
        if den_graph.shared_graph is None:
            raise ValueError("sMBR takes one denominator graph for the whole batch, not a ChainGraphBatch of distinct graphs")
        if den_graph.batch_size != B:
            raise ValueError("input batch size ({}) does not equal to graph batch size ({})".format(B, den_graph.batch_size))
        den_graph = den_graph.shared_graph
    if not isinstance(den_graph, ChainGraph):
        raise ValueError("sMBR needs a ChainGraph (or a ChainGraphBatch of one), got {}".format(type(den_graph)))
    if den_graph.log_domain:
        raise ValueError("sMBR runs over the probability-domain denominator graph, not a log-domain graph")
    return den_graph


class SMBRFunction(torch.autograd.Function):
    """sum_b E_b of include/pychain_hip.h (pychain_hip_smbr_*), differentiable in the network output: the gradient is written by
    the forward call for an upstream gradient of 1; backward rescales it (as PosteriorNumeratorFunction does)."""

    @staticmethod
    def forward(ctx, input, lengths, den_graph, targets, leaky_coefficient, classes=None, targets_are_classes=False, kernels="lds"):
        x = input.detach()
        native.smbr_form_code(kernels, "expected_accuracy")                     # (ValueError, on CPU tensors too)
        if x.dim() != 3:
            raise ValueError("the network output must be [B, T, D], got %s" % list(x.shape))
        if not isinstance(targets, PosteriorTargets):
            raise ValueError("the reference must be PosteriorTargets, got %s" % type(targets))
        graph = _one_graph(den_graph, x.size(0))
        B, T, D = x.shape
        if classes is None:
            if targets_are_classes:
                raise ValueError("targets_are_classes needs `classes`, the map from pdf to class")
            cls = None
            targets.check(B, T, D)
        else:
            cls = native.smbr_classes(classes, D, x.device) + (bool(targets_are_classes),)       # (checked, uploaded once)
            targets.check(B, T, cls[1] if targets_are_classes else D)
        evaluate = lambda: SMBRFunction._evaluate(x, lengths, graph, targets, float(leaky_coefficient), cls, kernels)
        acc, grad, bad, closing = evaluate()
        ctx.grad_buf = grad
        ctx.again = _recompute(x, evaluate, lambda r: r[1])
        ctx.in_dtype = input.dtype
        out = acc.sum().to(torch.float32)
        out.per_seq, out.bad_count, out.closing = acc, bad, closing
        return out

    @staticmethod
    def _evaluate(x, lengths, graph, targets, coef, cls=None, kernels="lds"):
        """(E_b float64 [B], the gradient for an upstream gradient of 1, bad_count int32 [2], closing float32 [B]); `cls`: (the
        class map on x's device, C, targets_are_classes) or None; `kernels`: native.smbr's `form`"""
        kw = {} if cls is None else dict(classes=cls[0], num_classes=cls[1], targets_are_classes=cls[2])
        kw["form"] = kernels
        tg = targets.to(x.device)
        D = x.size(2)
        gt = native.smbr_graph(graph, D, x.device)                              # (checks the graph against D before anything runs)
        if x.is_cuda:
            xk = x if x.dtype in native._DTYPE_CODE else x.float()
            gamma = occupancies(xk.float(), lengths, graph, coef)               # stage 1: the denominator call as it is, fp32
            acc, grad, bad, closing, _ = native.smbr(gt, graph.num_states, xk, lengths, gamma, tg.pdfs, tg.probs, coef, **kw)
        else:
            gamma = occupancies(x.float(), lengths, graph, coef)
            acc, grad, bad, closing, _ = native.cpu_smbr(gt, graph.num_states, x, lengths, gamma, tg.pdfs, tg.probs, coef, **kw)
        return acc, grad, bad, closing

    @staticmethod
    def backward(ctx, g):
        return _grad_written_in_forward(ctx, g), None, None, None, None, None, None, None


def expected_accuracy(x, lengths, den_graph, targets, leaky_coefficient=1e-5, *, classes=None, targets_are_classes=False, kernels="lds"):
    """The expected frame accuracy sum_b E_b of the denominator's paths against `targets` (PosteriorTargets: an alignment through
    PosteriorTargets.from_alignment, or posterior targets), as a 0-dim tensor differentiable in x (neither the clamp nor the
    reference is differentiated).  `den_graph`: a probability-domain ChainGraph, or a ChainGraphBatch made of one.  Of the
    result: `.per_seq` float64 [B] (NaN for a sequence that went bad), `.bad_count` int32 [2] (the sequences that went bad; the
    target entries that name a pdf the network output does not have), `.closing` float32 [B] (a diagnostic of the recursions:
    zero in exact arithmetic, in fp32 the uncentred residue of the frame accuracies' rounding summed over the sequence - it grows
    with the length and bounds nothing).

    `classes`: an integer tensor [D], the class of every pdf (C = max + 1) - the accuracy of pdf n at a frame is then the sum of
    the frame's q_k whose pdf has n's class, so a path is credited on any pdf of the right class.  `targets_are_classes`: the ids
    of `targets` are classes already (PosteriorTargets.to_classes, or a reference from another tree) and are held against C.
    `bad_count[1]` then counts the entries out of range of what they name.  The int32 device copy of `classes` is cached until
    the tensor is replaced or edited in place; making it reads the tensor on the host (one synchronisation for a device tensor).
    ValueError for a map of the wrong length or dtype, a negative entry, or targets_are_classes without classes.

    `kernels` (device tensors): "lds", the default - four state vectors and four rows of a frame in the 160 KiB
    of a CU's LDS, a graph and tree beyond that refused (3000 states with more than about 7 200 pdfs); "auto" - those kernels
    where they fit, else the general ones, which take any graph and tree and are slower; "rows" / "global" - the two general forms
    by name.  Every form gives the same bits on a shape it takes.  ValueError for anything else; CPU tensors accept the keyword
    and run the one host twin."""
    return SMBRFunction.apply(x, lengths, den_graph, targets, leaky_coefficient, classes, targets_are_classes, kernels)


class SMBRLoss(nn.Module):
    """-sum_b E_b, divided by the number of frames when `avg`: the sMBR criterion to MINIMISE, usually interpolated with
    ChainLoss by plain addition.  `classes`: the accuracy by class (expected_accuracy).  `kernels`: "lds" (the default), "auto" for
    a tree beyond the LDS of a CU, "rows", "global" (expected_accuracy)."""

    def __init__(self, den_graph, leaky_coefficient=1e-5, avg=True, classes=None, kernels="lds"):
        super(SMBRLoss, self).__init__()
        self.den_graph = den_graph
        self.leaky_coefficient = leaky_coefficient
        self.avg = avg
        self.classes = classes
        self.kernels = kernels
        native.smbr_form_code(kernels, "SMBRLoss")

    def forward(self, x, x_lengths, targets, targets_are_classes=False):
        acc = expected_accuracy(x, x_lengths, self.den_graph, targets, self.leaky_coefficient, classes=self.classes,
                                targets_are_classes=targets_are_classes, kernels=self.kernels)
        loss = -acc
        if self.avg:
            loss = loss / torch.as_tensor(x_lengths).sum().to(device=acc.device, dtype=acc.dtype)
        loss.per_seq, loss.bad_count, loss.closing = acc.per_seq, acc.bad_count, acc.closing
        return loss
