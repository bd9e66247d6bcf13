"""Expected arc counts and a denominator whose graph weights train (include/pychain_hip.h: pychain_hip_den_arc_counts,
pychain_hip_den_arc_counts_general; csrc/arc_counts.hip).

With every arc probability p_k of the denominator graph replaced by p_k exp(w_k), the objective log Z_b(w) has the gradient

    c(b,k) = d log Z_b / d w_k = the expected number of times a path of sequence b takes arc k

    counts = expected_arc_counts(y, lengths, den_graph).counts                     # E-step statistics at w = 0
    w = torch.zeros(den_graph.num_transitions, requires_grad=True)                 # a learnable phone bigram / LM scale
    den = den_log_partition(y, lengths, den_graph, w)                              # sum_b log Z_b(w), differentiable in y and w
    loss = (den - ChainFunction.apply(y, lengths, num_graphs, 1e-5)) / frames

`leaky_probs`, `initial_probs` and `final_probs` of the graph are held fixed: they are not recomputed from the weighted graph and
not differentiated; neither is the clamp of the network output.  Device tensors run on the HIP kernels, CPU tensors on the
library's host twin - never one for the other.  Nothing here synchronises with the host; the calls run on the current stream."""
import torch

from . import native
from .loss import _grad_written_in_forward, _recompute
from .smbr import _one_graph

__all__ = ["ArcCounts", "DenLogPartitionFunction", "den_log_partition", "expected_arc_counts"]


class ArcCounts(object):
    """`counts` float64 [K] in the order of forward_transitions (sum_b u_b c(b,k)), `counts_per_seq` float64 [B,K] or None (not
    weighted), `objf_per_seq` float64 [B] (log Z_b; NaN for a sequence that went bad), `bad_count` int32 [2] (the sequences that
    went bad; the arc weights that are not finite, taken as 0)."""
    __slots__ = ("counts", "counts_per_seq", "objf_per_seq", "bad_count")

    def __init__(self, counts, counts_per_seq, objf_per_seq, bad_count):
        self.counts, self.counts_per_seq, self.objf_per_seq, self.bad_count = counts, counts_per_seq, objf_per_seq, bad_count


def _call(x, lengths, graph, coef, w, u, with_grad, per_seq, kernels="lds"):
    """(objf_per_seq, counts, counts_per_seq, grad, bad_count) of native.den_arc_counts / native.cpu_den_arc_counts by x's device;
    `kernels`: their `form`"""
    if x.dim() != 3:
        raise ValueError("the network output must be [B, T, D], got %s" % list(x.shape))
    gt = native.smbr_graph(graph, x.size(2), x.device)                          # (checks the graph against D before anything runs)
    if x.is_cuda:
        xk = x if x.dtype in native._DTYPE_CODE else x.float()
        return native.den_arc_counts(gt, graph.num_states, xk, lengths, coef, w, u, with_grad=with_grad, per_seq=per_seq, form=kernels)
    return native.cpu_den_arc_counts(gt, graph.num_states, x, lengths, coef, w, u, with_grad=with_grad, per_seq=per_seq, form=kernels)


def expected_arc_counts(x, lengths, den_graph, leaky_coefficient=1e-5, *, arc_log_weights=None, utt_weights=None, per_seq=False,
                        kernels="lds"):
    """The expected arc counts of the denominator's path distribution on the network output `x` [B,T,D]: an ArcCounts.  Not
    differentiable.  `den_graph`: a probability-domain ChainGraph, or a ChainGraphBatch made of one.  `arc_log_weights`: a float
    tensor [K] in the order of forward_transitions, None = zeros (the graph as it is); `utt_weights`: [B], the weight of every
    sequence in `counts`; `per_seq`: also the counts of every sequence.  Each sequence's counts sum to its length.  ValueError
    for a weight tensor of the wrong length or a dtype that is not float.

    `kernels` (device tensors): "lds", the default - two state vectors and two rows of a frame in the 160 KiB of a
    CU's LDS, a graph and tree beyond that refused (num_states + num_pdfs > 20416); "auto" - those kernels where they fit, else
    the general ones, which take any graph and tree and are slower; "rows" (num_states up to 20416) / "global" - the two general
    forms by name.  Every form gives the same bits on a shape it takes.  ValueError for anything else; CPU tensors accept the
    keyword and run the one host twin."""
    native.smbr_form_code(kernels, "expected_arc_counts")                       # (ValueError, on CPU tensors too)
    x = x.detach()
    graph = _one_graph(den_graph, x.size(0))
    with torch.no_grad():
        objf, counts, cps, _, bad = _call(x, lengths, graph, float(leaky_coefficient), arc_log_weights, utt_weights, False, per_seq, kernels)
    return ArcCounts(counts, cps, objf, bad)


class DenLogPartitionFunction(torch.autograd.Function):
    """sum_b u_b log Z_b(w), differentiable in the network output and in the arc log-weights.  The gradient of the network output
    is written by the forward call for an upstream gradient of 1 and rescaled in backward (as SMBRFunction does); the gradient of
    the weights is the upstream gradient times the counts."""

    @staticmethod
    def forward(ctx, input, lengths, den_graph, arc_log_weights, leaky_coefficient, utt_weights=None, kernels="lds"):
        x = input.detach()
        native.smbr_form_code(kernels, "den_log_partition")                     # (ValueError, on CPU tensors too)
        graph = _one_graph(den_graph, x.size(0))
        w = None if arc_log_weights is None else arc_log_weights.detach()
        want = bool(ctx.needs_input_grad[0])
        evaluate = lambda: _call(x, lengths, graph, float(leaky_coefficient), w, utt_weights, want, False, kernels)
        objf, counts, _, grad, bad = evaluate()
        ctx.grad_buf = grad
        ctx.again = _recompute(x, evaluate, lambda r: r[3])
        ctx.in_dtype = input.dtype
        ctx.counts = counts
        ctx.w_like = (arc_log_weights.dtype, arc_log_weights.device) if arc_log_weights is not None else None
        per = objf
        if utt_weights is not None:
            u = torch.as_tensor(utt_weights).detach().to(device=objf.device, dtype=objf.dtype)
            per = torch.where(u == 0, torch.zeros_like(objf), objf * u)        # (a bad sequence of weight 0 adds nothing)
        out = per.sum().to(torch.float32)
        out.per_seq, out.bad_count = objf, bad
        return out

    @staticmethod
    def backward(ctx, g):
        gx = _grad_written_in_forward(ctx, g)
        gw = None
        if ctx.w_like is not None and ctx.needs_input_grad[3]:
            dtype, device = ctx.w_like
            gw = (ctx.counts * g.to(ctx.counts.dtype)).to(device=device, dtype=dtype)
        return gx, None, None, gw, None, None, None


def den_log_partition(x, lengths, den_graph, arc_log_weights, leaky_coefficient=1e-5, utt_weights=None, *, kernels="lds"):
    """sum_b u_b log Z_b(w) of the denominator graph with every arc probability p_k replaced by p_k exp(w_k), as a 0-dim float32
    tensor differentiable in `x` and in `arc_log_weights` (a float tensor [K] in the order of forward_transitions; its gradient
    comes back in its dtype and on its device).  At w = 0 this is the denominator objective of ChainFunction.  Of the result:
    `.per_seq` float64 [B] (log Z_b, not weighted; NaN for a sequence that went bad - give it the weight 0, or check
    `.bad_count`), `.bad_count` int32 [2].  The graph's leaky, initial and final probabilities are held fixed.  `kernels`: "lds"
    (the default), "auto" for a graph and tree beyond the LDS of a CU, "rows", "global" (expected_arc_counts); a second backward
    recomputes through the same form."""
    return DenLogPartitionFunction.apply(x, lengths, den_graph, arc_log_weights, leaky_coefficient, utt_weights, kernels)
