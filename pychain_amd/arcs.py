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
library's host twin - never one for the other.  Nothing here synchronises with the host; the calls run on the current stream.

The NUMERATOR has the same pair (pychain_hip_num_arc_counts; csrc/num_arcs.hip), with weights per sequence - its
graphs differ from utterance to utterance - added to the arc LOG-probabilities:

    c = expected_num_arc_counts(y, lengths, num_graphs).counts_per_seq            # [B,K]: which arcs each utterance takes
    num = num_log_partition(y, lengths, num_graphs, theta * loops_num)            # sum_b log P_b(w), differentiable in y and w
    den = den_log_partition(y, lengths, den_graph, theta * loops_den)             # a parameter tied across both graphs trains"""
import torch

from . import native
from .loss import _grad_written_in_forward, _recompute
from .smbr import _one_graph

__all__ = ["ArcCounts", "DenLogPartitionFunction", "den_log_partition", "expected_arc_counts",
           "NumArcCounts", "NumLogPartitionFunction", "num_log_partition", "expected_num_arc_counts"]


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


# ---- the numerator ---------------------------------------------------------------------------------------------------------------
class NumArcCounts(object):
    """`counts_per_seq` float64 [B,K], K the batch's padded num_transitions, in the order of each row of forward_transitions
    (exact zeros for padding arcs and for a sequence without a finite log-probability); `objf_per_seq` float64 [B] (log P_b:
    -inf without an admissible path, NaN where an arc emits one); `bad_count` int32 [2] (what the numerator call counts; the arc
    weights that are not finite, taken as 0)."""
    __slots__ = ("counts_per_seq", "objf_per_seq", "bad_count")

    def __init__(self, counts_per_seq, objf_per_seq, bad_count):
        self.counts_per_seq, self.objf_per_seq, self.bad_count = counts_per_seq, objf_per_seq, bad_count


def _num_call(x, lengths, graphs, w, with_grad):
    """(objf_per_seq, counts_per_seq, grad, bad_count) of native.num_arc_counts / native.cpu_num_arc_counts by x's device, under
    the batch's time windows"""
    if x.dim() != 3:
        raise ValueError("the network output must be [B, T, D], got %s" % list(x.shape))
    if not getattr(graphs, "log_domain", False):
        raise ValueError("numerator arc counts need a log-domain ChainGraphBatch (probability-domain graphs: expected_arc_counts)")
    if x.size(0) != graphs.batch_size:
        raise ValueError("input batch size ({}) does not equal to graph batch size ({})".format(x.size(0), graphs.batch_size))
    tw = getattr(graphs, "time_windows", None)
    if not x.is_cuda:
        return native.cpu_num_arc_counts(graphs, x, lengths, w, with_grad=with_grad, windows=tw)
    gt = graphs.device_tensors(x.device)
    return native.num_arc_counts(gt, 0 if graphs.shared_graph is not None else 1, graphs.num_states, x, lengths, w, with_grad=with_grad,
                                 windows=None if tw is None else graphs.device_time_windows(x.device))


def expected_num_arc_counts(x, lengths, num_graphs, *, arc_log_weights=None):
    """The expected arc counts of the numerator's path distribution on the network output `x` [B,T,D]: a NumArcCounts.  Not
    differentiable.  `num_graphs`: a log-domain ChainGraphBatch; its time windows (set_time_windows) are honoured.
    `arc_log_weights`: a float tensor [B,K] added to the arc log-probabilities, None = the graphs as they are.  Every feasible
    sequence's counts sum to its length.  ValueError for weights of the wrong shape or of a dtype that is not float, and for a
    probability-domain batch."""
    x = x.detach()
    with torch.no_grad():
        objf, counts, _, bad = _num_call(x, lengths, num_graphs, arc_log_weights, False)
    return NumArcCounts(counts, objf, bad)


class NumLogPartitionFunction(torch.autograd.Function):
    """sum_b u_b log P_b(w), differentiable in the network output and in the arc log-weights [B,K].  The gradient of the network
    output is written by the forward call for an upstream gradient of 1 and rescaled in backward (as DenLogPartitionFunction
    does); the gradient of the weights is the upstream gradient times u_b c(b,k)."""

    @staticmethod
    def forward(ctx, input, lengths, num_graphs, arc_log_weights, utt_weights=None):
        x = input.detach()
        w = None if arc_log_weights is None else arc_log_weights.detach()
        want = bool(ctx.needs_input_grad[0])
        u = None
        if utt_weights is not None:
            u = torch.as_tensor(utt_weights).detach().to(device=x.device, dtype=torch.float64)
            if tuple(u.shape) != (x.size(0),):
                raise ValueError("utterance weights must have shape [%d], got %s" % (x.size(0), tuple(u.shape)))

        def evaluate():
            objf, counts, grad, bad = _num_call(x, lengths, num_graphs, w, want)
            if grad is not None and u is not None:
                grad.mul_(u.to(grad.dtype)[:, None, None])         # (a sequence of weight 0: exact zeros, it has no NaN rows)
            return objf, counts, grad, bad
        objf, counts, grad, bad = evaluate()
        ctx.grad_buf = grad
        ctx.again = _recompute(x, evaluate, lambda r: r[2])
        ctx.in_dtype = input.dtype
        ctx.counts = counts if u is None else counts * u[:, None]   # (a bad sequence's row is exact zeros)
        ctx.w_like = (arc_log_weights.dtype, arc_log_weights.device) if arc_log_weights is not None else None
        per = objf
        if u is not None:
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
        return gx, None, None, gw, None


def num_log_partition(x, lengths, num_graphs, arc_log_weights, utt_weights=None):
    """sum_b u_b log P_b(w) of the numerator graphs with every arc log-probability lp_k of sequence b replaced by lp_k + w(b,k),
    as a 0-dim float32 tensor differentiable in `x` and in `arc_log_weights` (a float tensor [B,K] of any strides, K the batch's
    padded num_transitions in the order of each row of forward_transitions; its gradient comes back in its dtype and on its
    device).  At w = 0 this is the numerator objective of ChainFunction.  Of the result: `.per_seq` float64 [B] (log P_b, not
    weighted; -inf or NaN for a sequence without a usable result - give it the weight 0, or check `.bad_count`), `.bad_count`
    int32 [2].  The batch's time windows are honoured; initial and final probabilities are held fixed.  Tied parameters need no
    API: `w = theta[param_of_arc]`, or `w = theta * is_self_loop`, and autograd does the rest."""
    if not getattr(num_graphs, "log_domain", False):
        raise ValueError("num_log_partition needs a log-domain ChainGraphBatch (probability-domain graphs: den_log_partition)")
    if arc_log_weights is not None and (not torch.is_tensor(arc_log_weights) or not arc_log_weights.is_floating_point()):
        raise ValueError("arc_log_weights must be a float tensor [B, K], got %s" % getattr(arc_log_weights, "dtype", type(arc_log_weights)))
    return NumLogPartitionFunction.apply(x, lengths, num_graphs, arc_log_weights, utt_weights)
