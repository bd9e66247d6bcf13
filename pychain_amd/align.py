"""Viterbi forced alignment: the best path through each utterance's numerator (supervision) graph.

    from pychain_amd import viterbi_align
    ali = viterbi_align(nnet_output, input_lengths, num_graphs)
    ali.pdfs    # int64 [B, T]: pdf consumed at frame t (the pdf of the arc taken from frame t to t+1); -1 for t >= L_b
    ali.states  # int32 [B, T+1]: state occupied before frame t, t = 0..L_b (states[b, L_b] = the final state); -1 beyond
    ali.score   # float64 [B]: best-path log-score, final weight included
    ali.ok      # bool [B]: score is finite

What the frame-level targets of a cross-entropy branch, a flat-start bootstrap or a transcript check are built from.  The
inputs follow ChainFunction's contract (the network output [B,T,D] in fp32 / bf16 / fp16, clamped to [-30, 30]; lengths
in any order, on any device).  Device tensors run on the HIP kernels (csrc/align.hip), CPU tensors on the host twin
(csrc/cpu.cpp) - never one for the other - and both give the same bits (include/pychain_hip.h: pychain_hip_align).  The
call is not differentiable, does not synchronise the host, and runs on the current stream.

alignment_windows turns an alignment into the time windows of constrained LF-MMI (ChainGraphBatch.set_time_windows): the next
model trains on numerators restricted to the previous model's alignment plus a tolerance -

    ali = viterbi_align(x_flat_start, lengths, num_graphs)
    num_graphs.set_time_windows(alignment_windows(ali, num_graphs.num_states, tolerance=2))
    loss = ChainLoss(den_graph)(x, lengths, num_graphs)

and the pass after that re-aligns with the new model INSIDE the windows of the previous alignment, at a wider tolerance, so that
alignments cannot jump between passes (constrained re-alignment, include/pychain_hip.h: pychain_hip_align_tw) -

    num_graphs.set_time_windows(alignment_windows(ali, num_graphs.num_states, tolerance=6))
    ali = viterbi_align(x_new_model, lengths, num_graphs, time_windows=True)
    num_graphs.set_time_windows(alignment_windows(ali, num_graphs.num_states, tolerance=2))
"""
import collections

import torch

from . import native
from .graph import ChainGraphBatch

__all__ = ["Alignment", "viterbi_align", "alignment_windows"]

Alignment = collections.namedtuple("Alignment", ["pdfs", "states", "score", "ok"])


def _explicit_windows(windows, num_graphs):
    """Explicit windows with the checks, the dtype conversion and the saturation of ChainGraphBatch.set_time_windows."""
    if not isinstance(windows, torch.Tensor) or windows.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8,
                                                                      torch.uint8):
        raise ValueError("viterbi_align: time_windows must be None, True or an integer tensor, got %s"
                         % (getattr(windows, "dtype", type(windows)),))
    if tuple(windows.shape) != (num_graphs.batch_size, num_graphs.num_states, 2):
        raise ValueError("viterbi_align: time_windows must have the shape [batch_size, num_states, 2] = [%d, %d, 2], got %s"
                         % (num_graphs.batch_size, num_graphs.num_states, list(windows.shape)))
    if windows.dtype == torch.int64:
        windows = windows.clamp(-2 ** 31, 2 ** 31 - 1)          # (any int32 value is legal: saturate, do not wrap)
    return windows.to(torch.int32).contiguous()


def viterbi_align(nnet_output, input_lengths, num_graphs, time_windows=None):
    """Best path through every sequence's log-domain numerator graph (a ChainGraphBatch, from one shared graph or a list).

    `time_windows`: None - the free best path (a batch that carries windows is refused: say which you mean); True - the best
    path among those that keep every state inside the batch's own windows (set_time_windows); an integer tensor
    [batch_size, num_states, 2] on any device - the same under these windows, whatever the batch carries.  A sequence whose
    windows admit no path has score -inf, ok False and every row -1."""
    if not isinstance(num_graphs, ChainGraphBatch):
        raise TypeError("viterbi_align: num_graphs must be a ChainGraphBatch")
    own = getattr(num_graphs, "time_windows", None)
    if time_windows is None and own is not None:
        raise ValueError("viterbi_align: this batch carries time windows (set_time_windows); pass time_windows=True to align "
                         "inside them (constrained re-alignment), explicit windows as a tensor, or align on a batch without them")
    if time_windows is True and own is None:
        raise ValueError("viterbi_align: time_windows=True, but this batch carries no time windows (set_time_windows)")
    if time_windows is False:
        raise ValueError("viterbi_align: time_windows must be None, True or an integer tensor")
    if not num_graphs.log_domain:
        raise ValueError("viterbi_align: the graphs must be log-domain numerator graphs (log_domain=True); denominator graphs "
                         "(leaky-HMM, probability domain) have no best-path meaning here")
    B = nnet_output.size(0)
    if B != num_graphs.batch_size:
        raise ValueError(
            "input batch size ({}) does not equal to graph batch size ({})"
            .format(B, num_graphs.batch_size))
    x = nnet_output.detach()
    with torch.no_grad():
        if time_windows is None:
            tw = None
        elif time_windows is True:
            tw = num_graphs.device_time_windows(x.device) if x.is_cuda else own
        else:
            tw = _explicit_windows(time_windows, num_graphs).to(x.device)
        if not x.is_cuda:
            score, states, pdfs, _ = native.cpu_align(num_graphs, x, input_lengths, windows=tw)
        else:
            gt = num_graphs.device_tensors(x.device)
            gstride = 0 if num_graphs.shared_graph is not None else 1
            score, states, pdfs, _ = native.align(gt, gstride, num_graphs.num_states, x, input_lengths, windows=tw)
        ok = torch.isfinite(score)
    return Alignment(pdfs, states, score, ok)


def alignment_windows(alignment, num_states, tolerance=0):
    """Time windows (int32 [B, num_states, 2] on the alignment's device) around an Alignment: for a sequence with `ok`, state h
    gets lo = max(0, first t with states[b, t] == h - left), hi = min(L_b, last such t + right), L_b = (number of
    states[b] >= 0) - 1; a state the path never visits gets (0, -1), never admissible.  A sequence without `ok` gets (0, T)
    for every state: it stays unconstrained.  `tolerance`: frames on both sides, or (left, right); non-negative integers.
    The aligned path stays admissible, so the constrained log-probability is >= alignment.score.  Torch ops only: no host
    sync.  (`num_states` must exceed every state of the alignment - the graphs' num_states.)"""
    if isinstance(tolerance, (tuple, list)):
        if len(tolerance) != 2:
            raise ValueError("tolerance must be an int or a pair (left, right)")
        left, right = tolerance
    else:
        left = right = tolerance
    for v in (left, right):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError("tolerance must be non-negative integers, got %r" % (tolerance,))
    H = int(num_states)
    if H <= 0:
        raise ValueError("num_states must be positive")
    states = alignment.states
    B, T1 = states.shape
    dev = states.device
    st = states.to(torch.int64)
    valid = (st >= 0) & (st < H)                     # (anything else is no state of these graphs: never scattered)
    idx = torch.where(valid, st, torch.zeros_like(st))
    t = torch.arange(T1, device=dev, dtype=torch.int64).expand(B, T1)
    first = torch.full((B, H), T1, dtype=torch.int64, device=dev)
    first.scatter_reduce_(1, idx, torch.where(valid, t, torch.full_like(t, T1)), reduce="amin")
    last = torch.full((B, H), -1, dtype=torch.int64, device=dev)
    last.scatter_reduce_(1, idx, torch.where(valid, t, torch.full_like(t, -1)), reduce="amax")
    L = ((st >= 0).sum(1) - 1).unsqueeze(1)
    visited = last >= 0
    lo = torch.where(visited, (first - left).clamp(min=0), torch.zeros_like(first))
    hi = torch.where(visited, torch.minimum(last + right, L), torch.full_like(last, -1))
    ok = alignment.ok.to(device=dev, dtype=torch.bool).unsqueeze(1)
    lo = torch.where(ok, lo, torch.zeros_like(lo))
    hi = torch.where(ok, hi, torch.full_like(hi, T1 - 1))
    return torch.stack([lo, hi], dim=-1).to(torch.int32)
