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
"""
import collections

import torch

from . import native
from .graph import ChainGraphBatch

__all__ = ["Alignment", "viterbi_align"]

Alignment = collections.namedtuple("Alignment", ["pdfs", "states", "score", "ok"])


def viterbi_align(nnet_output, input_lengths, num_graphs):
    """Best path through every sequence's log-domain numerator graph (a ChainGraphBatch, from one shared graph or a list)."""
    if not isinstance(num_graphs, ChainGraphBatch):
        raise TypeError("viterbi_align: num_graphs must be a ChainGraphBatch")
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
        if not x.is_cuda:
            score, states, pdfs, _ = native.cpu_align(num_graphs, x, input_lengths)
        else:
            gt = num_graphs.device_tensors(x.device)
            gstride = 0 if num_graphs.shared_graph is not None else 1
            score, states, pdfs, _ = native.align(gt, gstride, num_graphs.num_states, x, input_lengths)
        ok = torch.isfinite(score)
    return Alignment(pdfs, states, score, ok)
