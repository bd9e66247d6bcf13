"""viterbi_align on the MI355X: the HIP kernels (csrc/align.hip) give the same bits as the host twin (csrc/cpu.cpp) - scores
(compared as int64 words), states and pdfs - on the C3 numerator batch, on the long numerator cases, on a graph beyond the tile
kernel, for 2-byte inputs (against the host twin on their exact fp32 up-cast), on a side stream and from run to run.  Every
launch form of align_kernel, the block backtrace at every length, the largest tile graph, ties and the clamp / NaN row tails
run against the float64 reference of the ABI in tests/test_gpu_align_forms.py."""
import numpy as np
import pytest
import torch

from helpers import _rand_num_fst, long_case
from pychain_amd import ChainGraph, ChainGraphBatch, _lib, viterbi_align, synthetic as syn

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _same(dev, host):
    assert torch.equal(dev.score.cpu().view(torch.int64), host.score.view(torch.int64))
    assert torch.equal(dev.states.cpu(), host.states)
    assert torch.equal(dev.pdfs.cpu(), host.pdfs)
    assert torch.equal(dev.ok.cpu(), host.ok)


def _check(x, lengths, graphs):
    host = viterbi_align(x, lengths, graphs)
    calls = _lib.lib().pychain_hip_cpu_calls()
    dev = viterbi_align(x.to(DEV), lengths, graphs)
    torch.cuda.synchronize()
    assert _lib.lib().pychain_hip_cpu_calls() == calls          # device tensors never reach the host twin
    _same(dev, host)
    return dev, host


def test_c3_batch_shuffled_lengths_host_and_device():
    w = syn.make_workload("C3")
    perm = torch.from_numpy(np.random.RandomState(3).permutation(w["x"].shape[0]))
    x, lengths, graphs = w["x"][perm].contiguous(), w["lengths"][perm].contiguous(), w["num_graphs"]
    graphs.reorder(perm)
    dev, host = _check(x, lengths, graphs)
    assert bool(host.ok.all())
    dev2 = viterbi_align(x.to(DEV), lengths.to(DEV), graphs)         # lengths on the device
    _same(dev2, host)
    L = lengths.tolist()
    for b in (0, 17, 63):                                            # rows beyond the length are -1, in-kernel
        assert bool((dev.pdfs[b, L[b]:] == -1).all()) and bool((dev.states[b, L[b] + 1:] == -1).all())
        assert bool((dev.pdfs[b, :L[b]] >= 0).all())


@pytest.mark.parametrize("name", ["num_shared_T720", "fold_T751"])
def test_long_cases(name):
    case = long_case(name)
    _check(case["x"], case["lengths"], case["num"])


def test_general_kernel_graph():
    D = 70000                                                        # pdf-ids beyond 16 bits: num_needs_general
    rs = np.random.RandomState(8)
    fin = lambda H: {H - 1: 0.0, H - 3: -0.2}
    gs = [ChainGraph(_rand_num_fst(rs, h, h // 2, D, fin), log_domain=True) for h in (9, 14, 6)]
    gb = ChainGraphBatch(gs, max_num_transitions=max(g.num_transitions for g in gs), max_num_states=max(g.num_states for g in gs))
    assert not _lib.lib().pychain_hip_align_half_native(gb.num_states, gb.num_transitions, D)
    x = syn.make_input(3, 40, D, seed=5)
    dev, host = _check(x, torch.tensor([40, 33, 7]), gb)
    assert bool(host.ok.all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_inputs_equal_host_on_upcast(dtype):
    for x, lengths, graphs in ((lambda c: (c["x"], c["lengths"], c["num"]))(long_case("num_shared_T720")),
                               (lambda w: (w["x"], w["lengths"], w["num_graphs"]))(syn.make_workload("C3"))):
        xh = x.to(dtype)
        K = int(graphs.backward_transitions.shape[-2])
        assert _lib.lib().pychain_hip_align_half_native(graphs.num_states, K, xh.shape[2])
        dev = viterbi_align(xh.to(DEV), lengths, graphs)
        _same(dev, viterbi_align(xh.float(), lengths, graphs))


def test_nan_and_unreachable_match_host():
    case = long_case("num_shared_T720")
    x = case["x"].clone()
    g = case["num"].shared_graph
    x[0, 100, int(g.backward_transitions[5, 2])] = float("nan")     # a column the graph emits
    lengths = torch.tensor([720, 3])                                 # 3 frames cannot reach the final states of 700
    dev, host = _check(x, lengths, case["num"])
    assert torch.isnan(host.score[0]) and host.score[1] == -float("inf") and not bool(host.ok.any())
    assert bool((host.pdfs == -1).all()) and bool((host.states == -1).all())


def test_side_stream_and_repeat():
    case = long_case("fold_T751")
    xd = case["x"].to(DEV)
    ref = viterbi_align(xd, case["lengths"], case["num"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = viterbi_align(xd, case["lengths"], case["num"])
    s.synchronize()
    again = viterbi_align(xd, case["lengths"], case["num"])
    torch.cuda.synchronize()
    for a in (other, again):
        assert torch.equal(a.score.view(torch.int64), ref.score.view(torch.int64))
        assert torch.equal(a.states, ref.states) and torch.equal(a.pdfs, ref.pdfs)
