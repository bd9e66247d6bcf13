"""Alignment time windows on the MI355X (include/pychain_hip.h: pychain_hip_*_tw): the windowed numerator kernels against the host
twin (csrc/cpu.cpp) on the C3 batch, a shared graph of 700 states, the fused loss and a graph on the general kernels; full
windows bit-identical to none; the windowed fused loss against the windowed two-call path and across its schedules; 2-byte
rows; infeasible windows and the num_compat refusal.  The windowed and the free numerator against a plain float64
forward-backward - every launch form of num_fb_kernel, arbitrary and empty windows, an infeasible sequence among feasible
ones - run in tests/test_gpu_num_forms.py."""
import numpy as np
import pytest
import torch

from helpers import _rand_num_fst, long_case, rel_err
from pychain_amd import (ChainFunction, ChainGraph, ChainGraphBatch, ChainLoss, ChainLossFunction, _lib, _plan,
                         alignment_windows, native, viterbi_align, synthetic as syn)

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BIG = 2 ** 31 - 1


def _full(B, H, lo=-1, hi=BIG):
    w = torch.empty(B, H, 2, dtype=torch.int32)
    w[..., 0], w[..., 1] = lo, hi
    return w


def _windows(x, lengths, graphs, tau):
    """Windows at tolerance tau around the host twin's alignment of the same input."""
    ali = viterbi_align(x, lengths, graphs)
    assert bool(ali.ok.all())
    return alignment_windows(ali, graphs.num_states, tau)


def _device_vs_host(x, lengths, graphs, w):
    """Per-sequence objective and gradient of the windowed numerator on the device against the host twin."""
    ho, hg, hbad = native.cpu_forward_backward(graphs, x, lengths, windows=w)
    free, _, _ = native.cpu_forward_backward(graphs, x, lengths)
    assert int(hbad) == 0 and bool((ho < free).any())                  # (the windows constrain)
    graphs.set_time_windows(w)
    calls = _lib.lib().pychain_hip_cpu_calls()
    xd = x.to(DEV)
    gstride = 0 if graphs.shared_graph is not None else 1
    for ld in (lengths, lengths.to(DEV)):
        do, dg, dbad = native.num_forward_backward(graphs.device_tensors(xd.device), gstride, graphs.num_states, xd, ld,
                                                   windows=graphs.device_time_windows(xd.device))
        torch.cuda.synchronize()
        assert int(dbad) == 0
        assert float(((do.cpu().double() - ho.double()).abs() / ho.double().abs()).max()) <= 1e-6
        assert rel_err(dg.cpu().numpy(), hg.numpy()) <= 1e-5
    xx = xd.clone().requires_grad_(True)                               # ChainFunction takes the batch's own windows
    o = ChainFunction.apply(xx, lengths, graphs)
    o.backward()
    torch.cuda.synchronize()
    assert _lib.lib().pychain_hip_cpu_calls() == calls                 # device tensors never reach the host twin
    assert abs(float(o) - float(ho.double().sum())) <= 1e-6 * abs(float(ho.double().sum()))
    assert rel_err(xx.grad.cpu().numpy(), hg.numpy()) <= 1e-5
    graphs.set_time_windows(None)


@pytest.mark.parametrize("tau", [0, 3])
def test_c3_batch_shuffled_device_equals_host(tau):
    w = syn.make_workload("C3")
    perm = torch.from_numpy(np.random.RandomState(5).permutation(w["x"].shape[0]))
    x, lengths, graphs = w["x"][perm].contiguous(), w["lengths"][perm].contiguous(), w["num_graphs"]
    graphs.reorder(perm)
    _device_vs_host(x, lengths, graphs, _windows(x, lengths, graphs, tau))


def test_shared_graph_over_512_states():
    case = long_case("num_shared_T720")
    x, lengths, graphs = case["x"], case["lengths"], case["num"]
    assert graphs.num_states > 512 and graphs.shared_graph is not None
    _device_vs_host(x, lengths, graphs, _windows(x, lengths, graphs, 2))


def test_general_kernel_graph():
    D = 70000                                                          # pdf-ids beyond 16 bits: num_needs_general
    rs = np.random.RandomState(8)
    fin = lambda H: {H - 1: 0.0, H - 3: -0.2}
    gs = [ChainGraph(_rand_num_fst(rs, h, h // 2, D, fin), log_domain=True) for h in (9, 14, 6)]
    gb = ChainGraphBatch(gs, max_num_transitions=max(g.num_transitions for g in gs), max_num_states=max(g.num_states for g in gs))
    assert not _lib.lib().pychain_hip_num_half_native(gb.num_states, gb.num_transitions, D)
    x = syn.make_input(3, 40, D, seed=5)
    lengths = torch.tensor([40, 33, 12])
    _device_vs_host(x, lengths, gb, _windows(x, lengths, gb, 1))


def test_fold_case_fused_numerator_equals_host():
    case = long_case("fold_T751")
    x, lengths, graphs, den = case["x"], case["lengths"], case["num"], case["den"]
    w = _windows(x, lengths, graphs, 2)
    ho, _, hbad = native.cpu_forward_backward(graphs, x, lengths, windows=w)
    assert int(hbad) == 0
    xd = x.to(DEV)
    plan = _plan.graph_plan(den, xd.shape[2], xd.device)
    graphs.set_time_windows(w)
    _, num_objf, bad, _, _ = native.chain_loss_forward(plan, graphs.device_tensors(xd.device), 1, graphs.num_states, xd, lengths,
                                                       with_grad=True, windows=graphs.device_time_windows(xd.device))
    torch.cuda.synchronize()
    assert int(bad.sum()) == 0
    assert float(((num_objf.cpu().double() - ho.double()).abs() / ho.double().abs()).max()) <= 1e-6
    # the fused loss against the two-call path, both windowed
    outs = []
    for fused in (True, False):
        xx = xd.clone().requires_grad_(True)
        m = ChainLoss(den, 1e-5, avg=True)
        m.fused = fused
        loss = m(xx, lengths, graphs)
        loss.backward()
        outs.append((float(loss), xx.grad.cpu().numpy()))
    assert abs(outs[0][0] - outs[1][0]) <= 1e-6 * abs(outs[1][0])
    assert rel_err(outs[0][1], outs[1][1]) <= 2e-6
    graphs.set_time_windows(None)


def _loss_step(den, x, lengths, num, retain=False):
    xx = x.clone().requires_grad_(True)
    loss = ChainLoss(den, 1e-5)(xx, lengths, num)
    loss.backward(retain_graph=retain)
    torch.cuda.synchronize()
    out = (float(loss.detach()), xx.grad.clone(), loss.totals_all.clone(), loss.bad_count.clone())
    if retain:
        xx.grad = None
        loss.backward()
        torch.cuda.synchronize()
        out = out + (xx.grad.clone(),)
    return out


def _c3_small(B=6, T=400, seed=21):
    cfg = syn.CONFIGS["C3"]
    den = syn.make_den_graph(cfg["H"], cfg["K"], cfg["D"], seed=0)
    L = torch.tensor([T, T - 1, T // 2 + 31, T // 3, 77, 40] * (B // 6) + [T] * (B % 6))
    x = syn.make_input(B, T, cfg["D"], seed=seed)
    return den, x, L, syn.make_num_graphs(L.tolist(), cfg["D"], seed=300)


def test_full_windows_bit_identical_on_device():
    den, x, L, num = _c3_small()
    xd = x.to(DEV)
    gt, H = num.device_tensors(xd.device), num.num_states
    a = native.num_forward_backward(gt, 1, H, xd, L)
    b = native.num_forward_backward(gt, 1, H, xd, L, windows=_full(num.batch_size, H).to(DEV))
    c = native.num_forward_backward(gt, 1, H, xd, L, windows=_full(num.batch_size, H, 0, x.shape[1]).to(DEV))
    torch.cuda.synchronize()
    for u, v, z in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, z)
    ref = _loss_step(den, xd, L, num)
    num.set_time_windows(_full(num.batch_size, H))
    got = _loss_step(den, xd, L, num)
    num.set_time_windows(None)
    assert ref[0] == got[0] and all(torch.equal(u, v) for u, v in zip(ref[1:], got[1:]))


def test_windowed_fused_loss_schedules():
    den, x, L, num = _c3_small(B=16, T=300)
    xd = x.to(DEV)
    num.set_time_windows(_windows(x, L, num, 2))
    outs = []
    for fused in (True, False):
        xx = xd.clone().requires_grad_(True)
        m = ChainLoss(den, 1e-5, avg=True)
        m.fused = fused
        loss = m(xx, L, num)
        (loss * 3.0).backward()
        outs.append((float(loss), xx.grad.cpu().numpy()))
    assert abs(outs[0][0] - outs[1][0]) <= 1e-6 * abs(outs[1][0])
    assert rel_err(outs[0][1], outs[1][1]) <= 2e-6
    ref = _loss_step(den, xd, L, num, retain=True)
    assert int(ref[3].sum()) == 0
    assert torch.equal(ref[1], ref[4])                                 # second backward over a retained graph
    try:
        ChainLossFunction.overlap = False
        no_overlap = _loss_step(den, xd, L, num)
    finally:
        ChainLossFunction.overlap = True
    assert torch.equal(no_overlap[1], ref[1])
    for n in (2, 0):
        with _lib.option("chain_slices", n):
            s = _loss_step(den, xd, L, num)
        assert s[0] == ref[0] and torch.equal(s[1], ref[1]), n
    num.set_time_windows(None)
    free = _loss_step(den, xd, L, num)
    assert free[0] < ref[0]                                            # (fewer numerator paths: a larger loss)


def _both_ways(fn):
    outs = []
    for flag in (True, False):
        native.HALF_ROWS = flag
        try:
            outs.append(fn())
        finally:
            native.HALF_ROWS = True
        torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_two_byte_rows_windowed(dtype):
    den, x, L, num = _c3_small(B=4, T=130)
    L = torch.tensor([130, 129, 64, 30])
    num = syn.make_num_graphs(L.tolist(), x.shape[2], seed=300)
    xh = x.to(DEV).to(dtype)
    num.set_time_windows(_windows(xh.float().cpu(), L, num, 1))

    def fn_step():
        xx = xh.clone().requires_grad_(True)
        o = ChainFunction.apply(xx, L, num)
        o.backward()
        return float(o.detach()), xx.grad

    (o1, g1), (o0, g0) = _both_ways(fn_step)
    assert g1.dtype == dtype and o1 == o0 and torch.equal(g1, g0)
    (l1, h1, t1, _), (l0, h0, t0, _) = _both_ways(lambda: _loss_step(den, xh, L, num))
    assert h1.dtype == dtype and l1 == l0 and torch.equal(h1, h0) and torch.equal(t1, t0)
    num.set_time_windows(None)


def test_infeasible_sequence_and_compat():
    den, x, L, num = _c3_small()
    xd = x.to(DEV)
    w = _full(num.batch_size, num.num_states)
    w[2, :, 0], w[2, :, 1] = 9, 8                                      # lo > hi: no path
    num.set_time_windows(w)
    loss, _, totals, bad = _loss_step(den, xd, L, num)
    # (the device counts the numerator's failed checks - every occupancy wave of that sequence - as it does for a graph
    # without a path of length L; the host twin counts sequences)
    assert int(bad[0]) == 0 and int(bad[1]) >= 1 and float(totals[2]) == float(bad.sum())
    assert loss == float("inf")
    with _lib.option("num_compat", 1):
        with pytest.raises(_lib.PychainHipError):
            ChainLoss(den, 1e-5)(xd, L, num)
        with pytest.raises(_lib.PychainHipError):
            ChainFunction.apply(xd, L, num)
    num.set_time_windows(None)
