"""Alignment time windows on numerator graphs (constrained LF-MMI, include/pychain_hip.h: pychain_hip_*_tw) on CPU tensors: the
host twin against brute-force path enumeration, full windows against none bit for bit, masked occupancies, alignment_windows
and the Python plumbing (reorder, pickling, shard_batch, errors).  No GPU."""
import pickle

import numpy as np
import pytest
import torch

from helpers import _rand_num_fst, batch_from_npz, graph_from_npz, long_case
from pychain_amd import (Alignment, ChainFunction, ChainGraph, ChainGraphBatch, ChainLoss, alignment_windows, native,
                         viterbi_align, synthetic as syn)
from pychain_amd.parallel import shard_batch

BIG = 2 ** 31 - 1


def _objf_grad(x, lengths, graphs):
    xx = x.clone().requires_grad_(True)
    o = ChainFunction.apply(xx, lengths, graphs)
    o.backward()
    return float(o.detach()), xx.grad.clone()


def _per_seq(x, lengths, graphs, windows=None):
    return native.cpu_forward_backward(graphs, x, lengths, windows=windows)


def _full(B, H, lo=0, hi=BIG):
    w = torch.empty(B, H, 2, dtype=torch.int32)
    w[..., 0], w[..., 1] = lo, hi
    return w


def _brute(g, x, L, win):
    """(logP, posteriors [L, D]) over every path of length L whose state lies in its window at every time index."""
    ft = g.forward_transitions.numpy()
    lp = g.forward_transition_probs.numpy().astype(np.float64)
    init = g.initial_probs.numpy().astype(np.float64)
    fin = g.final_probs.numpy().astype(np.float64)
    xd = x.numpy().astype(np.float64)
    out = {}
    for s, d, p in ft:
        out.setdefault(int(s), []).append((int(d), int(p)))
    arcs_from = {s: [k for k in range(len(ft)) if ft[k][0] == s] for s in range(g.num_states)}
    adm = lambda h, t: win[h][0] <= t <= win[h][1]
    paths = []

    def walk(h, t, w, pdfs):
        if not adm(h, t):
            return
        if t == L:
            if fin[h] > -np.inf:
                paths.append((w + fin[h], pdfs))
            return
        for k in arcs_from[h]:
            d, p = int(ft[k][1]), int(ft[k][2])
            walk(d, t + 1, w + (lp[k] + xd[t, p]), pdfs + [p])

    for h0 in range(g.num_states):
        if init[h0] > -np.inf:
            walk(h0, 0, init[h0], [])
    post = np.zeros((L, x.shape[1]))
    if not paths:
        return -np.inf, post
    ws = np.array([w for w, _ in paths])
    m = ws.max()
    logp = m + np.log(np.exp(ws - m).sum())
    for w, pdfs in paths:
        for t, p in enumerate(pdfs):
            post[t, p] += np.exp(w - logp)
    return logp, post


def test_brute_force_tiny_graphs():
    rs = np.random.RandomState(3)
    D = 4
    feasible = 0
    for trial in range(80):
        H, L = int(rs.randint(2, 6)), int(rs.randint(1, 7))
        fin = lambda n: {n - 1: 0.0, 0: -0.7}
        g = ChainGraph(_rand_num_fst(rs, H, int(rs.randint(0, 4)), D, fin), log_domain=True)
        x = torch.from_numpy(rs.normal(0, 2, size=(1, L, D)).astype(np.float32))
        lo = rs.randint(-1, L // 2 + 2, size=H)
        win = np.stack([lo, lo + rs.randint(-1, L + 3, size=H)], axis=1).astype(np.int32)
        gb = ChainGraphBatch(g, 1)
        gb.set_time_windows(torch.from_numpy(win).unsqueeze(0))
        o, grad = _objf_grad(x, torch.tensor([L]), gb)
        ref, post = _brute(g, x[0], L, win)
        if ref == -np.inf:
            assert o == -np.inf, (trial, o)
            assert bool((grad == 0).all())
            continue
        feasible += 1
        assert abs(o - ref) <= 1e-6 * max(1.0, abs(ref)), (trial, o, ref)
        assert np.abs(grad[0].numpy() - post).max() <= 1e-6, trial
    assert feasible >= 10


def test_full_windows_are_bit_identical_g2(golden):
    z = golden("g2_c1_chainloss")
    numb = batch_from_npz(z, "numbatch_")
    x, lengths = torch.from_numpy(z["x"]), torch.from_numpy(z["lengths"])
    B, H = numb.batch_size, numb.num_states
    ref = _per_seq(x, lengths, numb)
    for w in (_full(B, H, 0, x.shape[1]), _full(B, H, -5, BIG), _full(B, H, -2 ** 31, BIG)):
        got = _per_seq(x, lengths, numb, w)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
    numb.set_time_windows(_full(B, H, -3, x.shape[1] + 4))
    o, g = _objf_grad(x, lengths, numb)
    numb.set_time_windows(None)
    o0, g0 = _objf_grad(x, lengths, numb)
    assert o == o0 and torch.equal(g, g0)


def test_full_windows_are_bit_identical_long_shared():
    case = long_case("num_shared_T720")
    gb, x, lengths = case["num"], case["x"], case["lengths"]
    ref = _per_seq(x, lengths, gb)
    got = _per_seq(x, lengths, gb, _full(gb.batch_size, gb.num_states, -1, 10 ** 6))
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_forbidden_emission_has_zero_gradient():
    rs = np.random.RandomState(8)
    D = 6
    g = ChainGraph(_rand_num_fst(rs, 7, 6, D, lambda n: {n - 1: 0.0}), log_domain=True)
    L = 12
    x = torch.from_numpy(rs.normal(0, 1, size=(1, L, D)).astype(np.float32))
    ft = g.forward_transitions.numpy()
    checked = 0
    for t, p in [(2, int(ft[0][2])), (5, int(ft[3][2])), (9, int(ft[5][2]))]:
        emitters = sorted({int(s) for s, _, q in ft if q == p})
        w = _full(1, g.num_states, 0, L)
        for h in emitters:                         # admissible everywhere but at t
            w[0, h] = torch.tensor([t + 1, L], dtype=torch.int32) if t < L // 2 else torch.tensor([0, t - 1], dtype=torch.int32)
        gb = ChainGraphBatch(g, 1)
        gb.set_time_windows(w)
        o, grad = _objf_grad(x, torch.tensor([L]), gb)
        assert float(grad[0, t, p]) == 0.0
        if np.isfinite(o):
            checked += 1
            assert abs(float(grad[0].sum()) - L) < 1e-4          # (every frame's occupancies still sum to one)
    assert checked >= 1


def test_alignment_windows_exact():
    states = torch.tensor([[0, 0, 1, 1, 2, -1, -1],
                           [0, 1, 2, 3, 3, 3, 4],
                           [-1, -1, -1, -1, -1, -1, -1]], dtype=torch.int32)
    ali = Alignment(torch.zeros(3, 6, dtype=torch.int64), states, torch.tensor([-1.0, -2.0, -np.inf], dtype=torch.float64),
                    torch.tensor([True, True, False]))
    w = alignment_windows(ali, 5, tolerance=(1, 2))
    assert w.dtype == torch.int32 and tuple(w.shape) == (3, 5, 2)
    assert w[0].tolist() == [[0, 3], [1, 4], [3, 4], [0, -1], [0, -1]]
    assert w[1].tolist() == [[0, 2], [0, 3], [1, 4], [2, 6], [5, 6]]
    assert w[2].tolist() == [[0, 6]] * 5
    w0 = alignment_windows(ali, 5, tolerance=0)
    assert w0[1].tolist() == [[0, 0], [1, 1], [2, 2], [3, 5], [6, 6]]
    assert alignment_windows(ali, 6, 1)[0, 5].tolist() == [0, -1]
    for bad in (-1, (1, -1), (1, 2, 3), 1.5, True):
        with pytest.raises(ValueError):
            alignment_windows(ali, 5, bad)


def _branching_batch(seed, sizes, D):
    rs = np.random.RandomState(seed)
    fin = lambda H: {H - 1: 0.0, H - 2: -0.4}
    gs = [ChainGraph(_rand_num_fst(rs, h, h, D, fin), log_domain=True) for h in sizes]
    return ChainGraphBatch(gs, max_num_transitions=max(g.num_transitions for g in gs), max_num_states=max(g.num_states for g in gs))


def test_alignment_windows_bounds_and_monotone():
    D = 19
    gb = _branching_batch(4, [12, 25, 7, 18], D)
    x = syn.make_input(4, 70, D, seed=44)
    lengths = torch.tensor([70, 51, 23, 66])
    ali = viterbi_align(x, lengths, gb)
    assert bool(ali.ok.all())
    free, _, _ = _per_seq(x, lengths, gb)
    prev = None
    for tol in (0, 1, 2, 5):
        w = alignment_windows(ali, gb.num_states, tol)
        o, _, bad = _per_seq(x, lengths, gb, w)
        assert int(bad) == 0
        o64 = o.double()
        assert bool((ali.score <= o64 + 1e-5 * o64.abs()).all()), (tol, ali.score, o)
        assert bool((o <= free + 1e-5 * free.abs()).all())
        if prev is not None:
            assert bool((prev <= o + 1e-5 * o.abs()).all())
        prev = o
    assert bool((prev < free).any())                # (a tolerance of 5 frames still excludes paths)


def test_infeasible_sequence():
    D = 11
    gb = _branching_batch(6, [9, 14, 6], D)
    x = syn.make_input(3, 40, D, seed=5)
    lengths = torch.tensor([40, 31, 22])
    B, H = gb.batch_size, gb.num_states
    full = _full(B, H, 0, 40)
    w = full.clone()
    w[1, :, 0], w[1, :, 1] = 5, 4                   # lo > hi: never
    o, g, bad = _per_seq(x, lengths, gb, w)
    of, gf, badf = _per_seq(x, lengths, gb, full)
    assert float(o[1]) == -np.inf and int(bad) == 1 and int(badf) == 0
    for b in (0, 2):
        assert torch.equal(o[b], of[b]) and torch.equal(g[b], gf[b])
    assert bool((g[1] == 0).all())


def test_chainloss_on_cpu_uses_windows(golden):
    z = golden("g2_c1_chainloss")
    den, numb = graph_from_npz(z, "den_"), batch_from_npz(z, "numbatch_")
    x, lengths = torch.from_numpy(z["x"]), torch.from_numpy(z["lengths"])
    ali = viterbi_align(x, lengths, numb)
    w = alignment_windows(ali, numb.num_states, 1)
    free = float(ChainLoss(den, 1e-5, avg=False)(x, lengths, numb))
    numb.set_time_windows(w)
    loss = float(ChainLoss(den, 1e-5, avg=False)(x, lengths, numb))
    num, _, _ = _per_seq(x, lengths, numb, w)
    dn, _, _ = native.cpu_forward_backward(ChainGraphBatch(den, numb.batch_size), x, lengths, 1e-5)
    expect = -(float(num.sum()) - float(dn.sum()))
    assert abs(loss - expect) <= 1e-6 * abs(expect)
    assert loss != free and loss >= free           # (fewer numerator paths: a larger loss)


def _check_reorder(gb, x, lengths, order):
    w = torch.from_numpy(np.random.RandomState(1).randint(-1, 8, size=(gb.batch_size, gb.num_states, 2))).to(torch.int32)
    w[..., 1] += 30
    gb.set_time_windows(w)
    o, _, _ = _per_seq(x, lengths, gb)              # (no windows passed: what the batch's own are worth is checked below)
    ow, _, _ = native.cpu_forward_backward(gb, x, lengths, windows=gb.time_windows)
    gb.reorder(order)
    assert torch.equal(gb.time_windows, w[order])
    o2, _, _ = native.cpu_forward_backward(gb, x[order], lengths[order], windows=gb.time_windows)
    assert torch.equal(o2, ow[order])
    assert not torch.equal(ow, o)


def test_reorder_carries_windows():
    D = 13
    x = syn.make_input(4, 36, D, seed=2)
    lengths = torch.tensor([36, 30, 33, 25])
    order = torch.tensor([2, 0, 3, 1])
    packed = _branching_batch(7, [8, 11, 6, 9], D)
    assert packed._packed_consistent()
    _check_reorder(packed, x, lengths, order)
    sel = _branching_batch(7, [8, 11, 6, 9], D)
    sel.set_time_windows(_full(4, sel.num_states, 0, 40))
    sel.reorder(torch.tensor([3, 1]))
    assert tuple(sel.time_windows.shape) == (2, sel.num_states, 2)
    rs = np.random.RandomState(2)
    shared = ChainGraphBatch(ChainGraph(_rand_num_fst(rs, 10, 6, D, lambda n: {n - 1: 0.0}), log_domain=True), 4)
    _check_reorder(shared, x, lengths, order)
    assert shared.shared_graph is not None


def test_reorder_python_collated(golden):
    z = golden("g2_c1_chainloss")
    numb = batch_from_npz(z, "numbatch_")
    assert not numb._packed_consistent()
    x, lengths = torch.from_numpy(z["x"]), torch.from_numpy(z["lengths"])
    order = torch.arange(numb.batch_size - 1, -1, -1)
    _check_reorder(numb, x, lengths, order)


def test_pickle_and_shard_batch_keep_windows():
    D = 9
    gb = _branching_batch(9, [6, 8, 5, 7], D)
    w = _full(4, gb.num_states, 0, 20)
    w[2, 1] = torch.tensor([3, 9], dtype=torch.int32)
    gb.set_time_windows(w.to(torch.int64))
    assert gb.time_windows.dtype == torch.int32 and gb.time_windows.is_contiguous()
    back = pickle.loads(pickle.dumps(gb))
    assert torch.equal(back.time_windows, w)
    lengths = torch.tensor([20, 17, 19, 12])
    _, ls, gs, idx = shard_batch(None, lengths, gb, 2, 1)
    assert torch.equal(gs.time_windows, w[idx])
    assert torch.equal(gb.time_windows, w)          # (the global batch keeps its own)
    # a batch pickled before windows existed (no attribute) loads with none
    old = _branching_batch(9, [6, 8], D)
    st = old.__getstate__()
    st.pop("time_windows", None)
    fresh = ChainGraphBatch.__new__(ChainGraphBatch)
    fresh.__setstate__(st)
    assert fresh.time_windows is None


def test_errors():
    D = 7
    gb = _branching_batch(10, [5, 6], D)
    H = gb.num_states
    with pytest.raises(ValueError):
        gb.set_time_windows(torch.zeros(2, H + 1, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        gb.set_time_windows(torch.zeros(2, H, 2, dtype=torch.float32))
    with pytest.raises(ValueError):
        gb.set_time_windows(np.zeros((2, H, 2), dtype=np.int32))
    rs = np.random.RandomState(0)
    den = ChainGraph(_rand_num_fst(rs, 5, 3, D, lambda n: {n - 1: 0.0}), log_domain=False)
    with pytest.raises(ValueError):
        ChainGraphBatch(den, 2).set_time_windows(torch.zeros(2, 5, 2, dtype=torch.int32))
    gb.set_time_windows(_full(2, H))
    x = syn.make_input(2, 10, D, seed=1)
    with pytest.raises(ValueError):
        viterbi_align(x, torch.tensor([10, 8]), gb)
    gb.set_time_windows(None)
    assert gb.time_windows is None
    viterbi_align(x, torch.tensor([10, 8]), gb)
