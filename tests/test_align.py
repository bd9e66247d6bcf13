"""viterbi_align on CPU tensors (the host twin, csrc/cpu.cpp: pychain_hip_cpu_align) against a plain numpy Viterbi (tests/num_reference.py:
np_viterbi) in fp64 with the association and tie rules of include/pychain_hip.h, against brute force on tiny graphs, hand-predicted ties, a
planted path, the numerator objective (log-sum >= max) and its error contract.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

from helpers import _rand_num_fst, long_case
from num_reference import np_viterbi
from pychain_amd import Alignment, ChainGraph, ChainGraphBatch, native, viterbi_align, synthetic as syn
from pychain_amd.simplefst import StdVectorFst


def _assert_identical(ali, ref):
    score, states, pdfs = ref[:3]
    assert isinstance(ali, Alignment)
    assert ali.score.dtype == torch.float64 and ali.states.dtype == torch.int32 and ali.pdfs.dtype == torch.int64
    assert np.array_equal(ali.score.numpy(), score, equal_nan=True)
    assert np.array_equal(ali.states.numpy(), states)
    assert np.array_equal(ali.pdfs.numpy(), pdfs)
    assert np.array_equal(ali.ok.numpy(), np.isfinite(score))


def _branching_batch(seed, sizes, D):
    rs = np.random.RandomState(seed)
    fin = lambda H: {H - 1: 0.0, H - 2: -0.4}
    gs = [ChainGraph(_rand_num_fst(rs, h, h, D, fin), log_domain=True) for h in sizes]
    return ChainGraphBatch(gs, max_num_transitions=max(g.num_transitions for g in gs), max_num_states=max(g.num_states for g in gs))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_twin_equals_numpy_branching(seed):
    D = 23
    gb = _branching_batch(seed, [12, 30, 5, 19], D)
    x = syn.make_input(4, 61, D, seed=seed + 40)
    lengths = torch.tensor([61, 40, 9, 33])[torch.from_numpy(np.random.RandomState(seed).permutation(4))]
    ali = viterbi_align(x, lengths, gb)
    _assert_identical(ali, np_viterbi(gb, x, lengths))
    assert int(ali.ok.sum()) >= 3                          # (a 30-state graph cannot be crossed in 9 frames)


def test_host_twin_equals_numpy_shared_graph():
    rs = np.random.RandomState(9)
    g = ChainGraph(_rand_num_fst(rs, 25, 30, 17, lambda H: {H - 1: 0.0}), log_domain=True)
    gb = ChainGraphBatch(g, 3)
    x = syn.make_input(3, 50, 17, seed=3)
    lengths = torch.tensor([50, 26, 44])
    _assert_identical(viterbi_align(x, lengths, gb), np_viterbi(gb, x, lengths))


@pytest.mark.parametrize("name", ["num_shared_T720", "fold_T751"])
def test_host_twin_equals_numpy_long_cases(name):
    case = long_case(name)
    ali = viterbi_align(case["x"], case["lengths"], case["num"])
    _assert_identical(ali, np_viterbi(case["num"], case["x"], case["lengths"]))
    assert bool(ali.ok.all())


def _tiny_graph(rs, H, D):
    arcs = []
    for s in range(H):
        for d in range(H):
            for _ in range(rs.randint(0, 3)):
                arcs.append((s, d, int(rs.randint(D)), float(np.float32(-rs.uniform(0.1, 2.0)))))
    if not arcs:
        arcs = [(0, 0, 0, -1.0)]
    arcs.sort(key=lambda a: a[0])
    finals = {h: float(np.float32(-rs.uniform(0, 1))) for h in range(H) if rs.rand() < 0.6} or {H - 1: 0.0}
    return ChainGraph(StdVectorFst.from_arcs(H, 0, arcs, finals), log_domain=True), arcs, finals


def test_brute_force_tiny_graphs():
    rs = np.random.RandomState(21)
    D = 5
    for trial in range(25):
        H, L = int(rs.randint(1, 5)), int(rs.randint(1, 7))
        g, arcs, finals = _tiny_graph(rs, H, D)
        x = torch.from_numpy(rs.normal(0, 2, size=(1, L, D)).astype(np.float32))
        ali = viterbi_align(x, torch.tensor([L]), ChainGraphBatch(g, 1))
        xd = x[0].numpy().astype(np.float64)
        init = g.initial_probs.numpy().astype(np.float64)
        best = -np.inf
        for path in itertools.product(range(len(arcs)), repeat=L):       # every arc sequence
            a = [arcs[k] for k in path]
            if any(a[i][1] != a[i + 1][0] for i in range(L - 1)) or a[-1][1] not in finals:
                continue
            v = init[a[0][0]] + sum(float(np.float32(p)) + xd[t, pdf] for t, (_, _, pdf, p) in enumerate(a)) + finals[a[-1][1]]
            best = max(best, v)
        sc = float(ali.score[0])
        if best == -np.inf:
            assert sc == -np.inf and not bool(ali.ok[0])
            continue
        assert abs(sc - best) <= 1e-12 * max(1.0, abs(best)), (trial, sc, best)
        # the returned path re-scores, in the recursion's association, to exactly the score
        st, pd = ali.states[0].numpy(), ali.pdfs[0].numpy()
        s = np.float64(init[st[0]])
        for t in range(L):
            lps = [np.float64(np.float32(p)) for (a0, a1, pdf, p) in arcs if a0 == st[t] and a1 == st[t + 1] and pdf == pd[t]]
            assert lps, (trial, t)
            s = s + (max(lps) + np.float64(np.clip(np.float32(x[0, t, pd[t]]), -30, 30)))
        assert s + np.float64(np.float32(finals[int(st[L])])) == sc


def _diamond():
    # 0 -> {1, 2} -> 3, 3 loops; every arc -1: the two branches always tie
    arcs = [(0, 1, 0, -1.0), (0, 2, 1, -1.0), (1, 3, 2, -1.0), (2, 3, 3, -1.0), (3, 3, 4, -1.0)]
    return arcs


def test_ties_take_the_earliest_arc_and_lowest_state():
    g = ChainGraph(StdVectorFst.from_arcs(4, 0, _diamond(), {3: 0.0}), log_domain=True)
    ali = viterbi_align(torch.zeros(1, 4, 5), torch.tensor([3]), ChainGraphBatch(g, 1))
    # arcs entering 3 in list order: 1->3, 2->3, 3->3; at t = 2 the two branches tie and 1->3 (first) wins
    assert ali.states[0].tolist() == [0, 1, 3, 3, -1] and ali.pdfs[0].tolist() == [0, 2, 4, -1]
    assert float(ali.score[0]) == -3.0
    # states 1 and 2 final with the same weight after one frame: the lower state wins
    g2 = ChainGraph(StdVectorFst.from_arcs(4, 0, _diamond(), {1: 0.0, 2: 0.0}), log_domain=True)
    ali2 = viterbi_align(torch.zeros(1, 1, 5), torch.tensor([1]), ChainGraphBatch(g2, 1))
    assert ali2.states[0].tolist() == [0, 1] and ali2.pdfs[0].tolist() == [0]


def test_planted_path_is_recovered():
    rs = np.random.RandomState(4)
    H, L = 30, 40
    arcs = []
    for s in range(H):                                     # self-loop, next, skip: every arc its own pdf
        for d in (s, s + 1, s + 2):
            if d < H:
                arcs.append((s, d, len(arcs), float(np.float32(-rs.uniform(0.5, 1.3)))))
    D = len(arcs)
    g = ChainGraph(StdVectorFst.from_arcs(H, 0, arcs, {h: 0.0 for h in range(H)}), log_domain=True)
    for trial in range(5):
        s, planted = 0, []
        for t in range(L):
            out = [a for a in arcs if a[0] == s]
            a = out[rs.randint(len(out))]
            planted.append(a[2])
            s = a[1]
        x = torch.full((1, L + 5, D), -30.0)
        x[0, torch.arange(L), torch.tensor(planted)] = 30.0
        ali = viterbi_align(x, torch.tensor([L]), ChainGraphBatch(g, 1))
        assert ali.pdfs[0, :L].tolist() == planted and bool((ali.pdfs[0, L:] == -1).all())


def test_score_bounded_by_numerator_objective():
    w = syn.make_workload("C1")
    for x, lengths, gb in ((w["x"], w["lengths"], w["num_graphs"]),
                           (syn.make_input(4, 61, 23, seed=7), torch.tensor([61, 50, 12, 33]), _branching_batch(5, [12, 30, 5, 19], 23))):
        ali = viterbi_align(x, lengths, gb)
        objf, _, bad = native.cpu_forward_backward(gb, x, lengths)
        assert int(bad) == 0 and bool(ali.ok.all())
        o = objf.double()
        assert bool((ali.score <= o + 1e-6 * o.abs()).all()), (ali.score, o)


def test_unreachable_and_nan():
    gb = _branching_batch(3, [20, 8], 11)
    x = syn.make_input(2, 30, 11, seed=2)
    ali = viterbi_align(x, torch.tensor([30, 30]), gb)
    assert bool(ali.ok.all())
    _assert_identical(viterbi_align(x, torch.tensor([30, 3]), gb), np_viterbi(gb, x, torch.tensor([30, 3])))
    # a graph whose final state is 5 steps away, aligned over 2 frames: no path
    chain = ChainGraph(StdVectorFst.from_arcs(6, 0, [(s, s + 1, s, -0.5) for s in range(5)], {5: 0.0}), log_domain=True)
    un = viterbi_align(torch.zeros(1, 4, 6), torch.tensor([2]), ChainGraphBatch(chain, 1))
    assert float(un.score[0]) == -np.inf and not bool(un.ok[0])
    assert un.states[0].tolist() == [-1] * 5 and un.pdfs[0].tolist() == [-1] * 4
    # a NaN in a column the graph emits -> NaN score, rows -1; in a column no arc emits -> no effect
    used = set(gb.backward_transitions[1, :int(gb.backward_transition_indices[1, :, 1].max()), 2].tolist())
    xn = x.clone()
    xn[1, 17, sorted(used)[0]] = float("nan")
    a2 = viterbi_align(xn, torch.tensor([30, 30]), gb)
    assert torch.isnan(a2.score[1]) and not bool(a2.ok[1]) and bool(a2.ok[0])
    assert bool((a2.pdfs[1] == -1).all()) and bool((a2.states[1] == -1).all())
    assert torch.equal(a2.pdfs[0], ali.pdfs[0]) and a2.score[0] == ali.score[0]
    unused = sorted(set(range(11)) - used)
    if unused:
        xu = x.clone()
        xu[1, 17, unused[0]] = float("nan")
        a3 = viterbi_align(xu, torch.tensor([30, 30]), gb)
        assert torch.equal(a3.pdfs, ali.pdfs) and torch.equal(a3.score, ali.score)
    # a NaN beyond the sequence's length is not read
    xl = x.clone()
    xl[1, 25, sorted(used)[0]] = float("nan")
    a4 = viterbi_align(xl, torch.tensor([30, 20]), gb)
    assert bool(a4.ok.all())


def test_errors():
    w = syn.make_workload("C1")
    with pytest.raises(ValueError, match="log_domain"):
        viterbi_align(w["x"], w["lengths"], ChainGraphBatch(w["den_graph"], 2))
    with pytest.raises(ValueError, match="batch size"):
        viterbi_align(w["x"][:1], w["lengths"][:1], w["num_graphs"])
    for bad in ([0, 37], [51, 37]):
        with pytest.raises(ValueError, match="sequence lengths"):
            viterbi_align(w["x"], torch.tensor(bad), w["num_graphs"])
    with pytest.raises(ValueError, match="entries"):
        viterbi_align(w["x"], torch.tensor([50]), w["num_graphs"])


def test_half_and_grad_inputs():
    w = syn.make_workload("C1")
    xb = w["x"].to(torch.bfloat16).requires_grad_(True)
    a = viterbi_align(xb, w["lengths"], w["num_graphs"])
    ref = viterbi_align(xb.detach().float(), w["lengths"], w["num_graphs"])
    assert torch.equal(a.score, ref.score) and torch.equal(a.pdfs, ref.pdfs) and not a.score.requires_grad
    with torch.no_grad():
        assert torch.equal(viterbi_align(w["x"], w["lengths"].tolist(), w["num_graphs"]).states,
                           viterbi_align(w["x"], w["lengths"], w["num_graphs"]).states)
