"""Constrained re-alignment on CPU tensors (the host twin, csrc/cpu.cpp: pychain_hip_cpu_align_tw) against the float64
reference of the ABI (tests/align_tw_reference.py: np_viterbi_tw), bit for bit: windows displaced to another input's alignment
(feasible, and away from the free best path), arbitrary windows with a planted infeasible sequence, ties under an emptied
chain, windows that admit everything, a sequence's own windows, the NaN rule, and viterbi_align's argument handling.  What the
cases claim is asserted on the reference before the library is held to it.  The device runs them in test_gpu_align_tw.py.
No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import num_cases as nc
from align_tw_reference import admits, displaced_windows, frames_differing, np_viterbi_tw, windows_around
from num_reference import check_alignment, np_viterbi
from pychain_amd import ChainGraph, ChainGraphBatch, _lib, native, viterbi_align, synthetic as syn
from pychain_amd.simplefst import StdVectorFst

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = torch.int64


def host_equals_reference(x, lengths, graphs, w):
    """native.cpu_align and viterbi_align (explicit windows, and the batch's own) against np_viterbi_tw."""
    ref = np_viterbi_tw(graphs, x, lengths, w)
    score, states, pdfs, bad = native.cpu_align(graphs, x, lengths, windows=w)
    check_alignment(score, states, pdfs, torch.isfinite(score), bad, ref, lengths)
    ali = viterbi_align(x, lengths, graphs, time_windows=w)
    check_alignment(ali.score, ali.states, ali.pdfs, ali.ok, int((~ali.ok).sum()), ref, lengths)
    if w is not None:
        graphs.set_time_windows(w)
        try:
            own = viterbi_align(x, lengths, graphs, time_windows=True)
        finally:
            graphs.set_time_windows(None)
        assert _same(own, ali)
    return ref


def _same(a, b):
    return (torch.equal(a.score.view(BITS), b.score.view(BITS)) and torch.equal(a.states, b.states) and torch.equal(a.pdfs, b.pdfs)
            and torch.equal(a.ok, b.ok))


def other_input(x, seed, scale=1.0):
    return syn.make_input(x.shape[0], x.shape[1], x.shape[2], seed=seed) * scale


def displaced_case_holds(x, lengths, graphs, x2, tau):
    """The reference's own facts about displaced windows, then the host twin against it.  Returns (constrained, free, other)."""
    w, other = displaced_windows(x2, lengths, graphs, tau)
    free = np_viterbi(graphs, x, lengths)
    con = np_viterbi_tw(graphs, x, lengths, w)
    assert bool(np.isfinite(con[0]).all())                         # every sequence stays feasible
    assert all(admits(w, con, lengths)) and all(admits(w, other, lengths))
    assert bool((con[0] <= free[0]).all())                         # a maximum over a subset of the paths
    if tau == 0:                                                   # no room: the constrained path is the other input's
        assert frames_differing(con, other, lengths) == [0] * len(lengths)
    host_equals_reference(x, lengths, graphs, w)
    return con, free, other


# ---- the form matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0, 2])
@pytest.mark.parametrize("D", [4, 48, 1001])
def test_form_case_displaced_windows(D, tau):
    x, lengths, graphs = nc.form_case(D)
    con, free, other = displaced_case_holds(x, lengths, graphs, other_input(x, 991, 6.0), tau)
    from_free, from_other = frames_differing(con, free, lengths), frames_differing(con, other, lengths)
    print("D=%d tau=%d: frames differing from the free path %s, from the other input's %s" % (D, tau, from_free, from_other))
    assert any(from_free)                                          # the windows exclude the free best path
    if tau == 2:                                                   # a real search: neither the free path nor the other input's
        assert any(a > 0 and b > 0 for a, b in zip(from_free, from_other))


@pytest.mark.parametrize("tau", [0, 2])
def test_shared_graph_displaced_windows(tau):
    g = nc.all_final_graph(150, 48)
    lengths = torch.tensor([60, 47, 33, 5])
    x, graphs = syn.make_input(4, 60, 48, seed=7), ChainGraphBatch(g, 4)
    con, free, other = displaced_case_holds(x, lengths, graphs, other_input(x, 992), tau)
    from_free, from_other = frames_differing(con, free, lengths), frames_differing(con, other, lengths)
    print("shared tau=%d: frames differing from the free path %s, from the other input's %s" % (tau, from_free, from_other))
    assert any(from_free)
    if tau == 2:
        assert any(a > 0 and b > 0 for a, b in zip(from_free, from_other))


@pytest.mark.parametrize("D", [4, 48, 1001])
def test_form_case_perturbed_windows_infeasible_middle(D):
    x, lengths, graphs, w = nc.form_windows_case(D)
    ref = host_equals_reference(x, lengths, graphs, w)
    free = np_viterbi(graphs, x, lengths)
    assert np.isfinite(ref[0]).tolist() == [True, False, True]     # every sequence feasible, but the planted one
    assert ref[0][1] == -np.inf and bool((ref[1][1] == -1).all()) and bool((ref[2][1] == -1).all())
    assert bool((ref[0][[0, 2]] <= free[0][[0, 2]]).all())


def test_shared701_windows_sequence_2_infeasible():
    x, lengths, graphs, w = nc.shared701_case()
    ref = host_equals_reference(x, lengths, graphs, w)
    free = np_viterbi(graphs, x, lengths)
    assert np.isfinite(ref[0]).tolist() == [True, True, False, True] and ref[0][2] == -np.inf
    assert bool((ref[0][[0, 1, 3]] <= free[0][[0, 1, 3]]).all())


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
def emptied_chain_windows(graphs):
    """Everything admissible but the chain that starts at state 1, which never is."""
    w = nc.full_windows(graphs.batch_size, graphs.num_states)
    first = nc.TIE_STARTS[0]
    w[:, first:first + nc.TIE_CHAIN, 0], w[:, first:first + nc.TIE_CHAIN, 1] = 0, -1
    return w


def check_ties_moved(ref, lengths):
    L = lengths.numpy()
    assert np.array_equal(ref[3], L) and bool((ref[4] == 1).all())     # every frame still ties between the two arcs, the end between chains
    for b in range(len(L)):
        assert int(ref[1][b, L[b]]) == nc.TIE_STARTS[1] + nc.TIE_CHAIN - 1   # the next chain's last state
        assert bool((ref[2][b, :L[b]] % 2 == 0).all())             # the first arc of every pair


def test_ties_with_the_first_chain_emptied():
    x, lengths, graphs = nc.ties_case()
    ref = host_equals_reference(x, lengths, graphs, emptied_chain_windows(graphs))
    check_ties_moved(ref, lengths)
    free = np_viterbi(graphs, x, lengths)
    assert np.array_equal(ref[0], free[0])                         # (the chains are identical: the same score, another end state)


# ---- windows that change nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["form48", "form1001_nan", "ties"])
def test_full_windows_equal_the_unwindowed_call(case):
    x, lengths, graphs = {"form48": lambda: nc.form_case(48), "form1001_nan": lambda: nc.form_case(1001, nan=True),
                          "ties": nc.ties_case}[case]()
    B, H = graphs.batch_size, graphs.num_states
    free = native.cpu_align(graphs, x, lengths)
    exact = torch.stack([torch.zeros(B, H, dtype=torch.int32), lengths.to(torch.int32).unsqueeze(1).expand(B, H)], dim=-1)
    for w in (nc.full_windows(B, H), nc.full_windows(B, H, 0, int(lengths.max())), exact):
        got = native.cpu_align(graphs, x, lengths, windows=w)
        assert torch.equal(got[0].view(BITS), free[0].view(BITS))      # score words, a NaN's too
        assert torch.equal(got[1], free[1]) and torch.equal(got[2], free[2]) and torch.equal(got[3], free[3])
        assert _same(viterbi_align(x, lengths, graphs, time_windows=w), viterbi_align(x, lengths, graphs))


@pytest.mark.parametrize("case", ["form48", "shared701", "ties"])
def test_own_windows_at_tolerance_0_give_the_free_alignment(case):
    x, lengths, graphs = {"form48": lambda: nc.form_case(48), "shared701": lambda: nc.shared701_case(windows=False),
                          "ties": nc.ties_case}[case]()
    free = np_viterbi(graphs, x, lengths)
    w = windows_around(free, graphs.num_states, 0)
    ref = host_equals_reference(x, lengths, graphs, w)
    assert np.array_equal(ref[0].view(np.int64), free[0].view(np.int64))
    assert np.array_equal(ref[1], free[1]) and np.array_equal(ref[2], free[2])


# ---- the NaN rule ------------------------------------------------------------------------------------------------------------------------
def test_nan_that_reaches_only_masked_states_goes_no_further():
    """Two parallel branches from state 0: A = state 1 (its arcs emit pdf 0), B = state 2 (pdf 1), both final; a NaN in column 0."""
    arcs = [(0, 1, 0, -0.1), (0, 2, 1, -0.1), (1, 1, 0, -0.2), (2, 2, 1, -0.2)]
    g = ChainGraph(StdVectorFst.from_arcs(3, 0, arcs, {1: 0.0, 2: -0.3}), log_domain=True)
    graphs = ChainGraphBatch(g, 2)
    L = 5
    lengths = torch.tensor([L, L - 1])
    x = syn.make_input(2, L, 2, seed=3)
    x[..., 0] += 4.0                                               # (A is the better branch where it is allowed)
    clean = np_viterbi(graphs, x, lengths)
    assert clean[1][0, :L + 1].tolist() == [0, 1, 1, 1, 1, 1]
    x[0, 2, 0] = float("nan")                                      # sequence 0 only, on the arcs 2 -> 3 of branch A
    free = host_equals_reference(x, lengths, graphs, None)
    assert np.isnan(free[0][0]) and np.isfinite(free[0][1])
    w = nc.full_windows(2, 3)
    w[:, 1, 0], w[:, 1, 1] = 0, -1                                 # A never admissible
    ref = host_equals_reference(x, lengths, graphs, w)
    assert bool(np.isfinite(ref[0]).all())
    assert ref[1][0, :L + 1].tolist() == [0, 2, 2, 2, 2, 2] and ref[2][0, :L].tolist() == [1] * L
    xb = x.clone()
    xb[0, 2, 0] = 0.0
    assert ref[0][0] == np_viterbi_tw(graphs, xb, lengths, w)[0][0]     # (branch B's score whatever column 0 holds)
    for lo, hi in ((0, L), (3, 3), (-1, nc.BIG)):                  # A admissible when the NaN arrives (t + 1 = 3): NaN again
        w[:, 1, 0], w[:, 1, 1] = lo, hi
        ref = host_equals_reference(x, lengths, graphs, w)
        assert np.isnan(ref[0][0]) and np.isfinite(ref[0][1]) and bool((ref[1][0] == -1).all())
    w[:, 1, 0], w[:, 1, 1] = 4, L                                  # admissible only after it: no path through A, no NaN
    ref = host_equals_reference(x, lengths, graphs, w)
    assert bool(np.isfinite(ref[0]).all()) and ref[1][0, :L + 1].tolist() == [0, 2, 2, 2, 2, 2]
    # a final term counts only where its state is admissible at L: a NaN final weight on state 1, admissible up to L - 1
    gn = ChainGraph(StdVectorFst.from_arcs(3, 0, arcs, {1: 0.0, 2: -0.3}), log_domain=True)
    gn.final_probs[1] = float("nan")
    gnb = ChainGraphBatch(gn, 2)
    assert bool(np.isnan(host_equals_reference(xb, lengths, gnb, None)[0]).all())
    w = nc.full_windows(2, 3)
    w[:, 1, 0], w[:, 1, 1] = 0, L - 1
    ref = host_equals_reference(xb, lengths, gnb, w)
    assert np.isfinite(ref[0][0]) and np.isnan(ref[0][1])          # (sequence 1 has L - 1 frames: state 1 is admissible at its end)


# ---- viterbi_align's arguments -------------------------------------------------------------------------------------------------------
def test_viterbi_align_time_windows_argument():
    x, lengths, graphs = nc.form_case(4)
    B, H = graphs.batch_size, graphs.num_states
    free = viterbi_align(x, lengths, graphs)
    with pytest.raises(ValueError):
        viterbi_align(x, lengths, graphs, time_windows=True)       # the batch carries none
    for bad in (torch.zeros(B, H + 1, 2, dtype=torch.int32), torch.zeros(B, H, dtype=torch.int32), torch.zeros(B + 1, H, 2, dtype=torch.int32),
                torch.zeros(B, H, 2, dtype=torch.float32), np.zeros((B, H, 2), dtype=np.int32), False):
        with pytest.raises(ValueError):
            viterbi_align(x, lengths, graphs, time_windows=bad)
    with pytest.raises(ValueError):
        native.cpu_align(graphs, x, lengths, windows=torch.zeros(B, H, 2, dtype=torch.int64))    # (the native layer takes int32 only)
    wide = torch.empty(B, H, 2, dtype=torch.int64)
    wide[..., 0], wide[..., 1] = -2 ** 40, 2 ** 40                 # saturates to int32; wrapping would give (0, 0)
    assert _same(viterbi_align(x, lengths, graphs, time_windows=wide), free)
    w, _ = displaced_windows(other_input(x, 991, 6.0), lengths, graphs, 2)
    con = viterbi_align(x, lengths, graphs, time_windows=w)
    for dtype in (torch.int16, torch.int64):
        assert _same(viterbi_align(x, lengths, graphs, time_windows=w.to(dtype)), con)
    spaced = torch.zeros(B, H, 4, dtype=torch.int32)
    spaced[..., ::2] = w
    assert _same(viterbi_align(x, lengths, graphs, time_windows=spaced[..., ::2]), con)      # (a view that is not contiguous)
    graphs.set_time_windows(nc.full_windows(B, H))
    with pytest.raises(ValueError, match="time_windows"):          # the default still refuses a windowed batch, and says what to pass
        viterbi_align(x, lengths, graphs)
    assert _same(viterbi_align(x, lengths, graphs, time_windows=True), free)
    assert _same(viterbi_align(x, lengths, graphs, time_windows=w), con)     # explicit windows: whatever the batch carries
    graphs.set_time_windows(None)
    assert _same(viterbi_align(x, lengths, graphs), free)


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 26
    for name in ("pychain_hip_align_tw", "pychain_hip_cpu_align_tw"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    assert "pychain_hip_align takes none either" not in header
