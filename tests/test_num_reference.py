"""The float64 references of tests/num_reference.py against brute-force path enumeration, and the host twins (csrc/cpu.cpp:
pychain_hip_cpu_align, pychain_hip_cpu_num_forward_backward[_tw]) against the references on every case of tests/num_cases.py -
alignments bit for bit, the numerator within the project's 1e-5 - together with the conditions that keep those cases honest
(values beyond the clamp are emitted, the NaN is met, ties happen at both levels, windows constrain and one sequence of each
windowed batch is infeasible).  The device runs the same cases in test_gpu_align_forms.py / test_gpu_num_forms.py.  No GPU."""
import numpy as np
import pytest
import torch

import num_cases as nc
from helpers import _rand_num_fst
from num_reference import check_alignment, check_numerator, np_num_fb, np_viterbi
from pychain_amd import ChainGraph, ChainGraphBatch, native, viterbi_align
from test_time_windows import _brute


def host_alignment_equals_reference(x, lengths, graphs):
    ref = np_viterbi(graphs, x, lengths)
    ali = viterbi_align(x, lengths, graphs)
    score, states, pdfs, bad = native.cpu_align(graphs, x, lengths)
    assert torch.equal(ali.states, states) and torch.equal(ali.pdfs, pdfs)
    check_alignment(score, states, pdfs, ali.ok, bad, ref, lengths)
    return ref


def host_numerator_equals_reference(x, lengths, graphs, windows=None):
    ref = np_num_fb(graphs, x, lengths, windows)
    objf, grad, bad = native.cpu_forward_backward(graphs, x, lengths, windows=windows)
    check_numerator(objf.numpy(), grad.numpy(), bad, ref, lengths)
    return ref


# ---- the references themselves ------------------------------------------------------------------------------------------------------
def test_np_num_fb_equals_brute_force_windowed_and_free():
    rs = np.random.RandomState(3)
    D = 4
    feasible = infeasible = 0
    for trial in range(80):
        H, L = int(rs.randint(2, 6)), int(rs.randint(1, 7))
        fin = lambda n: {n - 1: 0.0, 0: -0.7}
        g = ChainGraph(_rand_num_fst(rs, H, int(rs.randint(0, 4)), D, fin), log_domain=True)
        x = torch.from_numpy(rs.normal(0, 2, size=(1, L + 1, D)).astype(np.float32))
        lo = rs.randint(-1, L // 2 + 2, size=H)
        win = np.stack([lo, lo + rs.randint(-1, L + 3, size=H)], axis=1).astype(np.int32)
        gb = ChainGraphBatch(g, 1)
        for w in (win, None):
            logp, grad, feas = np_num_fb(gb, x, torch.tensor([L]), None if w is None else torch.from_numpy(w).unsqueeze(0))
            ref, post = _brute(g, x[0], L, w if w is not None else np.array([[0, L]] * H))
            assert bool(feas[0]) == bool(ref > -np.inf)
            assert not grad[0, L:].any()
            if ref == -np.inf:
                infeasible += 1
                assert logp[0] == -np.inf and not grad.any()
                continue
            feasible += 1
            assert abs(logp[0] - ref) <= 1e-12 * max(1.0, abs(ref)), (trial, logp[0], ref)
            assert np.abs(grad[0, :L] - post).max() <= 1e-12, trial
    assert feasible >= 60 and infeasible >= 10


def test_np_viterbi_counts_ties():
    from pychain_amd.simplefst import StdVectorFst
    arcs = [(0, 1, 0, -1.0), (0, 2, 1, -1.0), (1, 3, 2, -1.0), (2, 3, 3, -1.0), (3, 3, 4, -1.0)]
    g = ChainGraph(StdVectorFst.from_arcs(4, 0, arcs, {3: 0.0}), log_domain=True)
    r = np_viterbi(ChainGraphBatch(g, 1), torch.zeros(1, 4, 5), torch.tensor([3]))
    assert r[1][0].tolist() == [0, 1, 3, 3, -1] and r[3].tolist() == [1] and r[4].tolist() == [0]
    g2 = ChainGraph(StdVectorFst.from_arcs(4, 0, arcs, {1: 0.0, 2: 0.0}), log_domain=True)
    r2 = np_viterbi(ChainGraphBatch(g2, 1), torch.zeros(1, 1, 5), torch.tensor([1]))
    assert r2[1][0].tolist() == [0, 1] and r2[3].tolist() == [0] and r2[4].tolist() == [1]


# ---- a. the form matrix ----------------------------------------------------------------------------------------------------------------
def test_form_boundary_pair_straddles_the_tile_kernels():
    d_in, d_out = nc.form_boundary_D()
    gb = nc.form_graphs(4)
    H, K = gb.num_states, int(gb.backward_transitions.shape[-2])
    assert d_out == d_in + 1 and nc.on_tile_path(H, K, d_in) and not nc.on_tile_path(H, K, d_out)
    assert 16388 < d_in < 65535
    assert nc.form_of(d_in) == "<1,0>"
    assert {nc.form_of(D) for D in nc.FORM_D} == {"<4,4,LD>", "<4,8,LD>", "<4,8>", "<1,8>", "<1,0>"}
    assert any(h % 2 for h in nc.FORM_SIZES) and gb.num_states == max(nc.FORM_SIZES)


def _form_ds():
    return list(nc.FORM_D) + ["tile_last", "general_first"]


def _resolve_d(D):
    return nc.form_boundary_D()[("tile_last", "general_first").index(D)] if isinstance(D, str) else D


@pytest.mark.parametrize("D", _form_ds())
def test_form_matrix_host_alignment(D):
    D = _resolve_d(D)
    x, lengths, graphs = nc.form_case(D)
    up, down = nc.emitted_beyond_clamp(x, lengths, graphs)
    assert up > 0 and down > 0                                     # (the clamp is exercised in both directions)
    ref = host_alignment_equals_reference(x, lengths, graphs)
    assert bool(np.isfinite(ref[0]).all())
    xn, _, _ = nc.form_case(D, nan=True)
    refn = host_alignment_equals_reference(xn, lengths, graphs)
    assert np.isnan(refn[0][1]) and bool((refn[1][1] == -1).all()) and bool((refn[2][1] == -1).all())
    for b in (0, 2):                                               # (the other sequences are as without the NaN)
        assert refn[0][b] == ref[0][b] and np.array_equal(refn[2][b], ref[2][b])


@pytest.mark.parametrize("D", _form_ds())
def test_form_matrix_host_numerator(D):
    D = _resolve_d(D)
    x, lengths, graphs, w = nc.form_windows_case(D)
    free = host_numerator_equals_reference(x, lengths, graphs)
    assert bool(free[2].all())
    full = host_numerator_equals_reference(x, lengths, graphs, nc.full_windows(graphs.batch_size, graphs.num_states))
    assert np.array_equal(full[0], free[0]) and np.array_equal(full[1], free[1])
    win = host_numerator_equals_reference(x, lengths, graphs, w)
    _check_window_shares(win, free, infeasible=1)


def _check_window_shares(win, free, infeasible):
    feas = win[2]
    B = feas.size
    assert 2 * int(feas.sum()) >= B and not feas[infeasible] and 0 < infeasible < B - 1
    assert bool((win[0][feas] < free[0][feas]).all())              # (the windows exclude paths of every feasible sequence)


def test_perturbed_windows_use_every_kind():
    x, lengths, graphs, w = nc.shared701_case()
    w = w.numpy().astype(np.int64)
    assert bool((w[..., 0] == -1).any()) and bool((w[..., 1] == nc.BIG).any()) and bool((w[..., 1] < w[..., 0]).any())
    assert bool(((w[..., 1] < w[..., 0]) & (w[..., 0] > 0)).any())


def test_shared701_host_numerator():
    x, lengths, graphs, w = nc.shared701_case()
    free = host_numerator_equals_reference(x, lengths, graphs)
    assert bool(free[2].all())
    win = host_numerator_equals_reference(x, lengths, graphs, w)
    _check_window_shares(win, free, infeasible=2)


# ---- b. the backtrace sweeps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B,D", nc.SWEEPS)
def test_sweep_host_alignment(H, B, D):
    x, lengths, graphs = nc.sweep_case(H, B, D)
    assert lengths.tolist() == list(range(1, B + 1)) and x.shape[1] == B
    g = graphs.shared_graph
    assert g.num_states == H and bool(torch.isfinite(g.final_probs).all())
    assert torch.unique(g.final_probs).numel() == H                # (small distinct final weights)
    ref = host_alignment_equals_reference(x, lengths, graphs)
    assert bool(np.isfinite(ref[0]).all())                         # every sweep sequence is ok


def test_sweep_4000_states_is_on_the_tile_path():
    g = nc.all_final_graph(4000, 48)
    assert g.num_transitions == 8399 and nc.on_tile_path(4000, 8399, 48)


def test_single_frame_host_alignment():
    x, lengths, graphs = nc.single_frame_case()
    assert tuple(x.shape[:2]) == (1, 1)
    ref = host_alignment_equals_reference(x, lengths, graphs)
    assert np.isfinite(ref[0][0])


# ---- c. the largest tile graph ---------------------------------------------------------------------------------------------------------
def test_tile_boundary_pair_and_host_alignment():
    h_in, h_out = nc.tile_boundary_H()
    assert h_out == h_in + 1 and h_in > 4000
    assert nc.on_tile_path(h_in, nc.tile_family_K(h_in), 48) and not nc.on_tile_path(h_out, nc.tile_family_K(h_out), 48)
    h_odd = next(H for H in range(h_in, 4000, -1) if nc.tile_family_K(H) % 2)
    for H in (h_in, h_out, h_odd):
        x, lengths, graphs = nc.largest_tile_case(H)
        ref = host_alignment_equals_reference(x, lengths, graphs)
        assert bool(np.isfinite(ref[0]).all())


# ---- d. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_ties_host_alignment(dtype):
    x, lengths, graphs = nc.ties_case()
    assert torch.equal(x.to(dtype).float(), x)                     # quarter-multiples are exact in bf16 and fp16
    assert torch.equal(x * 4, torch.round(x * 4)) and torch.equal(x[..., 1::2], x[..., 0::2])
    ref = host_alignment_equals_reference(x.to(dtype).float(), lengths, graphs)
    L = lengths.numpy()
    assert np.array_equal(ref[3], L) and bool((ref[4] == 1).all())     # every frame ties between two arcs, the end between chains
    for b in range(3):
        assert int(ref[1][b, L[b]]) == nc.TIE_STARTS[0] + nc.TIE_CHAIN - 1       # the lowest of the four final states
        assert bool((ref[2][b, :L[b]] % 2 == 0).all())             # the first arc of every pair
