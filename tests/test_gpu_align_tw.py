"""Constrained re-alignment on the MI355X (csrc/align.hip: the TW forms of align_kernel and align_general_kernel) against the
float64 reference of the ABI (tests/align_tw_reference.py: np_viterbi_tw), bit for bit: every launch form by row width with
fp32 and 2-byte rows under windows displaced to another input's alignment, arbitrary windows with an infeasible middle
sequence, lengths 1..64 through the h + 512 loop and the block backtrace, the last tile graph and the first general one, ties
under an emptied chain, windows that change nothing, and the round trip into the constrained numerator.
tests/test_align_tw.py holds the host twin to the same reference and checks that the cases are what they claim."""
import numpy as np
import pytest
import torch

import num_cases as nc
from align_tw_reference import displaced_windows, frames_differing, np_viterbi_tw
from num_reference import check_alignment, np_viterbi
from pychain_amd import ChainFunction, _lib, alignment_windows, native, viterbi_align
from test_align_tw import check_ties_moved, emptied_chain_windows, other_input

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
HALF = (torch.bfloat16, torch.float16)
BITS = torch.int64


def _gt(graphs):
    return graphs.device_tensors(torch.device(DEV)), 0 if graphs.shared_graph is not None else 1


def _device_equals_reference(x, lengths, graphs, w, ref=None):
    """native.align under `w` (lengths on the host and on the device) and viterbi_align on device tensors (explicit windows and
    the batch's own) against np_viterbi_tw on the fp32 value of the same input (`ref`: that, where the caller has it)."""
    if ref is None:
        ref = np_viterbi_tw(graphs, x.float(), lengths, w)
    gt, gstride = _gt(graphs)
    calls = _lib.lib().pychain_hip_cpu_calls()
    xd, wd = x.to(DEV), w.to(DEV)
    for ld in (lengths, lengths.to(DEV)):
        score, states, pdfs, bad = native.align(gt, gstride, graphs.num_states, xd, ld, windows=wd)
        torch.cuda.synchronize()
        check_alignment(score.cpu(), states.cpu(), pdfs.cpu(), torch.isfinite(score).cpu(), bad.cpu(), ref, lengths)
    ali = viterbi_align(xd, lengths, graphs, time_windows=w)
    graphs.set_time_windows(w)
    try:
        own = viterbi_align(xd, lengths, graphs, time_windows=True)
    finally:
        graphs.set_time_windows(None)
    torch.cuda.synchronize()
    assert _lib.lib().pychain_hip_cpu_calls() == calls              # device tensors never reach the host twin
    for a in (ali, own):
        assert a.score.device.type == "cuda"
        check_alignment(a.score.cpu(), a.states.cpu(), a.pdfs.cpu(), a.ok.cpu(), int((~a.ok).sum()), ref, lengths)
    return ref, ali


def _half_native(graphs, D):
    return bool(_lib.lib().pychain_hip_align_half_native(graphs.num_states, int(graphs.backward_transitions.shape[-2]), D))


def _all_dtypes(x, lengths, graphs, w, expect_half=None, ref=None, halves=HALF):
    """fp32 and, where the kernels read 2-byte rows, bf16 and fp16 against the reference on their exact fp32 up-cast."""
    half = _half_native(graphs, x.shape[2])
    if expect_half is not None:
        assert half == expect_half
    ref, _ = _device_equals_reference(x, lengths, graphs, w, ref)
    if half:
        for dtype in halves:
            _device_equals_reference(x.to(dtype), lengths, graphs, w)
    return ref


def _displaced(x, lengths, graphs, seed, scale=1.0, tau=2):
    """Windows at tolerance `tau` around another input's alignment, and what the reference says of them: feasible, the free
    path excluded, and a sequence whose constrained path is neither the free one nor the other input's."""
    w, other = displaced_windows(other_input(x, seed, scale), lengths, graphs, tau)
    free, con = np_viterbi(graphs, x, lengths), np_viterbi_tw(graphs, x, lengths, w)
    assert bool(np.isfinite(con[0]).all()) and bool((con[0] <= free[0]).all())
    assert any(a > 0 and b > 0 for a, b in zip(frames_differing(con, free, lengths), frames_differing(con, other, lengths)))
    return w, con


def _same(a, b):
    return all(torch.equal(p.view(BITS) if p.dtype == torch.float64 else p, q.view(BITS) if q.dtype == torch.float64 else q)
               for p, q in zip(a, b))


# ---- every launch form -----------------------------------------------------------------------------------------------------------------
HALF_NATIVE_D = {4: True, 48: True, 2048: True, 2052: True, 4096: True, 4100: True, 8408: True, 16384: True, 16388: False,
                 1001: False, 4095: False, 4097: False, "tile_last": False, "general_first": False}


@pytest.mark.parametrize("D", list(nc.FORM_D) + ["tile_last", "general_first"])
def test_form_matrix_displaced_windows(D):
    expect_half = HALF_NATIVE_D[D]
    if isinstance(D, str):
        pair = nc.form_boundary_D()
        D = pair[("tile_last", "general_first").index(D)]
    x, lengths, graphs = nc.form_case(D)
    w, con = _displaced(x, lengths, graphs, 991, 6.0)
    ref = _all_dtypes(x, lengths, graphs, w, expect_half, con)
    assert bool(np.isfinite(ref[0]).all())


@pytest.mark.parametrize("D", [48, 1001])
def test_form_matrix_perturbed_windows_infeasible_middle(D):
    x, lengths, graphs, w = nc.form_windows_case(D)
    ref = _all_dtypes(x, lengths, graphs, w)
    assert np.isfinite(ref[0]).tolist() == [True, False, True] and ref[0][1] == -np.inf
    # (check_alignment held the neighbours' rows to the reference bit for bit: untouched by the sequence between them)
    assert bool((ref[1][1] == -1).all()) and bool((ref[1][0, :lengths[0] + 1] >= 0).all()) and bool((ref[1][2, :lengths[2] + 1] >= 0).all())


# ---- the h + 512 loop and the block backtrace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B,D", [(701, 64, 48), (4000, 64, 48)])
def test_backtrace_sweep_displaced_windows(H, B, D):
    x, lengths, graphs = nc.sweep_case(H, B, D)
    assert nc.on_tile_path(H, graphs.shared_graph.num_transitions, D) and lengths.tolist() == list(range(1, B + 1))
    w, con = _displaced(x, lengths, graphs, 993)
    ref = _all_dtypes(x, lengths, graphs, w, True, con, HALF if H < 1000 else HALF[:1])     # (the larger reference: bf16 only)
    assert bool(np.isfinite(ref[0]).all())


def test_last_tile_graph_and_first_general():
    h_in, h_out = nc.tile_boundary_H()
    assert h_out == h_in + 1
    for H, tile in ((h_in, True), (h_out, False)):
        x, lengths, graphs = nc.largest_tile_case(H)
        assert nc.on_tile_path(H, graphs.shared_graph.num_transitions, 48) == tile
        w, con = _displaced(x, lengths, graphs, 994)
        ref = _all_dtypes(x, lengths, graphs, w, tile, con)
        assert bool(np.isfinite(ref[0]).all())


def test_shared701_windows_sequence_2_infeasible():
    x, lengths, graphs, w = nc.shared701_case()
    ref = _all_dtypes(x, lengths, graphs, w, True)
    assert np.isfinite(ref[0]).tolist() == [True, True, False, True]


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_ties_with_the_first_chain_emptied(dtype):
    x, lengths, graphs = nc.ties_case()
    xh = x.to(dtype)
    assert torch.equal(xh.float(), x) and _half_native(graphs, x.shape[2])
    w = emptied_chain_windows(graphs)
    ref, dev = _device_equals_reference(xh, lengths, graphs, w)
    check_ties_moved(ref, lengths)
    host = viterbi_align(x, lengths, graphs, time_windows=w)            # the tie case is also equal to the host twin
    assert torch.equal(dev.score.cpu().view(BITS), host.score.view(BITS))
    assert torch.equal(dev.states.cpu(), host.states) and torch.equal(dev.pdfs.cpu(), host.pdfs)


# ---- windows that change nothing -------------------------------------------------------------------------------------------------------
def _nothing_cases(name):
    if name == "general_first":
        return nc.form_case(nc.form_boundary_D()[1])
    return {"form48": lambda: nc.form_case(48), "form1001_nan": lambda: nc.form_case(1001, nan=True), "form8408": lambda: nc.form_case(8408),
            "ties": nc.ties_case, "sweep701": lambda: nc.sweep_case(701, 64, 48)}[name]()


@pytest.mark.parametrize("name", ["form48", "form1001_nan", "form8408", "general_first", "ties", "sweep701"])
def test_full_windows_equal_the_unwindowed_call(name):
    x, lengths, graphs = _nothing_cases(name)
    gt, gstride = _gt(graphs)
    B, H = graphs.batch_size, graphs.num_states
    exact = torch.stack([torch.zeros(B, H, dtype=torch.int32), lengths.to(torch.int32).unsqueeze(1).expand(B, H)], dim=-1)
    for xd in [x.to(DEV)] + ([x.to(DEV, torch.bfloat16)] if _half_native(graphs, x.shape[2]) else []):
        free = native.align(gt, gstride, H, xd, lengths)
        for w in (nc.full_windows(B, H), nc.full_windows(B, H, 0, int(lengths.max())), exact):
            got = native.align(gt, gstride, H, xd, lengths, windows=w.to(DEV))
            assert _same(got, free)                                 # score words (a NaN's too), states, pdfs, bad_count


@pytest.mark.parametrize("name", ["form48", "form8408", "general_first", "ties", "sweep701"])
def test_own_windows_at_tolerance_0_give_the_free_alignment(name):
    x, lengths, graphs = _nothing_cases(name)
    xd = x.to(DEV)
    free = viterbi_align(xd, lengths, graphs)
    assert bool(free.ok.all())
    w = alignment_windows(free, graphs.num_states, 0)
    assert w.device.type == "cuda"
    own = viterbi_align(xd, lengths, graphs, time_windows=w)
    assert _same(own, free)


# ---- into the constrained numerator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["form48", "sweep701"])
def test_round_trip_into_the_constrained_numerator(name):
    x, lengths, graphs = _nothing_cases(name)
    w, _ = _displaced(x, lengths, graphs, 991 if name == "form48" else 993, 6.0 if name == "form48" else 1.0)
    xd = x.to(DEV)
    con = viterbi_align(xd, lengths, graphs, time_windows=w)
    assert bool(con.ok.all())
    graphs.set_time_windows(alignment_windows(con, graphs.num_states, 0))
    try:
        gt, gstride = _gt(graphs)
        objf, _, bad = native.num_forward_backward(gt, gstride, graphs.num_states, xd, lengths, windows=graphs.device_time_windows(DEV))
        total = ChainFunction.apply(xd, lengths, graphs)
        torch.cuda.synchronize()
    finally:
        graphs.set_time_windows(None)
    score = con.score.cpu().numpy()
    logp = objf.double().cpu().numpy()
    assert int(bad) == 0
    print("%s: min (logP - score) / |score| = %.3e" % (name, float(((logp - score) / np.abs(score)).min())))
    assert bool((logp >= score - 1e-6 * np.abs(score)).all())       # the constrained path is among the admitted ones
    assert float(total) >= float(score.sum()) - 1e-6 * float(np.abs(score).sum())
