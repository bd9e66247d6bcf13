"""viterbi_align on the MI355X against the float64 reference of the ABI (tests/num_reference.py: np_viterbi), bit for bit, on the
cases of tests/num_cases.py: every launch form of align_kernel by row width (launch_align: <4,4,LD> <4,8,LD> <4,8> <1,8> <1,0>,
fp32 and 2-byte rows, the last tile shape and the first general one) with values beyond the clamp and a NaN in the last column;
lengths 1..B through the block backtrace at 150 / 701 / 1500 / 4000 states (every residue of L modulo the block, one to
dozens of blocks) and T = 1; the largest graph the tile kernels take and the first they do not; exact ties between parallel
arcs and between final states in different lanes, waves and passes of the h + 512 loop.  tests/test_num_reference.py holds the
host twin to the same reference and checks that the cases are what they claim."""
import numpy as np
import pytest
import torch

import num_cases as nc
from num_reference import check_alignment, np_viterbi
from pychain_amd import _lib, native, viterbi_align

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
HALF = (torch.bfloat16, torch.float16)


def _device_equals_reference(x, lengths, graphs):
    """native.align (lengths on the host and on the device) and viterbi_align on device tensors against np_viterbi on the
    fp32 value of the same input."""
    ref = np_viterbi(graphs, x.float(), lengths)
    gt = graphs.device_tensors(torch.device(DEV))
    gstride = 0 if graphs.shared_graph is not None else 1
    calls = _lib.lib().pychain_hip_cpu_calls()
    xd = x.to(DEV)
    for ld in (lengths, lengths.to(DEV)):
        score, states, pdfs, bad = native.align(gt, gstride, graphs.num_states, xd, ld)
        torch.cuda.synchronize()
        check_alignment(score.cpu(), states.cpu(), pdfs.cpu(), torch.isfinite(score).cpu(), bad.cpu(), ref, lengths)
    ali = viterbi_align(xd, lengths, graphs)
    torch.cuda.synchronize()
    assert _lib.lib().pychain_hip_cpu_calls() == calls              # device tensors never reach the host twin
    check_alignment(ali.score.cpu(), ali.states.cpu(), ali.pdfs.cpu(), ali.ok.cpu(), int((~ali.ok).sum()), ref, lengths)
    return ref, ali


def _half_native(graphs, D):
    return bool(_lib.lib().pychain_hip_align_half_native(graphs.num_states, int(graphs.backward_transitions.shape[-2]), D))


def _all_dtypes(x, lengths, graphs, expect_half=None):
    """fp32 and, where the kernels read 2-byte rows, bf16 and fp16 against the reference on their exact fp32 up-cast."""
    half = _half_native(graphs, x.shape[2])
    if expect_half is not None:
        assert half == expect_half
    ref, _ = _device_equals_reference(x, lengths, graphs)
    if half:
        for dtype in HALF:
            _device_equals_reference(x.to(dtype), lengths, graphs)
    return ref


# the D of the form matrix where align_kernel reads 2-byte rows (D % 4 == 0 within the register-staged float4 forms)
HALF_NATIVE_D = {4: True, 48: True, 2048: True, 2052: True, 4096: True, 4100: True, 8408: True, 16384: True, 16388: False,
                 1001: False, 4095: False, 4097: False, "tile_last": False, "general_first": False}


@pytest.mark.parametrize("D", list(nc.FORM_D) + ["tile_last", "general_first"])
def test_form_matrix(D):
    expect_half = HALF_NATIVE_D[D]
    if isinstance(D, str):
        pair = nc.form_boundary_D()
        D = pair[("tile_last", "general_first").index(D)]
    x, lengths, graphs = nc.form_case(D)
    ref = _all_dtypes(x, lengths, graphs, expect_half)
    assert bool(np.isfinite(ref[0]).all())
    xn, _, _ = nc.form_case(D, nan=True)
    refn = _all_dtypes(xn, lengths, graphs, expect_half)
    assert np.isnan(refn[0][1]) and bool(np.isfinite(refn[0][[0, 2]]).all())


def test_form_boundary_pair_straddles_the_tile_kernels():
    d_in, d_out = nc.form_boundary_D()
    gb = nc.form_graphs(4)
    H, K = gb.num_states, int(gb.backward_transitions.shape[-2])
    assert d_out == d_in + 1 and nc.on_tile_path(H, K, d_in) and not nc.on_tile_path(H, K, d_out)


@pytest.mark.parametrize("H,B,D", nc.SWEEPS)
def test_backtrace_sweep(H, B, D):
    x, lengths, graphs = nc.sweep_case(H, B, D)
    assert nc.on_tile_path(H, graphs.shared_graph.num_transitions, D)
    ref = _all_dtypes(x, lengths, graphs, D % 4 == 0)
    assert bool(np.isfinite(ref[0]).all())


def test_single_frame():
    x, lengths, graphs = nc.single_frame_case()
    ref = _all_dtypes(x, lengths, graphs, True)
    assert np.isfinite(ref[0][0])


def test_largest_tile_graph_and_first_general():
    h_in, h_out = nc.tile_boundary_H()
    assert h_out == h_in + 1
    h_odd = next(H for H in range(h_in, 4000, -1) if nc.tile_family_K(H) % 2)   # (an odd K: 8 K is 8 mod 16, align_walk_bytes)
    for H, tile in ((h_in, True), (h_out, False), (h_odd, True)):
        x, lengths, graphs = nc.largest_tile_case(H)
        assert nc.on_tile_path(H, graphs.shared_graph.num_transitions, 48) == tile
        ref = _all_dtypes(x, lengths, graphs, tile)
        assert bool(np.isfinite(ref[0]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_ties(dtype):
    x, lengths, graphs = nc.ties_case()
    xh = x.to(dtype)
    assert torch.equal(xh.float(), x) and _half_native(graphs, x.shape[2])
    ref, dev = _device_equals_reference(xh, lengths, graphs)
    L = lengths.numpy()
    assert np.array_equal(ref[3], L) and bool((ref[4] == 1).all())  # (ties at every frame and at the end)
    host = viterbi_align(x, lengths, graphs)                           # the tie case is also equal to the host twin
    assert torch.equal(dev.score.cpu().view(torch.int64), host.score.view(torch.int64))
    assert torch.equal(dev.states.cpu(), host.states) and torch.equal(dev.pdfs.cpu(), host.pdfs)
    for b in range(3):
        assert int(dev.states[b, L[b]]) == nc.TIE_STARTS[0] + nc.TIE_CHAIN - 1
