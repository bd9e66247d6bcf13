"""Expected arc counts of the numerator on the MI355X (include/pychain_hip.h: pychain_hip_num_arc_counts; csrc/num_arcs.hip;
DESIGN.md §3.31) against the float64 references of tests/num_arcs_reference.py, over the builders of tests/num_cases.py: one row
width per launch form of the recursions, 2-byte rows, more than 512 states with and without windows (two count runs, one of
exactly 64 frames), parallel arcs, both sides of the tile boundary (the tile and the general recursions), the LDS-staged against
the gathered form of the count kernel, the identities, autograd.  The checks are tests/num_arcs_checks.py, shared with
tests/test_num_arcs.py.  Bound: num_arcs_checks.BOUND = 1e-5."""
import numpy as np
import pytest
import torch

import num_arcs_checks as ck
import num_arcs_reference as nr
import num_cases as nc
from pychain_amd import _lib, expected_num_arc_counts

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wkind", [None, "normal"])
@pytest.mark.parametrize("D", ck.FORM_D)
def test_form_matrix(D, wkind):
    calls = _lib.lib().pychain_hip_cpu_calls()
    r = ck.check_case("form%d" % D, wkind, DEV)
    assert _lib.lib().pychain_hip_cpu_calls() == calls                          # the kernels, not the host twin
    assert r[1].is_cuda and r[3].tolist() == [0, 0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_two_byte_rows(dtype):
    """D = 2048: the counts equal the fp32 call on the up-cast input bit for bit where the rows are up-cast ahead of the ABI
    (pychain_hip_num_half_native 0), and lie within the bound of it where the recursions read the 2-byte rows themselves"""
    x, lengths, graphs = nc.form_case(2048)
    K = nr.padded_K(graphs)
    w = torch.from_numpy((0.5 * np.random.RandomState(77).randn(3, K)).astype(np.float32))
    xh = x.to(dtype)
    rh = ck.run(xh, lengths, graphs, w, device=DEV)
    rf = ck.run(xh.float(), lengths, graphs, w, device=DEV)
    native_rows = _lib.lib().pychain_hip_num_half_native(graphs.num_states, K, 2048)
    d = nr.counts_distance(rh[1].cpu().numpy(), rf[1].cpu().numpy())
    print("%s rows (native %d): counts against the fp32 call on the up-cast input %.3e" % (dtype, native_rows, d))
    if native_rows == 0:
        assert ck.same_bits(rh[1], rf[1]) and ck.same_bits(rh[0], rf[0])
    assert d <= ck.BOUND
    ck.check(rh, nr.np_num_arc_counts(graphs, xh.float(), lengths, w), lengths, graphs, "cuda_form2048_%s" % str(dtype)[6:])


@pytest.mark.parametrize("wkind", [None, "normal"])
@pytest.mark.parametrize("name", ["shared701", "shared701_tw"])
def test_more_than_512_states_and_windows(name, wkind):
    r = ck.check_case(name, wkind, DEV)
    if name == "shared701_tw":
        fb_bad = ck.run_fb(*ck.case(name)[:3], ck.case(name)[3], DEV)[2]
        assert r[0][2] == -float("inf") and not r[1][2].any() and int(r[3][0]) == int(fb_bad[0]) >= 1


def test_full_windows_give_the_bits_of_no_windows():
    a, b = ck.run_with_full_windows(DEV)
    assert ck.same_bits(a[0], b[0]) and ck.same_bits(a[1], b[1]) and ck.same_bits(a[2], b[2])


def test_an_infeasible_sequence_leaves_the_others_bits():
    """shared701 under its windows: the feasible sequences' counts are those of a batch without the infeasible one"""
    x, lengths, graphs, windows = ck.case("shared701_tw")
    w = ck.weights("shared701_tw", "normal")
    whole = ck.run(x, lengths, graphs, w, windows, device=DEV)
    keep = [0, 1, 3]
    from pychain_amd import ChainGraphBatch
    part = ck.run(x[keep], lengths[keep], ChainGraphBatch(graphs.shared_graph, 3), w[keep], windows[keep], device=DEV)
    assert ck.same_bits(whole[1][keep], part[1]) and ck.same_bits(whole[0][keep], part[0])


def test_parallel_arcs_with_different_weights():
    r = ck.check_case("ties", "normal", DEV)
    c = r[1].cpu().numpy()
    assert np.abs(c[:, 0] - c[:, 1]).max() > 1e-3


@pytest.mark.parametrize("name", ["tile_last", "tile_first"])
def test_both_sides_of_the_tile_boundary(name):
    """the last graph on the tile recursions, the first on the general ones"""
    x, _, graphs, _ = ck.case(name)
    assert nc.on_tile_path(graphs.num_states, nr.padded_K(graphs), x.shape[2]) == (name == "tile_last")
    ck.check_case(name, "normal", DEV)


@pytest.mark.parametrize("name", ["form4", "shared701_tw", "ties", "tile_first"])
def test_staged_and_gathered_count_kernels_give_the_same_bits(name):
    """option num_arcs_gather forces the gathered form where the LDS-staged one runs by default: K beyond the 1024 arcs a staged
    workgroup sums in registers (shared701, ties, tile_first), H beyond one stride of its threads, windows with -inf states"""
    staged = ck.run_case(name, "normal", DEV)
    with _lib.option("num_arcs_gather", 1):
        gathered = ck.run_case(name, "normal", DEV)
    assert ck.same_bits(staged[1], gathered[1]) and ck.same_bits(staged[0], gathered[0]) and ck.same_bits(staged[2], gathered[2])
    assert staged[3].tolist() == gathered[3].tolist()
    x, lengths, graphs, _ = ck.case(name)
    ck.check(gathered, ck.reference(name, "normal"), lengths, graphs, "cuda_gathered_%s" % name)


@pytest.mark.parametrize("name,wkind", [("form4", None), ("form4", "normal"), ("shared701_tw", None), ("shared701_tw", "normal")])
def test_counts_by_pdf_are_the_summed_gradient(name, wkind):
    ck.check_by_pdf(name, wkind, DEV)


@pytest.mark.parametrize("name", ["form4", "form2052", "shared701_tw", "ties", "tile_first"])
def test_identities(name):
    ck.check_identities(name, DEV)


@pytest.mark.parametrize("name", ["form4", "shared701"])
def test_weights_that_are_not_finite(name):
    ck.check_bad_weights(name, DEV)


def test_host_twin_against_device():
    for name in ("form4", "shared701_tw"):
        d, h = ck.run_case(name, "normal", DEV), ck.run_case(name, "normal", "cpu")
        feas = np.isfinite(h[0].numpy())
        dc = nr.counts_distance(d[1].cpu().numpy()[feas], h[1].numpy()[feas])
        print("%s: device against the host twin: counts %.3e" % (name, dc))
        assert np.array_equal(np.isfinite(d[0].cpu().numpy()), feas) and dc <= ck.BOUND


def test_autograd_against_fp64():
    ck.check_autograd("form4", DEV)


def test_autograd_under_windows_with_a_zero_weight_on_the_infeasible_sequence():
    ck.check_autograd("formtw4", DEV, utt=[1.0, 0.0, 0.5])


@pytest.mark.parametrize("name", ["degenerate", "small"])
def test_tied_scalar_in_both_graphs(name):
    ck.check_tied_scalar(name, DEV)


def test_public_call_on_the_device():
    x, lengths, graphs, _ = ck.case("form4")
    w = ck.weights("form4", "normal")
    r = expected_num_arc_counts(x.to(DEV), lengths, graphs, arc_log_weights=w.to(DEV).to(torch.float64))
    want = ck.run(x, lengths, graphs, w, with_grad=False, device=DEV)
    assert r.counts_per_seq.is_cuda and ck.same_bits(r.counts_per_seq, want[1]) and ck.same_bits(r.objf_per_seq, want[0])
    assert r.bad_count.tolist() == [0, 0]
