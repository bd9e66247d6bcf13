"""Expected arc counts of the numerator on CPU tensors (include/pychain_hip.h: pychain_hip_cpu_num_arc_counts, the host twin;
DESIGN.md §3.31) against the float64 references of tests/num_arcs_reference.py, over the builders of tests/num_cases.py; the
references against each other and against their planted faults; the identities, autograd, and the surface of the ABI.  The
checks themselves are tests/num_arcs_checks.py, shared with tests/test_gpu_num_arcs.py.  Bound: num_arcs_checks.BOUND = 1e-5."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import arc_counts_reference as ar
import num_arcs_checks as ck
import num_arcs_reference as nr
from pychain_amd import ChainGraphBatch, _lib, expected_num_arc_counts, native, num_log_partition

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = "cpu"


# ---- the references ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["form4", "formtw4", "ties"])
def test_references_agree(name):
    """numpy logaddexp recursions and torch float64 autograd of the same objective: counts, gradient and log P to 1e-12"""
    x, lengths, graphs, windows = ck.case(name)
    w = ck.weights(name, "normal")
    logp, counts, grad, feas = nr.np_num_arc_counts(graphs, x, lengths, w, windows)
    tlp, tgw, tgx = nr.torch_num_arc_counts(graphs, x, lengths, w, windows)
    assert np.array_equal(np.isfinite(tlp), feas) and feas.sum() >= 2
    d = (nr.counts_distance(tgw, counts), nr.counts_distance(tgx, grad), float((np.abs(tlp[feas] - logp[feas]) / np.abs(logp[feas])).max()))
    print("%s: numpy against torch autograd: counts %.3e gradient %.3e log P %.3e" % ((name,) + d))
    assert max(d) <= 1e-12


@pytest.mark.parametrize("fault", nr.FAULTS)
@pytest.mark.parametrize("name", ["form4", "ties"])
def test_planted_faults_show(name, fault):
    """each planted fault moves the reference's counts by more than a hundred bounds"""
    x, lengths, graphs, windows = ck.case(name)
    w = ck.weights(name, "normal")
    good = ck.reference(name, "normal")[1]
    d = nr.counts_distance(nr.np_num_arc_counts(graphs, x, lengths, w, windows, fault=fault)[1], good)
    print("%s %s: %.3e" % (name, fault, d))
    assert d > 100 * ck.BOUND


# ---- the host twin against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", [None, "normal"])
@pytest.mark.parametrize("D", ck.FORM_D)
def test_form_matrix(D, wkind):
    calls = _lib.lib().pychain_hip_cpu_calls()
    ck.check_case("form%d" % D, wkind, CPU)
    assert _lib.lib().pychain_hip_cpu_calls() == calls + 1


@pytest.mark.parametrize("wkind", [None, "normal"])
@pytest.mark.parametrize("name", ["shared701", "shared701_tw"])
def test_more_than_512_states_and_windows(name, wkind):
    r = ck.check_case(name, wkind, CPU)
    if name == "shared701_tw":
        assert r[0][2] == -float("inf") and not r[1][2].any() and int(r[3][0]) >= 1


def test_full_windows_give_the_bits_of_no_windows():
    a, b = ck.run_with_full_windows(CPU)
    assert ck.same_bits(a[0], b[0]) and ck.same_bits(a[1], b[1]) and ck.same_bits(a[2], b[2])


def test_parallel_arcs_with_different_weights():
    """ties_case: the two arcs of every pair differ in nothing but their pdf; with different weights their counts differ, and the
    backward copies found the right ones"""
    r = ck.check_case("ties", "normal", CPU)
    c = r[1].numpy()
    assert np.abs(c[:, 0] - c[:, 1]).max() > 1e-3


@pytest.mark.parametrize("name", ["tile_last", "tile_first"])
def test_both_sides_of_the_tile_boundary(name):
    ck.check_case(name, "normal", CPU)


@pytest.mark.parametrize("name,wkind", [("form4", None), ("form4", "normal"), ("shared701_tw", None), ("shared701_tw", "normal")])
def test_counts_by_pdf_are_the_summed_gradient(name, wkind):
    ck.check_by_pdf(name, wkind, CPU)


@pytest.mark.parametrize("name", ["form4", "shared701_tw", "ties"])
def test_identities(name):
    ck.check_identities(name, CPU)


@pytest.mark.parametrize("name", ["form4", "shared701"])
def test_weights_that_are_not_finite(name):
    ck.check_bad_weights(name, CPU)


# ---- autograd ------------------------------------------------------------------------------------------------------------------------
def test_autograd_against_fp64():
    ck.check_autograd("form4", CPU)


def test_autograd_under_windows_with_a_zero_weight_on_the_infeasible_sequence():
    ck.check_autograd("formtw4", CPU, utt=[1.0, 0.0, 0.5])


def test_weights_of_any_strides():
    x, lengths, graphs, _ = ck.case("form4")
    w0 = ck.weights("form4", "normal")
    want = num_log_partition(x, lengths, graphs, w0.clone().requires_grad_(True))
    base = w0.t().contiguous().requires_grad_(True)                         # [K,B] storage, read as its transpose
    got = num_log_partition(x, lengths, graphs, base.t())
    assert float(got.detach()) == float(want.detach())
    got.backward()
    row = w0[:1].clone().requires_grad_(True)                               # one row of weights expanded over the batch
    out = num_log_partition(x, lengths, graphs, row.expand(3, -1))
    out.backward()
    c = expected_num_arc_counts(x, lengths, graphs, arc_log_weights=row.detach().expand(3, -1)).counts_per_seq
    assert torch.equal(base.grad, expected_num_arc_counts(x, lengths, graphs, arc_log_weights=w0).counts_per_seq.float().t())
    assert row.grad.shape == (1, c.shape[1]) and torch.allclose(row.grad.double(), c.sum(0, keepdim=True), rtol=1e-6, atol=1e-9)
    half = w0.to(torch.float64).requires_grad_(True)
    num_log_partition(x, lengths, graphs, half).backward()
    assert half.grad.dtype == torch.float64


@pytest.mark.parametrize("name", ["degenerate", "small"])
def test_tied_scalar_in_both_graphs(name):
    ck.check_tied_scalar(name, CPU)


# ---- the surface -----------------------------------------------------------------------------------------------------------------------
NEW = ("pychain_hip_num_arc_counts_workspace_bytes", "pychain_hip_num_arc_counts", "pychain_hip_cpu_num_arc_counts")


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 32
    for name in NEW:
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    import pychain
    import pychain_amd
    assert pychain.expected_num_arc_counts is expected_num_arc_counts is pychain_amd.expected_num_arc_counts
    assert pychain.num_log_partition is num_log_partition and pychain.NumArcCounts is pychain_amd.NumArcCounts
    from pychain_amd import build_ext
    assert "num_arcs.hip" in build_ext.SOURCES


def test_workspace_query():
    L = _lib.lib()
    q = L.pychain_hip_num_arc_counts_workspace_bytes
    assert q(0, 1, 1, 1, 1) == 0 and q(1, 1, 1, 1, 0) == 0
    sizes = [q(3, T, 40, 90, 48) for T in (1, 63, 64, 65, 500, 1500)]
    assert sizes[0] > L.pychain_hip_num_workspace_bytes(3, 1, 40, 90, 48) > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    # the partial rows: B ceil(T / 64) rows of K doubles
    assert q(64, 1500, 400, 800, 3000) - L.pychain_hip_num_workspace_bytes(64, 1500, 400, 800, 3000) >= 64 * 24 * 800 * 8


def _raw_call(grad_mode):
    x, lengths, graphs, _ = ck.case("form4")
    ts, stride = native._cpu_graph(graphs, False)
    B, T, D = x.shape
    H, K = int(ts[1].shape[-2]), int(ts[0].shape[-2])
    objf, counts, bad = torch.zeros(B, dtype=torch.float64), torch.zeros(B, K, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    lc = lengths.to(torch.int64)
    L = _lib.lib()
    dev = L.pychain_hip_num_arc_counts(*[t.data_ptr() for t in ts], stride, x.data_ptr(), 0, lc.data_ptr(), B, T, D, H, K, grad_mode, 1.0,
                                       None, objf.data_ptr(), None, counts.data_ptr(), bad.data_ptr(), objf.data_ptr(), 1, None, None)
    dmsg = L.pychain_hip_last_error().decode()
    host = L.pychain_hip_cpu_num_arc_counts(*[t.data_ptr() for t in ts], stride, x.data_ptr(), lc.data_ptr(), B, T, D, H, K, grad_mode, 1.0,
                                            None, objf.data_ptr(), None, counts.data_ptr(), bad.data_ptr(), 1, None)
    return dev, dmsg, host, L.pychain_hip_last_error().decode()


def test_refusals():
    """made before the device is touched: host pointers never reach a kernel"""
    dev, dmsg, host, hmsg = _raw_call(_lib.GRAD_LOG)
    assert dev == -1 and "PYCHAIN_HIP_GRAD_LINEAR" in dmsg and host == -1 and "grad_mode" in hmsg
    with _lib.option("num_compat", 1):
        dev, dmsg, _, _ = _raw_call(_lib.GRAD_LINEAR)
    assert dev == -2 and "num_compat" in dmsg and "arc weights" in dmsg
    x, lengths, graphs, _ = ck.case("form4")
    K = nr.padded_K(graphs)
    for w in (torch.zeros(3, K + 1), torch.zeros(K), torch.zeros(2, K)):
        with pytest.raises(ValueError, match="one entry per sequence and arc"):
            expected_num_arc_counts(x, lengths, graphs, arc_log_weights=w)
    with pytest.raises(ValueError, match="float tensor"):
        expected_num_arc_counts(x, lengths, graphs, arc_log_weights=torch.zeros(3, K, dtype=torch.int64))
    with pytest.raises(ValueError, match="float tensor"):
        num_log_partition(x, lengths, graphs, [[0.0] * K] * 3)
    den = ar.case("small")
    with pytest.raises(ValueError, match="log-domain"):
        expected_num_arc_counts(den[1], den[2], ChainGraphBatch(den[0], 4))
    with pytest.raises(ValueError, match="log-domain"):
        num_log_partition(den[1], den[2], ChainGraphBatch(den[0], 4), None)


def test_not_differentiable_and_honours_the_batch_windows():
    x, lengths, graphs, windows = ck.case("formtw4")
    r0 = expected_num_arc_counts(x.clone().requires_grad_(True), lengths, graphs)
    assert not r0.counts_per_seq.requires_grad and bool(torch.isfinite(r0.objf_per_seq).all())
    graphs.set_time_windows(windows)
    try:
        r1 = expected_num_arc_counts(x, lengths, graphs)
    finally:
        graphs.set_time_windows(None)
    want = ck.run(x, lengths, graphs, None, windows, with_grad=False)
    assert ck.same_bits(r1.counts_per_seq, want[1]) and ck.same_bits(r1.objf_per_seq, want[0]) and r1.objf_per_seq[1] == -float("inf")
    assert r1.bad_count.dtype == torch.int32 and r1.bad_count.tolist() == [1, 0]


def test_header_compiles_as_c(tmp_path):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("gcc") or shutil.which("cc") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cc is not None, "no C compiler: neither gcc nor cc on PATH, nor %s" % rocm_clang
    graph = "const int32_t*, const int32_t*, const float*, const int32_t*, const int32_t*, const float*, const float*, const float*, int,\n    "
    tail = "int, int, int, int, int, int, float, const float*, double*, float*, double*, int32_t*, "
    src = tmp_path / "h.c"
    src.write_text('#include "pychain_hip.h"\n'
                   'static size_t (*ws)(int, int, int, int, int) = pychain_hip_num_arc_counts_workspace_bytes;\n'
                   'static int (*dev)(' + graph + 'const void*, int, const int64_t*, ' + tail +
                   'void*, size_t, void*, const int32_t*) = pychain_hip_num_arc_counts;\n'
                   'static int (*host)(' + graph + 'const float*, const int64_t*, ' + tail +
                   'int, const int32_t*) = pychain_hip_cpu_num_arc_counts;\n'
                   'int main(void) { return ws == 0 || dev == 0 || host == 0 || PYCHAIN_HIP_ABI_VERSION < 32; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True, text=True)
