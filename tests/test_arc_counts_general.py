"""The general arc-count kernels (include/pychain_hip.h: pychain_hip_den_arc_counts_general and its three queries)
without a GPU: ABI 31 and the new symbols; which form a shape runs under PYCHAIN_HIP_SMBR_AUTO, the edges LDS / ROWS and ROWS /
GLOBAL taken from the two LDS queries, the refusals of LDS and ROWS asked for by name on a shape they cannot hold; the workspace
query; the entry point's refusal before the device is touched; the `kernels` keyword on CPU tensors - checked, and every valid
value the bits of the default call (there is one host twin).  The kernels themselves: tests/test_gpu_arc_counts_general.py."""
import os
import re

import pytest
import torch

import arc_counts_general_cases as gc
import arc_counts_reference as ar
from arc_counts_general_cases import AUTO, GLOBAL, LDS, ROWS
from pychain_amd import _lib, den_log_partition, expected_arc_counts, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024
NEW = ("pychain_hip_den_arc_counts_form", "pychain_hip_den_arc_counts_general_lds_bytes",
       "pychain_hip_den_arc_counts_general_workspace_bytes", "pychain_hip_den_arc_counts_general")


def _last_error():
    return _lib.lib().pychain_hip_last_error().decode()


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 31
    for name in NEW:
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS


@pytest.mark.parametrize("H,D,form", [(3000, 3456, LDS), (3000, 8408, LDS)] +
                         [(c["H"], c["D"], c["form"]) for c in gc.SHAPES.values()])
def test_the_form_a_shape_runs(H, D, form):
    L = _lib.lib()
    assert L.pychain_hip_den_arc_counts_form(H, D, AUTO) == form
    # AUTO is the LDS form exactly where the LDS query is within a CU, and a form asked for by name that fits is that form
    assert (form == LDS) == (L.pychain_hip_den_arc_counts_lds_bytes(H, D) <= BUDGET)
    assert L.pychain_hip_den_arc_counts_form(H, D, GLOBAL) == GLOBAL
    if form != GLOBAL:
        assert L.pychain_hip_den_arc_counts_form(H, D, ROWS) == ROWS
    if form == LDS:
        assert L.pychain_hip_den_arc_counts_form(H, D, LDS) == LDS


def test_the_edge_between_lds_and_rows():
    L = _lib.lib()
    q = L.pychain_hip_den_arc_counts_lds_bytes
    D = max(d for d in range(16384, 24576) if q(37, d) <= BUDGET)              # found from the query, not written in
    assert q(37, D) <= BUDGET < q(37, D + 1)
    assert D + 1 == gc.SHAPES["pdfs_beyond"]["D"]                              # the shape is the first beyond
    assert L.pychain_hip_den_arc_counts_form(37, D, AUTO) == LDS and L.pychain_hip_den_arc_counts_form(37, D + 1, AUTO) == ROWS
    assert L.pychain_hip_den_arc_counts_form(37, D, LDS) == LDS and L.pychain_hip_den_arc_counts_form(37, D + 1, LDS) == -2
    for H in (1, 37, 3000, 20000):                                             # AUTO is LDS exactly where the LDS query is within
        for d in (1, 130, 416, 417, 17416, 17417, 20379, 20380, 40000):
            assert (L.pychain_hip_den_arc_counts_form(H, d, AUTO) == LDS) == (q(H, d) <= BUDGET)


def test_the_edge_between_rows_and_global():
    L = _lib.lib()
    q = L.pychain_hip_den_arc_counts_general_lds_bytes
    assert q(0) == 0 and q(-3) == 0
    H = max(h for h in range(16384, 32768) if q(h) <= BUDGET)
    assert q(H) <= BUDGET < q(H + 1) and q(H + 1) - q(H) == 8                  # one double-buffered state vector
    assert q(37) == (2 * 37 + 64) * 4 + 256
    for D in (130, 8408, 40000):                                               # (beyond the LDS form at any of them)
        assert L.pychain_hip_den_arc_counts_form(H, D, AUTO) == ROWS and L.pychain_hip_den_arc_counts_form(H + 1, D, AUTO) == GLOBAL
    assert L.pychain_hip_den_arc_counts_form(H, 130, ROWS) == ROWS and L.pychain_hip_den_arc_counts_form(H + 1, 130, ROWS) == -2
    # the rows form needs less than the LDS form at every shape
    assert all(q(h) < L.pychain_hip_den_arc_counts_lds_bytes(h, d) for h, d in ((37, 23), (3000, 3456), (H, 1), (1, 1)))


def test_refusals_of_a_form_asked_for_by_name():
    L = _lib.lib()
    c = gc.SHAPES["pdfs_beyond"]
    assert L.pychain_hip_den_arc_counts_form(c["H"], c["D"], LDS) == -2
    msg = _last_error()
    need = L.pychain_hip_den_arc_counts_lds_bytes(c["H"], c["D"])
    assert "37 states" in msg and "20380 pdfs" in msg and str(need) in msg and str(BUDGET) in msg and need > BUDGET
    c = gc.SHAPES["states_beyond"]
    assert L.pychain_hip_den_arc_counts_form(c["H"], c["D"], ROWS) == -2
    msg = _last_error()
    assert "20500 states" in msg and str(L.pychain_hip_den_arc_counts_general_lds_bytes(c["H"])) in msg and str(BUDGET) in msg
    assert L.pychain_hip_den_arc_counts_form(c["H"], c["D"], LDS) == -2
    for requested in (-1, 4, 17):
        assert L.pychain_hip_den_arc_counts_form(37, 23, requested) == -1 and "form" in _last_error()
    for H, D in ((0, 23), (37, 0), (-1, 23), (37, -5)):
        assert L.pychain_hip_den_arc_counts_form(H, D, AUTO) == -1 and "form" in _last_error()


def test_the_workspace_query():
    L = _lib.lib()
    q, old = L.pychain_hip_den_arc_counts_general_workspace_bytes, L.pychain_hip_den_arc_counts_workspace_bytes
    for args in ((0, 5, 7, 9, 11), (2, 0, 7, 9, 11), (2, 5, 0, 9, 11), (2, 5, 7, 0, 11), (2, 5, 7, 9, 0), (2, 5, 7, 9, -1)):
        assert q(*args) == 0
    shapes = [(c["B"], c["T"], c["H"], c["K"], c["D"]) for c in gc.SHAPES.values()]
    for B, T, H, K, D in shapes + [(64, 1500, 3000, 30000, 3456), (32, 2000, 3000, 30000, 8408)]:
        w = q(B, T, H, K, D)
        items = B * ((T + 63) // 64)
        row = (2 * D + 63) // 64 * 64                                          # floats of a scratch row
        rows = (2 * B + min(items, gc.COUNT_WGS)) * row                        # the recursions', the counts'
        assert w >= old(B, T, H, K) + 4 * rows
        assert w - old(B, T, H, K) <= 4 * rows + 256 * 2                       # ... and each region's rounding to 256 bytes, no more
        assert q(B, T, H, K, D + 64) > w                                       # (it grows with D)
    c = gc.SHAPES["many_items"]
    assert c["B"] * ((c["T"] + 63) // 64) > gc.COUNT_WGS                       # the shape that makes a workgroup take a second item


def test_the_entry_point_refuses_before_the_device_is_touched():
    L = _lib.lib()
    nulls = [None] * 11 + [37, 150, None, None, 0, None, 2, 3, 23, 0.1, None, 1.0, None, None, None, None, None, None, None, 0, None]
    assert L.pychain_hip_den_arc_counts_general(*nulls, AUTO) == -1
    assert "den_arc_counts_general" in _last_error() and "null pointer" in _last_error()
    for form in (9, -1, 4):
        assert L.pychain_hip_den_arc_counts_general(*nulls, form) == -1
        assert "den_arc_counts_general" in _last_error() and "form" in _last_error()


def test_kernels_is_checked():
    g, y, lengths = ar.case("small")
    w = ar.weights("small", "normal")
    for bad in ("nonsense", "LDS", "", None, 2):
        with pytest.raises(ValueError, match="kernels"):
            expected_arc_counts(y, lengths, g, kernels=bad)
        with pytest.raises(ValueError, match="kernels"):
            den_log_partition(y, lengths, g, w, kernels=bad)
    with pytest.raises(ValueError, match="den_arc_counts: the kernels must be one of 'lds', 'auto', 'rows', 'global'"):
        native.smbr_form_code("nonsense", who="den_arc_counts")
    with pytest.raises(TypeError):                                              # a keyword
        expected_arc_counts(y, lengths, g, 1e-5, None, None, False, "auto")
    with pytest.raises(TypeError):
        den_log_partition(y, lengths, g, w, 1e-5, None, "auto")


def test_on_cpu_tensors_every_form_is_the_host_twin():
    g, y, lengths = ar.case("small")
    w0 = ar.weights("small", "normal")
    u = torch.tensor([1.0, 0.5, 2.0, 0.25])

    def call(**kw):
        res = expected_arc_counts(y, lengths, g, 0.1, arc_log_weights=w0, utt_weights=u, per_seq=True, **kw)
        x = y.clone().requires_grad_(True)
        w = w0.clone().requires_grad_(True)
        out = den_log_partition(x, lengths, g, w, 0.1, utt_weights=u, **kw)
        (3.0 * out).backward()
        return res.counts, res.counts_per_seq, res.objf_per_seq, res.bad_count, x.grad, w.grad, out.detach(), out.per_seq

    calls = _lib.lib().pychain_hip_cpu_calls()
    want = call()
    per_call = _lib.lib().pychain_hip_cpu_calls() - calls
    assert per_call > 0 and float(want[4].abs().max()) > 0 and float(want[5].abs().max()) > 0
    for kernels in ("lds", "auto", "rows", "global"):
        calls = _lib.lib().pychain_hip_cpu_calls()
        got = call(kernels=kernels)
        assert _lib.lib().pychain_hip_cpu_calls() - calls == per_call          # the same host twin
        assert all(torch.equal(p, q) for p, q in zip(got, want))
