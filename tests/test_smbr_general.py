"""The general sMBR kernels (include/pychain_hip.h: pychain_hip_smbr_forward_backward_general and its three queries; DESIGN.md
§3.28) without a GPU: ABI 29 and the new symbols; which form a shape runs under PYCHAIN_HIP_SMBR_AUTO, the edge between ROWS and
GLOBAL taken from the LDS query, the refusals of LDS and ROWS asked for by name on a shape they cannot hold; the workspace query;
the entry point's refusal before the device is touched; the `kernels` keyword on CPU tensors - checked, and every valid value the
bits of the default call (there is one host twin).  The kernels themselves: tests/test_gpu_smbr_general.py."""
import os
import re

import pytest
import torch

import smbr_class_reference as cr
import smbr_reference as sr
from pychain_amd import PosteriorTargets, SMBRLoss, _lib, expected_accuracy, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, LDS, ROWS, GLOBAL = 0, 1, 2, 3
BUDGET = 160 * 1024
NEW = ("pychain_hip_smbr_form", "pychain_hip_smbr_general_lds_bytes", "pychain_hip_smbr_general_workspace_bytes",
       "pychain_hip_smbr_forward_backward_general")


def _last_error():
    return _lib.lib().pychain_hip_last_error().decode()


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 29
    for name in NEW:
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    for name, value in (("AUTO", AUTO), ("LDS", LDS), ("ROWS", ROWS), ("GLOBAL", GLOBAL)):
        assert int(re.search(r"#define PYCHAIN_HIP_SMBR_%s\s+(\d+)" % name, header).group(1)) == value == getattr(_lib, "SMBR_" + name)


@pytest.mark.parametrize("H,D,C,form", [(3000, 3456, 0, LDS), (37, 10160, 0, LDS), (37, 10180, 0, ROWS), (3000, 8408, 0, ROWS),
                                        (3000, 8408, 8408, ROWS), (12000, 130, 0, GLOBAL), (11000, 8408, 0, GLOBAL)])
def test_the_form_a_shape_runs(H, D, C, form):
    L = _lib.lib()
    assert L.pychain_hip_smbr_form(H, D, C, AUTO) == form
    # AUTO is the LDS form exactly where the LDS query is within a CU, and a form asked for by name that fits is that form
    assert (form == LDS) == (L.pychain_hip_smbr_lds_bytes(H, D, C) <= BUDGET)
    assert L.pychain_hip_smbr_form(H, D, C, GLOBAL) == GLOBAL
    if form != GLOBAL:
        assert L.pychain_hip_smbr_form(H, D, C, ROWS) == ROWS
    if form == LDS:
        assert L.pychain_hip_smbr_form(H, D, C, LDS) == LDS


def test_the_edge_between_rows_and_global():
    L = _lib.lib()
    q = L.pychain_hip_smbr_general_lds_bytes
    assert q(0) == 0 and q(-3) == 0
    H = max(h for h in range(8192, 16384) if q(h) <= BUDGET)
    assert q(H) <= BUDGET < q(H + 1) and q(H + 1) - q(H) == 16            # four state vectors
    for D, C in ((130, 0), (20000, 0), (20000, 20000)):                     # (beyond the LDS form at any of them)
        assert L.pychain_hip_smbr_form(H, D, C, AUTO) == ROWS and L.pychain_hip_smbr_form(H + 1, D, C, AUTO) == GLOBAL
    assert L.pychain_hip_smbr_form(H, 130, 0, ROWS) == ROWS and L.pychain_hip_smbr_form(H + 1, 130, 0, ROWS) == -2
    # a graph that small runs the LDS form with few pdfs: the rows form needs less than the LDS form at every shape
    assert all(q(h) < L.pychain_hip_smbr_lds_bytes(h, d, 0) for h, d in ((37, 23), (3000, 3456), (H, 1)))


def test_refusals_of_a_form_asked_for_by_name():
    L = _lib.lib()
    assert L.pychain_hip_smbr_form(37, 10180, 0, LDS) == -2
    msg = _last_error()
    assert "37 states" in msg and "10180 pdfs" in msg and str(L.pychain_hip_smbr_lds_bytes(37, 10180, 0)) in msg and str(BUDGET) in msg
    assert L.pychain_hip_smbr_form(37, 10000, 700, LDS) == -2               # (the class table counts)
    assert "700 classes" in _last_error() and L.pychain_hip_smbr_form(37, 10000, 0, LDS) == LDS
    assert L.pychain_hip_smbr_form(12000, 130, 0, ROWS) == -2
    msg = _last_error()
    assert "12000 states" in msg and str(L.pychain_hip_smbr_general_lds_bytes(12000)) in msg and str(BUDGET) in msg
    for requested in (-1, 4, 17):
        assert L.pychain_hip_smbr_form(37, 23, 0, requested) == -1 and "form" in _last_error()
    for H, D, C in ((0, 23, 0), (37, 0, 0), (37, 23, -1)):
        assert L.pychain_hip_smbr_form(H, D, C, AUTO) == -1


def test_the_workspace_query():
    L = _lib.lib()
    q, old = L.pychain_hip_smbr_general_workspace_bytes, L.pychain_hip_smbr_workspace_bytes
    for args in ((0, 5, 7, 9, 0), (2, 0, 7, 9, 0), (2, 5, 0, 9, 0), (2, 5, 7, 0, 0), (2, 5, 7, 9, -1)):
        assert q(*args) == 0
    for B, T, H, D, C in ((2, 3, 37, 10180, 0), (2, 6, 3000, 8408, 0), (2, 6, 3000, 8408, 8408), (1, 3, 11000, 8408, 0),
                          (64, 1500, 3000, 3456, 40), (32, 2000, 3000, 8408, 0)):
        w = q(B, T, H, D, C)
        items = B * ((T + 7) // 8)
        rows = 2 * B * (4 * D + C) + min(items, 512) * (2 * D + C)         # floats of scratch: the recursions', the gradient's
        assert w >= old(B, T, H) + 4 * rows
        assert w - old(B, T, H) <= 4 * rows + 256 * (2 * B + 512 + 2)      # ... and the rounding to 256 bytes, no more
        assert q(B, T, H, D, C + 64) > w                                   # (a class is a float in every set of rows)


def test_the_entry_point_refuses_before_the_device_is_touched():
    L = _lib.lib()
    nulls = [None] * 11 + [37, 150, None, 0, None, 4, 17, 23, None, None, 2, None, 0.1, 1.0, None, None, None, None, None, None, 0, None]
    assert L.pychain_hip_smbr_forward_backward_general(*nulls, None, 0, 0, AUTO) == -1
    assert "smbr_forward_backward_general" in _last_error() and "null pointer" in _last_error()
    assert L.pychain_hip_smbr_forward_backward_general(*nulls, None, 0, 1, AUTO) == -1 and "targets_are_classes" in _last_error()
    assert L.pychain_hip_smbr_forward_backward_general(*nulls, None, 0, 0, 9) == -1 and "form" in _last_error()


def test_kernels_is_checked():
    g, y, lengths, pdfs, probs = sr.case("small")
    tg = PosteriorTargets(pdfs, probs)
    for bad in ("nonsense", "LDS", "", None, 2):
        with pytest.raises(ValueError, match="kernels"):
            expected_accuracy(y, lengths, g, tg, kernels=bad)
        with pytest.raises(ValueError, match="kernels"):
            SMBRLoss(g, kernels=bad)
    with pytest.raises(ValueError, match="kernels"):
        native.smbr_form_code("nonsense")
    assert [native.smbr_form_code(k) for k in ("auto", "lds", "rows", "global")] == [AUTO, LDS, ROWS, GLOBAL]
    with pytest.raises(TypeError):                                          # a keyword
        expected_accuracy(y, lengths, g, tg, 1e-5, None, False, "auto")


@pytest.mark.parametrize("which", [None, "phones"])
def test_on_cpu_tensors_every_form_is_the_host_twin(which):
    g, y, lengths, pdfs, probs = cr.case("small")
    tg = PosteriorTargets(pdfs, probs)
    classes = None if which is None else cr.classes(which, y.size(2))

    def call(**kw):
        x = y.clone().requires_grad_(True)
        acc = expected_accuracy(x, lengths, g, tg, leaky_coefficient=0.1, classes=classes, **kw)
        acc.backward()
        return x.grad, acc

    calls = _lib.lib().pychain_hip_cpu_calls()
    want, acc0 = call()
    per_call = _lib.lib().pychain_hip_cpu_calls() - calls
    assert per_call > 0 and float(want.abs().max()) > 0
    for kernels in ("lds", "auto", "rows", "global"):
        calls = _lib.lib().pychain_hip_cpu_calls()
        grad, acc = call(kernels=kernels)
        assert _lib.lib().pychain_hip_cpu_calls() - calls == per_call          # the same host twins
        assert torch.equal(grad, want) and torch.equal(acc.per_seq, acc0.per_seq) and torch.equal(acc.closing, acc0.closing)
        assert torch.equal(acc.bad_count, acc0.bad_count)
    x = y.clone().requires_grad_(True)
    loss = SMBRLoss(g, leaky_coefficient=0.1, avg=False, classes=classes, kernels="auto")(x, lengths, tg)
    loss.backward()
    assert torch.equal(x.grad, -want) and torch.equal(loss.per_seq, acc0.per_seq)
