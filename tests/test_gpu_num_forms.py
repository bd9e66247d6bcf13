"""The numerator (free and under time windows) on the MI355X against a plain float64 forward-backward (tests/num_reference.py:
np_num_fb) at the project's bounds - objective and gradient within 1e-5 - on the cases of tests/num_cases.py: every launch
form of num_fb_kernel by row width (launch_num_fb: <4,4,LD> <4,8,LD> <4,8> <1,8> <1,0>, the last tile shape and the first
general one) and a shared graph of 701 states; each with no windows, with windows that admit everything (bit-identical to none)
and with arbitrary windows (shrunk, shifted, empty, lo = -1, hi = 2^31 - 1; one infeasible sequence in the middle of the
batch); through native.num_forward_backward (lengths on the host and on the device) and through ChainFunction with
set_time_windows; 2-byte rows where the kernels read them.  tests/test_num_reference.py holds the host twin to the same
reference and checks that the cases are what they claim."""
import numpy as np
import pytest
import torch

import num_cases as nc
from helpers import record_parity
from num_reference import check_numerator, np_num_fb
from pychain_amd import ChainFunction, _lib, native

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

# what rounding the gradient to a 2-byte type adds, relative to each element: half an ulp of a p-bit significand is at most
# 2^-p of the value (bf16: p = 8, fp16: p = 11); fp16 is subnormal below 2^-14, where half an ulp is 2^-25 absolute
HALF_ULP = {torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25)}


def _native(x, lengths, graphs, windows):
    gt = graphs.device_tensors(torch.device(DEV))
    gstride = 0 if graphs.shared_graph is not None else 1
    wd = None if windows is None else windows.to(DEV)
    out = native.num_forward_backward(gt, gstride, graphs.num_states, x, lengths, windows=wd)
    torch.cuda.synchronize()
    return out


def _check_bad(bad, feas):
    """The device counts the numerator's failed checks (at least one per sequence without a path), the host twin sequences:
    zero exactly where every sequence is feasible."""
    n = int((~feas).sum())
    assert (int(bad) == 0) == (n == 0) and int(bad) >= n


def _device_equals_reference(name, x, lengths, graphs, windows, ref):
    """native.num_forward_backward and ChainFunction on device tensors against np_num_fb of the fp32 value of the same input.
    Returns the largest (objective, gradient) distances."""
    calls = _lib.lib().pychain_hip_cpu_calls()
    xd = x.to(DEV)
    logp, rgrad, feas = ref
    worst = [0.0, 0.0]
    for ld in (lengths, lengths.to(DEV)):
        objf, grad, bad = _native(xd, ld, graphs, windows)
        assert grad.dtype == torch.float32
        d = check_numerator(objf.cpu().numpy(), grad.cpu().numpy(), None, ref, lengths)
        _check_bad(bad, feas)
        worst = [max(a, b) for a, b in zip(worst, d)]
    graphs.set_time_windows(windows)                                  # ChainFunction takes the batch's own windows
    try:
        xx = xd.clone().requires_grad_(True)
        o = ChainFunction.apply(xx, lengths, graphs)
        o.backward()
        torch.cuda.synchronize()
    finally:
        graphs.set_time_windows(None)
    assert _lib.lib().pychain_hip_cpu_calls() == calls               # device tensors never reach the host twin
    _check_bad(ChainFunction.last_bad_count, feas)
    total = float(logp.sum())                                         # (-inf with an infeasible sequence)
    if np.isfinite(total):
        d_o = abs(float(o) - total) / abs(total)
        assert d_o <= 1e-5, d_o
        worst[0] = max(worst[0], d_o)
    else:
        assert float(o) == total
    g = xx.grad
    assert g.dtype == x.dtype
    gn = g.float().cpu().numpy().astype(np.float64)
    for b in np.nonzero(~feas)[0]:
        assert not gn[b].any()
    scale = np.abs(rgrad).max()
    if x.dtype == torch.float32:
        d_g = float(np.abs(gn - rgrad).max() / scale)
        assert d_g <= 1e-5, d_g
        worst[1] = max(worst[1], d_g)
    else:
        # the fp32 gradient v lies within 1e-5 max|ref| of the reference; rounding it moves it by at most u |v| (+ the subnormal step)
        u, sub = HALF_ULP[x.dtype]
        fp32_bound = 1e-5 * scale
        bound = fp32_bound + u * (np.abs(rgrad) + fp32_bound) + sub
        excess = float((np.abs(gn - rgrad) - bound).max())
        assert excess <= 0.0, excess
        record_parity(name + "_rounded", grad_abs_over_bound=float((np.abs(gn - rgrad) / bound).max()))
    record_parity(name, objf_rel=worst[0], grad_rel=worst[1])
    print("%s: objective %.3e gradient %.3e" % (name, worst[0], worst[1]))
    return worst


def _full_windows_same_bits(x, lengths, graphs):
    xd = x.to(DEV)
    a = _native(xd, lengths, graphs, None)
    for w in (nc.full_windows(graphs.batch_size, graphs.num_states), nc.full_windows(graphs.batch_size, graphs.num_states, 0, x.shape[1])):
        b = _native(xd, lengths, graphs, w)
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def _case(name, x, lengths, graphs, windows, infeasible, expect_half=None):
    K = int(graphs.backward_transitions.shape[-2])
    half = bool(_lib.lib().pychain_hip_num_half_native(graphs.num_states, K, x.shape[2]))
    if expect_half is not None:
        assert half == expect_half
    for dtype in (torch.float32, torch.bfloat16, torch.float16) if half else (torch.float32,):
        xt = x.to(dtype)
        tag = "%s_%s" % (name, str(dtype).split(".")[-1])
        free = np_num_fb(graphs, xt.float(), lengths)
        win = np_num_fb(graphs, xt.float(), lengths, windows)
        assert bool(free[2].all()) and not win[2][infeasible] and 2 * int(win[2].sum()) >= win[2].size
        _device_equals_reference(tag + "_free", xt, lengths, graphs, None, free)
        _device_equals_reference(tag + "_full", xt, lengths, graphs, nc.full_windows(graphs.batch_size, graphs.num_states), free)
        _device_equals_reference(tag + "_windows", xt, lengths, graphs, windows, win)
        _full_windows_same_bits(xt, lengths, graphs)


# the D of the form matrix where num_fb_kernel reads 2-byte rows (D % 4 == 0 within the register-staged float4 forms)
HALF_NATIVE_D = {4: True, 48: True, 2048: True, 2052: True, 4096: True, 4100: True, 8408: True, 16384: True, 16388: False,
                 1001: False, 4095: False, 4097: False, "tile_last": False, "general_first": False}


@pytest.mark.parametrize("D", list(nc.FORM_D) + ["tile_last", "general_first"])
def test_form_matrix(D):
    expect_half = HALF_NATIVE_D[D]
    if isinstance(D, str):
        D = nc.form_boundary_D()[("tile_last", "general_first").index(D)]
    x, lengths, graphs, w = nc.form_windows_case(D)
    _case("num_forms_D%d" % D, x, lengths, graphs, w, 1, expect_half)


def test_shared_graph_701_states():
    x, lengths, graphs, w = nc.shared701_case()
    _case("num_forms_shared701", x, lengths, graphs, w, 2, True)
