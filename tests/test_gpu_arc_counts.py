"""Expected arc counts (include/pychain_hip.h: pychain_hip_den_arc_counts; csrc/arc_counts.hip) on the MI355X
against the fp64 recursions of tests/arc_counts_reference, at leaky coefficients 0.1 and 1e-5, with w = None and w = 0.5 N(0,1):
the three shapes of smbr_reference.case (a thread owns two states; a state nothing enters, a state nothing leaves, a pdf no arc
carries, lengths down to 1); a graph of 2100 states; a sequence of 1500 frames beside 400, 100 and 48 (24 count workgroups, the
last one short; every K here is no multiple of the 256 threads of the small kernels).  Then the host twin, 2-byte rows, the
plan kernels at w = 0, two calls, views and misaligned tensors, a NaN, the exact zeros, the refusal beyond the LDS, autograd.

Tolerance (arc_counts_reference.reference; the rule of smbr_reference.bound): 1e-5 on max |d counts| / max |counts|, on
max |d grad| / max |grad| and on the relative log Z_b, or twice the fp32 restatement's own distance where that is beyond 5e-6.
Every measured distance goes through helpers.record_parity."""
import numpy as np
import pytest
import torch

import arc_counts_reference as ar
from helpers import record_parity
from pychain_amd import ChainFunction, ChainGraphBatch, _lib, den_log_partition, expected_arc_counts, native

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
WKINDS = (None, "normal")


def _call(name, coef, wkind=None, dtype=torch.float32, device=DEV, y=None, u=None, w=None):
    """(objf_per_seq, counts, counts_per_seq, grad, bad_count) of the native call of a case"""
    g, y0, lengths = ar.case(name)
    x = (y0 if y is None else y).to(device=device, dtype=dtype)
    w = ar.weights(name, wkind) if w is None else w
    gt = native.smbr_graph(g, x.size(2), x.device)
    fn = native.den_arc_counts if x.is_cuda else native.cpu_den_arc_counts
    return fn(gt, g.num_states, x, lengths, coef, w, u, per_seq=True)


def _triple(r):
    return r[0].cpu().numpy(), r[2].cpu().numpy(), r[3].double().cpu().numpy()


@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("coef", ar.COEFS)
@pytest.mark.parametrize("name", ar.CASES)
def test_against_fp64(name, coef, wkind):
    ref, (bound, d32) = ar.reference(name, coef, wkind)
    calls = _lib.lib().pychain_hip_cpu_calls()
    r = _call(name, coef, wkind)
    assert _lib.lib().pychain_hip_cpu_calls() == calls                        # the kernels, not the host twin
    dc, dg, dz = ar.distances(_triple(r), ref)
    dsum = ar.dist(r[1].cpu().numpy(), ref[1].sum(0))
    print("%s c=%g w=%s: counts %.3g summed %.3g grad %.3g logZ %.3g (fp32 restatement %.3g, bound %.3g)" % (name, coef, wkind, dc, dsum, dg, dz, d32, bound))
    record_parity("arc_counts_gpu_%s_c%g_w%s" % (name, coef, wkind), counts=dc, counts_summed=dsum, grad=dg, logz=dz, f32_reference=d32, bound=bound)
    assert r[0].dtype == r[1].dtype == r[2].dtype == torch.float64 and r[3].dtype == torch.float32 and r[1].is_cuda
    assert dc <= bound and dsum <= bound and dg <= bound and dz <= bound
    assert r[4].tolist() == [0, 0]
    lengths = ar.case(name)[2]
    assert np.abs(r[2].cpu().numpy().sum(1) - lengths.numpy()).max() <= bound * float(lengths.max())     # sum_k c(b,k) = L_b
    g = r[3].cpu().numpy()
    for b, L in enumerate(lengths.tolist()):
        assert not g[b, L:].any()                                             # rows beyond a length: exact zeros
    if name == "degenerate":
        assert not g[:, :, 8].any()                                           # the pdf no arc carries


@pytest.mark.parametrize("coef", ar.COEFS)
@pytest.mark.parametrize("name", ar.CASES)
def test_host_twin_against_device(name, coef):
    _, (bound, _) = ar.reference(name, coef, "normal")
    dev, host = _triple(_call(name, coef, "normal")), _triple(_call(name, coef, "normal", device="cpu"))
    dc, dg, dz = ar.distances(dev, host)
    record_parity("arc_counts_gpu_twin_%s_c%g" % (name, coef), counts=dc, grad=dg, logz=dz, bound=bound)
    print("%s c=%g: device against twin counts %.3g grad %.3g logZ %.3g (bound %.3g)" % (name, coef, dc, dg, dz, bound))
    assert dc <= bound and dg <= bound and dz <= bound


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_two_byte_rows(name, dtype):
    yh = ar.case(name)[1].to(dtype)
    rh = _call(name, 0.1, "normal", dtype=dtype, y=yh)
    rf = _call(name, 0.1, "normal", y=yh.float())
    assert rh[3].dtype == dtype and rf[3].dtype == torch.float32
    assert torch.equal(rh[3], rf[3].to(dtype))                                # the fp32 call on the up-cast input, rounded once
    assert torch.equal(rh[0], rf[0]) and torch.equal(rh[1], rf[1]) and torch.equal(rh[2], rf[2])


@pytest.mark.parametrize("name", ["small", "wide"])
def test_plan_kernels_at_zero_weights(name):
    g, y, lengths = ar.case(name)
    _, (bound, _) = ar.reference(name, 1e-5, None)
    r = _call(name, 1e-5)
    x = y.to(DEV).requires_grad_(True)
    den = ChainFunction.apply(x, lengths, ChainGraphBatch(g, y.size(0)), 1e-5)
    den.backward()
    dz = ar.value_dist(r[0].cpu().numpy(), den._objf_per_seq.double().cpu().numpy())
    dg = ar.dist(r[3].cpu().numpy(), x.grad.double().cpu().numpy())
    record_parity("arc_counts_gpu_plan_%s" % name, logz=dz, grad=dg, bound=bound)
    print("%s: against the plan kernels logZ %.3g gamma %.3g (bound %.3g)" % (name, dz, dg, bound))
    assert dz <= bound and dg <= bound


@pytest.mark.parametrize("name", ["small", "long"])
def test_two_calls_give_the_same_bits(name):
    a, b = _call(name, 1e-5, "normal"), _call(name, 1e-5, "normal")
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_zero_weights_are_no_weights():
    K = ar.case("small")[0].num_transitions
    a, b = _call("small", 0.1), _call("small", 0.1, w=torch.zeros(K))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_views_slices_and_misaligned_tensors():
    g, y, lengths = ar.case("small")
    B, T, D = y.shape
    K = g.num_transitions
    w, u = ar.weights("small", "normal"), torch.tensor([1.0, 0.5, 2.0, 0.25])
    want = _call("small", 0.1, w=w.to(DEV), u=u.to(DEV))
    # x: a slice of a wider layer's output (strided), and a contiguous view 4 bytes off the 16-byte grid
    wide = torch.zeros(B, T, D + 5, device=DEV)
    wide[:, :, 2:D + 2] = y.to(DEV)
    flat = torch.zeros(B * T * D + 1, device=DEV)
    flat[1:] = y.to(DEV).reshape(-1)
    off = flat[1:].view(B, T, D)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    # w, u: every second element of a longer tensor, and views off the grid
    w2 = torch.zeros(2 * K + 1, device=DEV)
    w2[1::2] = w.to(DEV)
    u2 = torch.zeros(B + 1, device=DEV)
    u2[1:] = u.to(DEV)
    for x, ww, uu in ((wide[:, :, 2:D + 2], w2[1::2], u2[1:]), (off, w2[1::2].clone(), u.to(DEV)), (y.to(DEV), w, u)):
        got = _call("small", 0.1, y=x, w=ww, u=uu)
        assert all(torch.equal(p, q) for p, q in zip(got, want))


def test_nan_and_weight_zero():
    g, y, lengths = ar.case("small")
    K = g.num_transitions
    y3 = y.clone()
    y3[1, 3, 5] = float("nan")
    y3[1, 12, 5] = float("nan")                                               # (beyond the length of 9: not read)
    bad = _call("small", 0.1, "normal", y=y3)
    zero = _call("small", 0.1, "normal", u=torch.tensor([1.0, 0.0, 1.0, 1.0]))
    assert bad[4].tolist() == [1, 0]                                          # counted once
    assert bool(torch.isnan(bad[0][1])) and not bad[2][1].any()
    keep = [0, 2, 3]
    assert torch.equal(bad[1], zero[1])                                       # exact zeros into the counts
    assert torch.equal(bad[0][keep], zero[0][keep]) and torch.equal(bad[2][keep], zero[2][keep]) and torch.equal(bad[3][keep], zero[3][keep])
    assert not zero[3][1].any() and zero[4].tolist() == [0, 0]                # weight 0: an exact zero gradient
    # a weight that is not finite: counted, taken as 0
    w = ar.weights("small", "normal").clone()
    w0 = w.clone()
    w[7], w0[7] = float("inf"), 0.0
    a, b = _call("small", 0.1, w=w), _call("small", 0.1, w=w0)
    assert a[4].tolist() == [0, 1] and all(torch.equal(p, q) for p, q in zip(a[:4], b[:4]))


def test_beyond_the_lds_is_refused():
    g = ar.case("degenerate")[0]
    D = 21000                                                                 # (2 * 12 + 2 * 21000 + 64) * 4 + 256 bytes > 160 KiB
    x = torch.zeros(1, 2, D, device=DEV)
    with pytest.raises(_lib.PychainHipError) as e:
        expected_arc_counts(x, torch.tensor([2]), g)
    need = _lib.lib().pychain_hip_den_arc_counts_lds_bytes(12, D)
    assert need == (2 * 12 + 2 * D + 64) * 4 + 256 and need > 160 * 1024
    assert "12 states" in str(e.value) and "%d pdfs" % D in str(e.value) and str(need) in str(e.value) and str(160 * 1024) in str(e.value)


def test_public_calls_and_backward():
    g, y, lengths = ar.case("small")
    ref, (bound, _) = ar.reference("small", 0.1, "normal")
    u = torch.tensor([1.0, 0.5, 2.0, 0.25])
    res = expected_arc_counts(y.to(DEV), lengths, ChainGraphBatch(g, 4), 0.1, arc_log_weights=ar.weights("small", "normal"), utt_weights=u)
    assert res.counts_per_seq is None and res.counts.is_cuda and res.bad_count.tolist() == [0, 0]
    assert ar.dist(res.counts.cpu().numpy(), (u.double().numpy()[:, None] * ref[1]).sum(0)) <= bound
    x = y.to(DEV).requires_grad_(True)
    w = ar.weights("small", "normal").to(torch.float64).requires_grad_(True)  # fp64, on the host: the gradient comes back so
    out = den_log_partition(x, lengths, g, w, 0.1, utt_weights=u)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.is_cuda and out.per_seq.dtype == torch.float64
    total = float((u.double().numpy() * ref[0]).sum())
    assert abs(float(out.detach()) - total) <= bound * abs(total)
    (3.0 * out).backward(retain_graph=True)
    assert w.grad.dtype == torch.float64 and not w.grad.is_cuda and x.grad.dtype == torch.float32
    assert ar.dist(w.grad.numpy(), 3.0 * (u.double().numpy()[:, None] * ref[1]).sum(0)) <= bound
    assert ar.dist(x.grad.double().cpu().numpy(), 3.0 * u.double().numpy()[:, None, None] * ref[2]) <= bound
    first = (x.grad.clone(), w.grad.clone())
    x.grad, w.grad = None, None
    (3.0 * out).backward()                                                    # a second backward over the retained graph
    assert torch.equal(x.grad, first[0]) and torch.equal(w.grad, first[1])
