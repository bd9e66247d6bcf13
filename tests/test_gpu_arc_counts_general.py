"""The general arc-count kernels (include/pychain_hip.h: pychain_hip_den_arc_counts_general; csrc/arc_counts.hip)
on the MI355X.  Where the LDS form runs too - the six cases of tests/arc_counts_reference, 2-byte rows, and `many_items`, whose
540 count items are more than the 512 workgroups of the persistent count launch - "rows", "global" and "auto" are held to the
BITS of "lds" on every output.  Beyond the LDS (tests/arc_counts_general_cases: a tree, a graph, and both beyond it) the form
that runs is held to the fp64 recursions at leaky coefficients 0.1 and 1e-5, with w = None and w = 0.5 N(0,1); then autograd, the
refusals, the host twin, two calls, a misaligned view, a zero utterance weight, NaNs, a weight that is not finite, and a fault
planted into the host reference to show that the shapes see what they are meant to see.

Tolerance (arc_counts_general_cases.reference; the rule of arc_counts_reference.reference): 1e-5 on max |d counts| / max |counts|,
on max |d grad| / max |grad| and on the relative log Z_b, or twice the fp32 restatement's own distance where that is beyond 5e-6.
On the CPU the restatement sits 5.8e-8 to 2.7e-7 from fp64 on the four shapes beyond the LDS, so every bound there is 1e-5.
Every measured distance goes through helpers.record_parity."""
import numpy as np
import pytest
import torch

import arc_counts_general_cases as gc
import arc_counts_reference as ar
from helpers import record_parity
from pychain_amd import _lib, den_log_partition, expected_arc_counts, native

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
WKINDS = (None, "normal")
GENERAL = ("rows", "global", "auto")
FORM_NAME = {gc.LDS: "lds", gc.ROWS: "rows", gc.GLOBAL: "global"}


def _call(mod, name, coef, wkind=None, form="lds", dtype=torch.float32, device=DEV, y=None, u=None, w=None):
    """(objf_per_seq, counts, counts_per_seq, grad, bad_count) of the native call of a case of `mod` (ar or gc)"""
    g, y0, lengths = mod.case(name)
    x = (y0 if y is None else y).to(device=device, dtype=dtype)
    w = mod.weights(name, wkind) if w is None else w
    gt = native.smbr_graph(g, x.size(2), x.device)
    fn = native.den_arc_counts if x.is_cuda else native.cpu_den_arc_counts
    return fn(gt, g.num_states, x, lengths, coef, w, u, per_seq=True, form=form)


def _partition(mod, name, coef, wkind, kernels):
    """(the value, its per_seq, d / dx, d / dw or None) of den_log_partition on a case"""
    g, y, lengths = mod.case(name)
    x = y.to(DEV).requires_grad_(True)
    w = mod.weights(name, wkind)
    w = None if w is None else w.to(DEV).requires_grad_(True)
    out = den_log_partition(x, lengths, g, w, coef, kernels=kernels)
    out.backward()
    return out.detach(), out.per_seq, x.grad, None if w is None else w.grad


def _same(a, b):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


def _triple(r):
    return r[0].cpu().numpy(), r[2].cpu().numpy(), r[3].double().cpu().numpy()


# ---- the bits of the LDS form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("name,coef", [(n, c) for n in ("small", "wide", "degenerate", "states2100", "long_row") for c in ar.COEFS] +
                         [("long", 1e-5)])
def test_the_bits_of_the_lds_form(name, coef, wkind):
    calls = _lib.lib().pychain_hip_cpu_calls()
    want = _call(ar, name, coef, wkind)
    want_p = _partition(ar, name, coef, wkind, "lds")
    assert float(want[3].abs().max()) > 0 and float(want[1].abs().max()) > 0
    for form in GENERAL:
        assert _same(_call(ar, name, coef, wkind, form=form), want), form
        assert _same(_partition(ar, name, coef, wkind, form), want_p), form
    assert _lib.lib().pychain_hip_cpu_calls() == calls                        # the kernels, not the host twin


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_bits_of_the_lds_form_on_two_byte_rows(name, dtype):
    yh = ar.case(name)[1].to(dtype)
    want = _call(ar, name, 0.1, "normal", dtype=dtype, y=yh)
    assert want[3].dtype == dtype
    for form in GENERAL:
        assert _same(_call(ar, name, 0.1, "normal", form=form, dtype=dtype, y=yh), want), form


def test_many_items():
    """More count items than workgroups: some workgroups of the persistent launch take a second item."""
    coef, wkind = 1e-5, "normal"
    ref, (bound, d32) = gc.reference("many_items", coef, wkind)
    want = _call(gc, "many_items", coef, wkind)
    for form in ("rows", "global"):
        assert _same(_call(gc, "many_items", coef, wkind, form=form), want), form
    dc, dg, dz = gc.distances(_triple(want), ref)
    print("many_items: counts %.3g grad %.3g logZ %.3g (fp32 restatement %.3g, bound %.3g)" % (dc, dg, dz, d32, bound))
    record_parity("arc_counts_general_many_items", counts=dc, grad=dg, logz=dz, f32_reference=d32, bound=bound)
    assert dc <= bound and dg <= bound and dz <= bound and want[4].tolist() == [0, 0]


# ---- beyond the LDS: against fp64 -----------------------------------------------------------------------------------------------
def _refused_by_default(name, coef=0.1):
    c = gc.SHAPES[name]
    with pytest.raises(_lib.PychainHipError) as e:
        _call(gc, name, coef)
    need = _lib.lib().pychain_hip_den_arc_counts_lds_bytes(c["H"], c["D"])
    msg = str(e.value)
    assert "(-2)" in msg and "pychain_hip_den_arc_counts failed" in msg
    assert "%d states and %d pdfs need %d bytes" % (c["H"], c["D"], need) in msg and str(160 * 1024) in msg


@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("coef", ar.COEFS)
@pytest.mark.parametrize("name", gc.BEYOND)
def test_against_fp64_beyond_the_lds(name, coef, wkind):
    c = gc.SHAPES[name]
    assert _lib.lib().pychain_hip_den_arc_counts_form(c["H"], c["D"], gc.AUTO) == c["form"] != gc.LDS
    _refused_by_default(name, coef)
    ref, (bound, d32) = gc.reference(name, coef, wkind)
    calls = _lib.lib().pychain_hip_cpu_calls()
    r = _call(gc, name, coef, wkind, form="auto")
    assert _lib.lib().pychain_hip_cpu_calls() == calls                        # the kernels, not the host twin
    dc, dg, dz = gc.distances(_triple(r), ref)
    dsum = ar.dist(r[1].cpu().numpy(), ref[1].sum(0))
    print("%s c=%g w=%s: counts %.3g summed %.3g grad %.3g logZ %.3g (fp32 restatement %.3g, bound %.3g)" % (name, coef, wkind, dc, dsum, dg, dz, d32, bound))
    record_parity("arc_counts_general_%s_c%g_w%s" % (name, coef, wkind), counts=dc, counts_summed=dsum, grad=dg, logz=dz, f32_reference=d32, bound=bound)
    assert r[0].dtype == r[1].dtype == r[2].dtype == torch.float64 and r[3].dtype == torch.float32 and r[1].is_cuda
    assert r[4].dtype == torch.int32 and r[4].tolist() == [0, 0]
    assert np.isfinite(r[0].cpu().numpy()).all()
    assert dc <= bound and dsum <= bound and dg <= bound and dz <= bound
    lengths = gc.case(name)[2]
    assert np.abs(r[2].cpu().numpy().sum(1) - lengths.numpy()).max() <= bound * float(lengths.max())     # sum_k c(b,k) = L_b
    g = r[3].cpu().numpy()
    for b, L in enumerate(lengths.tolist()):
        assert not g[b, L:].any()                                             # rows beyond a length: exact zeros
    # the form by name is the form "auto" ran
    assert _same(_call(gc, name, coef, wkind, form=FORM_NAME[c["form"]]), r)


def test_autograd_beyond_the_lds():
    name, coef = "pdfs_beyond", 0.1
    g, y, lengths = gc.case(name)
    _, (bound, _) = gc.reference(name, coef, "normal")
    Z, C, G = gc.batch(gc.autograd, g, y, lengths, gc.weights(name, "normal"), coef)
    out, per_seq, gx, gw = _partition(gc, name, coef, "normal", "auto")
    dz = ar.value_dist(per_seq.cpu().numpy(), Z)
    dw, dx = ar.dist(gw.cpu().numpy(), C.sum(0)), ar.dist(gx.double().cpu().numpy(), G)
    print("%s autograd: logZ %.3g d/dw %.3g d/dx %.3g (bound %.3g)" % (name, dz, dw, dx, bound))
    record_parity("arc_counts_general_autograd_%s" % name, logz=dz, grad_w=dw, grad_x=dx, bound=bound)
    assert dz <= bound and dw <= bound and dx <= bound
    assert abs(float(out) - Z.sum()) <= bound * abs(Z.sum())


def test_a_second_backward_goes_through_the_same_form():
    """The recomputation for a second backward would be refused under the default form at this shape."""
    g, y, lengths = gc.case("pdfs_beyond")
    x = y.to(DEV).requires_grad_(True)
    w = gc.weights("pdfs_beyond", "normal").to(DEV).requires_grad_(True)
    out = den_log_partition(x, lengths, g, w, 0.1, kernels="auto")
    (3.0 * out).backward(retain_graph=True)
    first = (x.grad.clone(), w.grad.clone())
    assert float(first[0].abs().max()) > 0 and float(first[1].abs().max()) > 0
    x.grad, w.grad = None, None
    (3.0 * out).backward()
    assert torch.equal(x.grad, first[0]) and torch.equal(w.grad, first[1])


def test_a_form_by_name_beyond_its_reach():
    for name in ("states_beyond", "both_beyond"):                             # "rows" on a graph only "global" holds
        c = gc.SHAPES[name]
        g, y, lengths = gc.case(name)
        with pytest.raises(_lib.PychainHipError) as e:
            expected_arc_counts(y.to(DEV), lengths, g, 0.1, kernels="rows")
        msg = str(e.value)
        assert "(-2)" in msg and "den_arc_counts_general" in msg and "%d states" % c["H"] in msg and str(160 * 1024) in msg
        assert str(_lib.lib().pychain_hip_den_arc_counts_general_lds_bytes(c["H"])) in msg
    for name in gc.BEYOND:                                                    # "lds" by name is the default call: what it raised
        c = gc.SHAPES[name]
        g, y, lengths = gc.case(name)
        _refused_by_default(name)
        with pytest.raises(_lib.PychainHipError) as e:
            den_log_partition(y.to(DEV), lengths, g, None, 0.1, kernels="lds")
        assert "(-2)" in str(e.value) and "%d states and %d pdfs need" % (c["H"], c["D"]) in str(e.value)


# ---- further cases at the shapes beyond the LDS -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", ar.COEFS)
def test_host_twin_against_device(coef):
    _, (bound, _) = gc.reference("wide_tree", coef, "normal")
    dev, host = _triple(_call(gc, "wide_tree", coef, "normal", form="auto")), _triple(_call(gc, "wide_tree", coef, "normal", device="cpu"))
    dc, dg, dz = gc.distances(dev, host)
    record_parity("arc_counts_general_twin_wide_tree_c%g" % coef, counts=dc, grad=dg, logz=dz, bound=bound)
    print("wide_tree c=%g: device against twin counts %.3g grad %.3g logZ %.3g (bound %.3g)" % (coef, dc, dg, dz, bound))
    assert dc <= bound and dg <= bound and dz <= bound


@pytest.mark.parametrize("name", ["wide_tree", "states_beyond"])
def test_two_calls_give_the_same_bits(name):
    a, b = _call(gc, name, 1e-5, "normal", form="auto"), _call(gc, name, 1e-5, "normal", form="auto")
    assert _same(a, b)


@pytest.mark.parametrize("name", ["pdfs_beyond", "states_beyond"])
def test_a_view_off_the_16_byte_grid(name):
    y = gc.case(name)[1]
    B, T, D = y.shape
    flat = torch.zeros(B * T * D + 1, device=DEV)
    flat[1:] = y.to(DEV).reshape(-1)
    off = flat[1:].view(B, T, D)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    aligned = off.clone()
    assert aligned.data_ptr() % 16 == 0
    assert _same(_call(gc, name, 0.1, "normal", form="auto", y=off), _call(gc, name, 0.1, "normal", form="auto", y=aligned))


@pytest.mark.parametrize("name", ["wide_tree", "states_beyond"])
def test_an_utterance_weight_of_zero(name):
    full = _call(gc, name, 0.1, "normal", form="auto")
    zero = _call(gc, name, 0.1, "normal", form="auto", u=torch.tensor([1.0, 0.0]))
    assert torch.equal(zero[1], full[2][0])                                   # the counts without that sequence's contribution
    assert torch.equal(zero[0], full[0]) and torch.equal(zero[2], full[2])    # log Z_b and the counts of a sequence: not weighted
    assert torch.equal(zero[3][0], full[3][0]) and not zero[3][1].any() and zero[4].tolist() == [0, 0]


def test_nan_and_a_weight_that_is_not_finite():
    name = "pdfs_beyond"
    g, y, lengths = gc.case(name)
    carried = set(ar.graph_arrays(g)[2].tolist())
    n = next(d for d in range(4097, y.size(2)) if d not in carried)           # beyond the 4096 elements held in registers
    clean = _call(gc, name, 0.1, "normal", form="auto")
    y1 = y.clone()
    y1[1, 2, n] = float("nan")                                                # beyond the length of 1: not seen
    assert _same(_call(gc, name, 0.1, "normal", form="auto", y=y1), clean)
    y2 = y1.clone()
    y2[0, 1, n] = float("nan")                                                # a live row, a pdf no arc carries
    bad = _call(gc, name, 0.1, "normal", form="auto", y=y2)
    assert bad[4].tolist() == [1, 0]                                          # that sequence alone, counted once
    assert bool(torch.isnan(bad[0][0])) and not bad[2][0].any()
    assert torch.equal(bad[1], clean[2][1])                                   # left out of the counts
    assert torch.equal(bad[0][1], clean[0][1]) and torch.equal(bad[2][1], clean[2][1]) and torch.equal(bad[3][1], clean[3][1])
    # a weight that is not finite: counted, taken as 0
    w = gc.weights("wide_tree", "normal").clone()
    w0 = w.clone()
    w[7], w0[7] = float("inf"), 0.0
    w[20001], w0[20001] = float("nan"), 0.0
    a, b = _call(gc, "wide_tree", 0.1, form="auto", w=w), _call(gc, "wide_tree", 0.1, form="auto", w=w0)
    assert a[4].tolist() == [0, 2] and b[4].tolist() == [0, 0] and _same(a[:4], b[:4])


@pytest.mark.parametrize("fault", ar.FAULTS[:1])
def test_a_planted_fault_shows_at_wide_tree(fault):
    """On the host reference only: the shape sees what it is meant to see."""
    g, y, lengths = gc.case("wide_tree")
    ref, (bound, _) = gc.reference("wide_tree", 0.1, "normal")
    wrong = gc.batch(gc.counts, g, y, lengths, gc.weights("wide_tree", "normal"), 0.1, fault=fault)
    dc = ar.dist(wrong[1], ref[1])
    print("wide_tree %s: counts moved by %.3g (bound %.3g)" % (fault, dc, bound))
    assert dc > 100 * bound
