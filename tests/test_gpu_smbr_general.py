"""The general sMBR kernels (csrc/smbr_general.hip; include/pychain_hip.h: pychain_hip_smbr_forward_backward_general; DESIGN.md
§3.28) on the MI355X.

SAME BITS where the LDS kernels run too: the cases of tests/smbr_reference at leaky coefficients 0.1 and 1e-5 - `wide` has more
states than a recursion workgroup has threads, `degenerate` a pdf no arc carries -, pdf-level and under the maps `phones` and
`identity` of tests/smbr_class_reference on that file's own targets, fp32, bf16 and fp16 rows: kernels="rows" and "global" each
give torch.equal to "lds" on the gradient, per_seq, closing and bad_count.  `long_row` (37 states, 4200 pdfs: within the LDS, beyond
the 4096 elements of a row the recursion threads hold in registers) does the same pdf-level and under `phones`, fp32 and bf16, and
holds "lds" to the fp64 recursions.

AGAINST FP64 beyond the LDS of a CU, under kernels="auto" with the form asserted through pychain_hip_smbr_form: the shape
tests/test_gpu_smbr.py shows refused by default (37 states, 10180 pdfs), C4's graph (3000 states, 8408 pdfs) pdf-level, by
`phones` and by identity classes (C = D), a graph of 12 000 states, and one with both beyond - lengths down to one frame, K = 3
targets on pdfs arcs carry with a repeat and a padding entry.  Tolerance: smbr_reference.bound, the class rule for classes - 1e-5
on max |d grad| / max |grad| and the relative error of E_b, or twice the fp32 numpy recursions' own distance from fp64 where that
is beyond 5e-6; row sums and `closing` are held to the same bound.  On these shapes and targets the fp32 numpy recursions sit
8.1e-8 to 9.3e-7 from fp64, so every bound is 1e-5; the host twin is 1.9e-8 to 3.2e-7 from fp64 and the device 4.1e-8 to 6.7e-7
(profiles/smbr_general.md).  Every measured distance goes through helpers.record_parity.

And at those shapes: the host twin against the device; two calls bit for bit; a view of x off the 16-byte grid; the counts and a
NaN."""
import numpy as np
import pytest
import torch

import smbr_class_reference as cr
import smbr_reference as sr
from helpers import record_parity
from pychain_amd import PosteriorTargets, _lib, expected_accuracy, synthetic as syn

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
AUTO, LDS, ROWS, GLOBAL = 0, 1, 2, 3
BUDGET = 160 * 1024

SHAPES = {
    "refused_today": dict(H=37, K=150, D=10180, B=2, T=3, lengths=[3, 1], form=ROWS),
    "c4_graph": dict(H=3000, K=30000, D=8408, B=2, T=6, lengths=[6, 4], form=ROWS),
    "states_beyond": dict(H=12000, K=40000, D=130, B=2, T=5, lengths=[5, 2], form=GLOBAL),
    "both_beyond": dict(H=11000, K=36000, D=8408, B=1, T=3, lengths=[3], form=GLOBAL),
    # within the LDS, with a row of more than the 4096 elements the recursion threads hold in registers: four arcs carry pdfs beyond
    "long_row": dict(H=37, K=150, D=4200, B=2, T=3, lengths=[3, 1], form=LDS),
}
BEYOND = [(name, which) for name in SHAPES if SHAPES[name]["form"] != LDS for which in (None, "phones")] + [("c4_graph", "identity")]
_made, _refs = {}, {}


def shape(name):
    """(graph, y float32 [B,T,D], lengths, pdfs int32 [B,T,3], probs float32 [B,T,3]) of SHAPES[name], made once and shared: every
    target names a pdf an arc carries; every even frame has a pdf twice, every odd frame a padding entry."""
    if name not in _made:
        c = SHAPES[name]
        B, T, D = c["B"], c["T"], c["D"]
        g = syn.make_den_graph(c["H"], c["K"], D, seed=3)
        y = syn.make_input(B, T, D, seed=5)
        carried = np.unique(g.forward_transitions[:, 2].numpy())
        pdfs = np.stack([carried[syn.randint(21 + k, B * T, len(carried))].reshape(B, T) for k in range(3)], -1).astype(np.int32)
        pdfs[:, 0::2, 1] = pdfs[:, 0::2, 0]
        pdfs[:, 1::2, 2] = -1
        probs = (0.05 + syn.uniform(24, B * T * 3)).reshape(B, T, 3).astype(np.float32)
        _made[name] = (g, y, torch.tensor(c["lengths"]), torch.from_numpy(pdfs), torch.from_numpy(probs))
    return _made[name]


def reference(name, which, coef):
    """((E [B], grad [B,T,D], closing [B]), bound, the fp32 recursions' distance, max |grad|) by the fp64 recursions, once per process"""
    key = (name, which, coef)
    if key not in _refs:
        g, y, lengths, pdfs, probs = shape(name)
        pd, pr = pdfs.numpy(), probs.numpy()
        if which is None:
            ref = sr.batch(sr.recursions, g, y, lengths, pd, pr, coef)
            bound, d32 = sr.bound(g, y, lengths, pd, pr, coef, ref)
            scale = float(np.abs(ref[1]).max())
        else:
            cls = cr.class_map(which, y.size(2))
            ref = cr.batch(sr.recursions, g, y, lengths, pd, pr, cls, coef)
            w32 = cr.batch(sr.recursions, g, y, lengths, pd, pr, cls, coef, dtype=np.float32)
            scale = float(np.abs(ref[1]).max())
            d32 = max(cr.grad_dist(w32[1], ref[1], scale), sr.value_dist(w32[0], ref[0]))
            bound = 2.0 * d32 if d32 > sr.F32_SLACK else sr.BAR
        _refs[key] = (ref, bound, d32, scale)
    return _refs[key]


def _run(case, coef, kernels, which=None, dtype=torch.float32, device=DEV, y=None, pdfs=None):
    g, y0, lengths, p0, probs = case
    x = (y0 if y is None else y).detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    classes = None if which is None else cr.classes(which, y0.size(2))
    tg = PosteriorTargets(p0, probs) if pdfs is None else PosteriorTargets(pdfs, probs.to(pdfs.device))
    acc = expected_accuracy(x, lengths, g, tg, leaky_coefficient=coef, classes=classes, kernels=kernels)
    acc.backward()
    return x, acc


def _same(a, b):
    (xa, acca), (xb, accb) = a, b
    return (torch.equal(xa.grad, xb.grad) and torch.equal(acca.per_seq, accb.per_seq) and torch.equal(acca.bad_count, accb.bad_count)
            and torch.equal(acca.closing, accb.closing))          # (no NaN in these)


# ---- the same bits on shapes the LDS form takes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("which", [None, "phones", "identity"])
@pytest.mark.parametrize("name", ["small", "wide", "degenerate"])
def test_the_bits_of_the_lds_form(name, which, coef):
    case = sr.case(name) if which is None else cr.case(name)
    c = sr.CASES[name]
    C = 0 if which is None else int(cr.class_map(which, c["D"]).max()) + 1
    assert _lib.lib().pychain_hip_smbr_form(c["H"], c["D"], C, AUTO) == LDS
    calls = _lib.lib().pychain_hip_cpu_calls()
    lds = _run(case, coef, "lds", which)
    assert float(lds[0].grad.abs().max()) > 0 and lds[1].bad_count.tolist() == [0, 0]
    for kernels in ("rows", "global", "auto"):
        assert _same(_run(case, coef, kernels, which), lds), kernels
    assert _lib.lib().pychain_hip_cpu_calls() == calls                        # the kernels, not the host twins


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("which", [None, "phones"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_bits_of_the_lds_form_on_two_byte_rows(name, which, dtype):
    case = sr.case(name) if which is None else cr.case(name)
    lds = _run(case, 0.1, "lds", which, dtype=dtype)
    assert lds[0].grad.dtype == dtype and float(lds[0].grad.float().abs().max()) > 0
    for kernels in ("rows", "global"):
        assert _same(_run(case, 0.1, kernels, which, dtype=dtype), lds), kernels


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", [None, "phones"])
def test_the_bits_of_the_lds_form_on_a_long_row(which, dtype):
    """4200 pdfs: the elements beyond 4096 take the tail loops of the row's staging and of the dense companion row, in every form.
    "rows" and "global" give the bits of "lds"; "lds" is held to the fp64 recursions on the rows it saw (two-byte: the fp32 call
    on the up-cast input, rounded once, as tests/test_gpu_smbr.py holds them)."""
    c = SHAPES["long_row"]
    case = shape("long_row")
    g, y, lengths, pdfs, probs = case
    D = c["D"]
    assert int(g.forward_transitions[:, 2].max()) >= 4096                     # arcs carry pdfs of the tail
    C = 0 if which is None else int(cr.class_map(which, D).max()) + 1
    assert _lib.lib().pychain_hip_smbr_form(c["H"], D, C, AUTO) == LDS
    up = y.to(dtype).float()
    lds = _run(case, 0.1, "lds", which, dtype=dtype, y=up)
    assert lds[0].grad.dtype == dtype and float(lds[0].grad.float().abs().max()) > 0 and lds[1].bad_count.tolist() == [0, 0]
    for kernels in ("rows", "global"):
        assert _same(_run(case, 0.1, kernels, which, dtype=dtype, y=up), lds), kernels
    (want, bound, d32, scale), f32 = reference("long_row", which, 0.1), lds
    if dtype != torch.float32:
        f32 = _run(case, 0.1, "lds", which, y=up)
        assert torch.equal(lds[0].grad, f32[0].grad.to(dtype))
        assert torch.equal(lds[1].per_seq, f32[1].per_seq) and torch.equal(lds[1].closing, f32[1].closing)
        pd, pr = pdfs.numpy(), probs.numpy()
        want = (sr.batch(sr.recursions, g, up, lengths, pd, pr, 0.1) if which is None else
                cr.batch(sr.recursions, g, up, lengths, pd, pr, cr.class_map(which, D), 0.1))
    dv = sr.value_dist(f32[1].per_seq.cpu().numpy(), want[0])
    dg = cr.grad_dist(f32[0].grad.cpu().numpy(), want[1], scale)
    closing = float(f32[1].closing.abs().max())
    print("long_row %s %s: E %.3g grad %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (which, dtype, dv, dg, closing, d32, bound))
    record_parity("smbr_general_long_row_%s_%s" % (which or "pdf", str(dtype).split(".")[-1]), value=dv, grad=dg, closing=closing,
                  f32_reference=d32, bound=bound)
    assert dv <= bound and dg <= bound and closing <= bound


# ---- against fp64 beyond the LDS ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("name,which", BEYOND)
def test_against_fp64_beyond_the_lds(name, which, coef):
    c = SHAPES[name]
    case = shape(name)
    (E, G, _), bound, d32, scale = reference(name, which, coef)
    C = 0 if which is None else int(cr.class_map(which, c["D"]).max()) + 1
    L = _lib.lib()
    assert L.pychain_hip_smbr_lds_bytes(c["H"], c["D"], C) > BUDGET           # the default call refuses this shape
    assert L.pychain_hip_smbr_form(c["H"], c["D"], C, AUTO) == c["form"]
    calls = L.pychain_hip_cpu_calls()
    x, acc = _run(case, coef, "auto", which)
    assert L.pychain_hip_cpu_calls() == calls                                 # the kernels, not the host twins
    g = x.grad.cpu().numpy()
    per_seq = acc.per_seq.cpu().numpy()
    dv, dg = sr.value_dist(per_seq, E), cr.grad_dist(g, G, scale)
    rows = float(np.abs(g.astype(np.float64).sum(-1)).max() / scale)
    closing = float(acc.closing.abs().max())
    print("%s %s c=%g: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (name, which, coef, dv, dg, rows, closing, d32, bound))
    record_parity("smbr_general_%s_%s_c%g" % (name, which or "pdf", coef), value=dv, grad=dg, rows=rows, closing=closing,
                  f32_reference=d32, bound=bound)
    assert scale > 0 and (E > 0).all()                                        # the targets name pdfs arcs carry
    assert acc.is_cuda and x.grad.dtype == torch.float32 and acc.per_seq.dtype == torch.float64
    assert abs(float(acc.detach()) - E.sum()) <= bound * abs(E.sum())
    assert dv <= bound and dg <= bound and rows <= bound and closing <= bound
    assert acc.bad_count.tolist() == [0, 0]
    for b, n in enumerate(c["lengths"]):
        assert not g[b, n:].any()                                             # rows beyond a length: exact zeros


def test_a_form_asked_for_by_name_beyond_its_reach_is_refused():
    case = shape("states_beyond")
    x = case[1].to(DEV)
    tg = PosteriorTargets(case[3], case[4])
    with pytest.raises(_lib.PychainHipError, match=r"\(-2\).*rows form.*12000 states"):
        expected_accuracy(x, case[2], case[0], tg, kernels="rows")
    case = shape("refused_today")
    with pytest.raises(_lib.PychainHipError, match=r"\(-2\).*37 states and 10180 pdfs"):      # the default, as it was
        expected_accuracy(case[1].to(DEV), case[2], case[0], PosteriorTargets(case[3], case[4]))


# ---- further cases at those shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", sr.COEFS)
def test_host_twin_against_device_at_c4s_graph(coef):
    case = shape("c4_graph")
    _, bound, _, scale = reference("c4_graph", None, coef)
    x, acc = _run(case, coef, "auto")
    xc, accc = _run(case, coef, "auto", device="cpu")
    dv = sr.value_dist(acc.per_seq.cpu().numpy(), accc.per_seq.numpy())
    dg = cr.grad_dist(x.grad.cpu().numpy(), xc.grad.double().numpy(), scale)
    record_parity("smbr_general_twin_c4_graph_c%g" % coef, value=dv, grad=dg)
    print("c4_graph c=%g: twin against device E %.3g grad %.3g (bound %.3g)" % (coef, dv, dg, bound))
    assert dv <= bound and dg <= bound


@pytest.mark.parametrize("which", [None, "phones"])
def test_two_calls_give_the_same_bits_at_c4s_graph(which):
    case = shape("c4_graph")
    assert _same(_run(case, 1e-5, "auto", which), _run(case, 1e-5, "auto", which))


def test_a_view_off_the_16_byte_grid():
    g, y, lengths, pdfs, probs = shape("refused_today")
    buf = torch.empty(y.numel() + 1, device=DEV)
    view = buf[1:].view(y.shape)
    view.copy_(y)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    tg = PosteriorTargets(pdfs, probs)
    xv = view.requires_grad_(True)
    accv = expected_accuracy(xv, lengths, g, tg, leaky_coefficient=0.1, kernels="auto")
    accv.backward()
    xc = view.detach().clone().requires_grad_(True)
    assert xc.data_ptr() % 16 == 0
    accc = expected_accuracy(xc, lengths, g, tg, leaky_coefficient=0.1, kernels="auto")
    accc.backward()
    assert float(xc.grad.abs().max()) > 0 and _same((xv, accv), (xc, accc))


def test_counts_and_nan():
    case = shape("refused_today")
    g, y, lengths, pdfs, probs = case
    D = y.size(2)
    x, clean = _run(case, 0.1, "auto")
    assert clean.bad_count.tolist() == [0, 0]
    # an entry that names pdf >= D (device targets are not inspected): counted, otherwise ignored
    p2 = pdfs.clone()
    assert int(p2[0, 1, 2]) < 0 and int(lengths[1]) == 1
    p2[0, 1, 2] = D                                                           # (was padding)
    p2[1, 2, 0] = D + 3                                                       # (frame 2 of a sequence of 1: not looked at)
    x2, acc2 = _run(case, 0.1, "auto", pdfs=p2.to(DEV))
    assert acc2.bad_count.tolist() == [0, 1]
    assert torch.equal(acc2.per_seq, clean.per_seq) and torch.equal(x2.grad, x.grad) and torch.equal(acc2.closing, clean.closing)
    # a NaN in a live row, on a pdf no arc carries: that sequence goes bad, the other keeps its bits
    carried = set(g.forward_transitions[:, 2].tolist())
    free = next(n for n in range(5000, D) if n not in carried)                # (beyond the 4096 elements a thread holds in registers)
    y3 = y.clone()
    y3[0, 2, free] = float("nan")
    y3[1, 2, 7] = float("nan")                                                # (beyond the length: not seen)
    x3, acc3 = _run(case, 0.1, "auto", y=y3)
    assert acc3.bad_count.tolist() == [1, 0]
    assert bool(torch.isnan(acc3.per_seq[0])) and bool(torch.isnan(acc3.closing[0]))
    assert torch.equal(acc3.per_seq[1], clean.per_seq[1]) and torch.equal(acc3.closing[1], clean.closing[1])
    assert torch.equal(x3.grad[1], x.grad[1])
