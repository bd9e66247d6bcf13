"""Lattice-free sMBR (csrc/smbr.hip) on the MI355X where the cases of tests/test_gpu_smbr*.py stop: the long
and peaked cases of tests/smbr_long_cases (up to 1500 frames, rows beyond the +-30 clamp) at leaky coefficients 0.1 and 1e-5,
pdf-level and under the class map `phones`, against the fp64 recursions and against the host twin; bf16 and fp16 rows beyond
the clamp; the same bits twice, with the cached workspace grown and reused in between; graphs of more than 2048 states (three
states per recursion thread, up to six per gradient thread); frames of more than 64 target entries, with repeats and padding
among them, as pdf targets and as class targets.

Tolerance: smbr_reference.bound, unchanged - 1e-5 on max |d grad| / max |grad| and on the relative error of E_b, or twice the fp32
numpy recursions' own distance where that is beyond 5e-6; the row sums are held to the same bound.  `closing`, the uncentred
diagnostic, grows with the length (tests/test_smbr_long.py) and is only required to be finite on the long cases; it is recorded
with closing / L.  Every test checks that no host twin ran in place of a kernel, bad_count == [0, 0], and exact zeros beyond
each length.  Every distance goes through helpers.record_parity; profiles/smbr_long_parity.md has them."""
import numpy as np
import pytest
import torch

import smbr_class_reference as cr
import smbr_long_cases as lc
import smbr_reference as sr
from helpers import record_parity
from pychain_amd import PosteriorTargets, _lib, expected_accuracy

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
LONG = sorted(lc.LONG_CASES)


def _run(case, form, coef, dtype=torch.float32, device=DEV, y=None, targets=None, **kw):
    """One call on `device` and its backward: (grad, acc).  On the GPU no host twin may run."""
    g, y0, lengths, pdfs, probs = case
    x = (y0 if y is None else y).detach().clone().to(device=device, dtype=dtype).requires_grad_(True)     # (a leaf of its own)
    calls = _lib.lib().pychain_hip_cpu_calls()
    acc = expected_accuracy(x, lengths, g, targets or PosteriorTargets(pdfs, probs), leaky_coefficient=coef,
                            classes=lc.classes(form, y0.size(2)), **kw)
    acc.backward()
    if device != "cpu":
        assert _lib.lib().pychain_hip_cpu_calls() == calls                    # the kernels, not the host twins
    return x.grad, acc


def _clean(case, grad, acc):
    """what every call on clean inputs must show"""
    assert acc.bad_count.tolist() == [0, 0]
    g = grad.float().cpu().numpy()
    for b, L in enumerate(case[2].tolist()):
        assert not g[b, L:].any()                                             # rows beyond a length: exact zeros
    return g


def _against_fp64(tag, name, form, coef, closing_bounded):
    """the device call of a case against fp64, recorded and held to the bound; returns (grad, acc, bound, scale)"""
    case = lc.case(name)
    ref, (bound, d32), scale = lc.reference(name, form, coef)
    lengths = case[2].tolist()
    grad, acc = _run(case, form, coef)
    g = _clean(case, grad, acc)
    (dv, dg, rows), seqs = lc.distances(acc.per_seq.cpu().numpy(), g, ref)
    closing = acc.closing.double().abs().cpu().numpy()
    print("%s %s c=%g: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (name, form, coef, dv, dg, rows, closing.max(), d32, bound))
    record_parity("%s_%s_%s_c%g" % (tag, name, form, coef), value=dv, grad=dg, rows=rows, f32_reference=d32, bound=bound,
                  closing=closing.max(), closing_per_frame=(closing / np.asarray(lengths)).max())
    own = lc.per_sequence(name, form, coef) if name == "ladder" else None
    if name in lc.LONG_CASES:
        for b, L in enumerate(lengths):
            print("  sequence %d, %d frames: E %.3g grad %.3g rows %.3g closing %.3g (%.3g a frame)%s" % (
                (b, L) + seqs[b] + (closing[b], closing[b] / L, " own bound %.3g" % own[b][0] if own else "")))
            record_parity("%s_%s_%s_c%g_L%d" % (tag, name, form, coef, L), value=seqs[b][0], grad=seqs[b][1], rows=seqs[b][2], closing=closing[b],
                          closing_per_frame=closing[b] / L, **(dict(bound=own[b][0], f32_reference=own[b][1]) if own else {}))
    assert acc.is_cuda and acc.dtype == torch.float32 and acc.per_seq.dtype == torch.float64 and grad.dtype == torch.float32
    assert abs(float(acc.detach()) - ref[0].sum()) <= bound * abs(ref[0].sum())
    assert dv <= bound and dg <= bound and rows <= bound
    assert np.isfinite(closing).all() and (not closing_bounded or closing.max() <= bound)
    if own:                                                                   # the ladder: every length against a bound of its own too
        for b in range(len(lengths)):
            assert max(seqs[b]) <= own[b][0]
    return grad, acc, bound, scale


def _against_the_twin(tag, name, form, coef, grad, acc, bound, scale):
    case = lc.case(name)
    gc, accc = _run(case, form, coef, device="cpu")
    dv = sr.value_dist(acc.per_seq.cpu().numpy(), accc.per_seq.numpy())
    dg = cr.grad_dist(grad.cpu().numpy(), gc.double().numpy(), scale)
    print("%s %s c=%g: twin against device E %.3g grad %.3g (bound %.3g)" % (name, form, coef, dv, dg, bound))
    record_parity("%s_twin_%s_%s_c%g" % (tag, name, form, coef), value=dv, grad=dg, bound=bound)
    assert dv <= bound and dg <= bound


@pytest.mark.parametrize("coef", lc.COEFS)
@pytest.mark.parametrize("form", ["pdf", "phones"])
@pytest.mark.parametrize("name", LONG)
def test_long_cases_against_fp64(name, form, coef):
    _against_fp64("smbr_long_gpu", name, form, coef, closing_bounded=False)


@pytest.mark.parametrize("coef", lc.COEFS)
@pytest.mark.parametrize("form", ["pdf", "phones"])
@pytest.mark.parametrize("name", LONG)
def test_host_twin_against_device(name, form, coef):
    case = lc.case(name)
    _, (bound, _), scale = lc.reference(name, form, coef)
    grad, acc = _run(case, form, coef)
    _clean(case, grad, acc)
    _against_the_twin("smbr_long_gpu", name, form, coef, grad, acc, bound, scale)


@pytest.mark.parametrize("coef", lc.COEFS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("form", ["pdf", "phones"])
def test_two_byte_rows_beyond_the_clamp(form, dtype, coef):
    case = lc.case("clamp")
    gh, acch = _run(case, form, coef, dtype=dtype)
    up = case[1].to(dtype).float()
    assert float(up.max()) > 30.0 and float(up.min()) < -30.0                 # both sides of the clamp survive the rounding
    gf, accf = _run(case, form, coef, y=up)
    _clean(case, gh, acch), _clean(case, gf, accf)
    assert gh.dtype == dtype and gf.dtype == torch.float32
    assert torch.equal(gh, gf.to(dtype))                                      # the fp32 call on the up-cast input, rounded once
    assert torch.equal(acch.per_seq, accf.per_seq) and torch.equal(acch.closing, accf.closing)
    ref, (bound, d32), _ = lc.reference("clamp", form, coef, y=up)            # fp64 on the up-cast input
    (dv, dg, rows), _ = lc.distances(accf.per_seq.cpu().numpy(), gf.cpu().numpy(), ref)
    tag = "smbr_long_gpu_%s_clamp_%s_c%g" % (str(dtype).split(".")[1], form, coef)
    print("%s: E %.3g grad %.3g rows %.3g (fp32 reference %.3g, bound %.3g)" % (tag, dv, dg, rows, d32, bound))
    record_parity(tag, value=dv, grad=dg, rows=rows, f32_reference=d32, bound=bound)
    assert dv <= bound and dg <= bound and rows <= bound


@pytest.mark.parametrize("form", ["pdf", "phones"])
def test_the_same_bits_twice_over_a_workspace_that_grew(form):
    small = sr.case("small") if form == "pdf" else cr.case("small")
    ladder = lc.case("ladder")
    same = lambda p, q: torch.equal(p[0], q[0]) and torch.equal(p[1].per_seq, q[1].per_seq) and torch.equal(p[1].closing, q[1].closing)
    s1 = _run(small, form, 1e-5)
    l1 = _run(ladder, form, 1e-5)                                             # (88 times the frames of `small`: the cached workspace grows)
    l2 = _run(ladder, form, 1e-5)
    s2 = _run(small, form, 1e-5)                                              # (... and is reused, larger than the call needs)
    assert same(l1, l2) and same(s1, s2)
    _clean(ladder, *l1), _clean(ladder, *l2)
    assert s2[1].bad_count.tolist() == [0, 0]
    (_, G, _), (bound, _) = sr.reference("small", 1e-5) if form == "pdf" else cr.reference("small", "phones", 1e-5)[:2]
    assert sr.grad_dist(s2[0].cpu().numpy(), G) <= bound                      # (and they are the right bits)


@pytest.mark.parametrize("form", ["pdf", "phones"])
@pytest.mark.parametrize("name", sorted(lc.WIDE_CASES))
def test_three_states_per_thread(name, form):
    coef = lc.WIDE_CASES[name]["coef"]
    assert lc.WIDE_CASES[name]["H"] > 2 * 1024
    grad, acc, bound, scale = _against_fp64("smbr_long_gpu", name, form, coef, closing_bounded=True)
    assert scale > 1e-3
    _against_the_twin("smbr_long_gpu", name, form, coef, grad, acc, bound, scale)


@pytest.mark.parametrize("coef", lc.COEFS)
@pytest.mark.parametrize("name", sorted(lc.MANY_CASES))
def test_more_than_64_target_entries_a_frame(name, coef):
    case = lc.case(name)
    g, y, lengths, pdfs, probs = case
    assert pdfs.size(2) > 64
    for form in ("pdf", "phones"):
        grad, acc, bound, scale = _against_fp64("smbr_long_gpu", name, form, coef, closing_bounded=True)
        assert scale > 1e-3
        _against_the_twin("smbr_long_gpu", name, form, coef, grad, acc, bound, scale)
    # class-id targets: the bits of the pdf targets (`grad`, `acc`: the call under `phones`)
    tc = PosteriorTargets(pdfs, probs).to_classes(lc.classes("phones", y.size(2)))
    gc, accc = _run(case, "phones", coef, targets=tc, targets_are_classes=True)
    _clean(case, gc, accc)
    assert torch.equal(grad, gc) and torch.equal(acc.per_seq, accc.per_seq) and torch.equal(acc.closing, accc.closing)
