"""Lattice-free sMBR at training lengths and on peaked rows, without a GPU: the host twins through the
Python API on tests/smbr_long_cases - sequences of up to 1500 frames, rows beyond the +-30 clamp, 300 states and 130 pdfs - in the
pdf-level form and under the class maps `identity` and `phones`, against the fp64 recursions, and against the double-backward
autograd evaluation on the sequences of 100 frames or fewer; the graphs of more than 2048 states and the frames of more than 64
target entries that tests/test_gpu_smbr_long.py runs on the device.

Tolerance: smbr_reference.bound, unchanged - 1e-5 on max |d grad| / max |grad| and on the relative error of E_b, or twice the fp32
numpy recursions' own distance where that is beyond 5e-6; the row sums are held to the same bound.  `closing` is the UNCENTRED
diagnostic: it accumulates the rounding of e(t) frame by frame (2e-3 at 1500 frames) and is only required to be finite here; it
is recorded with closing / L.  Every distance goes through helpers.record_parity.

What these tests found.  Before the gradient rows of the pdf-level form were centred by their own mean, the pdf-level twin was
2.9e-2 from fp64 on the 1500 frames of `ladder` at coefficient 0.1 (bound 7.3e-5), 6.4e-3 on `clamp` (bound 2.9e-4), 1.5e-4 on
`mid` (6.1e-5) and 7.6e-5 / 2.1e-4 on `flat` (1e-5): the row-sum error to three digits.  The class forms were 1e-7 from fp64
throughout, as they are now; profiles/smbr_long_parity.md has every figure."""
import numpy as np
import pytest
import torch

import smbr_class_reference as cr
import smbr_long_cases as lc
import smbr_reference as sr
from helpers import record_parity
from pychain_amd import PosteriorTargets, _lib, expected_accuracy

LONG = sorted(lc.LONG_CASES)
SHORT = 100                     # sequences of at most this many frames are evaluated by autograd too
_auto = {}


def _autograd(name, form, coef, b):
    """(E, grad [L,D]) of sequence b by double-backward autograd in fp64, once per process."""
    key = (name, "identity" if form == "pdf" else form, coef, b)
    if key not in _auto:
        g, y, lengths, pdfs, probs = lc.case(name)
        L, cls = int(lengths[b]), lc.class_map(form, y.size(2))
        A = cr.dense_class_accuracy(pdfs.numpy()[b, :L], probs.numpy()[b, :L], cls, int(cls.max()) + 1)
        _auto[key] = sr.autograd(sr.graph_arrays(g), y[b, :L].double().numpy(), A, coef)
    return _auto[key]


def _twin(name, form, coef):
    g, y, lengths, pdfs, probs = lc.case(name)
    x = y.clone().requires_grad_(True)
    calls = _lib.lib().pychain_hip_cpu_calls()
    acc = expected_accuracy(x, lengths, g, PosteriorTargets(pdfs, probs), leaky_coefficient=coef, classes=lc.classes(form, y.size(2)))
    assert _lib.lib().pychain_hip_cpu_calls() > calls
    acc.backward()
    return x.grad, acc


@pytest.mark.parametrize("coef", lc.COEFS)
@pytest.mark.parametrize("form", ["pdf", "phones"])
@pytest.mark.parametrize("name", LONG)
def test_the_reference_is_usable(name, form, coef):
    """The expected accuracy is neither negligible nor saturated and the gradient is not rounding noise.  The window on E_b / L_b
    is for the cases whose reference is an alignment of the rows (ladder, clamp, mid: 0.50 to 0.83 measured).  The reference of
    `flat` is random by construction - E_b / L_b is the mean credit of a pdf, sum q / D = 0.037 whatever the rows (0.11 by
    class) -, so there the window cannot hold and the gradient alone is required: max |grad| = 0.36."""
    (E, G, _), _, scale = lc.reference(name, form, coef)
    lengths = lc.case(name)[2].numpy()
    print("%s %s c=%g: E/L %s max |grad| %.3g" % (name, form, coef, np.round(E / lengths, 3).tolist(), scale))
    assert scale > 1e-3 and (E > 0).all()
    if name != "flat":
        assert ((E / lengths > 0.3) & (E / lengths < 0.95)).all()
    for b, L in enumerate(lengths.tolist()):
        assert np.abs(G[b, :L]).max() > 1e-3 and not G[b, L:].any()


@pytest.mark.parametrize("coef", lc.COEFS)
@pytest.mark.parametrize("form", ["pdf", "phones"])
@pytest.mark.parametrize("name", ["ladder", "mid"])                            # (`clamp` and `flat` have no short sequence)
def test_the_two_references_agree_on_the_short_sequences(name, form, coef):
    """1e-10: five orders inside the tightest bound of the tests, so either evaluation is the same reference.  (1e-12 on the 17
    Gaussian frames of smbr_reference.CASES; fp64 carries 100 peaked frames a little less well.)"""
    (E, G, _), _, _ = lc.reference(name, form, coef)
    short = [b for b, L in enumerate(lc.case(name)[2].tolist()) if L <= SHORT]
    assert short
    for b in short:
        Ea, Ga = _autograd(name, form, coef, b)
        L = Ga.shape[0]
        d = sr.grad_dist(G[b, :L], Ga)
        print("%s %s c=%g, sequence %d (%d frames): E %.3g grad %.3g" % (name, form, coef, b, L, abs(E[b] - Ea) / abs(Ea), d))
        assert abs(E[b] - Ea) <= 1e-10 * abs(Ea) and d <= 1e-10


@pytest.mark.parametrize("coef", lc.COEFS)
@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("name", LONG)
def test_host_twin_against_fp64(name, form, coef):
    ref, (bound, d32), scale = lc.reference(name, form, coef)
    lengths = lc.case(name)[2].tolist()
    grad, acc = _twin(name, form, coef)
    g = grad.numpy()
    (dv, dg, rows), seqs = lc.distances(acc.per_seq.numpy(), g, ref)
    closing = acc.closing.double().abs().numpy()
    print("%s %s c=%g: E %.3g grad %.3g rows %.3g (fp32 reference %.3g, bound %.3g)" % (name, form, coef, dv, dg, rows, d32, bound))
    record_parity("smbr_long_cpu_%s_%s_c%g" % (name, form, coef), value=dv, grad=dg, rows=rows, f32_reference=d32, bound=bound,
                  closing=closing.max(), closing_per_frame=(closing / np.asarray(lengths)).max())
    own = lc.per_sequence(name, form, coef) if name == "ladder" else None
    for b, L in enumerate(lengths):
        print("  sequence %d, %d frames: E %.3g grad %.3g rows %.3g closing %.3g (%.3g a frame)%s" % (
            (b, L) + seqs[b] + (closing[b], closing[b] / L, " own bound %.3g" % own[b][0] if own else "")))
        record_parity("smbr_long_cpu_%s_%s_c%g_L%d" % (name, form, coef, L), value=seqs[b][0], grad=seqs[b][1], rows=seqs[b][2],
                      closing=closing[b], closing_per_frame=closing[b] / L, **(dict(bound=own[b][0], f32_reference=own[b][1]) if own else {}))
    assert grad.dtype == torch.float32 and acc.per_seq.dtype == torch.float64
    assert abs(float(acc.detach()) - ref[0].sum()) <= bound * abs(ref[0].sum())
    assert dv <= bound and dg <= bound and rows <= bound
    assert np.isfinite(closing).all()                          # the uncentred diagnostic: not bounded at length (module docstring)
    assert acc.bad_count.tolist() == [0, 0]
    for b, L in enumerate(lengths):
        assert not g[b, L:].any()                              # rows beyond a length: exact zeros
        if own:                                                # the ladder: every length against a bound of its own too
            assert max(seqs[b]) <= own[b][0]
        if L <= SHORT:                                         # nothing hand-derived: the autograd evaluation
            Ea, Ga = _autograd(name, form, coef, b)
            assert abs(float(acc.per_seq[b]) - Ea) <= bound * abs(Ea)
            assert np.abs(g[b, :L].astype(np.float64) - Ga).max() <= bound * scale


@pytest.mark.parametrize("form", ["pdf", "phones"])
@pytest.mark.parametrize("name", sorted(lc.WIDE_CASES) + sorted(lc.MANY_CASES))
def test_host_twin_on_the_shapes_of_the_device_tests(name, form):
    """More than 2048 states; more than 64 target entries a frame with repeats and padding among them.  (The fp32 numpy
    recursions are within 5e-6 of fp64 on all of them here, so the rule gives the project's 1e-5.)"""
    c = lc.WIDE_CASES.get(name) or lc.MANY_CASES[name]
    for coef in ([c["coef"]] if "coef" in c else lc.COEFS):
        ref, (bound, d32), scale = lc.reference(name, form, coef)
        grad, acc = _twin(name, form, coef)
        (dv, dg, rows), _ = lc.distances(acc.per_seq.numpy(), grad.numpy(), ref)
        closing = float(acc.closing.abs().max())
        print("%s %s c=%g: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (name, form, coef, dv, dg, rows, closing, d32, bound))
        record_parity("smbr_long_cpu_%s_%s_c%g" % (name, form, coef), value=dv, grad=dg, rows=rows, closing=closing, f32_reference=d32, bound=bound)
        assert scale > 1e-3 and (ref[0] > 0).all()
        assert dv <= bound and dg <= bound and rows <= bound and closing <= bound
        assert acc.bad_count.tolist() == [0, 0]
        for b, L in enumerate(lc.case(name)[2].tolist()):
            assert not grad[b, L:].any()


def test_the_many_entry_cases_hold_what_they_are_for():
    for name, c in lc.MANY_CASES.items():
        pdfs = lc.case(name)[3].numpy()
        Kt = c["Kt"]
        assert pdfs.shape[2] == Kt > 64
        live = pdfs[0, :c["lengths"][0]]
        assert (live[:, :64] < 0).any() and (live[:, 64:] < 0).any()              # padding in both chunks of a wave
        assert (live[3:, 66] == live[3:, 1]).all() and (live[:, 1] >= 0).all()     # a repeat across the chunks
        assert (live[1::2, Kt - 1] == live[1::2, 0]).all() and (live[:, 0] >= 0).all()
        assert (live[2, 64:] < 0).all() and (live[3, 64:] >= 0).any()
