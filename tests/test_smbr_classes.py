"""Lattice-free sMBR with the accuracy by class (include/pychain_hip.h: pychain_hip_smbr_*_classes) without a GPU:
the two fp64 evaluations of tests/smbr_reference on the class-level rows against each other, the planted faults, and the host
twins through the Python API against fp64 for every case x map x coefficient - value, gradient, row sums, `closing`; the identity
map against the pdf-level call; one class; class targets bit for bit; `classes=None` bit for bit; `bad_count` under both kinds
of ids; SMBRLoss; every refusal; ABI 28.

Tolerance (smbr_class_reference.reference): 1e-5 on max |d grad| / max |grad| and on the relative error of E_b, or twice the fp32
numpy recursions' own distance where that is beyond 5e-6; the row sums and `closing` are held to the same bound.  Under the map
`one` the gradient is zero and the distances are relative to max |grad| of the pdf-level reference.

Measured on these cases: the fp64 recursions against fp64 autograd 1.3e-14 or less; the fp32 numpy recursions 5e-9 to 1.5e-6 from
fp64, so every bound is 1e-5; under `one` the fp32 numpy gradient is up to 1.5e-6 of the pdf-level one and the host twin's up to
6e-7.  A table made from the first entry of a class only moves the gradient by 0.53 to 0.92 of max |grad|, pdf-level credit
where class credit is due by 0.55 to 1.06 - at least 52 000 bounds."""
import os
import re

import numpy as np
import pytest
import torch

import smbr_class_reference as cr
import smbr_reference as sr
from helpers import record_parity
from pychain_amd import PosteriorTargets, SMBRLoss, _lib, expected_accuracy, native
from pychain_amd.loss import occupancies

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(sr.CASES)


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("which", cr.MAPS)
@pytest.mark.parametrize("name", NAMES)
def test_the_two_references_agree(name, which, coef):
    g, y, lengths, pdfs, probs = cr.case(name)
    cls = cr.class_map(which, y.size(2))
    (E, G, closing), _, scale = cr.reference(name, which, coef)
    E2, G2, _ = cr.batch(sr.autograd, g, y, lengths, pdfs.numpy(), probs.numpy(), cls, coef)
    dv, dg = float(np.abs(E - E2).max() / max(1.0, np.abs(E2).max())), cr.grad_dist(G, G2, scale)
    print("%s %s c=%g: recursions against autograd E %.3g grad %.3g" % (name, which, coef, dv, dg))
    assert dv <= 1e-12 and dg <= 1e-12
    assert np.abs(closing).max() <= 1e-12 and np.abs(G.sum(-1)).max() <= 1e-12 * scale
    assert E[-1] == 0.0 and not G[-1].any()                    # the utterance without targets
    if which == "one":                                         # one class: every path scores sum q, nothing to learn
        want = np.array([float(probs[b, :L][pdfs[b, :L] >= 0].double().sum()) for b, L in enumerate(lengths.tolist())])
        assert np.abs(E - want).max() <= 1e-12 * want.max() and np.abs(G).max() <= 1e-12 * scale


@pytest.mark.parametrize("fault", cr.FAULTS)
@pytest.mark.parametrize("name", NAMES)
def test_the_cases_see_a_planted_fault(name, fault):
    g, y, lengths, pdfs, probs = cr.case(name)
    cls = cr.class_map("phones", y.size(2))
    (_, G, _), (bound, _), scale = cr.reference(name, "phones", 0.1)
    Gf = cr.batch(sr.recursions, g, y, lengths, pdfs.numpy(), probs.numpy(), cls, 0.1, fault=fault)[1]
    moved = cr.grad_dist(Gf, G, scale)
    print("%s %s: moves the gradient by %.3g, bound %.3g" % (name, fault, moved, bound))
    assert moved > 100.0 * bound


def _call(name, which, coef, device="cpu", dtype=torch.float32, y=None, targets=None, **kw):
    g, y0, lengths, pdfs, probs = cr.case(name)
    x = (y0 if y is None else y).detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    classes = None if which is None else cr.classes(which, y0.size(2))
    acc = expected_accuracy(x, lengths, g, targets or PosteriorTargets(pdfs, probs), leaky_coefficient=coef, classes=classes, **kw)
    acc.backward()
    return x, acc


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("which", cr.MAPS)
@pytest.mark.parametrize("name", NAMES)
def test_host_twin_against_fp64(name, which, coef):
    (E, G, _), (bound, d32), scale = cr.reference(name, which, coef)
    calls = _lib.lib().pychain_hip_cpu_calls()
    x, acc = _call(name, which, coef)
    assert _lib.lib().pychain_hip_cpu_calls() > calls
    g = x.grad.numpy()
    dv, dg = sr.value_dist(acc.per_seq.numpy(), E), cr.grad_dist(g, G, scale)
    rows = float(np.abs(g.astype(np.float64).sum(-1)).max() / scale)
    closing = float(acc.closing.abs().max())
    print("%s %s c=%g: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (name, which, coef, dv, dg, rows, closing, d32, bound))
    record_parity("smbr_classes_cpu_%s_%s_c%g" % (name, which, coef), value=dv, grad=dg, rows=rows, closing=closing, f32_reference=d32)
    assert acc.dtype == torch.float32 and acc.per_seq.dtype == torch.float64 and x.grad.dtype == torch.float32
    assert abs(float(acc.detach()) - E.sum()) <= bound * abs(E.sum())
    assert dv <= bound and dg <= bound and rows <= bound and closing <= bound
    assert acc.bad_count.tolist() == [0, 0]
    assert float(acc.per_seq[-1]) == 0.0 and not bool(x.grad[-1].any())          # no targets: exactly nothing
    for b, L in enumerate(cr.case(name)[2].tolist()):
        assert not bool(x.grad[b, L:].any())
    if name == "degenerate":
        assert not bool(x.grad[:, :, 8].any())                                   # the pdf no arc carries, in a class that is credited


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("name", NAMES)
def test_identity_is_the_pdf_level_call(name, coef):
    _, (bound, _), scale = cr.reference(name, "identity", coef)
    x, acc = _call(name, "identity", coef)
    xp, accp = _call(name, None, coef)
    dv, dg = sr.value_dist(acc.per_seq.numpy(), accp.per_seq.numpy()), cr.grad_dist(x.grad.numpy(), xp.grad.double().numpy(), scale)
    print("%s c=%g: identity map against the pdf-level call E %.3g grad %.3g (bound %.3g)" % (name, coef, dv, dg, bound))
    assert dv <= 2.0 * bound and dg <= 2.0 * bound


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("name", NAMES)
def test_one_class(name, coef):
    g, y, lengths, pdfs, probs = cr.case(name)
    (E, G, _), (bound, d32), scale = cr.reference(name, "one", coef)
    x, acc = _call(name, "one", coef)
    want = np.array([float(probs[b, :L][pdfs[b, :L] >= 0].double().sum()) for b, L in enumerate(lengths.tolist())])
    ratio = float(x.grad.abs().max()) / scale                  # against max |grad| of the pdf-level reference
    print("%s c=%g: one class, E %.3g from sum q, max |grad| %.3g of the pdf-level one (fp32 numpy %.3g)" % (
        name, coef, sr.value_dist(acc.per_seq.numpy(), want), ratio, d32))
    assert sr.value_dist(acc.per_seq.numpy(), want) <= bound
    assert ratio <= max(1e-5, 2.0 * float(np.abs(cr.batch(sr.recursions, g, y, lengths, pdfs.numpy(), probs.numpy(), cr.class_map("one", y.size(2)),
                                                            coef, dtype=np.float32)[1]).max()) / scale)


@pytest.mark.parametrize("which", ["phones", "one"])
@pytest.mark.parametrize("name", ["small", "degenerate"])
def test_class_targets_give_the_bits_of_pdf_targets(name, which):
    g, y, lengths, pdfs, probs = cr.case(name)
    tc = PosteriorTargets(pdfs, probs).to_classes(cr.classes(which, y.size(2)))
    assert torch.equal(tc.pdfs < 0, pdfs < 0) and tc.pdfs.dtype == torch.int32 and tc.probs is not None
    x, acc = _call(name, which, 0.1)
    xc, accc = _call(name, which, 0.1, targets=tc, targets_are_classes=True)
    assert torch.equal(x.grad, xc.grad) and torch.equal(acc.per_seq, accc.per_seq) and torch.equal(acc.closing, accc.closing)
    assert accc.bad_count.tolist() == [0, 0]


@pytest.mark.parametrize("name", ["small", "wide"])
def test_without_classes_it_is_the_call_it_was(name):
    g, y, lengths, pdfs, probs = cr.case(name)
    x, acc = _call(name, None, 0.1)
    gt = native.smbr_graph(g, y.size(2), torch.device("cpu"))
    gamma = occupancies(y, lengths, g, 0.1)                                                      # (what expected_accuracy hands the twins)
    was = native.cpu_smbr(gt, g.num_states, y, lengths, gamma, pdfs, probs, 0.1)                  # (positional: the call of ABI 27)
    assert torch.equal(acc.per_seq, was[0]) and torch.equal(x.grad, was[1]) and torch.equal(acc.closing, was[3])
    # the class entry points with a null map forward to the pdf-level ones
    L = _lib.lib()
    lc = lengths.to(torch.int64)
    B, T, D = y.shape
    facc, facc2 = torch.zeros(B, T), torch.zeros(B, T)
    acc1, acc2 = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    bad = torch.zeros(2, dtype=torch.int32)
    head = lambda f, a: (gamma.data_ptr(), lc.data_ptr(), B, T, D, pdfs.data_ptr(), probs.data_ptr(), 2, f.data_ptr(), a.data_ptr(), bad.data_ptr(), 1)
    assert L.pychain_hip_cpu_smbr_frame_accuracy(*head(facc, acc1)) == 0
    assert L.pychain_hip_cpu_smbr_frame_accuracy_classes(*head(facc2, acc2), None, 0, 0) == 0
    assert torch.equal(facc, facc2) and torch.equal(acc1, acc2) and torch.equal(acc1, was[0])
    g1, g2, c1, c2 = torch.zeros(B, T, D), torch.zeros(B, T, D), torch.zeros(B), torch.zeros(B)
    body = lambda gr, a, c: (*[t.data_ptr() for t in gt], g.num_states, g.num_transitions, y.data_ptr(), lc.data_ptr(), B, T, D, pdfs.data_ptr(),
                             probs.data_ptr(), 2, facc.data_ptr(), 0.1, 1.0, None, gr.data_ptr(), a.data_ptr(), c.data_ptr(), bad.data_ptr(), 1)
    assert L.pychain_hip_cpu_smbr_forward_backward(*body(g1, acc1, c1)) == 0
    assert L.pychain_hip_cpu_smbr_forward_backward_classes(*body(g2, acc2, c2), None, 0, 0) == 0
    assert torch.equal(g1, g2) and torch.equal(c1, c2) and torch.equal(g1, was[1])


def test_bad_count_under_both_kinds_of_ids():
    g, y, lengths, pdfs, probs = cr.case("small")
    D = y.size(2)
    classes = cr.classes("phones", D)
    C = int(classes.max()) + 1
    x, clean = _call("small", "phones", 0.1)
    # pdf targets: >= D is out of range - C <= id < D is a pdf like any other
    p2 = pdfs.clone()
    assert int(p2[0, 5, 1]) < 0
    p2[0, 5, 1] = D                                            # (was padding)
    p2[1, 12, 0] = D + 3                                       # (frame 12 of a sequence of 9: not looked at)
    gt = native.smbr_graph(g, D, torch.device("cpu"))
    gamma = occupancies(y, lengths, g, 0.1)
    got = native.cpu_smbr(gt, g.num_states, y, lengths, gamma, p2, probs, 0.1, classes=classes, num_classes=C)
    assert got[2].tolist() == [0, 1] and torch.equal(got[0], clean.per_seq) and torch.equal(got[1], x.grad)
    # class targets: >= C is out of range; to_classes leaves an out-of-range pdf out of range
    tc = PosteriorTargets._of(p2, probs).to_classes(classes)
    assert int(tc.pdfs[0, 5, 1]) >= C and int(tc.pdfs.max()) >= C
    got = native.cpu_smbr(gt, g.num_states, y, lengths, gamma, tc.pdfs, probs, 0.1, classes=classes, num_classes=C, targets_are_classes=True)
    assert got[2].tolist() == [0, 1] and torch.equal(got[0], clean.per_seq) and torch.equal(got[1], x.grad)
    c2 = tc.pdfs.clone()
    assert int(c2[0, 2, 0]) < 0 and int(p2[0, 5, 1]) == D and C < D
    c2[0, 2, 0] = C                                            # (was padding) an id a pdf could have: as a class out of range
    got = native.cpu_smbr(gt, g.num_states, y, lengths, gamma, c2, probs, 0.1, classes=classes, num_classes=C, targets_are_classes=True)
    assert got[2].tolist() == [0, 2] and torch.equal(got[0], clean.per_seq) and torch.equal(got[1], x.grad)
    # a NaN in a live row: that sequence's E is NaN, the others are untouched
    y2 = y.clone()
    y2[1, 3, 5] = float("nan")
    got = native.cpu_smbr(gt, g.num_states, y2, lengths, gamma, pdfs, probs, 0.1, classes=classes, num_classes=C)
    assert got[2].tolist() == [1, 0] and bool(torch.isnan(got[0][1])) and bool(torch.isnan(got[3][1]))
    keep = [0, 2, 3]
    assert torch.equal(got[0][keep], clean.per_seq[keep]) and torch.equal(got[1][keep], x.grad[keep])


@pytest.mark.parametrize("avg", [True, False])
def test_loss_with_classes_avg_and_upstream_gradient(avg):
    g, y, lengths, pdfs, probs = cr.case("small")
    (E, G, _), (bound, _), scale = cr.reference("small", "phones", 0.1)
    classes = cr.classes("phones", y.size(2))
    x = y.clone().requires_grad_(True)
    loss = SMBRLoss(g, leaky_coefficient=0.1, avg=avg, classes=classes)(x, lengths, PosteriorTargets(pdfs, probs))
    (2.5 * loss).backward()
    norm = float(lengths.sum()) if avg else 1.0
    assert abs(float(loss.detach()) + E.sum() / norm) <= bound * abs(E.sum() / norm)
    assert cr.grad_dist(x.grad.numpy(), -2.5 * G / norm, 2.5 * scale / norm) <= bound
    assert loss.per_seq.shape == (4,) and loss.bad_count.tolist() == [0, 0] and loss.closing.shape == (4,)
    # class targets through the module
    x2 = y.clone().requires_grad_(True)
    loss2 = SMBRLoss(g, leaky_coefficient=0.1, avg=avg, classes=classes)(x2, lengths, PosteriorTargets(pdfs, probs).to_classes(classes),
                                                                          targets_are_classes=True)
    (2.5 * loss2).backward()
    assert torch.equal(loss2, loss) and torch.equal(x2.grad, x.grad)


def test_the_device_copy_of_the_map_is_cached():
    classes = cr.classes("phones", 23)
    a, C = native.smbr_classes(classes, 23, torch.device("cpu"))
    assert C == 8 and a.dtype == torch.int32 and native.smbr_classes(classes, 23, torch.device("cpu"))[0] is a
    classes[0] = 0                                             # an in-place edit: made again
    assert native.smbr_classes(classes, 23, torch.device("cpu"))[0] is not a
    b, C = native.smbr_classes(cr.class_map("one", 23), 23, torch.device("cpu"))       # (a numpy array, int64)
    assert C == 1 and b.dtype == torch.int32


def test_refusals():
    g, y, lengths, pdfs, probs = cr.case("small")
    tg = PosteriorTargets(pdfs, probs)
    D = y.size(2)
    classes = cr.classes("phones", D)
    C = int(classes.max()) + 1
    with pytest.raises(ValueError, match=r"classes must be \[D\]"):
        expected_accuracy(y, lengths, g, tg, classes=classes[:-1])
    with pytest.raises(ValueError, match=r"classes must be \[D\]"):
        expected_accuracy(y, lengths, g, tg, classes=classes.view(1, -1))
    neg = classes.clone()
    neg[3] = -1
    with pytest.raises(ValueError, match="negative"):
        expected_accuracy(y, lengths, g, tg, classes=neg)
    with pytest.raises(ValueError, match="integer"):
        expected_accuracy(y, lengths, g, tg, classes=classes.float())
    with pytest.raises(ValueError, match="integer"):
        expected_accuracy(y, lengths, g, tg, classes=classes > 0)
    with pytest.raises(ValueError, match="targets_are_classes needs"):
        expected_accuracy(y, lengths, g, tg, targets_are_classes=True)
    with pytest.raises(ValueError, match="targets_are_classes needs"):
        SMBRLoss(g)(y, lengths, tg, targets_are_classes=True)
    with pytest.raises(TypeError):                             # keyword arguments
        expected_accuracy(y, lengths, g, tg, 1e-5, classes)
    # class targets are held against C, pdf targets against D
    assert int(pdfs.max()) >= C
    with pytest.raises(ValueError, match="name pdf"):
        expected_accuracy(y, lengths, g, tg, classes=classes, targets_are_classes=True)
    p2 = pdfs.clone()
    p2[0, 0, 0] = D
    with pytest.raises(ValueError, match="name pdf"):
        expected_accuracy(y, lengths, g, PosteriorTargets(p2, probs), classes=classes)
    with pytest.raises(ValueError, match="integer"):
        tg.to_classes(classes.float())
    # the C ABI
    L = _lib.lib()
    gt = native.smbr_graph(g, D, torch.device("cpu"))
    lc = lengths.to(torch.int64)
    gamma, facc = torch.zeros(4, 17, D), torch.zeros(4, 17)
    acc, closing, bad, grad = torch.zeros(4, dtype=torch.float64), torch.zeros(4), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 17, D)
    fa = lambda cp, c, tc: L.pychain_hip_cpu_smbr_frame_accuracy_classes(gamma.data_ptr(), lc.data_ptr(), 4, 17, D, pdfs.data_ptr(), probs.data_ptr(), 2,
                                                                         facc.data_ptr(), acc.data_ptr(), bad.data_ptr(), 1, cp, c, tc)
    assert fa(classes.data_ptr(), 0, 0) == -1 and "num_classes" in L.pychain_hip_last_error().decode()
    assert fa(None, C, 1) == -1 and "targets_are_classes" in L.pychain_hip_last_error().decode()
    assert fa(classes.data_ptr(), C, 0) == 0 and fa(classes.data_ptr(), C, 1) == 0
    fb = lambda cp, c, tc: L.pychain_hip_cpu_smbr_forward_backward_classes(
        *[t.data_ptr() for t in gt], 37, 150, y.data_ptr(), lc.data_ptr(), 4, 17, D, pdfs.data_ptr(), probs.data_ptr(), 2,
        facc.data_ptr(), 0.1, 1.0, None, grad.data_ptr(), acc.data_ptr(), closing.data_ptr(), bad.data_ptr(), 1, cp, c, tc)
    assert fb(classes.data_ptr(), -2, 0) == -1 and fb(None, 0, 1) == -1 and fb(classes.data_ptr(), C, 0) == 0
    # the device entry points refuse before the device is touched
    assert L.pychain_hip_smbr_frame_accuracy_classes(None, None, 4, 17, D, None, None, 2, None, None, None, None, classes.data_ptr(), C, 0, None, 0) == -1
    assert L.pychain_hip_smbr_frame_accuracy_classes(None, None, 4, 17, D, None, None, 2, None, None, None, None, None, 0, 1, None, 0) == -1
    assert "targets_are_classes" in L.pychain_hip_last_error().decode()
    assert L.pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(0, 5) == 0
    assert L.pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(3, 5) >= 8 * 15


def test_the_lds_query():
    L = _lib.lib()
    assert L.pychain_hip_smbr_lds_bytes(0, 5, 0) == 0 and L.pychain_hip_smbr_lds_bytes(5, 5, -1) == 0
    # the pdf-level form: the edge the existing refusal sits on (tests/test_gpu_smbr.py: D = 10160 runs, 10180 is refused)
    assert L.pychain_hip_smbr_lds_bytes(37, 10160, 0) <= 160 * 1024 < L.pychain_hip_smbr_lds_bytes(37, 10180, 0)
    assert L.pychain_hip_smbr_lds_bytes(3000, 3456, 0) == (4 * 3000 + 4 * 3456 + 128) * 4
    # a class table is one float a class
    for C in (1, 40, 3456):
        assert L.pychain_hip_smbr_lds_bytes(3000, 3456, C) == L.pychain_hip_smbr_lds_bytes(3000, 3456, 0) + 4 * C


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 28
    for name in ("pychain_hip_smbr_frame_accuracy_classes", "pychain_hip_smbr_forward_backward_classes",
                 "pychain_hip_cpu_smbr_frame_accuracy_classes", "pychain_hip_cpu_smbr_forward_backward_classes",
                 "pychain_hip_smbr_frame_accuracy_classes_workspace_bytes", "pychain_hip_smbr_lds_bytes"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
