"""Lattice-free sMBR with the accuracy by class (include/pychain_hip.h: pychain_hip_smbr_*_classes; csrc/smbr.hip: smbr_class_*;
DESIGN.md §3.27) on the MI355X against the fp64 recursions of tests/smbr_class_reference: the cases of smbr_reference under the
maps `phones`, `identity` and `one` at leaky coefficients 0.1 and 1e-5; the host twin; bf16 and fp16 rows; two calls bit for bit;
the counts and a NaN; class targets bit for bit; the recursion and gradient workgroups at the edge of the LDS with as many classes
as pdfs (more than the 1024 threads and the 4096 elements a thread holds in registers), and the refusal just beyond.

Tolerance (smbr_class_reference.reference): 1e-5 on max |d grad| / max |grad| and on the relative error of E_b, or twice the fp32
numpy recursions' own distance where that is beyond 5e-6; the row sums and `closing` are held to the same bound.  Under `one` the
gradient is zero and distances are relative to max |grad| of the pdf-level reference.  Every measured distance goes through
helpers.record_parity; the worst are in profiles/smbr_classes_parity.md."""
import numpy as np
import pytest
import torch

import smbr_class_reference as cr
import smbr_reference as sr
from helpers import record_parity
from pychain_amd import PosteriorTargets, _lib, expected_accuracy, synthetic as syn

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NAMES = sorted(sr.CASES)


def _call(name, which, coef, dtype=torch.float32, device=DEV, y=None, targets=None, **kw):
    g, y0, lengths, pdfs, probs = cr.case(name)
    x = (y0 if y is None else y).detach().clone().to(device=device, dtype=dtype).requires_grad_(True)     # (a leaf of its own)
    acc = expected_accuracy(x, lengths, g, targets or PosteriorTargets(pdfs, probs), leaky_coefficient=coef,
                            classes=cr.classes(which, y0.size(2)), **kw)
    acc.backward()
    return x, acc


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("which", cr.MAPS)
@pytest.mark.parametrize("name", NAMES)
def test_against_fp64(name, which, coef):
    (E, G, _), (bound, d32), scale = cr.reference(name, which, coef)
    calls = _lib.lib().pychain_hip_cpu_calls()
    x, acc = _call(name, which, coef)
    assert _lib.lib().pychain_hip_cpu_calls() == calls                        # the kernels, not the host twins
    g = x.grad.cpu().numpy()
    per_seq = acc.per_seq.cpu().numpy()
    dv, dg = sr.value_dist(per_seq, E), cr.grad_dist(g, G, scale)
    rows = float(np.abs(g.astype(np.float64).sum(-1)).max() / scale)
    closing = float(acc.closing.abs().max())
    print("%s %s c=%g: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (name, which, coef, dv, dg, rows, closing, d32, bound))
    record_parity("smbr_classes_gpu_%s_%s_c%g" % (name, which, coef), value=dv, grad=dg, rows=rows, closing=closing, f32_reference=d32, bound=bound)
    assert acc.is_cuda and acc.dtype == torch.float32 and acc.per_seq.dtype == torch.float64 and x.grad.dtype == torch.float32
    assert abs(float(acc.detach()) - E.sum()) <= bound * abs(E.sum())
    assert dv <= bound and dg <= bound and rows <= bound and closing <= bound
    assert acc.bad_count.tolist() == [0, 0]
    assert per_seq[-1] == 0.0 and not g[-1].any()                             # no targets: exactly nothing
    for b, L in enumerate(cr.case(name)[2].tolist()):
        assert not g[b, L:].any()                                             # rows beyond a length: exact zeros
    if name == "degenerate":
        assert not g[:, :, 8].any()                                           # the pdf no arc carries, in a class that is credited


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("which", cr.MAPS)
@pytest.mark.parametrize("name", NAMES)
def test_host_twin_against_device(name, which, coef):
    _, (bound, _), scale = cr.reference(name, which, coef)
    x, acc = _call(name, which, coef)
    xc, accc = _call(name, which, coef, device="cpu")
    dv = sr.value_dist(acc.per_seq.cpu().numpy(), accc.per_seq.numpy())
    dg = cr.grad_dist(x.grad.cpu().numpy(), xc.grad.double().numpy(), scale)
    record_parity("smbr_classes_gpu_twin_%s_%s_c%g" % (name, which, coef), value=dv, grad=dg)
    print("%s %s c=%g: twin against device E %.3g grad %.3g (bound %.3g)" % (name, which, coef, dv, dg, bound))
    assert dv <= bound and dg <= bound


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_two_byte_rows(name, dtype):
    xh, acch = _call(name, "phones", 0.1, dtype=dtype)
    up = xh.detach().float().cpu()
    xf, accf = _call(name, "phones", 0.1, y=up)
    assert xh.grad.dtype == dtype and xf.grad.dtype == torch.float32
    assert torch.equal(xh.grad, xf.grad.to(dtype))                            # the fp32 call on the up-cast input, rounded once
    assert torch.equal(acch.per_seq, accf.per_seq) and torch.equal(acch.closing, accf.closing)
    _, (bound, _), _ = cr.reference(name, "phones", 0.1)
    g, y, lengths, pdfs, probs = cr.case(name)
    want = cr.batch(sr.recursions, g, up, lengths, pdfs.numpy(), probs.numpy(), cr.class_map("phones", y.size(2)), 0.1)
    assert cr.grad_dist(xf.grad.cpu().numpy(), want[1], float(np.abs(want[1]).max())) <= bound


@pytest.mark.parametrize("which", ["phones", "identity"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_two_calls_give_the_same_bits(name, which):
    x1, a1 = _call(name, which, 1e-5)
    x2, a2 = _call(name, which, 1e-5)
    assert torch.equal(x1.grad, x2.grad) and torch.equal(a1.per_seq, a2.per_seq) and torch.equal(a1.closing, a2.closing)


def test_counts_and_nan():
    g, y, lengths, pdfs, probs = cr.case("small")
    D = y.size(2)
    classes = cr.classes("phones", D)
    C = int(classes.max()) + 1
    x, clean = _call("small", "phones", 0.1)
    # an entry that names pdf >= D (device targets are not inspected): counted, otherwise ignored
    p2 = pdfs.clone()
    assert int(p2[0, 5, 1]) < 0
    p2[0, 5, 1] = D                                                           # (was padding)
    p2[1, 12, 0] = D + 3                                                      # (frame 12 of a sequence of 9: not looked at)
    x2, acc = _call("small", "phones", 0.1, targets=PosteriorTargets(p2.to(DEV), probs.to(DEV)))
    assert acc.bad_count.tolist() == [0, 1]
    assert torch.equal(acc.per_seq, clean.per_seq) and torch.equal(x2.grad, x.grad)
    # the same as class targets, and a class id >= C
    tc = PosteriorTargets._of(p2, probs).to_classes(classes)
    c2 = tc.pdfs.clone()
    assert int(c2[0, 2, 0]) < 0 and int(c2[0, 5, 1]) >= C
    c2[0, 2, 0] = C                                                           # (was padding)
    x4, acc4 = _call("small", "phones", 0.1, targets=PosteriorTargets(c2.to(DEV), probs.to(DEV)), targets_are_classes=True)
    assert acc4.bad_count.tolist() == [0, 2]
    assert torch.equal(acc4.per_seq, clean.per_seq) and torch.equal(x4.grad, x.grad)
    # a NaN in a live row
    y3 = y.clone()
    y3[1, 3, 5] = float("nan")
    y3[1, 12, 5] = float("nan")                                               # (beyond the length: not read)
    x3, acc3 = _call("small", "phones", 0.1, y=y3)
    assert acc3.bad_count.tolist() == [1, 0]
    assert bool(torch.isnan(acc3.per_seq[1])) and bool(torch.isnan(acc3.closing[1]))
    keep = [0, 2, 3]
    assert torch.equal(acc3.per_seq[keep], clean.per_seq[keep]) and torch.equal(x3.grad[keep], x.grad[keep])


@pytest.mark.parametrize("which", ["phones", "one"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_class_targets_give_the_bits_of_pdf_targets(name, which):
    g, y, lengths, pdfs, probs = cr.case(name)
    tc = PosteriorTargets(pdfs, probs).to_classes(cr.classes(which, y.size(2)))
    x, acc = _call(name, which, 0.1)
    xc, accc = _call(name, which, 0.1, targets=tc, targets_are_classes=True)
    assert torch.equal(x.grad, xc.grad) and torch.equal(acc.per_seq, accc.per_seq) and torch.equal(acc.closing, accc.closing)
    assert accc.bad_count.tolist() == [0, 0]


def test_sixteen_byte_loads():
    # D a multiple of 4: the accuracy pass reads gamma and the map 16 bytes at a time (every case above has an odd D or D % 4 = 2);
    # more frames than a workgroup of the pass has waves, two sequences, classes of three pdfs
    H, D, B, T, lengths = 37, 264, 2, 11, [11, 6]
    g = syn.make_den_graph(H, 150, D, seed=3)
    y = syn.make_input(B, T, D, seed=5)
    pdfs = syn.randint(31, B * T * 2, D).reshape(B, T, 2).astype(np.int32)
    pdfs[:, 1::3, 1] = -1
    probs = (0.05 + syn.uniform(32, B * T * 2)).reshape(B, T, 2).astype(np.float32)
    cls = np.arange(D) // 3
    want = cr.batch(sr.recursions, g, y, lengths, pdfs, probs, cls, 0.1)
    w32 = cr.batch(sr.recursions, g, y, lengths, pdfs, probs, cls, 0.1, dtype=np.float32)
    scale = float(np.abs(want[1]).max())
    d32 = max(cr.grad_dist(w32[1], want[1], scale), sr.value_dist(w32[0], want[0]))
    bound = 2.0 * d32 if d32 > sr.F32_SLACK else sr.BAR
    tg = PosteriorTargets(torch.from_numpy(pdfs), torch.from_numpy(probs))
    x = y.to(DEV).requires_grad_(True)
    acc = expected_accuracy(x, torch.tensor(lengths), g, tg, leaky_coefficient=0.1, classes=torch.from_numpy(cls))
    acc.backward()
    xc = y.clone().requires_grad_(True)
    accc = expected_accuracy(xc, torch.tensor(lengths), g, tg, leaky_coefficient=0.1, classes=torch.from_numpy(cls))
    dv, dg = sr.value_dist(acc.per_seq.cpu().numpy(), want[0]), cr.grad_dist(x.grad.cpu().numpy(), want[1], scale)
    print("D=%d: E %.3g grad %.3g (fp32 reference %.3g, bound %.3g); E against the twin %.3g" % (
        D, dv, dg, d32, bound, sr.value_dist(acc.per_seq.cpu().numpy(), accc.per_seq.numpy())))
    record_parity("smbr_classes_gpu_wide_loads", value=dv, grad=dg, f32_reference=d32, bound=bound)
    assert dv <= bound and dg <= bound and acc.bad_count.tolist() == [0, 0]
    assert sr.value_dist(acc.per_seq.cpu().numpy(), accc.per_seq.numpy()) <= bound


def test_the_lds_edge():
    # identity classes, so C = D: the largest D the query puts within the 160 KiB of a CU, and the refusal 32 pdfs beyond it
    H, budget = 37, 160 * 1024
    lds = lambda D: _lib.lib().pychain_hip_smbr_lds_bytes(H, D, D)
    D = max(d for d in range(4096, 16384) if lds(d) <= budget)
    assert lds(D) <= budget < lds(D + 1) and D > 4096
    g = syn.make_den_graph(H, 150, D + 32, seed=3)
    y = syn.make_input(1, 2, D + 32, seed=5).to(DEV)
    tg = PosteriorTargets(torch.zeros(1, 2, 1, dtype=torch.int32), torch.ones(1, 2, 1))
    msg = r"\(-2\).*%d states, %d pdfs and %d classes need %d bytes.*%d" % (H, D + 32, D + 32, lds(D + 32), budget)
    with pytest.raises(_lib.PychainHipError, match=msg):
        expected_accuracy(y, torch.tensor([2]), g, tg, classes=torch.arange(D + 32, dtype=torch.int32))
    # just inside: runs, held to fp64
    g = syn.make_den_graph(H, 150, D, seed=3)
    y = syn.make_input(1, 2, D, seed=5)
    cls = torch.arange(D, dtype=torch.int32)
    carried = g.forward_transitions[:, 2]
    tg = PosteriorTargets(torch.stack([carried[0], carried[-1]]).view(1, 2, 1).to(torch.int32), torch.ones(1, 2, 1))   # pdfs arcs carry
    x = y.to(DEV).requires_grad_(True)
    acc = expected_accuracy(x, torch.tensor([2]), g, tg, leaky_coefficient=0.1, classes=cls)
    acc.backward()
    want = cr.batch(sr.recursions, g, y, [2], tg.pdfs.numpy(), tg.probs.numpy(), cls.numpy(), 0.1)
    w32 = cr.batch(sr.recursions, g, y, [2], tg.pdfs.numpy(), tg.probs.numpy(), cls.numpy(), 0.1, dtype=np.float32)
    scale = float(np.abs(want[1]).max())
    d32 = max(cr.grad_dist(w32[1], want[1], scale), sr.value_dist(w32[0], want[0]))
    bound = 2.0 * d32 if d32 > sr.F32_SLACK else sr.BAR
    grad = x.grad.cpu().numpy()
    dv, dg = sr.value_dist(acc.per_seq.cpu().numpy(), want[0]), cr.grad_dist(grad, want[1], scale)
    rows = float(np.abs(grad.astype(np.float64).sum(-1)).max() / scale)
    closing = float(acc.closing.abs().max())
    print("D=C=%d (%d bytes of LDS): E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (D, lds(D), dv, dg, rows, closing, d32, bound))
    record_parity("smbr_classes_gpu_lds_edge", value=dv, grad=dg, rows=rows, closing=closing, f32_reference=d32, bound=bound)
    assert scale > 0 and want[0][0] > 0                                       # the targets name pdfs arcs carry
    assert acc.bad_count.tolist() == [0, 0] and dv <= bound and dg <= bound and rows <= bound and closing <= bound
