"""Lattice-free sMBR (include/pychain_hip.h: pychain_hip_smbr_*; csrc/smbr.hip) on the MI355X against the fp64
recursions of tests/smbr_reference, at leaky coefficients 0.1 and 1e-5: a small graph with ragged lengths down to one frame; a
graph of more states than a recursion workgroup has threads; a graph with a state nothing enters, a state nothing leaves and a
pdf no arc carries; bf16 and fp16 rows; the counts and a NaN; two calls bit for bit; the host twin; the refusal of a graph beyond
the LDS budget.  Every case's targets hold padding, a pdf twice in a frame and an utterance without targets.

Tolerance (smbr_reference.bound): 1e-5 on max |d grad| / max |grad| and on the relative error of E_b - the project's bound for
fp32 against fp64 -, or twice the fp32 reference's own distance where that is beyond 5e-6; the row sums and `closing` are held
to the same bound.  Every measured distance goes through helpers.record_parity."""
import numpy as np
import pytest
import torch

import smbr_reference as sr
from helpers import record_parity
from pychain_amd import ChainGraphBatch, PosteriorTargets, SMBRLoss, _lib, expected_accuracy, synthetic as syn

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NAMES = sorted(sr.CASES)


def _call(name, coef, dtype=torch.float32, device=DEV, y=None):
    g, y0, lengths, pdfs, probs = sr.case(name)
    x = (y0 if y is None else y).detach().clone().to(device=device, dtype=dtype).requires_grad_(True)     # (a leaf of its own)
    acc = expected_accuracy(x, lengths, g, PosteriorTargets(pdfs, probs), leaky_coefficient=coef)
    acc.backward()
    return x, acc


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("name", NAMES)
def test_against_fp64(name, coef):
    (E, G, _), (bound, d32) = sr.reference(name, coef)
    calls = _lib.lib().pychain_hip_cpu_calls()
    x, acc = _call(name, coef)
    assert _lib.lib().pychain_hip_cpu_calls() == calls                        # the kernels, not the host twins
    g = x.grad.cpu().numpy()
    per_seq = acc.per_seq.cpu().numpy()
    dv, dg = sr.value_dist(per_seq, E), sr.grad_dist(g, G)
    rows = float(np.abs(g.astype(np.float64).sum(-1)).max() / np.abs(G).max())
    closing = float(acc.closing.abs().max())
    print("%s c=%g: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (name, coef, dv, dg, rows, closing, d32, bound))
    record_parity("smbr_gpu_%s_c%g" % (name, coef), value=dv, grad=dg, rows=rows, closing=closing, f32_reference=d32, bound=bound)
    assert acc.is_cuda and acc.dtype == torch.float32 and acc.per_seq.dtype == torch.float64 and x.grad.dtype == torch.float32
    assert abs(float(acc.detach()) - E.sum()) <= bound * abs(E.sum())
    assert dv <= bound and dg <= bound and rows <= bound and closing <= bound
    assert acc.bad_count.tolist() == [0, 0]
    assert per_seq[-1] == 0.0 and not g[-1].any()                             # no targets: exactly nothing
    for b, L in enumerate(sr.case(name)[2].tolist()):
        assert not g[b, L:].any()                                             # rows beyond a length: exact zeros
    if name == "degenerate":
        assert not g[:, :, 8].any()                                           # the pdf no arc carries


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("name", NAMES)
def test_host_twin_against_device(name, coef):
    _, (bound, _) = sr.reference(name, coef)
    x, acc = _call(name, coef)
    xc, accc = _call(name, coef, device="cpu")
    dv = sr.value_dist(acc.per_seq.cpu().numpy(), accc.per_seq.numpy())
    dg = sr.grad_dist(x.grad.cpu().numpy(), xc.grad.double().numpy())
    record_parity("smbr_gpu_twin_%s_c%g" % (name, coef), value=dv, grad=dg)
    print("%s c=%g: twin against device E %.3g grad %.3g (bound %.3g)" % (name, coef, dv, dg, bound))
    assert dv <= bound and dg <= bound


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_two_byte_rows(name, dtype):
    xh, acch = _call(name, 0.1, dtype=dtype)
    up = xh.detach().float().cpu()
    xf, accf = _call(name, 0.1, y=up)
    assert xh.grad.dtype == dtype and xf.grad.dtype == torch.float32
    assert torch.equal(xh.grad, xf.grad.to(dtype))                            # the fp32 call on the up-cast input, rounded once
    assert torch.equal(acch.per_seq, accf.per_seq) and torch.equal(acch.closing, accf.closing)
    (_, G, _), (bound, _) = sr.reference(name, 0.1)
    g, y, lengths, pdfs, probs = sr.case(name)
    want = sr.batch(sr.recursions, g, up, lengths, pdfs.numpy(), probs.numpy(), 0.1)
    assert sr.grad_dist(xf.grad.cpu().numpy(), want[1]) <= bound


def test_counts_and_nan():
    g, y, lengths, pdfs, probs = sr.case("small")
    D = y.size(2)
    x, clean = _call("small", 0.1)
    # an entry that names pdf >= D (device targets are not inspected): counted, otherwise ignored
    p2 = pdfs.clone()
    p2[0, 1, 1] = D                                                           # (was padding)
    p2[1, 12, 0] = D + 3                                                      # (frame 12 of a sequence of 9: not looked at)
    x2 = y.to(DEV).requires_grad_(True)
    acc = expected_accuracy(x2, lengths, g, PosteriorTargets(p2.to(DEV), probs.to(DEV)), leaky_coefficient=0.1)
    acc.backward()
    assert acc.bad_count.tolist() == [0, 1]
    assert torch.equal(acc.per_seq, clean.per_seq) and torch.equal(x2.grad, x.grad)
    # a NaN in a live row
    y3 = y.clone()
    y3[1, 3, 5] = float("nan")
    y3[1, 12, 5] = float("nan")                                               # (beyond the length: not read)
    x3, acc3 = _call("small", 0.1, y=y3)
    assert acc3.bad_count.tolist() == [1, 0]
    assert bool(torch.isnan(acc3.per_seq[1])) and bool(torch.isnan(acc3.closing[1]))
    keep = [0, 2, 3]
    assert torch.equal(acc3.per_seq[keep], clean.per_seq[keep]) and torch.equal(x3.grad[keep], x.grad[keep])


@pytest.mark.parametrize("name", ["small", "wide"])
def test_two_calls_give_the_same_bits(name):
    x1, a1 = _call(name, 1e-5)
    x2, a2 = _call(name, 1e-5)
    assert torch.equal(x1.grad, x2.grad) and torch.equal(a1.per_seq, a2.per_seq) and torch.equal(a1.closing, a2.closing)


def test_loss_on_the_device():
    g, y, lengths, pdfs, probs = sr.case("small")
    (E, G, _), (bound, _) = sr.reference("small", 0.1)
    x = y.to(DEV).requires_grad_(True)
    loss = SMBRLoss(ChainGraphBatch(g, 4), leaky_coefficient=0.1, avg=True)(x, lengths.to(DEV), PosteriorTargets(pdfs, probs))
    (2.5 * loss).backward()
    norm = float(lengths.sum())
    assert abs(float(loss.detach()) + E.sum() / norm) <= bound * abs(E.sum() / norm)
    assert sr.grad_dist(x.grad.cpu().numpy(), -2.5 * G / norm) <= bound


def test_a_graph_beyond_the_lds_budget_is_refused():
    # the recursion workgroup keeps (4 H + 4 D + 128) floats in LDS: 160 KiB hold 4 (H + D) <= 40 832
    H, D = 37, 10180
    g = syn.make_den_graph(H, 150, D, seed=3)
    y = syn.make_input(1, 2, D, seed=5).to(DEV)
    tg = PosteriorTargets(torch.zeros(1, 2, 1, dtype=torch.int32), torch.ones(1, 2, 1))
    with pytest.raises(_lib.PychainHipError, match=r"\(-2\).*37 states and 10180 pdfs"):
        expected_accuracy(y, torch.tensor([2]), g, tg)
    D = 10160                                                                 # just inside: runs
    g = syn.make_den_graph(H, 150, D, seed=3)
    y = syn.make_input(1, 2, D, seed=5)
    tg = PosteriorTargets(torch.full((1, 2, 1), int(g.forward_transitions[0, 2]), dtype=torch.int32), torch.ones(1, 2, 1))   # a pdf an arc carries
    # the recursion and gradient kernels at nearly all of the LDS, rows beyond the 4096 elements a thread holds in registers
    x = y.to(DEV).requires_grad_(True)
    acc = expected_accuracy(x, torch.tensor([2]), g, tg, leaky_coefficient=0.1)
    acc.backward()
    want = sr.batch(sr.recursions, g, y, [2], tg.pdfs.numpy(), tg.probs.numpy(), 0.1)
    bound, d32 = sr.bound(g, y, [2], tg.pdfs.numpy(), tg.probs.numpy(), 0.1, want)
    grad = x.grad.cpu().numpy()
    dv, dg = sr.value_dist(acc.per_seq.cpu().numpy(), want[0]), sr.grad_dist(grad, want[1])
    rows = float(np.abs(grad.astype(np.float64).sum(-1)).max() / np.abs(want[1]).max())
    print("D=%d: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (D, dv, dg, rows, float(acc.closing.abs().max()), d32, bound))
    record_parity("smbr_gpu_lds_edge", value=dv, grad=dg, rows=rows, closing=float(acc.closing.abs().max()), f32_reference=d32, bound=bound)
    assert np.abs(want[1]).max() > 0 and want[0][0] > 0                      # the targets name a pdf an arc carries
    assert acc.bad_count.tolist() == [0, 0] and dv <= bound and dg <= bound and rows <= bound
    assert float(acc.closing.abs().max()) <= bound
