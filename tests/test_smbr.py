"""Lattice-free sMBR (include/pychain_hip.h: pychain_hip_smbr_*) without a GPU: the two fp64 evaluations of
tests/smbr_reference against each other, the planted faults, and the host twins through the Python API against fp64 - value and
gradient, `avg`, an upstream gradient, an utterance without targets, the row sums, `closing`, `bad_count`, every refusal, ABI 27.

Tolerance (smbr_reference.bound): 1e-5 on max |d grad| / max |grad| and on the relative error of E_b - the project's bound for
fp32 against fp64 -, or twice the fp32 reference's own distance where that is beyond 5e-6; the row sums and `closing` are held
to the same bound."""
import os
import re

import numpy as np
import pytest
import torch

import smbr_reference as sr
from helpers import record_parity
from pychain_amd import (ChainGraph, ChainGraphBatch, ChainLoss, PosteriorTargets, SMBRLoss, _lib, expected_accuracy, native,
                         synthetic as syn, viterbi_align)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(sr.CASES)


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("name", NAMES)
def test_the_two_references_agree(name, coef):
    g, y, lengths, pdfs, probs = sr.case(name)
    (E, G, closing), _ = sr.reference(name, coef)
    E2, G2, _ = sr.batch(sr.autograd, g, y, lengths, pdfs.numpy(), probs.numpy(), coef)
    assert np.abs(E - E2).max() <= 1e-12 * max(1.0, np.abs(E2).max()) and sr.grad_dist(G, G2) <= 1e-12
    assert np.abs(closing).max() <= 1e-12 and np.abs(G.sum(-1)).max() <= 1e-12 * np.abs(G).max()
    assert E[-1] == 0.0 and not G[-1].any()                    # the utterance without targets


@pytest.mark.parametrize("fault", sr.FAULTS)
@pytest.mark.parametrize("name", NAMES)
def test_the_cases_see_a_planted_fault(name, fault):
    g, y, lengths, pdfs, probs = sr.case(name)
    (_, G, _), (bound, _) = sr.reference(name, 0.1)
    Gf = sr.batch(sr.recursions, g, y, lengths, pdfs.numpy(), probs.numpy(), 0.1, fault=fault)[1]
    moved = sr.grad_dist(Gf, G)
    print("%s %s: moves the gradient by %.3g, bound %.3g" % (name, fault, moved, bound))
    assert moved > 100.0 * bound


def _call(name, coef, **kw):
    g, y, lengths, pdfs, probs = sr.case(name)
    x = y.clone().requires_grad_(True)
    acc = expected_accuracy(x, lengths, g, PosteriorTargets(pdfs, probs), leaky_coefficient=coef, **kw)
    return x, acc


@pytest.mark.parametrize("coef", sr.COEFS)
@pytest.mark.parametrize("name", NAMES)
def test_host_twin_against_fp64(name, coef):
    (E, G, _), (bound, d32) = sr.reference(name, coef)
    calls = _lib.lib().pychain_hip_cpu_calls()
    x, acc = _call(name, coef)
    assert _lib.lib().pychain_hip_cpu_calls() > calls
    acc.backward()
    g = x.grad.numpy()
    dv, dg = sr.value_dist(acc.per_seq.numpy(), E), sr.grad_dist(g, G)
    rows = float(np.abs(g.astype(np.float64).sum(-1)).max() / np.abs(G).max())
    closing = float(acc.closing.abs().max())
    print("%s c=%g: E %.3g grad %.3g rows %.3g closing %.3g (fp32 reference %.3g, bound %.3g)" % (name, coef, dv, dg, rows, closing, d32, bound))
    record_parity("smbr_cpu_%s_c%g" % (name, coef), value=dv, grad=dg, rows=rows, closing=closing, f32_reference=d32)
    assert acc.dtype == torch.float32 and acc.per_seq.dtype == torch.float64 and x.grad.dtype == torch.float32
    assert abs(float(acc.detach()) - E.sum()) <= bound * abs(E.sum())
    assert dv <= bound and dg <= bound and rows <= bound and closing <= bound
    assert acc.bad_count.tolist() == [0, 0]
    assert float(acc.per_seq[-1]) == 0.0 and not bool(x.grad[-1].any())          # no targets: exactly nothing
    lengths = sr.case(name)[2]
    for b, L in enumerate(lengths.tolist()):
        assert not bool(x.grad[b, L:].any())


@pytest.mark.parametrize("avg", [True, False])
def test_loss_avg_and_upstream_gradient(avg):
    g, y, lengths, pdfs, probs = sr.case("small")
    (E, G, _), (bound, _) = sr.reference("small", 0.1)
    x = y.clone().requires_grad_(True)
    loss = SMBRLoss(g, leaky_coefficient=0.1, avg=avg)(x, lengths, PosteriorTargets(pdfs, probs))
    (2.5 * loss).backward()
    norm = float(lengths.sum()) if avg else 1.0
    assert abs(float(loss) + E.sum() / norm) <= bound * abs(E.sum() / norm)
    assert sr.grad_dist(x.grad.numpy(), -2.5 * G / norm) <= bound
    assert loss.per_seq.shape == (4,) and loss.bad_count.tolist() == [0, 0] and loss.closing.shape == (4,)


def test_interpolation_with_chain_loss_and_an_alignment_as_reference():
    w = syn.make_workload("C1")
    y, lengths, den = w["x"], w["lengths"], w["den_graph"]
    ref = PosteriorTargets.from_alignment(viterbi_align(y, lengths, w["num_graphs"]))
    assert int((ref.pdfs >= 0).sum()) == int(lengths.sum())
    x = y.clone().requires_grad_(True)
    total = SMBRLoss(den)(x, lengths, ref) + 0.1 * ChainLoss(den)(x, lengths, w["num_graphs"])
    total.backward()
    x1, x2 = y.clone().requires_grad_(True), y.clone().requires_grad_(True)
    SMBRLoss(den)(x1, lengths, ref).backward()
    (0.1 * ChainLoss(den)(x2, lengths, w["num_graphs"])).backward()
    assert torch.equal(x.grad, x1.grad + x2.grad)               # plain autograd addition
    want = sr.batch(sr.recursions, den, y, lengths, ref.pdfs.numpy(), ref.probs.numpy(), 1e-5)
    bound, _ = sr.bound(den, y, lengths, ref.pdfs.numpy(), ref.probs.numpy(), 1e-5, want)
    assert sr.grad_dist(x1.grad.numpy() * -float(lengths.sum()), want[1]) <= bound
    # a second backward over a retained graph evaluates again
    x3 = y.clone().requires_grad_(True)
    acc = expected_accuracy(x3, lengths, ChainGraphBatch(den, 2), ref)
    acc.backward(retain_graph=True)
    first = x3.grad.clone()
    x3.grad = None
    acc.backward()
    assert torch.equal(first, x3.grad)


def test_bad_count_and_nan():
    g, y, lengths, pdfs, probs = sr.case("small")
    D = y.size(2)
    gt = native.smbr_graph(g, D, torch.device("cpu"))
    gamma = native.cpu_forward_backward(ChainGraphBatch(g, 4), y, lengths, 0.1)[1]
    clean = native.cpu_smbr(gt, g.num_states, y, lengths, gamma, pdfs, probs, 0.1)
    assert clean[2].tolist() == [0, 0]
    # an entry that names pdf >= D is counted and otherwise ignored; one beyond a length is not looked at
    p2 = pdfs.clone()
    p2[0, 1, 1] = D                                            # (was padding)
    p2[1, 12, 0] = D + 3                                       # (frame 12 of a sequence of 9)
    got = native.cpu_smbr(gt, g.num_states, y, lengths, gamma, p2, probs, 0.1)
    assert got[2].tolist() == [0, 1] and torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1])
    # a NaN in a live row: that sequence's E is NaN, the others are untouched
    y2 = y.clone()
    y2[1, 3, 5] = float("nan")
    got = native.cpu_smbr(gt, g.num_states, y2, lengths, gamma, pdfs, probs, 0.1)
    assert got[2].tolist() == [1, 0] and bool(torch.isnan(got[0][1])) and bool(torch.isnan(got[3][1]))
    keep = [0, 2, 3]
    assert torch.equal(got[0][keep], clean[0][keep]) and torch.equal(got[1][keep], clean[1][keep])
    y2[1, 12, 5] = float("nan")                                # beyond the length: not read
    assert native.cpu_smbr(gt, g.num_states, y2, lengths, gamma, pdfs, probs, 0.1)[2].tolist() == [1, 0]


def test_refusals():
    g, y, lengths, pdfs, probs = sr.case("small")
    tg = PosteriorTargets(pdfs, probs)
    w = syn.make_workload("C1")
    with pytest.raises(ValueError, match="log-domain"):
        expected_accuracy(w["x"], w["lengths"], ChainGraphBatch(ChainGraph(syn.make_num_fst(5, 40, 1), log_domain=True), 2),
                          PosteriorTargets(torch.zeros(2, 50, 1, dtype=torch.int32), torch.ones(2, 50, 1)))
    distinct = ChainGraphBatch([g, g, g, g], max_num_transitions=g.num_transitions, max_num_states=g.num_states)
    with pytest.raises(ValueError, match="distinct"):
        expected_accuracy(y, lengths, distinct, tg)
    with pytest.raises(ValueError, match="batch size"):
        expected_accuracy(y, lengths, ChainGraphBatch(g, 3), tg)
    with pytest.raises(ValueError, match="network output is"):
        expected_accuracy(y[:, :16], torch.tensor([16, 9, 2, 1]), g, tg)
    with pytest.raises(ValueError, match="name pdf"):
        expected_accuracy(y[:, :, :20], lengths, syn.make_den_graph(37, 150, 20, seed=3), tg)
    with pytest.raises(ValueError, match="PosteriorTargets"):
        expected_accuracy(y, lengths, g, (pdfs, probs))
    with pytest.raises(ValueError, match="names pdf"):       # the graph itself names a pdf the network output does not have
        expected_accuracy(y[:, :, :20], lengths, g, PosteriorTargets(pdfs.clamp_max(19), probs))
    # the C ABI: null pointers, sizes, the coefficient
    L = _lib.lib()
    gt = native.smbr_graph(g, 23, torch.device("cpu"))
    lc = lengths.to(torch.int64)
    gamma, facc = torch.zeros(4, 17, 23), torch.zeros(4, 17)
    acc, closing, bad, grad = torch.zeros(4, dtype=torch.float64), torch.zeros(4), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 17, 23)
    fa = lambda k, gp: L.pychain_hip_cpu_smbr_frame_accuracy(gp, lc.data_ptr(), 4, 17, 23, pdfs.data_ptr(), probs.data_ptr(), k,
                                                            facc.data_ptr(), acc.data_ptr(), bad.data_ptr(), 1)
    assert fa(0, gamma.data_ptr()) == -1 and fa(2, None) == -1 and fa(2, gamma.data_ptr()) == 0
    fb = lambda coef, k, gp: L.pychain_hip_cpu_smbr_forward_backward(
        *[t.data_ptr() for t in gt], 37, 150, y.data_ptr(), lc.data_ptr(), 4, 17, 23, pdfs.data_ptr(), probs.data_ptr(), k,
        facc.data_ptr(), coef, 1.0, None, gp, acc.data_ptr(), closing.data_ptr(), bad.data_ptr(), 1)
    assert fb(0.0, 2, grad.data_ptr()) == -1 and fb(1.0, 2, grad.data_ptr()) == -1 and fb(0.1, 0, grad.data_ptr()) == -1
    assert fb(0.1, 2, None) == -1 and fb(0.1, 2, grad.data_ptr()) == 0
    assert L.pychain_hip_smbr_workspace_bytes(0, 1, 1) == 0 and L.pychain_hip_smbr_workspace_bytes(2, 3, 5) >= 4 * 4 * 2 * 4 * 5


def test_the_by_pdf_order_is_cached_on_the_graph():
    g = syn.make_den_graph(20, 60, 40, seed=0)
    a = native.smbr_graph(g, 40, torch.device("cpu"))
    assert native.smbr_graph(g, 40, torch.device("cpu")) is a
    arcs, index = a[9].numpy(), a[10].numpy()
    pdf = g.forward_transitions[:, 2].numpy()
    assert index[0] == 0 and index[-1] == 60 and (np.diff(index) >= 0).all()
    for n in range(40):
        ids = arcs[index[n]:index[n + 1]]
        assert (pdf[ids] == n).all() and (np.diff(ids) > 0).all()               # stable
    g.forward_transition_probs.mul_(1.0)                                        # an in-place edit: built again
    assert native.smbr_graph(g, 40, torch.device("cpu")) is not a


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 27
    for name in ("pychain_hip_smbr_workspace_bytes", "pychain_hip_smbr_frame_accuracy", "pychain_hip_smbr_forward_backward",
                 "pychain_hip_cpu_smbr_frame_accuracy", "pychain_hip_cpu_smbr_forward_backward"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    import pychain
    import pychain_amd
    assert pychain.SMBRLoss is SMBRLoss is pychain_amd.SMBRLoss and pychain.expected_accuracy is expected_accuracy
