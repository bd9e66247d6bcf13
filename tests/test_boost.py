"""The boosted objective (LF-bMMI; include/pychain_hip.h: pychain_hip_boost_rows) on CPU tensors: the host twin
of the row pass against tests/boost_reference at the shapes the GPU tests use; ChainLoss(boost=b) against the fp64 reference
written from the definition - posterior supervision alone, with both regularisers, both weights and xent_targets, a second
backward, bf16, graph numerators with an alignment as the reference -; what boosting can and cannot do to log Z; validation;
ABI 25.  No GPU.  The pass is held to boost_reference's derived bound, ChainLoss to the library's fp64 bar, 1e-5 on the relative
value and on max |d grad| / max |grad|."""
import os
import re

import numpy as np
import pytest
import torch

import boost_reference as br
from helpers import record_parity
from pychain_amd import (ChainLoss, PosteriorTargets, _lib, boost_rows, native, posterior_targets, synthetic as syn,
                         viterbi_align)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = br.BAR
D = 40
LENGTHS = torch.tensor([37, 40, 1, 33])                    # ragged, in no order, one of a single frame
DEN = syn.make_den_graph(20, 60, D, seed=0)
L2, OOR = 5e-4, 0.01
BOOSTS = [0.1, 1.0]


# ---- the pass alone: the host twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", sorted(br.DTYPES))
@pytest.mark.parametrize("Dx", br.NATIVE_DS)
def test_host_twin_pass(Dx, dname):
    worst = 0.0
    live = np.zeros((br.NATIVE_B, br.NATIVE_T, Dx), dtype=bool)
    for b, L in enumerate(br.NATIVE_LENGTHS):
        live[b, :L] = True
    for K in br.NATIVE_KS:
        x, lengths, pdfs, probs = br.native_case(Dx, K, dname)
        # exp(clamp(x)) as the twin forms it: the same call on a batch without a single entry
        E, bad0 = native.cpu_boost_rows(x, lengths, torch.full_like(pdfs, -1), probs, 1.0, out=torch.zeros(x.shape))
        assert int(bad0) == 0
        for boost in (0.1, 1.0, 2.5):
            out = torch.full(x.shape, br.SENTINEL)
            e, bad = native.cpu_boost_rows(x, lengths, pdfs, probs, boost, out=out)
            assert e is out
            want, touched, bound, nbad = br.np_boost_rows(E.numpy(), lengths, pdfs.numpy(), probs.numpy(), boost)
            assert int(bad) == 1 == nbad
            g = e.numpy()
            assert touched.any() and not touched[~live].any()
            assert np.array_equal(g[live & ~touched].view(np.int32), E.numpy()[live & ~touched].view(np.int32))   # bit for bit
            assert bool((g[~live] == br.SENTINEL).all())                                   # nothing beyond the lengths is written
            r = float((np.abs(g.astype(np.float64) - want)[touched] / bound[touched]).max())
            worst = max(worst, r)
            # a repeated pdf gives the value of the merged entry
            mp, mq = br.merged_case(pdfs, probs)
            e2, _ = native.cpu_boost_rows(x, lengths, mp, mq, boost, out=torch.full(x.shape, br.SENTINEL))
            assert torch.equal(br.bits(e2), br.bits(e)), (K, boost)
        e0, _ = native.cpu_boost_rows(x, lengths, pdfs, probs, 0.0, out=torch.zeros(x.shape))
        assert np.array_equal(e0.numpy()[live].view(np.int32), E.numpy()[live].view(np.int32))           # boost 0: E everywhere
    print("D=%d %s: targeted elements %.3f of their bound" % (Dx, dname, worst))
    record_parity("boost_cpu_pass_D%d_%s" % (Dx, dname), targeted=worst)
    assert worst <= 1.0, worst


def test_a_nan_in_a_live_row_is_counted():
    x, lengths, pdfs, probs = br.native_case(8, 4)
    x[2, 1, 3] = float("nan")
    e, bad = native.cpu_boost_rows(x, lengths, pdfs, probs, 1.0)
    assert int(bad) == 2 and not bool(torch.isnan(e[2, 1]).any())


def test_public_boost_rows():
    x, lengths, pdfs, probs = br.native_case(8, 4)
    pdfs[0, 3, 0] = -1                                        # (PosteriorTargets on the host refuses pdf >= D)
    pdfs, probs = pdfs.clamp_max(7), torch.nan_to_num(probs, nan=0.0)
    e = boost_rows(x, lengths, PosteriorTargets(pdfs, probs), 1.0)
    want, _ = native.cpu_boost_rows(x, lengths, pdfs, probs, 1.0, out=torch.zeros(x.shape))
    assert e.dtype == torch.float32 and torch.equal(e, want) and not bool(e[1, 1:].any())
    with pytest.raises(ValueError):
        boost_rows(x, lengths, (pdfs, probs), 1.0)
    with pytest.raises(ValueError):
        native.cpu_boost_rows(x, lengths, pdfs, probs, -1.0)


# ---- through ChainLoss -----------------------------------------------------------------------------------------------------------
_SHARED = {}


def _case():
    """(x, lengths, targets K = 3): computed once and shared, never changed"""
    if "post" not in _SHARED:
        x = syn.make_input(4, 40, D, seed=5)
        teacher = syn.make_input(4, 40, D, seed=55) * 1.5
        _SHARED["post"] = (x, LENGTHS, posterior_targets(teacher, LENGTHS, DEN, 3))
    return _SHARED["post"]


def _graph_case():
    if "graph" not in _SHARED:
        x = syn.make_input(4, 40, D, seed=5)
        num = syn.make_num_graphs(LENGTHS.tolist(), D, seed=100)
        ali = viterbi_align(x, LENGTHS, num)
        assert bool(ali.ok.all())
        _SHARED["graph"] = (x, LENGTHS, num, PosteriorTargets.from_alignment(ali))
    return _SHARED["graph"]


def _hold(name, loss, grad, want):
    d = br.distances(loss.detach(), grad.float().numpy(), *want[:2])
    print("%s: loss %.3g, gradient %.3g (bar %.0e)" % (name, d[0], d[1], BAR))
    record_parity("boost_cpu_" + name, loss=d[0], grad=d[1])
    assert max(d) <= BAR, (name, d)


@pytest.mark.parametrize("avg", [True, False])
@pytest.mark.parametrize("boost", BOOSTS)
def test_posterior_supervision(boost, avg):
    x, lengths, targets = _case()
    assert targets.pdfs.size(2) == 3
    xx = x.clone().requires_grad_(True)
    loss = ChainLoss(DEN, 1e-5, avg=avg, boost=boost)(xx, lengths, targets)
    assert loss.boost == boost
    loss.backward(retain_graph=True)
    first = xx.grad.clone()
    xx.grad = None
    loss.backward()                                                  # a second backward over the retained graph
    assert torch.equal(xx.grad, first)
    _hold("post_b%g_avg%d" % (boost, avg), loss, first, br.reference(DEN, x, lengths, targets, targets, boost, avg))
    for b, L in enumerate(lengths.tolist()):
        assert not bool(first[b, L:].any())


@pytest.mark.parametrize("boost", BOOSTS)
def test_with_regularisers_weights_and_xent_targets(boost):
    x, lengths, targets = _case()
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.05
    x = torch.where(far, torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0, x)
    z = syn.make_input(4, 40, D, seed=77)
    u = torch.tensor([1.0, 0.5, 0.25, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    f[0, :5], f[1, 3] = 1.0, 0.0
    c = 0.2
    xx, zz = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
    crit = ChainLoss(DEN, 1e-5, avg=True, xent_regularize=c, output_l2_regularize=L2, out_of_range_regularize=OOR, boost=boost)
    loss = crit(xx, lengths, targets, xent_output=zz, utt_weights=u, deriv_weights=f, xent_targets=targets)
    loss.backward()
    # (with derivative weights the gradient is deliberately not that of the scalar: the reference scales the rows alike)
    want = br.reference(DEN, x, lengths, targets, targets, boost, True, u, f, (L2, OOR), z, targets, c)
    want_value = br.reference(DEN, x, lengths, targets, targets, boost, True, u, None, (L2, OOR), z, targets, c)[0]
    _hold("post_all_b%g" % boost, loss, xx.grad, (want_value, want[1]))
    dz = float(np.abs(zz.grad.numpy() - want[2]).max() / np.abs(want[2]).max())
    assert dz <= BAR, dz
    assert not bool(xx.grad[1, 3].any())


def test_bf16_network_output():
    """CPU tensors take the two-call route: each call evaluates in fp32 and rounds ITS gradient to bf16 where it hands it back -
    g_den = gamma_den / N and g_num = q / N, u |g_den| and u |g_num| with u = 2^-8 -, and autograd adds the two in bf16, u |g|
    more.  Against the fp32 run on the same values: u (|g_den| + |g_num| + |g|), g_den = g + q / N, plus the bar between two
    fp32 evaluations."""
    x, lengths, targets = _case()
    xh = x.to(torch.bfloat16).requires_grad_(True)
    xf = x.to(torch.bfloat16).float().requires_grad_(True)
    crit = ChainLoss(DEN, 1e-5, boost=1.0)
    lh, lf = crit(xh, lengths, targets), crit(xf, lengths, targets)
    lh.backward()
    lf.backward()
    assert xh.grad.dtype == torch.bfloat16
    g, want = xh.grad.float().numpy().astype(np.float64), xf.grad.numpy().astype(np.float64)
    g_num = br.dense(targets, lengths, D).numpy() / float(lengths.sum())
    bound = 2.0 ** -8 * (np.abs(want + g_num) + g_num + np.abs(want)) + BAR * np.abs(want).max()
    r = float((np.abs(g - want) / bound).max())
    print("bf16: gradient %.3f of its bound" % r)
    assert abs(float(lh.detach()) - float(lf.detach())) <= BAR * abs(float(lf.detach())) and r <= 1.0, r
    _hold("post_bf16_value", lf.detach(), xf.grad, br.reference(DEN, xf.detach(), lengths, targets, targets, 1.0))


@pytest.mark.parametrize("boost", BOOSTS)
def test_graph_numerators_with_an_alignment_as_the_reference(boost):
    x, lengths, num, bt = _graph_case()
    assert bt.pdfs.size(2) == 1
    xx = x.clone().requires_grad_(True)
    loss = ChainLoss(DEN, 1e-5, boost=boost)(xx, lengths, num, boost_targets=bt)
    loss.backward()
    _hold("graph_b%g" % boost, loss, xx.grad, br.reference(DEN, x, lengths, num, bt, boost))
    # with both regularisers and both weights through the same route
    u = torch.tensor([1.0, 0.5, 0.25, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    xx = x.clone().requires_grad_(True)
    crit = ChainLoss(DEN, 1e-5, output_l2_regularize=L2, out_of_range_regularize=OOR, boost=boost)
    loss = crit(xx, lengths, num, utt_weights=u, deriv_weights=f, boost_targets=bt)
    loss.backward()
    want = br.reference(DEN, x, lengths, num, bt, boost, True, u, f, (L2, OOR))
    _hold("graph_all_b%g" % boost, loss, xx.grad, (br.reference(DEN, x, lengths, num, bt, boost, True, u, None, (L2, OOR))[0], want[1]))


def test_boosting_cannot_raise_log_z():
    """Boosting only lowers denominator scores, so log Z cannot rise: the boosted objective num - log Z is at least the unboosted
    one on the same inputs - the returned loss, which is its negative (log Z - num) / N, is at most the unboosted loss - up to
    the bar; and it falls further as boost grows."""
    x, lengths, targets = _case()
    plain = float(ChainLoss(DEN, 1e-5)(x, lengths, targets))
    prev = plain
    for boost in BOOSTS:
        cur = float(ChainLoss(DEN, 1e-5, boost=boost)(x, lengths, targets))
        assert cur <= prev + BAR * abs(plain), (boost, cur, prev)
        prev = cur
    x, lengths, num, bt = _graph_case()
    plain = float(ChainLoss(DEN, 1e-5)(x, lengths, num))
    assert float(ChainLoss(DEN, 1e-5, boost=1.0)(x, lengths, num, boost_targets=bt)) <= plain + BAR * abs(plain)


def test_all_zero_probs_equal_the_unboosted_reference():
    x, lengths, targets = _case()
    zero = PosteriorTargets(targets.pdfs, torch.zeros_like(targets.probs))
    xx = x.clone().requires_grad_(True)
    loss = ChainLoss(DEN, 1e-5, boost=1.0)(xx, lengths, targets, boost_targets=zero)
    loss.backward()
    _hold("zero_probs", loss, xx.grad, br.reference(DEN, x, lengths, targets, None, 0.0))


def test_boost_zero_is_the_plain_call_bit_for_bit():
    x, lengths, targets = _case()
    _, _, num, bt = _graph_case()
    for sup, kw in ((targets, {}), (num, dict(boost_targets=bt))):
        a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        la, lb = ChainLoss(DEN, 1e-5)(a, lengths, sup), ChainLoss(DEN, 1e-5, boost=0.0)(b, lengths, sup, **kw)
        la.backward()
        lb.backward()
        assert torch.equal(br.bits(la.detach().reshape(1)), br.bits(lb.detach().reshape(1))) and torch.equal(br.bits(a.grad), br.bits(b.grad))
        assert not hasattr(lb, "boost")


def test_errors():
    x, lengths, targets = _case()
    _, _, num, bt = _graph_case()
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ChainLoss(DEN, 1e-5, boost=bad)
    crit = ChainLoss(DEN, 1e-5, boost=1.0)
    with pytest.raises(ValueError, match="from_alignment"):
        crit(x, lengths, num)                                        # graph supervision without boost_targets
    short = PosteriorTargets(bt.pdfs[:, :30], bt.probs[:, :30])
    with pytest.raises(ValueError):
        crit(x, lengths, num, boost_targets=short)                   # a shape mismatch of boost_targets
    with pytest.raises(ValueError):
        crit(x, lengths, targets, boost_targets=short)
    with pytest.raises(ValueError):
        crit(x, lengths, num, boost_targets=(bt.pdfs, bt.probs))     # not PosteriorTargets
    with pytest.raises(ValueError):
        crit(x, lengths, num, boost_targets=bt, xent_targets=bt)     # xent_targets go with posterior supervision, as without boost
    # the C ABI of the twin
    L = _lib.lib()
    rows, lc = torch.rand(2, 3, 4), torch.tensor([3, 2])
    pd, pr_ = torch.zeros(2, 3, 2, dtype=torch.int32), torch.ones(2, 3, 2)
    e, badc = torch.empty(2, 3, 4), torch.zeros(1, dtype=torch.int32)
    call = lambda k, boost, ep: L.pychain_hip_cpu_boost_rows(rows.data_ptr(), lc.data_ptr(), 2, 3, 4, pd.data_ptr(), pr_.data_ptr(), k, boost,
                                                             ep, badc.data_ptr(), 1)
    assert call(0, 1.0, e.data_ptr()) == -1 and call(2, -1.0, e.data_ptr()) == -1 and call(2, float("nan"), e.data_ptr()) == -1
    assert call(2, 1.0, None) == -1 and call(2, 1.0, e.data_ptr()) == 0


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 25
    for name in ("pychain_hip_boost_rows", "pychain_hip_cpu_boost_rows"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    import pychain
    import pychain_amd
    assert pychain.boost_rows is boost_rows is pychain_amd.boost_rows
