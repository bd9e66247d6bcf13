"""The boosted objective (LF-bMMI; include/pychain_hip.h: pychain_hip_boost_rows; csrc/boost.hip) on the MI355X
against tests/boost_reference.  The pass alone through native.boost_rows: rows of 1 .. 3456 pdfs, 1 .. 33 entries per frame,
fp32 / bf16 / fp16, NaN in all padding, a frame without entries, a pdf three times in a frame, one bad entry, x beyond the
clamp; untargeted elements bit for bit exp(clamp(x)), targeted ones within the derived bound, nothing written beyond a length.
Through the denominator: the rows of boost = 0 with input_is_exp against the call on x itself.  Through ChainLoss: posterior
supervision and graph numerators against the fp64 reference written from the definition, with the regularisers, the weights,
xent_targets, lengths on the device, a second backward and bf16; the device route against the CPU route.

The pass is held to boost_reference's derived bound, ChainLoss to the library's fp64 bar, 1e-5 on the relative value and on
max |d grad| / max |grad|.  Every measured distance goes through helpers.record_parity."""
import numpy as np
import pytest
import torch

import boost_reference as br
from helpers import record_parity
from pychain_amd import (ChainLoss, PosteriorTargets, _lib, _plan, boost_rows, native, posterior_targets, synthetic as syn,
                         viterbi_align)

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BAR = br.BAR
L2, OOR = 5e-4, 0.01
BOOSTS = [0.1, 1.0]


def _live(D):
    live = np.zeros((br.NATIVE_B, br.NATIVE_T, D), dtype=bool)
    for b, L in enumerate(br.NATIVE_LENGTHS):
        live[b, :L] = True
    return live


# ---- the pass alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", sorted(br.DTYPES))
@pytest.mark.parametrize("D", br.NATIVE_DS)
def test_native_pass(D, dname):
    L = _lib.lib()
    live = _live(D)
    worst = dict(targeted=0.0, twin=0.0)
    for K in br.NATIVE_KS:
        x, lengths, pdfs, probs = br.native_case(D, K, dname)
        xd, pd, q = x.to(DEV), pdfs.to(DEV), probs.to(DEV)
        calls = L.pychain_hip_cpu_calls()
        # exp(clamp(x)) as the denominator kernels form it: the rows of a batch without a single entry
        E, bad0 = native.boost_rows(xd, lengths, torch.full_like(pd, -1), q, 1.0, out=torch.zeros(x.shape, device=DEV))
        assert int(bad0) == 0
        E = E.cpu().numpy()
        for boost in (0.1, 1.0, 2.5):
            calls = L.pychain_hip_cpu_calls()
            out = torch.full(x.shape, br.SENTINEL, device=DEV)
            e, bad = native.boost_rows(xd, lengths, pd, q, boost, out=out)
            assert e is out
            want, touched, bound, nbad = br.np_boost_rows(E, lengths, pdfs.numpy(), probs.numpy(), boost)
            assert int(bad) == 1 == nbad
            g = e.cpu().numpy()
            assert touched.any() and not touched[~live].any()
            assert np.array_equal(g[live & ~touched].view(np.int32), E[live & ~touched].view(np.int32))     # bit for bit
            assert bool((g[~live] == br.SENTINEL).all())                                   # nothing beyond the lengths is written
            r = float((np.abs(g.astype(np.float64) - want)[touched] / bound[touched]).max())
            worst["targeted"] = max(worst["targeted"], r)
            # a repeated pdf gives the value of the merged entry; the same call gives the same bits
            mp, mq = br.merged_case(pdfs, probs)
            e2, _ = native.boost_rows(xd, lengths, mp.to(DEV), mq.to(DEV), boost, out=torch.full(x.shape, br.SENTINEL, device=DEV))
            e3, _ = native.boost_rows(xd, lengths, pd, q, boost, out=torch.full(x.shape, br.SENTINEL, device=DEV))
            assert torch.equal(br.bits(e2), br.bits(e)) and torch.equal(br.bits(e3), br.bits(e)), (K, boost)
            torch.cuda.synchronize()
            assert L.pychain_hip_cpu_calls() == calls                                      # device tensors never reach the host twin
            # the host twin: the same operation sequence with the host's exp2f where the device has v_exp_f32 - each exp2 within
            # an ulp (2^-23), so E within 2^-22 of the device's and a targeted element within twice its bound
            ht, _ = native.cpu_boost_rows(x, lengths, pdfs, probs, boost, out=torch.full(x.shape, br.SENTINEL))
            ht = ht.numpy().astype(np.float64)
            allow = np.where(touched, 2.0 * bound + 2.0 ** -22 * np.abs(want), 2.0 ** -22 * np.abs(want))
            worst["twin"] = max(worst["twin"], float((np.abs(ht - g)[live] / allow[live]).max()))
        e0, _ = native.boost_rows(xd, lengths, pd, q, 0.0, out=torch.zeros(x.shape, device=DEV))
        assert np.array_equal(e0.cpu().numpy()[live].view(np.int32), E[live].view(np.int32))               # boost 0: E everywhere
    print("D=%d %s: targeted elements %.3f of their bound, the host twin %.3f of its allowance" % (D, dname, worst["targeted"], worst["twin"]))
    record_parity("boost_pass_D%d_%s" % (D, dname), **worst)
    assert worst["targeted"] <= 1.0 and worst["twin"] <= 1.0, worst


def test_untargeted_rows_are_what_torch_forms_from_the_same_two_steps():
    """An independent look at E: exp2(fl32(clamp(x) * fp32(log2 e))) by torch on the device - the same two steps in another code
    base.  Its exp2 need not round as v_exp_f32 does: held to one ulp of each, 2^-22; the measured distance is printed."""
    x, lengths, pdfs, probs = br.native_case(3456, 8)
    xd = x.to(DEV)
    E, _ = native.boost_rows(xd, lengths, torch.full_like(pdfs, -1).to(DEV), probs.to(DEV), 1.0, out=torch.zeros(x.shape, device=DEV))
    ref = torch.exp2(xd.clamp(-30.0, 30.0) * 1.44269502162933349609375)
    live = torch.from_numpy(_live(3456)).to(DEV)
    d = float(((E - ref).abs() / ref)[live].max())
    same = bool(torch.equal(br.bits(E)[live], br.bits(ref)[live]))
    print("E against torch.exp2 of the rounded product: max relative distance %.3g, bit-identical %s" % (d, same))
    record_parity("boost_E_vs_torch", rel=d)
    assert d <= 2.0 ** -22, d


def test_a_nan_in_a_live_row_is_counted_and_bad_arguments_are_refused():
    x, lengths, pdfs, probs = br.native_case(8, 4)
    x[2, 1, 3] = float("nan")
    xd, pd, q = x.to(DEV), pdfs.to(DEV), probs.to(DEV)
    e, bad = native.boost_rows(xd, lengths, pd, q, 1.0)
    assert int(bad) == 2 and not bool(torch.isnan(e[2, 1]).any())
    L = _lib.lib()
    ld = lengths.to(DEV)
    out, badc = torch.empty(3, 9, 8, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda K, boost, ep, dt=_lib.F32: L.pychain_hip_boost_rows(xd.data_ptr(), dt, ld.data_ptr(), 3, 9, 8, pd.data_ptr(), q.data_ptr(), K,
                                                                      boost, ep, badc.data_ptr(), st)
    assert call(0, 1.0, out.data_ptr()) == -1                                              # K < 1
    assert call(4, -1.0, out.data_ptr()) == -1 and call(4, float("nan"), out.data_ptr()) == -1
    assert call(4, 1.0, out.data_ptr() + 4) == -1                                          # e not 16-byte aligned
    assert call(4, 1.0, None) == -1 and call(4, 1.0, out.data_ptr(), 7) == -1
    assert call(4, 1.0, out.data_ptr()) == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        native.boost_rows(x, lengths, pdfs, probs, 1.0)                                    # CPU tensors: no fallback either way


# ---- through the denominator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [40, 3456])
def test_rows_of_boost_zero_through_the_denominator(D):
    """native.boost_rows(boost = 0) then den_forward_backward(input_is_exp=True) against den_forward_backward(x): the same
    exp(clamp(x)) bits reach the same recursions.  Measured on the MI355X first: distance 0 at both widths,
    objective and gradient - so bit-identity is what is asserted (the 3e-7 between kernel forms is not needed)."""
    den = syn.make_den_graph(20, 60, D, seed=0)
    lengths = torch.tensor([37, 40, 1, 33])
    x = syn.make_input(4, 40, D, seed=5).to(DEV)
    pdfs = torch.randint(0, D, (4, 40, 3), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(DEV)
    probs = torch.rand(4, 40, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    plan = _plan.graph_plan(den, D, torch.device(DEV))
    objf, grad, bad = native.den_forward_backward(plan, x, lengths, 1e-5)
    e, _ = native.boost_rows(x, lengths, pdfs, probs, 0.0)
    objf2, grad2, bad2 = native.den_forward_backward(plan, e, lengths, 1e-5, input_is_exp=True)
    torch.cuda.synchronize()
    d_objf = float(((objf2 - objf).abs() / objf.abs()).max())
    d_grad = float((grad2 - grad).abs().max() / grad.abs().max())
    same = bool(torch.equal(br.bits(objf2), br.bits(objf)) and torch.equal(br.bits(grad2), br.bits(grad)))
    print("D=%d: objective %.3g, gradient %.3g, bit-identical %s" % (D, d_objf, d_grad, same))
    record_parity("boost_zero_den_D%d" % D, objf=d_objf, grad=d_grad, same=float(same))
    assert int(bad) == 0 == int(bad2)
    assert same, (d_objf, d_grad)


# ---- through ChainLoss ------------------------------------------------------------------------------------------------------------
D0 = 40
LENGTHS = torch.tensor([37, 40, 1, 33])
_SHARED = {}


def _case():
    """(x, lengths, targets K = 3 on the host, the denominator graph): computed once and shared, never changed"""
    if "post" not in _SHARED:
        den = syn.make_den_graph(20, 60, D0, seed=0)
        x = syn.make_input(4, 40, D0, seed=5)
        teacher = syn.make_input(4, 40, D0, seed=55) * 1.5
        _SHARED["post"] = (x, LENGTHS, posterior_targets(teacher, LENGTHS, den, 3), den)
    return _SHARED["post"]


def _graph_case():
    if "graph" not in _SHARED:
        x, lengths, _, den = _case()
        num = syn.make_num_graphs(lengths.tolist(), D0, seed=100)
        ali = viterbi_align(x.to(DEV), lengths, num)
        assert bool(ali.ok.all())
        _SHARED["graph"] = (x, lengths, num, PosteriorTargets.from_alignment(ali), den)
    return _SHARED["graph"]


def _want(boost, kind="post"):
    """the fp64 reference of the plain call at `boost`: computed once per (kind, boost)"""
    key = ("want", kind, boost)
    if key not in _SHARED:
        if kind == "post":
            x, lengths, targets, den = _case()
            _SHARED[key] = br.reference(den, x, lengths, targets, targets, boost)
        else:
            x, lengths, num, bt, den = _graph_case()
            _SHARED[key] = br.reference(den, x, lengths, num, bt, boost)
    return _SHARED[key]


class _Run(object):
    def __init__(self, den, x, lengths, sup, boost, device=DEV, lengths_dev=False, twice=False, reg=False, u=None, f=None, z=None,
                 c=0.0, boost_targets=None, fused=True):
        xd = x.detach().clone().to(device).requires_grad_(True)             # (a leaf of its own: the shared inputs are never changed)
        zd = None if z is None else z.detach().clone().to(device).requires_grad_(True)
        kw = dict(output_l2_regularize=L2, out_of_range_regularize=OOR) if reg else {}
        crit = ChainLoss(den, 1e-5, avg=True, xent_regularize=c, boost=boost, **kw)
        crit.fused = fused
        loss = crit(xd, lengths.to(device) if lengths_dev else lengths, sup, xent_output=zd, utt_weights=u, deriv_weights=f,
                    xent_targets=sup if z is not None else None, boost_targets=boost_targets)
        if twice:
            loss.backward(retain_graph=True)
            self.first = xd.grad.clone()
            xd.grad = None
            if zd is not None:
                zd.grad = None
        loss.backward()
        if device != "cpu":
            torch.cuda.synchronize()
        self.loss, self.gx, self.out = loss.detach().cpu(), xd.grad.cpu(), loss
        self.gz = None if zd is None else zd.grad.cpu()


def _hold(name, run, want):
    d = br.distances(run.loss, run.gx.float().numpy(), *want[:2])
    print("%s: loss %.3g, gradient %.3g (bar %.0e)" % (name, d[0], d[1], BAR))
    record_parity("boost_" + name, loss=d[0], grad=d[1])
    assert max(d) <= BAR, (name, d)


@pytest.mark.parametrize("boost", BOOSTS)
def test_posterior_supervision(boost):
    x, lengths, targets, den = _case()
    assert targets.pdfs.size(2) == 3
    calls = _lib.lib().pychain_hip_cpu_calls()
    on = _Run(den, x, lengths, targets, boost, twice=True)
    assert _lib.lib().pychain_hip_cpu_calls() == calls
    assert torch.equal(on.first.cpu(), on.gx)                                              # a second backward over a retained graph
    _hold("post_b%g" % boost, on, _want(boost))
    assert on.out.boost == boost and on.gx.dtype == torch.float32
    for b, L in enumerate(lengths.tolist()):
        assert not bool(on.gx[b, L:].any())
    # what the call reports: the totals of a fused call; the bad counts with the pass's own word last
    tot = on.out.totals_all.cpu()
    assert float(tot[0]) == float(tot[4]) == float(on.loss) and float(tot[1]) == float(lengths.sum()) and float(tot[2]) == 0.0
    assert tuple(on.out.bad_count.shape) == (3,) and int(on.out.bad_count.sum()) == 0
    # the unfused device route and the CPU route at the same inputs
    off, host = _Run(den, x, lengths, targets, boost, fused=False), _Run(den, x, lengths, targets, boost, device="cpu")
    _hold("post_unfused_b%g" % boost, off, _want(boost))
    _hold("post_device_vs_cpu_b%g" % boost, on, (float(host.loss), host.gx.numpy().astype(np.float64)))
    # lengths on the device
    _hold("post_devlen_b%g" % boost, _Run(den, x, lengths, targets, boost, lengths_dev=True), _want(boost))


@pytest.mark.parametrize("boost", BOOSTS)
def test_with_regularisers_weights_and_xent_targets(boost):
    x, lengths, targets, den = _case()
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.05
    x = torch.where(far, torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0, x)
    z = syn.make_input(4, 40, D0, seed=77)
    u = torch.tensor([1.0, 0.5, 0.25, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    f[0, :5], f[1, 3] = 1.0, 0.0
    c = 0.2
    want = br.reference(den, x, lengths, targets, targets, boost, True, u, f, (L2, OOR), z, targets, c)
    for name, kw in (("all", {}), ("all_devlen", dict(lengths_dev=True))):
        on = _Run(den, x, lengths, targets, boost, reg=True, u=u, f=f, z=z, c=c, twice=True, **kw)
        assert torch.equal(on.first.cpu(), on.gx)
        _hold("post_%s_b%g" % (name, boost), on, want)
        dz = float(np.abs(on.gz.numpy() - want[2]).max() / np.abs(want[2]).max())
        assert dz <= BAR, dz
        assert not bool(on.gx[1, 3].any())                                                 # a frame of derivative weight 0
        assert float(on.out.l2_term) > 0 and float(on.out.out_of_range_term) > 0 and float(on.out.xent_objf) < 0
        assert tuple(on.out.bad_count.shape) == (4,)


def test_bf16_network_output():
    """x in bf16 with D % 8 == 0 goes to the pass as it is; the boosted rows and the denominator's gradient on them are fp32.
    Against the fp32 run on the SAME values, u = 2^-8, as tests/test_gpu_post_targets.py derives its own bound plus the one extra
    cast: the denominator's gradient g_den = gamma_den / N is rounded to fp32 where the call stores it and to bf16 by the cast -
    (u + 2^-23) |g_den|, g_den = g + q / N -, the targets' pass rounds its one fma (2^-24, then u to bf16) on the result -
    (u + 2^-23) |g| -, and the two fp32 evaluations differ by no more than the bar: (u + 2^-23) (|g_den| + |g|) + bar max |g|."""
    x, lengths, targets, den = _case()
    xh = x.to(torch.bfloat16)
    on, ref = _Run(den, xh, lengths, targets, 1.0), _Run(den, xh.float(), lengths, targets, 1.0)
    assert on.gx.dtype == torch.bfloat16
    g, want = on.gx.float().numpy().astype(np.float64), ref.gx.numpy().astype(np.float64)
    g_den = want + br.dense(targets, lengths, D0).numpy() / float(lengths.sum())
    u = 2.0 ** -8
    bound = (u + 2.0 ** -23) * (np.abs(g_den) + np.abs(want)) + BAR * np.abs(want).max()
    r = float((np.abs(g - want) / bound).max())
    d_loss = abs(float(on.loss) - float(ref.loss)) / abs(float(ref.loss))
    print("bf16: loss %.3g (bar %.0e), gradient %.3f of its bound" % (d_loss, BAR, r))
    record_parity("boost_bf16", loss=d_loss, grad=r)
    assert d_loss <= BAR and r <= 1.0, (d_loss, r)
    _hold("post_bf16_values_fp32", ref, br.reference(den, xh.float(), lengths, targets, targets, 1.0))


@pytest.mark.parametrize("boost", BOOSTS)
def test_graph_numerators_with_an_alignment_as_the_reference(boost):
    x, lengths, num, bt, den = _graph_case()
    assert bt.pdfs.size(2) == 1 and bt.pdfs.is_cuda
    calls = _lib.lib().pychain_hip_cpu_calls()
    on = _Run(den, x, lengths, num, boost, boost_targets=bt, twice=True)
    assert _lib.lib().pychain_hip_cpu_calls() == calls
    assert torch.equal(on.first.cpu(), on.gx)
    _hold("graph_b%g" % boost, on, _want(boost, "graph"))
    host_bt = PosteriorTargets(bt.pdfs.cpu(), bt.probs.cpu())
    host = _Run(den, x, lengths, num, boost, device="cpu", boost_targets=host_bt)
    _hold("graph_device_vs_cpu_b%g" % boost, on, (float(host.loss), host.gx.numpy().astype(np.float64)))
    # both regularisers and both weights through the same route
    u = torch.tensor([1.0, 0.5, 0.25, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    _hold("graph_all_b%g" % boost, _Run(den, x, lengths, num, boost, boost_targets=bt, reg=True, u=u, f=f),
          br.reference(den, x, lengths, num, host_bt, boost, True, u, f, (L2, OOR)))


def test_boosting_cannot_raise_log_z_and_zero_probs_change_nothing():
    """Boosting only lowers denominator scores, so log Z cannot rise: the boosted objective num - log Z is at least the unboosted
    one on the same inputs - the returned loss, its negative (log Z - num) / N, is at most the unboosted loss - up to the bar.
    With all-zero probs every factor is exp(0): the unboosted reference within the bar."""
    x, lengths, targets, den = _case()
    plain = _want(0.0)
    prev = plain[0]
    for boost in BOOSTS:
        cur = float(_Run(den, x, lengths, targets, boost).loss)
        assert cur <= prev + BAR * abs(plain[0]), (boost, cur, prev)
        prev = cur
    zero = PosteriorTargets(targets.pdfs, torch.zeros_like(targets.probs))
    _hold("zero_probs", _Run(den, x, lengths, targets, 1.0, boost_targets=zero), plain)
    x, lengths, num, bt, den = _graph_case()
    plain = _want(0.0, "graph")
    assert float(_Run(den, x, lengths, num, 1.0, boost_targets=bt).loss) <= plain[0] + BAR * abs(plain[0])


def test_boost_zero_is_the_plain_call_bit_for_bit():
    x, lengths, targets, den = _case()
    _, _, num, bt, _ = _graph_case()
    for sup, kw in ((targets, {}), (num, dict(boost_targets=bt))):
        a, b = x.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
        la, lb = ChainLoss(den, 1e-5)(a, lengths, sup), ChainLoss(den, 1e-5, boost=0.0)(b, lengths, sup, **kw)
        la.backward()
        lb.backward()
        assert torch.equal(br.bits(la.detach().reshape(1)), br.bits(lb.detach().reshape(1))) and torch.equal(br.bits(a.grad), br.bits(b.grad))
        assert not hasattr(lb, "boost")


def test_c3_row_width_and_the_public_rows():
    """D = 3456, the benchmark's row width, K = 8, T = 64: ChainLoss against the reference, and boost_rows as a user calls it"""
    D, T = 3456, 64
    den = syn.make_den_graph(20, 60, D, seed=0)
    lengths = torch.tensor([T, T - 7, 1, T - 1])
    x = syn.make_input(4, T, D, seed=5)
    targets = posterior_targets(syn.make_input(4, T, D, seed=55) * 1.5, lengths, den, 8)
    _hold("c3_width", _Run(den, x, lengths, targets, 1.0), br.reference(den, x, lengths, targets, targets, 1.0))
    e = boost_rows(x.to(DEV), lengths, targets, 1.0)
    want = torch.exp(x.double().clamp(-30, 30) - br.dense(targets, lengths, D))
    live = torch.arange(T)[None, :] < lengths[:, None]
    d = float(((e.cpu().double() - want).abs() / want)[live].max())
    assert d <= 4e-6 and not bool(e.cpu()[~live].any()), d        # (|c| 6e-8 of the hardware exp at |c| <= 30 + 8: device_utils.h)
