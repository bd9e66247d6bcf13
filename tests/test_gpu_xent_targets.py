"""Cross-entropy against sparse targets (include/pychain_hip.h: pychain_hip_xent_targets; csrc/xent.hip, the sparse source of the
row kernel) on the MI355X: the native pass against tests/xent_targets_reference on post_reference.native_case inputs - every
row form (scalar D = 1, 3, 257; vector D = 8, 3456, the latter several iterations per thread; the re-reading form at
D = 24 580), K from 1 to more entries than threads, three dtypes, with and without the store -, the totals step, and
ChainLoss(..., xent_output=z, xent_targets=t) on the device route against the unfused route and the torch composition.

The bound of the native pass is measured, not chosen: the case's own fp32 distance + 1e-5 (+ u for a 2-byte gradient);
the ChainLoss comparisons use the library's bar, 1e-5 on the value and on max |d grad| / max |grad|, as tests/test_gpu_post_targets.py."""
import numpy as np
import pytest
import torch

import post_reference as pr
import xent_targets_reference as xr
from helpers import record_parity
from pychain_amd import ChainLoss, PosteriorTargets, _lib, native, parallel, posterior_targets, posterior_xent, synthetic as syn

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BAR = xr.BAR
C = 0.1
L2, OOR = 5e-4, 0.01
DTYPES = pr.DTYPES
_REF = {}


def _native(D, K, dname):
    """(z in `dname`, lengths, pdfs, probs, reference on the up-cast values, its fp32 distance): computed once, never changed"""
    key = (D, K, dname)
    if key not in _REF:
        z, lengths, pdfs, probs = pr.native_case(D, K, dname)
        ref = xr.np_xent_targets(z.float().numpy(), lengths, pdfs.numpy(), probs.numpy())
        _REF[key] = (z, lengths, pdfs, probs, ref, xr.fp32_distance(z, lengths, pdfs, probs, ref))
    return _REF[key]


def _run(z, lengths, pdfs, probs, **kw):
    res, bad = native.xent_targets(z.to(DEV), lengths, pdfs.to(DEV), probs.to(DEV), **kw)
    torch.cuda.synchronize()
    return res.objf.cpu(), None if res.grad is None else res.grad.cpu(), int(bad)


def _check_native(D, K, twin=True):
    calls = _lib.lib().pychain_hip_cpu_calls()
    upcast = None
    for dname in ("float32", "bfloat16", "float16"):
        z, lengths, pdfs, probs, ref, own = _native(D, K, dname)
        bo, bg = xr.bound(own, dname)
        objf, grad, bad = _run(z, lengths, pdfs, probs)
        assert bad == 1 == ref[2] and grad.dtype == DTYPES[dname]
        for b, L in enumerate(lengths.tolist()):
            assert not bool(grad[b, L:].any())                        # zeros beyond a length (z is NaN there)
        assert not bool(grad[0, 1].any())                             # the live frame without entries
        d = xr.distances(objf.numpy(), grad.float().numpy(), ref)
        print("D%d K%d %s: objective %.3e (bound %.3e) gradient %.3e (bound %.3e)" % (D, K, dname, d[0], bo, d[1], bg))
        record_parity("xent_targets_D%d_K%d_%s" % (D, K, dname), fp32_objf=own[0], fp32_grad=own[1], objf_rel=d[0], grad_rel=d[1])
        assert d[0] <= bo and d[1] <= bg, (dname, d, bo, bg)
        # the form without the store: the same objectives; a second run: the same bits
        o0, g0, _ = _run(z, lengths, pdfs, probs, with_grad=False)
        o1, g1, _ = _run(z, lengths, pdfs, probs)
        assert g0 is None and torch.equal(pr.bits(o0), pr.bits(objf))
        assert torch.equal(pr.bits(o1), pr.bits(objf)) and torch.equal(pr.bits(g1), pr.bits(grad))
        # the scale: grad_scale * grad_scale_dev / norm, the two read on the device
        o2, g2, _ = _run(z, lengths, pdfs, probs, grad_scale=-0.25, grad_scale_dev=torch.tensor(1.5), norm_dev=torch.tensor(7.0))
        d2 = xr.distances(o2.numpy(), g2.float().numpy() / float(pr.f32_scale(-0.25, 1.5, 7.0)), ref)
        assert torch.equal(o2, objf) and d2[1] <= bg, d2
        if dname != "float32":
            # 2-byte rows read as they are: the bits of the same call on the up-cast fp32 z
            ou, gu, _ = _run(z.float(), lengths, pdfs, probs)
            assert torch.equal(pr.bits(ou), pr.bits(objf)) and torch.equal(pr.bits(gu.to(DTYPES[dname])), pr.bits(grad))
        elif twin:
            # fp32: the device and the host twin agree within the same bound, sequence by sequence
            host, hbad = native.cpu_xent_targets(z, lengths, pdfs, probs)
            calls += 1
            assert int(hbad) == bad
            dh = xr.distances(objf.numpy(), grad.numpy(), (host.objf.numpy().astype(np.float64), host.grad.numpy().astype(np.float64)))
            assert dh[0] <= bo and dh[1] <= bg, dh
            # a frame without entries ignores a NaN row
            zn = z.clone()
            zn[0, 1, :] = float("nan")
            on, gn, _ = _run(zn, lengths, pdfs, probs)
            assert torch.equal(pr.bits(on), pr.bits(objf)) and torch.equal(pr.bits(gn), pr.bits(grad))
    assert _lib.lib().pychain_hip_cpu_calls() == calls                 # device tensors never reach the host twin


@pytest.mark.parametrize("K", [1, 3, 8, 33])
@pytest.mark.parametrize("D", pr.NATIVE_DS)
def test_native_pass_against_reference(D, K):
    _check_native(D, K)


def test_more_entries_than_threads():
    _check_native(257, 300, twin=False)


def test_a_nan_in_a_read_row_reaches_that_sequence_only():
    z, lengths, pdfs, probs, _, _ = _native(8, 3, "float32")
    pdfs = pdfs.clone()
    pdfs[2, 1, 0] = 3
    co, cg, _ = _run(z, lengths, pdfs, probs)
    zn = z.clone()
    zn[2, 1, 5] = float("nan")
    o, g, _ = _run(zn, lengths, pdfs, probs)
    assert bool(torch.isnan(o[2])) and torch.equal(o[:2], co[:2]) and torch.equal(g[:2], cg[:2])
    assert bool(torch.isnan(g[2, 1]).all()) and not bool(torch.isnan(g[2, 0]).any())


def test_a_row_beyond_the_lds_limit_takes_the_rereading_form():
    D, K = 24580, 8
    g = torch.Generator().manual_seed(3)
    z = torch.rand(1, 3, D, generator=g) * 20.0 - 10.0
    z[0, 2] = float("nan")
    lengths = torch.tensor([2])
    pdfs = torch.randint(0, D, (1, 3, K), generator=g).to(torch.int32)
    probs = torch.rand(1, 3, K, generator=g)
    pdfs[0, 0, :3] = D - 1                                             # one pdf three times, the last element of the row
    pdfs[0, 0, 3] = -1
    pdfs[0, 1, 0] = D                                                  # the bad entry
    pdfs[0, 2] = 2 ** 30
    probs[0, 2] = float("nan")
    for dname in ("float32", "bfloat16"):
        zt = z.to(DTYPES[dname])
        ref = xr.np_xent_targets(zt.float().numpy(), lengths, pdfs.numpy(), probs.numpy())
        own = xr.fp32_distance(zt, lengths, pdfs, probs, ref)
        bo, bg = xr.bound(own, dname)
        objf, grad, bad = _run(zt, lengths, pdfs, probs)
        d = xr.distances(objf.numpy(), grad.float().numpy(), ref)
        record_parity("xent_targets_D%d_K%d_%s" % (D, K, dname), fp32_objf=own[0], fp32_grad=own[1], objf_rel=d[0], grad_rel=d[1])
        assert bad == 1 and not bool(grad[0, 2].any()) and d[0] <= bo and d[1] <= bg, (d, bo, bg)
        o0, g0, _ = _run(zt, lengths, pdfs, probs, with_grad=False)
        assert g0 is None and torch.equal(o0, objf)


def test_xent_add_totals_contract():
    objf = torch.tensor([-3.5, 2.25, -100.0, 0.5], device=DEV)
    res = native.XentResult()
    res.objf, res.grad = objf, None
    before = torch.arange(8, dtype=torch.float32) + 0.5
    S = float(objf.double().sum())
    for norm in (None, torch.tensor(7.0)):
        for bad in (None, torch.tensor([3], dtype=torch.int32, device=DEV)):
            totals = before.to(DEV)
            native.xent_add_totals(res, bad, 0.5, norm, -0.1, totals)
            torch.cuda.synchronize()
            t, xt = totals.cpu(), res.totals.cpu()
            scaled = 0.5 * S / (1.0 if norm is None else 7.0)
            assert float(xt[1]) == float(np.float32(S)) and abs(float(xt[0]) - scaled) <= 2.0 ** -23 * abs(scaled)
            want = 0.5 - 0.1 * scaled
            assert abs(float(t[0]) - want) <= 2.0 ** -22 * (abs(want) + 0.5) and torch.equal(pr.bits(t[0:1]), pr.bits(t[4:5]))
            assert float(t[2]) == 2.5 + (0 if bad is None else 3)
            for i in (1, 3, 5, 6, 7):
                assert torch.equal(pr.bits(t[i:i + 1]), pr.bits(before[i:i + 1])), i
    native.xent_add_totals(res)                                        # no totals of a step: the two sums alone
    torch.cuda.synchronize()
    assert float(res.totals[1]) == float(np.float32(S)) == float(res.totals[0])


# ---- through ChainLoss ----------------------------------------------------------------------------------------------------------
LENGTHS = torch.tensor([37, 40, 9, 33])
_CASE = {}


def _case(D=40, T=40, k=6):
    """(x, z, lengths, targets on the host, the denominator graph): computed once and shared, never changed"""
    if (D, T) not in _CASE:
        lengths = LENGTHS if T == 40 else torch.tensor([T, T - 7, 9, T - 1])
        den = syn.make_den_graph(20, 60, D, seed=0)
        x = syn.make_input(4, T, D, seed=5)
        teacher = syn.make_input(4, T, D, seed=55) * 1.5
        z = syn.make_input(4, T, D, seed=75) * 1.5
        _CASE[(D, T)] = (x, z, lengths, posterior_targets(teacher, lengths, den, k), den)
    return _CASE[(D, T)]


class _Run(object):
    def __init__(self, den, x, z, lengths, targets, fused=True, lengths_dev=False, twice=False, avg=True, reg=False, u=None, f=None,
                 c=C, cls=ChainLoss):
        xd = x.to(DEV).requires_grad_(True)
        zd = None if z is None else z.to(DEV).requires_grad_(True)
        kw = dict(output_l2_regularize=L2, out_of_range_regularize=OOR) if reg else {}
        crit = cls(den, 1e-5, avg=avg, xent_regularize=c, **kw)
        if cls is ChainLoss:
            crit.fused = fused
        ld = lengths.to(DEV) if lengths_dev else lengths
        if zd is None:
            loss = crit(xd, ld, targets, utt_weights=u, deriv_weights=f)
        else:
            loss = crit(xd, ld, targets, xent_output=zd, utt_weights=u, deriv_weights=f, xent_targets=targets)
        if twice:
            loss.backward(retain_graph=True)
            self.first = (xd.grad.clone(), zd.grad.clone())
            xd.grad = zd.grad = None
        loss.backward()
        torch.cuda.synchronize()
        self.loss, self.gx, self.out = loss.detach().cpu(), xd.grad.cpu(), loss
        self.gz = None if zd is None or zd.grad is None else zd.grad.cpu()


def _composition(den, x, z, lengths, targets, avg=True, u=None, f=None, reg=None, c=C):
    """(loss, d loss / dx, d loss / dz) by the torch composition on the device: post_reference.composition (fp32) for the LF-MMI
    part, log_softmax + the gathered entries (fp64) for the xent term; the weights on the rows and the per-sequence terms."""
    value, gx = pr.composition(den, x.to(DEV), lengths, targets, avg, u, f, reg, dtype=torch.float32)
    B, T = x.size(0), x.size(1)
    z64 = z.to(DEV).double().requires_grad_(True)
    per = xr.torch_xent_per_seq(z64, lengths, targets.pdfs, targets.probs)
    per.sum().backward()
    ud = torch.ones(B, dtype=torch.float64) if u is None else u.double()
    n = float((ud * lengths).sum()) if avg else 1.0
    w = ud[:, None] * (torch.ones(B, T, dtype=torch.float64) if f is None else f.double())
    gz = -c * z64.grad.cpu() * w[..., None] / n
    xent = float(torch.where(ud != 0, ud * per.detach().cpu(), torch.zeros(())).sum()) / n
    return value - c * xent, gx, gz.numpy(), xent


def _hold(name, run, want, bar=BAR):
    d = pr.distances(run.loss, run.gx.float().numpy(), want[0], want[1])
    dz = float(np.abs(run.gz.float().numpy() - want[2]).max() / np.abs(want[2]).max())
    print("%s: loss %.3g, gradient %.3g, xent gradient %.3g (bar %.0e)" % (name, d[0], d[1], dz, bar))
    record_parity("xent_targets_" + name, loss=d[0], grad=d[1], zgrad=dz)
    assert max(d) <= bar and dz <= bar, (name, d, dz)


def _as_want(run):
    return float(run.loss), run.gx.numpy().astype(np.float64), run.gz.numpy().astype(np.float64)


def test_device_route_against_unfused_and_the_torch_composition():
    x, z, lengths, targets, den = _case()
    calls = _lib.lib().pychain_hip_cpu_calls()
    on, off = _Run(den, x, z, lengths, targets), _Run(den, x, z, lengths, targets, fused=False)
    comp = _composition(den, x, z, lengths, targets)
    assert _lib.lib().pychain_hip_cpu_calls() == calls
    _hold("fused_vs_composition", on, comp)
    _hold("unfused_vs_composition", off, comp)
    _hold("fused_vs_unfused", on, _as_want(off))
    assert on.gz.dtype == torch.float32
    for b, L in enumerate(lengths.tolist()):
        assert not bool(on.gz[b, L:].any())
    assert abs(float(on.out.xent_objf) - comp[3]) <= BAR * abs(comp[3])
    # y.grad with the term is y.grad without it, bit for bit; so are the other statistics of the step
    plain = _Run(den, x, None, lengths, targets)
    assert torch.equal(pr.bits(on.gx), pr.bits(plain.gx))
    ta, tp = on.out.totals_all.cpu(), plain.out.totals_all.cpu()
    for i in (1, 2, 3, 5, 6, 7):
        assert torch.equal(pr.bits(ta[i:i + 1]), pr.bits(tp[i:i + 1])), i
    # what ShardedChainLoss would all-reduce: the full loss
    assert float(ta[0]) == float(ta[4]) == float(on.loss) and float(ta[1]) == float(lengths.sum())
    assert tuple(on.out.bad_count.shape) == (3,) and int(on.out.bad_count.sum()) == 0 and tuple(plain.out.bad_count.shape) == (2,)
    # c == 0: the call without the term
    zero = _Run(den, x, z, lengths, targets, c=0.0)
    assert zero.gz is None and torch.equal(zero.loss, plain.loss) and torch.equal(pr.bits(zero.gx), pr.bits(plain.gx))
    # the same step gives the same bits
    again = _Run(den, x, z, lengths, targets)
    assert torch.equal(again.loss, on.loss) and torch.equal(pr.bits(again.gz), pr.bits(on.gz))


def test_with_both_regularisers_and_both_weights_and_lengths_on_the_device():
    x, z, lengths, targets, den = _case()
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.05
    x = torch.where(far, torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0, x)
    u = torch.tensor([1.0, 0.5, 0.25, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    f[0, :5], f[1, 3] = 1.0, 0.0
    for avg in (True, False):
        comp = _composition(den, x, z, lengths, targets, avg, u, f, (L2, OOR))
        on = _Run(den, x, z, lengths, targets, avg=avg, reg=True, u=u, f=f)
        off = _Run(den, x, z, lengths, targets, avg=avg, fused=False, reg=True, u=u, f=f)
        _hold("weights_reg_avg%d_fused_vs_composition" % avg, on, comp)
        _hold("weights_reg_avg%d_fused_vs_unfused" % avg, on, _as_want(off))
        assert abs(float(on.out.xent_objf) - comp[3]) <= BAR * abs(comp[3])      # the weighted amount
        assert not bool(on.gz[1, 3].any())                             # a frame of derivative weight 0
    comp = _composition(den, x, z, lengths, targets, True, u, f, (L2, OOR))
    _hold("devlen_weights_reg_vs_composition", _Run(den, x, z, lengths, targets, lengths_dev=True, reg=True, u=u, f=f), comp)
    x0, z0, _, _, _ = _case()
    _hold("devlen_vs_composition", _Run(den, x0, z0, lengths, targets, lengths_dev=True), _composition(den, x0, z0, lengths, targets))


def test_second_backward_over_a_retained_graph():
    x, z, lengths, targets, den = _case()
    for kw in (dict(), dict(fused=False), dict(lengths_dev=True), dict(reg=True, u=torch.tensor([1.0, 0.5, 0.25, 2.0]))):
        r = _Run(den, x, z, lengths, targets, twice=True, **kw)
        assert torch.equal(r.first[0].cpu(), r.gx) and torch.equal(r.first[1].cpu(), r.gz), kw


def test_bf16_outputs():
    """y and z in bf16 (D % 8 == 0: both go to the kernels as they are).  z's gradient has the bits of the fp32 run on the same
    values, rounded once; the value lies within the bar of it."""
    x, z, lengths, targets, den = _case()
    xh, zh = x.to(torch.bfloat16), z.to(torch.bfloat16)
    on, ref = _Run(den, xh, zh, lengths, targets), _Run(den, xh.float(), zh.float(), lengths, targets)
    assert on.gx.dtype == torch.bfloat16 and on.gz.dtype == torch.bfloat16
    assert torch.equal(pr.bits(on.gz), pr.bits(ref.gz.to(torch.bfloat16))) and bool(on.gz.any())
    assert abs(float(on.loss) - float(ref.loss)) <= BAR * abs(float(ref.loss))
    assert torch.equal(pr.bits(on.gx), pr.bits(_Run(den, xh, None, lengths, targets).gx))


def test_c3_row_width():
    x, z, lengths, targets, den = _case(D=3456, T=64, k=8)
    _hold("c3_width_fused_vs_composition", _Run(den, x, z, lengths, targets), _composition(den, x, z, lengths, targets))


def test_posterior_xent_and_the_sharded_loss_on_the_device():
    x, z, lengths, targets, den = _case()
    zd = z.to(DEV).requires_grad_(True)
    out = posterior_xent(zd, lengths, targets)
    (2.0 * out).backward()
    z64 = z.double().clone().requires_grad_(True)
    per = xr.torch_xent_per_seq(z64, lengths, targets.pdfs, targets.probs)
    (2.0 * per.sum()).backward()
    d = pr.distances(out.detach().cpu(), zd.grad.cpu().numpy(), float(per.detach().sum()), z64.grad.numpy())
    record_parity("xent_targets_posterior_xent_device", loss=d[0], grad=d[1])
    assert max(d) <= BAR and int(out.bad_count) == 0, d
    one = _Run(den, x, z, lengths, targets)
    sharded = _Run(den, x, z, lengths, targets, cls=parallel.ShardedChainLoss)
    _hold("sharded_world_of_one", sharded, _as_want(one))
