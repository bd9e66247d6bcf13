"""Posterior-target supervision (include/pychain_hip.h: pychain_hip_post_targets, pychain_hip_topk_rows; csrc/post.hip) on the
MI355X against tests/post_reference.  Through native.post_targets: rows of 1 .. 3456 pdfs, 1 .. 33 entries per frame (more
entries than pdfs included), fp32 / bf16 / fp16, the objective alone, the gradient over a known pattern, the device-side
scalars, the totals contract, padding that is never read, a frame without entries, a pdf three times in a frame, one bad entry;
the fp32 gradient bit for bit the host twin's and the same from run to run.  Through native.topk_rows: ties, NaNs, a floor that
leaves slots empty, normalised and not, rows held on chip and a row that is not.  Through ChainLoss: the device route against
fused = False and against the torch composition it replaces.

The native bounds are derived (tests/post_reference.py).  The ChainLoss comparisons use the library's fp64 bar, 1e-5 on the value
and on max |d grad| / max |grad|.  Every measured distance goes through helpers.record_parity."""
import numpy as np
import pytest
import torch

import post_reference as pr
from helpers import record_parity
from pychain_amd import (ChainLoss, PosteriorTargets, _lib, native, occupancies, posterior_numerator, posterior_targets,
                         synthetic as syn)

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BAR = 1e-5
L2, OOR = 5e-4, 0.01
DTYPES = pr.DTYPES


def _ratio(got, want, bound, mask):
    return float((np.abs(got.astype(np.float64) - want)[mask] / np.maximum(bound[mask], 1e-300)).max()) if mask.any() else 0.0


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("D", pr.NATIVE_DS)
def test_native_pass(D, dname):
    L = _lib.lib()
    worst = dict(objf=0.0, grad=0.0)
    for K in pr.NATIVE_KS:
        x, lengths, pdfs, probs = pr.native_case(D, K, dname)
        xf = x.float().numpy()
        xd, pd, q = x.to(DEV), pdfs.to(DEV), probs.to(DEV)
        pat = pr.grad_pattern(x.shape, dname)
        calls = L.pychain_hip_cpu_calls()
        ref0 = pr.np_post_targets(xf, lengths, pdfs.numpy(), probs.numpy())
        num, bad = native.post_targets(xd, lengths, pd, q)                                # the objective only
        assert int(bad) == 1 == ref0["bad"]
        ok = ~np.isnan(ref0["num"])
        r = _ratio(num.cpu().numpy(), ref0["num"], pr.objf_bound(ref0), ok)
        print("D=%d K=%d %s: objective %.3f of its bound" % (D, K, dname, r))
        worst["objf"] = max(worst["objf"], r)
        results = []
        for gsd, norm in ((None, None), (1.5, None), (None, 7.0), (1.5, 7.0)):
            s = pr.f32_scale(-0.25, gsd, norm)
            ref = pr.np_post_targets(xf, lengths, pdfs.numpy(), probs.numpy(), grad=pat.float().numpy(), s=s)
            kw = dict(grad_scale=-0.25, loss_scale=0.5,
                      grad_scale_dev=None if gsd is None else torch.tensor(gsd, device=DEV),
                      norm_dev=None if norm is None else torch.tensor(norm, device=DEV))
            den = torch.tensor([-3.5, 2.25, -1.0], device=DEV)
            g = pat.to(DEV)
            totals = torch.arange(8, dtype=torch.float32, device=DEV) + 0.5
            num2, bad2 = native.post_targets(xd, lengths, pd, q, grad=g, den_objf=den, totals=totals, **kw)
            assert torch.equal(num2, num) and int(bad2) == 1                              # (the sums do not depend on the scalars)
            t = ref["touched"]
            gc = g.cpu()
            r = _ratio(gc.float().numpy(), ref["want"], pr.grad_bound(ref["want"], dname), t)
            print("D=%d K=%d %s scalars %s: gradient %.3f of its bound" % (D, K, dname, (gsd, norm), r))
            worst["grad"] = max(worst["grad"], r)
            assert np.array_equal(pr.bits(gc).numpy()[~t], pr.bits(pat).numpy()[~t])      # untouched elements keep their bits
            want, keep = pr.np_totals(den.cpu().numpy(), ref, np.arange(8) + 0.5, 0.5, norm)
            tot = totals.cpu().numpy().astype(np.float64)
            b3, b0 = pr.totals_bounds(want, ref)
            assert abs(tot[3] - want[3]) <= b3 and abs(tot[0] - want[0]) <= b0 and tot[0] == tot[4], (tot, want)
            assert tot[2] == want[2] and all(tot[i] == i + 0.5 for i in keep)
            # the same call gives the same bits
            g2 = pat.to(DEV)
            num3, _ = native.post_targets(xd, lengths, pd, q, grad=g2, den_objf=den, totals=totals.clone(), **kw)
            assert torch.equal(pr.bits(g2), pr.bits(g)) and torch.equal(num3, num)
            results.append((gsd, norm, gc))
        torch.cuda.synchronize()
        assert L.pychain_hip_cpu_calls() == calls                                         # device tensors never reach the host twin
        if dname == "float32":
            # the host twin: the same fma on the same operands, so the same gradient bits
            for gsd, norm, gc in results:
                hg = pat.clone()
                native.cpu_post_targets(x, lengths, pdfs, probs, grad=hg, grad_scale=-0.25, grad_scale_dev=gsd, norm=norm)
                assert torch.equal(pr.bits(hg), pr.bits(gc)), (K, gsd, norm)
    record_parity("post_native_D%d_%s" % (D, dname), **worst)
    assert worst["objf"] <= 1.0 and worst["grad"] <= 1.0, worst


def test_a_nan_in_a_referenced_live_element_reaches_that_sequence_only():
    x, lengths, pdfs, probs = pr.native_case(8, 4)
    pdfs[2, 1, 0] = 3
    clean, _ = native.post_targets(x.to(DEV), lengths, pdfs.to(DEV), probs.to(DEV))
    x[2, 1, 3] = float("nan")
    num, _ = native.post_targets(x.to(DEV), lengths, pdfs.to(DEV), probs.to(DEV))
    assert bool(torch.isnan(num[2])) and torch.equal(num[:2], clean[:2])


def test_bad_arguments_are_refused():
    x, lengths, pdfs, probs = pr.native_case(8, 4)
    L = _lib.lib()
    xd, ld, pd, q = x.to(DEV), lengths.to(DEV), pdfs.to(DEV), probs.to(DEV)
    num, bad = torch.empty(3, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.pychain_hip_post_targets_workspace_bytes(3, 9), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda K, grad, wsp, nbytes, totals=None: L.pychain_hip_post_targets(
        xd.data_ptr(), _lib.F32, ld.data_ptr(), 3, 9, 8, pd.data_ptr(), q.data_ptr(), K, grad, 1.0, None, None, None, num.data_ptr(),
        bad.data_ptr(), 1.0, totals, wsp, nbytes, st)
    g = torch.zeros(3, 9, 8, device=DEV)
    assert call(0, None, ws.data_ptr(), ws.numel()) == -1                                  # K < 1
    assert call(4, g.data_ptr() + 4, ws.data_ptr(), ws.numel()) == -1                      # grad not 16-byte aligned
    assert call(4, None, ws.data_ptr() + 8, ws.numel() - 8) == -1                          # workspace not 16-byte aligned
    assert call(4, None, None, ws.numel()) == -1                                           # a required pointer
    assert call(4, None, ws.data_ptr(), ws.numel(), torch.zeros(8, device=DEV).data_ptr()) == -1    # totals without den_objf_per_seq
    assert call(4, None, ws.data_ptr(), 16) == -3
    assert call(4, None, ws.data_ptr(), ws.numel()) == 0
    op, ov = torch.empty(3, 9, 9, dtype=torch.int32, device=DEV), torch.empty(3, 9, 9, device=DEV)
    for K in (0, 9):
        assert L.pychain_hip_topk_rows(xd.data_ptr(), _lib.F32, ld.data_ptr(), 3, 9, 8, K, 0.0, 1, op.data_ptr(), ov.data_ptr(), st) == -1
    wide = torch.zeros(1, 1, 80, device=DEV)
    assert L.pychain_hip_topk_rows(wide.data_ptr(), _lib.F32, ld.data_ptr(), 1, 1, 80, 65, 0.0, 1, op.data_ptr(), ov.data_ptr(), st) == -1
    torch.cuda.synchronize()


# (9217: one element more than a row held on chip - the form that re-reads the row from memory)
@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("D", pr.NATIVE_DS + [9217])
def test_topk_rows(D, dname):
    rows, lengths = pr.topk_case(D, dname)
    rf = rows.float().numpy()
    rd = rows.to(DEV)
    calls = _lib.lib().pychain_hip_cpu_calls()
    ks = sorted({1, min(3, D), min(8, D), min(D, 64)}) if D <= 3456 else [8, 64]
    combos = ((0.0, True), (0.0, False), (0.3, True), (float("-inf"), False)) if D <= 3456 else ((0.0, True), (0.3, False))
    for K in ks:
        for floor, normalize in combos:
            want_p, want_v = pr.np_topk(rf, lengths, K, floor, normalize)
            got_p, got_v = native.topk_rows(rd, lengths, K, floor, normalize)
            assert np.array_equal(got_p.cpu().numpy(), want_p), (K, floor, normalize)
            assert pr.topk_values_ok(got_v.cpu().numpy(), want_v, normalize), (K, floor, normalize)
    # ties: a whole row of equal values gives the lowest indices, in order; a row below the floor stays empty
    k3 = min(D, 3)
    p, v = native.topk_rows(rd, lengths, k3, 0.0, False)
    p, v = p.cpu(), v.cpu()
    assert p[0, 0].tolist() == list(range(k3))
    if D > 2:
        assert p[0, 4].tolist() == [-1] * 3 and v[0, 4].tolist() == [0.0] * 3
    assert bool((p[1, 1:] == -1).all()) and bool((v[1, 1:] == 0).all())                    # padded frames are written -1 / 0
    assert _lib.lib().pychain_hip_cpu_calls() == calls


# ---- through ChainLoss ----------------------------------------------------------------------------------------------------------
D0 = 40
LENGTHS = torch.tensor([37, 40, 9, 33])
_CASE = {}


def _case(D=D0, T=40, k=6):
    """(x, lengths, targets on the host, the denominator graph): computed once and shared, never changed"""
    if (D, T) not in _CASE:
        lengths = LENGTHS if T == 40 else torch.tensor([T, T - 7, 9, T - 1])
        den = syn.make_den_graph(20, 60, D, seed=0)
        x = syn.make_input(4, T, D, seed=5)
        teacher = syn.make_input(4, T, D, seed=55) * 1.5
        _CASE[(D, T)] = (x, lengths, posterior_targets(teacher, lengths, den, k), den)
    return _CASE[(D, T)]


class _Run(object):
    def __init__(self, den, x, lengths, targets, fused=True, lengths_dev=False, twice=False, avg=True, reg=False, u=None, f=None):
        xd = x.to(DEV).requires_grad_(True)
        kw = dict(output_l2_regularize=L2, out_of_range_regularize=OOR) if reg else {}
        crit = ChainLoss(den, 1e-5, avg=avg, **kw)
        crit.fused = fused
        loss = crit(xd, lengths.to(DEV) if lengths_dev else lengths, targets, utt_weights=u, deriv_weights=f)
        if twice:
            loss.backward(retain_graph=True)
            self.first = xd.grad.clone()
            xd.grad = None
        loss.backward()
        torch.cuda.synchronize()
        self.loss, self.gx, self.out = loss.detach().cpu(), xd.grad.cpu(), loss


def _hold(name, run, want):
    d = pr.distances(run.loss, run.gx.float().numpy(), *want)
    print("%s: loss %.3g, gradient %.3g (bar %.0e)" % (name, d[0], d[1], BAR))
    record_parity("post_" + name, loss=d[0], grad=d[1])
    assert max(d) <= BAR, (name, d)


def test_device_route_against_unfused_and_the_torch_composition():
    x, lengths, targets, den = _case()
    calls = _lib.lib().pychain_hip_cpu_calls()
    on, off = _Run(den, x, lengths, targets), _Run(den, x, lengths, targets, fused=False)
    comp = pr.composition(den, x.to(DEV), lengths, targets, dtype=torch.float32)          # on the device
    assert _lib.lib().pychain_hip_cpu_calls() == calls
    _hold("fused_vs_composition", on, comp)
    _hold("unfused_vs_composition", off, comp)
    _hold("fused_vs_unfused", on, (float(off.loss), off.gx.numpy().astype(np.float64)))
    assert on.gx.dtype == torch.float32
    for b, L in enumerate(lengths.tolist()):
        assert not bool(on.gx[b, L:].any())
    # what the call reports: the totals of a fused call, the two bad counts
    tot = on.out.totals_all.cpu()
    assert float(tot[0]) == float(tot[4]) == float(on.loss) and float(tot[1]) == float(lengths.sum()) and float(tot[2]) == 0.0
    assert abs(float(tot[3]) / float(lengths.sum()) - float(on.loss)) <= 2.0 ** -22 * abs(float(on.loss))
    assert tuple(on.out.bad_count.shape) == (2,) and on.out.bad_count.dtype == torch.int32 and int(on.out.bad_count.sum()) == 0
    assert off.out.totals is None


def test_with_both_regularisers_and_both_weights():
    x, lengths, targets, den = _case()
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.05
    x = torch.where(far, torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0, x)
    u = torch.tensor([1.0, 0.5, 0.25, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    f[0, :5], f[1, 3] = 1.0, 0.0
    comp = pr.composition(den, x.to(DEV), lengths, targets, True, u, f, (L2, OOR), dtype=torch.float32)
    on = _Run(den, x, lengths, targets, reg=True, u=u, f=f)
    off = _Run(den, x, lengths, targets, fused=False, reg=True, u=u, f=f)
    _hold("weights_reg_fused_vs_composition", on, comp)
    _hold("weights_reg_fused_vs_unfused", on, (float(off.loss), off.gx.numpy().astype(np.float64)))
    n = float((u * lengths).sum())
    assert abs(float(on.out.weighted_frames) - n) <= 2.0 ** -23 * n
    assert float(on.out.l2_term) > 0 and float(on.out.out_of_range_term) > 0
    assert not bool(on.gx[1, 3].any())                                                      # a frame of derivative weight 0


def test_bf16_network_output():
    """x in bf16 with D % 8 == 0 goes to the kernels as it is; the gradient comes back in bf16, rounded twice.  Against the fp32
    run on the SAME values, with u = 2^-8: the denominator call rounds its own gradient g_den = gamma_den / N to bf16 where it
    stores it - u |g_den|, NOT u |g|: where gamma_den and q nearly cancel the error stays that of the larger operand -, the pass
    rounds its one fma (2^-24, then u to bf16) on the result - (u + 2^-23) |g| -, and the two fp32 evaluations differ by no more
    than the bar: u |g_den| + (u + 2^-23) |g| + bar * max |g|, g_den = g + q / N from the fp32 run.  The value within the bar."""
    x, lengths, targets, den = _case()
    xh = x.to(torch.bfloat16)
    on, ref = _Run(den, xh, lengths, targets), _Run(den, xh.float(), lengths, targets)
    assert on.gx.dtype == torch.bfloat16
    g, want = on.gx.float().numpy().astype(np.float64), ref.gx.numpy().astype(np.float64)
    q = torch.zeros(x.shape, dtype=torch.float64)
    q.scatter_add_(2, targets.pdfs.clamp_min(0).to(torch.int64), torch.where(targets.pdfs >= 0, targets.probs.double(), torch.zeros((), dtype=torch.float64)))
    g_den = want + q.numpy() / float(lengths.sum())
    u = 2.0 ** -8
    bound = u * np.abs(g_den) + (u + 2.0 ** -23) * np.abs(want) + BAR * np.abs(want).max()
    r = float((np.abs(g - want) / bound).max())
    d_loss = abs(float(on.loss) - float(ref.loss)) / abs(float(ref.loss))
    print("bf16: loss %.3g (bar %.0e), gradient %.3f of its bound" % (d_loss, BAR, r))
    record_parity("post_bf16", loss=d_loss, grad=r)
    assert d_loss <= BAR and r <= 1.0, (d_loss, r)


def test_lengths_on_the_device():
    x, lengths, targets, den = _case()
    comp = pr.composition(den, x.to(DEV), lengths, targets, dtype=torch.float32)
    _hold("devlen_fused_vs_composition", _Run(den, x, lengths, targets, lengths_dev=True), comp)
    u = torch.tensor([1.0, 0.5, 0.25, 2.0])
    comp = pr.composition(den, x.to(DEV), lengths, targets, True, u, None, (L2, OOR), dtype=torch.float32)
    _hold("devlen_weights_reg_vs_composition", _Run(den, x, lengths, targets, lengths_dev=True, reg=True, u=u), comp)


def test_second_backward_over_a_retained_graph():
    x, lengths, targets, den = _case()
    for kw in (dict(), dict(fused=False), dict(lengths_dev=True), dict(reg=True, u=torch.tensor([1.0, 0.5, 0.25, 2.0]))):
        r = _Run(den, x, lengths, targets, twice=True, **kw)
        assert torch.equal(r.first.cpu(), r.gx), kw


def test_an_utterance_of_weight_zero_whose_targets_reference_a_nan_contributes_exactly_zero():
    x, lengths, targets, den = _case()
    u = torch.tensor([1.0, 0.0, 1.0, 1.0])
    d = int(targets.pdfs[1, 2][targets.pdfs[1, 2] >= 0][0])
    xn = x.clone()
    xn[1, 2, d] = float("nan")
    other = x.clone()
    other[1] = syn.make_input(1, 40, D0, seed=77)[0]                                        # another utterance in its place
    a, b = _Run(den, xn, lengths, targets, u=u), _Run(den, other, lengths, targets, u=u)
    assert np.isfinite(float(a.loss)) and torch.equal(a.loss, b.loss)
    assert not bool(a.gx[1].any()) and not bool(torch.isnan(a.gx).any())
    assert torch.equal(pr.bits(a.gx[[0, 2, 3]]), pr.bits(b.gx[[0, 2, 3]]))


def test_c3_row_width():
    x, lengths, targets, den = _case(D=3456, T=64, k=8)
    comp = pr.composition(den, x.to(DEV), lengths, targets, dtype=torch.float32)
    _hold("c3_width_fused_vs_composition", _Run(den, x, lengths, targets), comp)


def test_posterior_numerator_on_the_device():
    x, lengths, targets, _ = _case()
    xd = x.to(DEV).requires_grad_(True)
    out = posterior_numerator(xd, lengths, targets)
    (2.0 * out).backward()
    x64 = x.double().clone().requires_grad_(True)
    per = pr.torch_numerator_per_seq(x64, lengths, targets.pdfs, targets.probs)
    (2.0 * per.sum()).backward()
    d = pr.distances(out.detach().cpu(), xd.grad.cpu().numpy(), float(per.detach().sum()), x64.grad.numpy())
    record_parity("post_numerator_device", loss=d[0], grad=d[1])
    assert max(d) <= BAR, d


def test_targets_with_k_equal_d_reproduce_the_occupancies_and_the_teacher_student_gradient():
    D = 8
    den = syn.make_den_graph(5, 14, D, seed=1)
    lengths = torch.tensor([12, 7])
    teacher, student = syn.make_input(2, 12, D, seed=2).to(DEV), syn.make_input(2, 12, D, seed=3).to(DEV)
    occ_t = occupancies(teacher, lengths, den)
    t = posterior_targets(teacher, lengths, den, D, normalize=False)
    assert isinstance(t, PosteriorTargets) and t.pdfs.is_cuda and t.pdfs.dtype == torch.int32
    dense = torch.zeros(2, 12, D, device=DEV)
    dense.scatter_add_(2, t.pdfs.clamp_min(0).to(torch.int64), torch.where(t.pdfs >= 0, t.probs, torch.zeros((), device=DEV)))
    assert torch.equal(dense, torch.where(occ_t >= 0, occ_t, torch.zeros((), device=DEV)).float())
    xs = student.clone().requires_grad_(True)
    ChainLoss(den, 1e-5, avg=False)(xs, lengths, t).backward()
    want = (occupancies(student, lengths, den).double() - occ_t.double()).cpu().numpy()
    d = float(np.abs(xs.grad.cpu().numpy() - want).max() / np.abs(want).max())
    record_parity("post_teacher_student", grad=d)
    assert d <= BAR, d
