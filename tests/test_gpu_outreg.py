"""Output L2 and the out-of-range penalty (include/pychain_hip.h: pychain_hip_output_reg; csrc/outreg.hip) on the MI355X against
tests/outreg_reference.np_outreg.  Through native.output_reg: every load form (rows of 1 .. 3456 elements, fp32 / bf16 / fp16),
the three gradient forms (objective only, ACCUM over a known pattern, LINEAR), the device-side scalars, padding that is never
read, a NaN in a live row.  Through ChainLoss: every route the term takes (fused speculative, overlap = False, fused = False,
with an xent output, with time windows, in slices), a second backward, device-side lengths, the C3 row width and length.

The bounds are derived, not chosen (tests/outreg_reference.py): 2^-23 for a sum (fp64 accumulation, at most two roundings to
fp32), 2^-22 for the loss scalar, and for the gradient 2^-24 |ref| + 8 * 2^-24 |s| (l2 |x| + 2 oor e) - the 7 fp32 roundings of
the operation sequence csrc/outreg.hip writes down, plus one - with u |ref| on top for a 2-byte gradient (u = 2^-8 bf16, 2^-11
fp16, and 2^-25 absolute for fp16 subnormals).  Every measured distance goes through helpers.record_parity as a fraction of
its bound."""
import numpy as np
import pytest
import torch

from helpers import long_case, record_parity
from outreg_reference import LOSS_REL, SUM_REL, grad_bound, np_outreg, term_magnitude, term_rel, worst_ratio
from pychain_amd import (ChainLoss, ChainLossFunction, _lib, alignment_windows, native, output_regularizer, viterbi_align,
                         synthetic as syn)

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
L2, OOR = 5e-4, 0.01
DS = [1, 3, 4, 7, 8, 255, 256, 257, 1028, 3456]
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def _x(B, T, D, dtype, seed=3):
    """Uniform in +-40 (both signs beyond the clamp), with exact +-30 and a -0.0 in live rows of sequence 0."""
    g = torch.Generator().manual_seed(seed + D)
    x = (torch.rand(B, T, D, generator=g) * 80.0 - 40.0).float()
    if T >= 3:
        x[0, 0, 0], x[0, 1, D - 1], x[0, 2, D // 2] = 30.0, -30.0, -0.0
    return x.to(dtype)


def _pattern(shape, dtype):
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 251.0) * 0.01 - 1.0).reshape(shape).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check_sums(res, ref, loss_scale, norm):
    R2, RO, _, loss = ref
    per = res.per_seq.cpu().numpy().astype(np.float64)
    tot = res.totals.cpu().numpy().astype(np.float64)
    d = [float((np.abs(per[:, 0] - R2) / (SUM_REL * R2)).max()),
         float(np.where(RO > 0, np.abs(per[:, 1] - RO) / np.where(RO > 0, SUM_REL * RO, 1.0), np.where(per[:, 1] == 0, 0.0, np.inf)).max()),
         abs(tot[1] - R2.sum()) / (SUM_REL * R2.sum()),
         abs(tot[2] - RO.sum()) / (SUM_REL * RO.sum()) if RO.sum() > 0 else (0.0 if tot[2] == 0 else np.inf)]
    want = loss_scale * loss / norm
    d.append(abs(tot[0] - want) / (SUM_REL * abs(want)) if want else (0.0 if tot[0] == 0 else np.inf))
    assert max(d) <= 1.0, d
    return max(d)


def _native_case(B, T, D, dname, lengths):
    dtype = DTYPES[dname]
    x = _x(B, T, D, dtype)
    for b, L in enumerate(lengths.tolist()):               # NaNs in every padded row change nothing: those rows are never read
        x[b, L:, :] = float("nan")
    xf = x.float().numpy()
    ref = np_outreg(xf, lengths, L2, OOR)
    mag = term_magnitude(xf, lengths, L2, OOR)
    xd = x.to(DEV)
    pat = _pattern(x.shape, dtype)
    calls = _lib.lib().pychain_hip_cpu_calls()
    worst = dict(sums=0.0, linear=0.0, accum=0.0)
    first = None
    for gs_dev, norm in ((None, None), (1.5, None), (None, 7.0), (1.5, 7.0)):
        s = 0.25 * (gs_dev or 1.0) / (norm or 1.0)
        kw = dict(grad_scale=0.25, loss_scale=0.5,
                  grad_scale_dev=None if gs_dev is None else torch.tensor(gs_dev, device=DEV),
                  norm_dev=None if norm is None else torch.tensor(norm, device=DEV))
        # LINEAR: s * term on live rows, exact zeros beyond the lengths; the totals of a fused call get the scaled term added
        totals = torch.arange(8, dtype=torch.float32, device=DEV) + 0.5
        lin = native.output_reg(xd, lengths, L2, OOR, totals=totals, **kw)
        worst["sums"] = max(worst["sums"], _check_sums(lin, ref, 0.5, norm or 1.0))
        assert lin.grad.dtype == dtype
        want = s * ref[2]
        worst["linear"] = max(worst["linear"], worst_ratio(lin.grad.float().cpu().numpy(), want, grad_bound(want, mag, s, dname)))
        tot = totals.cpu().numpy().astype(np.float64)
        full = 0.5 + 0.5 * ref[3] / (norm or 1.0)
        assert abs(tot[0] - full) <= LOSS_REL * abs(full) and tot[0] == tot[4] and list(tot[[1, 2, 3, 5, 6, 7]]) == [1.5, 2.5, 3.5, 5.5, 6.5, 7.5]
        # ACCUM over a known pattern: live rows get the term, rows beyond the lengths keep their bits
        g = pat.to(DEV)
        acc = native.output_reg(xd, lengths, L2, OOR, grad=g, grad_mode=_lib.GRAD_ACCUM, **kw)
        assert acc.grad is g and torch.equal(acc.per_seq, lin.per_seq) and torch.equal(acc.totals, lin.totals)
        want = pat.float().numpy().astype(np.float64) + s * ref[2]
        worst["accum"] = max(worst["accum"], worst_ratio(g.float().cpu().numpy(), want, grad_bound(want, mag, s, dname)))
        for b, L in enumerate(lengths.tolist()):
            assert torch.equal(_bits(g[b, L:].cpu()), _bits(pat[b, L:])), b
            assert not bool(lin.grad[b, L:].cpu().float().abs().sum() != 0) and not bool(torch.isnan(lin.grad[b, L:].float()).any()), b
        # the same call gives the same bits
        again = native.output_reg(xd, lengths, L2, OOR, **kw)
        assert torch.equal(_bits(again.grad), _bits(lin.grad)) and torch.equal(again.per_seq, lin.per_seq) and torch.equal(again.totals, lin.totals)
        if first is None:
            first = lin
        assert torch.equal(lin.per_seq, first.per_seq)      # (the sums do not depend on the scalars)
    # the objective-only form: the same sums, bit for bit, nothing else written
    obj = native.output_reg(xd, lengths, L2, OOR, with_grad=False, loss_scale=0.5)
    assert obj.grad is None and torch.equal(obj.per_seq, first.per_seq) and torch.equal(obj.totals, first.totals)
    torch.cuda.synchronize()
    assert _lib.lib().pychain_hip_cpu_calls() == calls       # device tensors never reach the host twin
    assert worst["linear"] <= 1.0 and worst["accum"] <= 1.0, worst
    return worst


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("D", DS)
def test_native_forms(D, dname):
    T = 24
    w = _native_case(4, T, D, dname, torch.tensor([T, 1, T - 1, 2]))
    record_parity("outreg_native_D%d_%s" % (D, dname), **w)


@pytest.mark.parametrize("dname", sorted(DTYPES))
def test_native_single_frame(dname):
    for D in (1, 8, 257):
        w = _native_case(1, 1, D, dname, torch.tensor([1]))
        record_parity("outreg_native_B1T1_D%d_%s" % (D, dname), **w)


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("D", [7, 256])
def test_a_nan_in_a_live_row_reaches_that_sequence_only(D, dname):
    T = 24
    lengths = torch.tensor([T, 1, T - 1, 2])
    x = _x(4, T, D, DTYPES[dname])
    clean = native.output_reg(x.to(DEV), lengths, L2, OOR)
    xn = x.clone()
    xn[2, 5, D - 1] = float("nan")
    xn[0, 3, 0] = float("inf")
    res = native.output_reg(xn.to(DEV), lengths, L2, OOR)
    per, ref = res.per_seq.cpu(), clean.per_seq.cpu()
    assert bool(torch.isnan(per[2]).all()) and bool(torch.isinf(per[0]).all())
    assert torch.equal(per[[1, 3]], ref[[1, 3]])             # the other sequences: bit-equal to the run without it
    assert bool(torch.isnan(res.totals[0]))
    g, g0 = res.grad.cpu(), clean.grad.cpu()
    assert torch.equal(_bits(g[[1, 3]]), _bits(g0[[1, 3]])) and bool(torch.isnan(g[2, 5, D - 1].float()))
    # what the torch composition makes of the same rows
    comp = np_outreg(xn.float().numpy(), lengths, L2, OOR)
    assert np.isnan(comp[0][2]) and np.isnan(comp[1][2]) and np.isinf(comp[0][0]) and np.isinf(comp[1][0])


def test_bad_arguments_are_refused():
    x = _x(2, 3, 8, torch.float32).to(DEV)
    lengths = torch.tensor([3, 2])
    for l2, oor in ((-1e-3, 0.0), (0.0, -1.0)):
        with pytest.raises(_lib.PychainHipError):
            native.output_reg(x, lengths, l2, oor)
    L = _lib.lib()
    ld = lengths.to(DEV)
    per = torch.empty(2, 2, device=DEV)
    ws = torch.empty(L.pychain_hip_output_reg_workspace_bytes(2, 3), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda lim, mode, nbytes: L.pychain_hip_output_reg(x.data_ptr(), _lib.F32, ld.data_ptr(), 2, 3, 8, L2, OOR, lim, mode, None, 1.0, None,
                                                              None, per.data_ptr(), 1.0, None, None, ws.data_ptr(), nbytes, st)
    assert call(-30.0, _lib.GRAD_LINEAR, ws.numel()) == -1 and call(30.0, _lib.GRAD_LOG, ws.numel()) == -1
    assert call(30.0, _lib.GRAD_LINEAR, 16) == -3 and call(30.0, _lib.GRAD_LINEAR, ws.numel()) == 0
    torch.cuda.synchronize()


# ---- through ChainLoss ----------------------------------------------------------------------------------------------------------
ROUTES = ("fused", "fused_backward", "unfused", "xent", "windows", "slices")


def _loss_case(D, B=4, T=24, seed=5):
    lengths = torch.tensor(([T, 9, T - 1, 14] + [5 + (7 * i) % (T - 4) for i in range(B)])[:B])
    graphs = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=8)
    x = syn.make_input(B, T, D, seed=seed)
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.1                   # a tenth of it far out
    x = torch.where(far, _x(B, T, D, torch.float32), x)
    return x, lengths, graphs, syn.make_den_graph(20, 60, D, seed=0)


class _Run(object):
    """One evaluation on the device: the loss, d loss / dx, what the call reported."""

    def __init__(self, route, den, x, lengths, graphs, reg, z=None, lengths_dev=False, twice=False):
        xd = x.to(DEV).requires_grad_(True)
        zd = None if z is None else z.to(DEV).requires_grad_(True)
        kw = dict(output_l2_regularize=L2, out_of_range_regularize=OOR) if reg else {}
        crit = ChainLoss(den, 1e-5, avg=True, xent_regularize=0.1 if z is not None else 0.0, **kw)
        crit.fused = route != "unfused"
        old = ChainLossFunction.overlap
        ChainLossFunction.overlap = route != "fused_backward"
        Ld = lengths.to(DEV) if lengths_dev else lengths
        try:
            loss = crit(xd, Ld, graphs) if zd is None else crit(xd, Ld, graphs, xent_output=zd)
            if twice:
                loss.backward(retain_graph=True)
                self.first = xd.grad.clone()
                xd.grad = None
            loss.backward()
        finally:
            ChainLossFunction.overlap = old
        torch.cuda.synchronize()
        self.loss, self.gx = loss.detach().cpu(), xd.grad.cpu()
        self.gz = None if zd is None else zd.grad.cpu()
        self.totals = None if loss.totals_all is None else loss.totals_all.cpu()
        self.bad = loss.bad_count
        self.l2_term, self.oor_term = getattr(loss, "l2_term", None), getattr(loss, "out_of_range_term", None)


def _same_statistics(a, b):
    """den / num objectives' sum, frames, bad count (totals[1..3], [5..7]), bad_count, z.grad: bit-identical.  (The unfused
    route has no totals: _check_route holds its objectives through the loss's decomposition.)"""
    bad = lambda r: torch.cat([t.reshape(-1).cpu() for t in (r.bad if isinstance(r.bad, (tuple, list)) else [r.bad])])
    assert torch.equal(bad(a), bad(b))
    if a.totals is not None:
        for i in (1, 2, 3, 5, 6, 7):
            assert torch.equal(a.totals[i], b.totals[i]), i
        assert torch.equal(a.totals[0], a.totals[4]) and float(a.totals[4]) == float(a.loss)
    if a.gz is not None:
        assert torch.equal(a.gz, b.gz)


def _check_route(name, route, x, lengths, graphs, den, **kw):
    z = syn.make_input(*x.shape, seed=77) * 1.5 if route == "xent" else None
    graphs.set_time_windows(alignment_windows(viterbi_align(x, lengths, graphs), graphs.num_states, tolerance=2) if route == "windows" else None)
    try:
        if route == "slices":
            with _lib.option("chain_slices", "2"):
                on, off = _Run(route, den, x, lengths, graphs, True, z, **kw), _Run(route, den, x, lengths, graphs, False, z, **kw)
        else:
            on, off = _Run(route, den, x, lengths, graphs, True, z, **kw), _Run(route, den, x, lengths, graphs, False, z, **kw)
    finally:
        graphs.set_time_windows(None)
    n = float(lengths.sum())
    ref = np_outreg(x.numpy(), lengths, L2, OOR)
    mag = term_magnitude(x.numpy(), lengths, L2, OOR)
    assert np.isfinite(float(off.loss))
    expect = float(off.loss) + ref[3] / n
    d_loss = abs(float(on.loss) - expect) / (LOSS_REL * (abs(float(off.loss)) + abs(expect)))
    want = off.gx.numpy().astype(np.float64) + ref[2] / n
    d_grad = worst_ratio(on.gx.numpy(), want, grad_bound(want, mag, 1.0 / n))
    print("%s %s: loss %.3f of its bound, gradient %.3f of its bound" % (name, route, d_loss, d_grad))
    record_parity("outreg_%s_%s" % (name, route), loss=d_loss, grad=d_grad)
    assert d_loss <= 1.0 and d_grad <= 1.0, (d_loss, d_grad)
    for b, L in enumerate(lengths.tolist()):
        assert not bool(on.gx[b, L:].any())
    _same_statistics(on, off)
    if route == "unfused":
        # two native calls make this route's loss and it has no totals to compare: its den / num objectives are held through the
        # decomposition instead - the loss is, bit for bit, the loss without the terms plus output_regularizer's term / frames
        term = output_regularizer(x.to(DEV), lengths, L2, OOR).detach().cpu() / lengths.sum()
        assert on.totals is None and off.totals is None and torch.equal(on.loss, off.loss + term)
    assert abs(float(on.l2_term) - 0.5 * L2 * ref[0].sum() / n) <= term_rel(True) * 0.5 * L2 * ref[0].sum() / n
    assert abs(float(on.oor_term) - OOR * ref[1].sum() / n) <= term_rel(True) * OOR * ref[1].sum() / n
    return on, off


@pytest.mark.parametrize("route", ROUTES)
def test_chain_loss_route(route):
    # (a call is cut into slices of a multiple of 8 sequences: 16 sequences are the fewest that make two of them)
    x, lengths, graphs, den = _loss_case(40, B=16 if route == "slices" else 4)
    _check_route("D40", route, x, lengths, graphs, den)


def test_second_backward_over_a_retained_graph():
    x, lengths, graphs, den = _loss_case(40)
    for route in ("fused", "fused_backward", "unfused"):
        r = _Run(route, den, x, lengths, graphs, True, twice=True)
        assert torch.equal(r.first.cpu(), r.gx), route


def test_lengths_on_the_device():
    x, lengths, graphs, den = _loss_case(40)
    for route in ("fused", "fused_backward"):
        on, off = _check_route("D40_devlen", route, x, lengths, graphs, den, lengths_dev=True)


def test_two_byte_network_output_through_the_fused_step():
    """bf16 / fp16 x on the speculative fused step: the stored 2-byte gradient is read, the term added, the sum rounded again."""
    x, lengths, graphs, den = _loss_case(48)
    n = float(lengths.sum())
    for dname in ("bfloat16", "float16"):
        xh = x.to(DTYPES[dname])
        on, off = _Run("fused", den, xh, lengths, graphs, True), _Run("fused", den, xh, lengths, graphs, False)
        assert on.gx.dtype == DTYPES[dname]
        ref = np_outreg(xh.float().numpy(), lengths, L2, OOR)
        mag = term_magnitude(xh.float().numpy(), lengths, L2, OOR)
        want = off.gx.float().numpy().astype(np.float64) + ref[2] / n
        d = worst_ratio(on.gx.float().numpy(), want, grad_bound(want, mag, 1.0 / n, dname))
        record_parity("outreg_D48_fused_" + dname, grad=d)
        assert d <= 1.0, d
        expect = float(off.loss) + ref[3] / n
        assert abs(float(on.loss) - expect) <= LOSS_REL * (abs(float(off.loss)) + abs(expect))
        _same_statistics(on, off)


def test_output_regularizer_on_the_device():
    x = _x(4, 24, 257, torch.float32)
    lengths = torch.tensor([24, 1, 23, 2])
    xd = x.to(DEV).requires_grad_(True)
    out = output_regularizer(xd, lengths.to(DEV), l2=L2, out_of_range=OOR)
    (2.0 * out).backward()
    ref = np_outreg(x.numpy(), lengths, L2, OOR)
    assert abs(float(out.detach()) - ref[3]) <= SUM_REL * ref[3]
    want = 2.0 * ref[2]
    assert worst_ratio(xd.grad.cpu().numpy(), want, grad_bound(want, term_magnitude(x.numpy(), lengths, L2, OOR), 2.0)) <= 1.0


def test_c3_row_width_and_length():
    case = long_case("c3_slice_num")               # 4 ragged utterances of up to 1500 frames, D = 3456, the C3 numerator graphs
    x, lengths, graphs = case["x"], case["lengths"], case["num"]
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.01                  # a per cent of it far out
    x = torch.where(far, (torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0), x)
    den = syn.make_den_graph(20, 60, x.shape[2], seed=0)
    _check_route("c3", "fused", x, lengths, graphs, den)
