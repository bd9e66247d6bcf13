"""Utterance weights and per-frame derivative weights (include/pychain_hip.h: pychain_hip_weight_rows; csrc/weights.hip) on the
MI355X.  Through native.weight_rows: every load form and every tail (rows of 1 .. 3456 elements, fp32 / bf16 / fp16) against
tests/weights_reference.np_weight_rows BIT FOR BIT - one IEEE multiply, one rounding, no tolerance -, a NaN in a row of each
kind (weight 0: gone; weight 1 and beyond the length: kept), the weighted sums and totals at their derived bounds.  Through
ChainLoss: every route the weights take (fused speculative, overlap = False, fused = False, with an xent output, with the
regularisers, with time windows, in slices), a second backward, lengths and weights on the device, ShardedChainLoss in a world
of one.  Every test that compares two calls pins option den_tseg to "0", the header's switch for bit-for-bit reproducibility.

avg=True under utterance weights: the semantics are x.grad = w * (what the same call WITH THE SAME N writes without weights), so
that is the reference - the fused call handed the same normaliser, N = sum u L, the way ChainLoss hands it (a host scale, or a
device scalar) - and the distance is held at 2 ulp of the element.  (Against the unweighted avg=True call, whose N is sum L, the
distance is not bounded per element: the occupancy kernels fold the scale into their per-frame normalisers before the
denominator's and the numerator's parts are subtracted.)"""
import numpy as np
import pytest
import torch

from helpers import record_parity
from test_gpu_outreg import _pattern
from weights_reference import LOSS_REL, SUM_REL, TERM_REL, draw_weights, np_weight_rows, np_weighted_sums, row_weights, same_bits
from pychain_amd import (ChainLoss, ChainLossFunction, _lib, _plan, alignment_windows, native, parallel, viterbi_align,
                         synthetic as syn)
from pychain_amd.loss import _normaliser

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DS = [1, 3, 4, 7, 8, 255, 256, 257, 1028, 3456]
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
B, T = 3, 7
LENGTHS = torch.tensor([7, 4, 1])
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}     # spacing / magnitude, at most


def _weights_with_every_kind_of_row(which, seed):
    """weights of tests/weights_reference.draw_weights with, among the live rows, one of weight 0 and one of weight 1"""
    u, f = draw_weights(B, T, seed, which)
    if which == "both":
        f[1, 2], f[0, 0] = 1.0, 0.0                          # u[1] = 1: w(1,2) = 1; w(0,0) = 0
    w = row_weights(B, T, u, f)
    live = np.zeros((B, T), dtype=bool)
    for b, L in enumerate(LENGTHS.tolist()):
        live[b, :L] = True
    zero, one = np.argwhere((w == 0) & live), np.argwhere((w == 1) & live)
    assert len(zero) and len(one)
    return u, f, tuple(zero[0]), tuple(one[0])


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("D", DS)
def test_native_rows_equal_the_reference_bit_for_bit(D, dname):
    dtype = DTYPES[dname]
    calls = _lib.lib().pychain_hip_cpu_calls()
    for which in ("u", "f", "both"):
        u, f, zero, one = _weights_with_every_kind_of_row(which, 11 + D)
        g0 = _pattern((B, T, D), dtype)
        g0[zero[0], zero[1], :] = float("nan")               # a weight-0 row: comes back as zeros
        g0[one[0], one[1], D - 1] = float("nan")             # a weight-1 row: its bits are kept
        g0[1, 5, 0] = float("nan")                           # beyond the four frames of sequence 1: its bits are kept
        ref = np_weight_rows(g0, LENGTHS, u, f)
        assert not bool(ref[zero[0], zero[1]].float().abs().sum() != 0) and bool(torch.isnan(ref[one[0], one[1], D - 1].float()))
        for dev_weights in (False, True):
            g = g0.to(DEV)
            mv = lambda t: t if t is None or not dev_weights else t.to(DEV)
            if u is None:
                assert native.weight_rows(g, mv(LENGTHS), None, mv(f)) is None
            else:
                den, num = torch.tensor([10.0, -3.5, float("-inf")]), torch.tensor([4.0, 2.25, float("nan")])     # (u[2] = 0)
                xent, reg = torch.tensor([-7.0, -1.5, float("nan")]), torch.tensor([[3.0, 1.0], [5.0, 0.5], [float("inf"), 2.0]])
                totals = torch.arange(8, dtype=torch.float32, device=DEV) + 0.5
                wsum = native.weight_rows(g, mv(LENGTHS), mv(u), mv(f), den_objf=den.to(DEV), num_objf=num.to(DEV), xent_objf=xent.to(DEV),
                                          xent_coef=-0.1, reg_per_seq=reg.to(DEV), l2=0.2, oor=0.3, loss_scale=0.25,
                                          norm_dev=torch.tensor(4.0, device=DEV), totals=totals)
                r = np_weighted_sums(u, LENGTHS, den.numpy(), num.numpy(), xent.numpy(), 0.1, reg.numpy(), 0.2, 0.3)
                tot, wsum = totals.cpu().double().numpy(), wsum.cpu().double().numpy()
                assert np.isfinite(tot).all() and np.isfinite(wsum).all()
                for got, want in zip(wsum, (r["lf"], r["sx"], r["s2"], r["so"], r["sl"])):
                    assert abs(got - want) <= SUM_REL * abs(want), (got, want)
                full = 0.25 * r["value"] / 4.0
                assert abs(tot[0] - full) <= LOSS_REL * 0.25 * r["mag"] / 4.0 and tot[0] == tot[4]
                assert abs(tot[1] - r["sl"]) <= SUM_REL * r["sl"] and abs(tot[3] - r["lf"]) <= SUM_REL * abs(r["lf"])
                assert list(tot[[2, 5, 6, 7]]) == [2.5, 5.5, 6.5, 7.5]
            assert g.dtype == dtype and same_bits(g, ref), (which, dev_weights)
    torch.cuda.synchronize()
    assert _lib.lib().pychain_hip_cpu_calls() == calls       # device tensors never reach the host twin


def test_native_bad_arguments_are_refused():
    g = _pattern((B, T, 8), torch.float32).to(DEV)
    with pytest.raises(ValueError):
        native.weight_rows(g, LENGTHS, None, None)
    L = _lib.lib()
    ld, u = LENGTHS.to(DEV), torch.ones(B, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda grad, uu, dtype, tot: L.pychain_hip_weight_rows(grad, dtype, ld.data_ptr(), B, T, 8, uu, None, None, None, None, 0.0, None,
                                                                  0.0, 0.0, 1.0, None, tot, None, st)
    tot = torch.zeros(8, device=DEV)
    assert call(g.data_ptr(), None, _lib.F32, None) == -1            # neither weight
    assert call(g.data_ptr(), u.data_ptr(), 7, None) == -1           # unknown dtype
    assert call(g.data_ptr() + 4, u.data_ptr(), _lib.F32, None) == -1
    assert call(None, u.data_ptr(), _lib.F32, None) == -1            # nothing to do
    assert call(None, u.data_ptr(), _lib.F32, tot.data_ptr()) == -1  # sums without the objectives
    assert call(g.data_ptr(), u.data_ptr(), _lib.F32, None) == 0
    torch.cuda.synchronize()


def test_c3_row_width():
    lengths = torch.tensor([64, 37])
    g0 = _pattern((2, 64, 3456), torch.bfloat16)
    u = torch.tensor([0.3, 3.0])
    f = torch.ones(2, 64)
    f[:, :10], f[0, 54:], f[1, 27:37] = 0.0, 0.5, 0.0
    for uu, ff in ((u, None), (None, f), (u, f)):
        g = g0.to(DEV)
        native.weight_rows(g, lengths, uu, ff)
        assert same_bits(g, np_weight_rows(g0, lengths, uu, ff))


# ---- through ChainLoss ----------------------------------------------------------------------------------------------------------
L2, OOR = 5e-4, 0.01


def _loss_case(D, nseq=4, Tx=24, seed=5):
    lengths = torch.tensor(([Tx, 9, Tx - 1, 14] + [5 + (7 * i) % (Tx - 4) for i in range(nseq)])[:nseq])
    graphs = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=8)
    x = syn.make_input(nseq, Tx, D, seed=seed)
    return x, lengths, graphs, syn.make_den_graph(20, 60, D, seed=0)


def _case_weights(nseq, Tx, lengths, which="both"):
    """utterance weights that are all != 1 but one, one of them 0; derivative weights that are 1 except at the utterances' edges,
    with a few other values"""
    u = torch.tensor(([0.5, 3.0, 0.0, 1.0] + [0.3 + 0.1 * i for i in range(nseq)])[:nseq]) if which in ("u", "both") else None
    f = None
    if which in ("f", "both"):
        f = torch.ones(nseq, Tx)
        for b, L in enumerate(lengths.tolist()):
            f[b, :2] = 0.0
            f[b, max(L - 2, 0):L] = 0.0
        f[0, 5], f[1, 4] = 0.3, 3.0
    return u, f


class _Run(object):
    """One evaluation on the device: the loss, d loss / dx, what the call reported."""

    def __init__(self, route, den, x, lengths, graphs, wts, avg=False, z=None, reg=False, on_device=False, twice=False):
        xd = x.to(DEV).requires_grad_(True)
        zd = None if z is None else z.to(DEV).requires_grad_(True)
        kw = dict(output_l2_regularize=L2, out_of_range_regularize=OOR) if reg else {}
        crit = ChainLoss(den, 1e-5, avg=avg, xent_regularize=0.1 if z is not None else 0.0, **kw)
        crit.fused = route != "unfused"
        old = ChainLossFunction.overlap
        ChainLossFunction.overlap = route != "fused_backward"
        mv = lambda t: t.to(DEV) if on_device and t is not None else t
        wkw = {} if wts is None else dict(utt_weights=mv(wts[0]), deriv_weights=mv(wts[1]))
        try:
            loss = crit(xd, mv(lengths), graphs, xent_output=zd, **wkw) if (zd is not None or wkw) else crit(xd, mv(lengths), graphs)
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
        self.out = loss


def _per_seq(den, x, lengths, graphs, z=None, reg=False, unfused=False):
    """the per-sequence objectives of the unweighted step, from the library's own device calls of the same route"""
    xd = x.to(DEV)
    plan = _plan.graph_plan(den, x.shape[2], xd.device)
    gt = graphs.device_tensors(xd.device)
    gstride = 0 if graphs.shared_graph is not None else 1
    tw = graphs.device_time_windows(xd.device) if getattr(graphs, "time_windows", None) is not None else None
    if unfused:
        out = dict(den=native.den_forward_backward(plan, xd, lengths, 1e-5)[0].cpu().numpy(),
                   num=native.num_forward_backward(gt, gstride, graphs.num_states, xd, lengths, windows=tw)[0].cpu().numpy(), xent=None, reg=None)
        if z is not None:
            out["xent"] = native.num_xent(gt, gstride, graphs.num_states, xd, lengths, z.to(DEV), with_grad=False, windows=tw).objf.cpu().numpy()
    else:
        r = native.chain_loss_forward(plan, gt, gstride, graphs.num_states, xd, lengths, 1e-5, windows=tw,
                                      xent=None if z is None else (z.to(DEV), False, 0.1))
        out = dict(den=r[0].cpu().numpy(), num=r[1].cpu().numpy(), xent=None, reg=None)
        if z is not None:
            out["xent"] = r[3].xent.objf.cpu().numpy()
    if reg:
        out["reg"] = native.output_reg(xd, lengths, L2, OOR, with_grad=False).per_seq.cpu().numpy()
    return out


def _check_weighted(name, route, den, x, lengths, graphs, wts, z=None, reg=False, **kw):
    """avg=False: the weighted call's gradients are round(w * the unweighted call's), bit for bit; its loss and what it reports
    are the fp64 weighted sums of the unweighted step's per-sequence objectives"""
    with _lib.option("den_tseg", "0"):
        off = _Run(route, den, x, lengths, graphs, None, z=z, reg=reg, **kw)
        on = _Run(route, den, x, lengths, graphs, wts, z=z, reg=reg, **kw)
        per = _per_seq(den, x, lengths, graphs, z, reg, unfused=route == "unfused")
    u, f = wts
    assert same_bits(on.gx, np_weight_rows(off.gx, lengths, u, f)), (name, route)
    if z is not None:
        assert same_bits(on.gz, np_weight_rows(off.gz, lengths, u, f)), (name, route)
    r = np_weighted_sums(u, lengths, per["den"], per["num"], per["xent"], 0.1 if z is not None else 0.0, per["reg"],
                         L2 if reg else 0.0, OOR if reg else 0.0)
    if u is None:
        assert torch.equal(on.loss, off.loss)                # derivative weights change no sum
        if on.totals is not None:
            assert torch.equal(on.totals, off.totals)
    else:
        d = abs(float(on.loss) - r["value"]) / (LOSS_REL * r["mag"])
        print("%s %s: loss %.3f of its bound" % (name, route, d))
        record_parity("weights_%s_%s" % (name, route), loss=d)
        assert d <= 1.0
        if on.totals is not None:
            t = on.totals.double().numpy()
            assert t[0] == t[4] == float(on.loss) and abs(t[1] - r["sl"]) <= SUM_REL * r["sl"] and abs(t[3] - r["lf"]) <= SUM_REL * r["mag"]
            for i in (2, 5, 6, 7):
                assert torch.equal(on.totals[i], off.totals[i]), i
        if z is not None:
            assert abs(float(on.out.xent_objf) - r["sx"]) <= SUM_REL * abs(r["sx"])
        if reg:
            assert abs(float(on.out.l2_term) - 0.5 * L2 * r["s2"]) <= TERM_REL * 0.5 * L2 * r["s2"]
            assert abs(float(on.out.out_of_range_term) - OOR * r["so"]) <= TERM_REL * OOR * r["so"]
    assert abs(float(on.out.weighted_frames) - r["sl"]) <= SUM_REL * r["sl"]
    return on, off


@pytest.mark.parametrize("dname", ["float32", "bfloat16"])
def test_fused_chain_loss(dname):
    """(D = 48: rows the fused call takes as 2-byte rows, so the gradient the weights scale is the bf16 one)"""
    x, lengths, graphs, den = _loss_case(48)
    x = x.to(DTYPES[dname])
    for which in ("u", "f", "both"):
        _check_weighted("D48_" + dname + "_" + which, "fused", den, x, lengths, graphs, _case_weights(4, 24, lengths, which))
    with _lib.option("den_tseg", "0"):
        off = _Run("fused", den, x, lengths, graphs, None)
        ones = _Run("fused", den, x, lengths, graphs, (torch.ones(4), torch.ones(4, 24)))
        assert same_bits(ones.gx, off.gx) and ones.gx.dtype == DTYPES[dname]
        # avg=True, derivative weights only: N is unchanged, so the rows are round(w * the unweighted call's) again
        f = _case_weights(4, 24, lengths, "f")[1]
        off = _Run("fused", den, x, lengths, graphs, None, avg=True)
        on = _Run("fused", den, x, lengths, graphs, (None, f), avg=True)
        assert same_bits(on.gx, np_weight_rows(off.gx, lengths, None, f)) and torch.equal(on.loss, off.loss)


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dname", ["float32", "bfloat16"])
def test_fused_chain_loss_averaged_under_utterance_weights(dname, on_device):
    x, lengths, graphs, den = _loss_case(48)
    x = x.to(DTYPES[dname])
    u, f = _case_weights(4, 24, lengths)
    mv = lambda t: t.to(DEV) if on_device else t
    with _lib.option("den_tseg", "0"):
        on = _Run("fused", den, x, lengths, graphs, (u, f), avg=True, on_device=on_device)
        # the same call with the same N and no weights
        hscale, dnorm = _normaliser(True, mv(lengths), mv(u))
        assert (dnorm is not None) == on_device
        xd = x.to(DEV)
        plan = _plan.graph_plan(den, 48, xd.device)
        r = native.chain_loss_forward(plan, graphs.device_tensors(xd.device), 0 if graphs.shared_graph is not None else 1,
                                      graphs.num_states, xd, lengths, 1e-5, with_grad=True, grad_scale=hscale, norm_dev=dnorm)
        per = dict(den=r[0].cpu().numpy(), num=r[1].cpu().numpy())
        same_n = r[3].grad.cpu()
    assert same_n.dtype == DTYPES[dname]
    want = np_weight_rows(same_n, lengths, u, f).double()
    err, ulp = (on.gx.double() - want).abs(), ULP[DTYPES[dname]] * want.abs()
    ulps = float((err / ulp.clamp_min(1e-300)).max())                     # (a zero element must be a zero: its ulp is 0)
    print("averaged under utterance weights, %s, device=%s: %.3f ulp" % (dname, on_device, ulps))
    record_parity("weights_avg_%s_dev%d" % (dname, on_device), ulp=ulps)
    assert on.gx.dtype == DTYPES[dname] and ulps <= 2.0
    s = np_weighted_sums(u, lengths, per["den"], per["num"])
    assert abs(float(on.loss) - s["value"] / s["sl"]) <= LOSS_REL * s["mag"] / s["sl"]
    assert abs(float(on.out.weighted_frames) - s["sl"]) <= SUM_REL * s["sl"]


ROUTES = ("fused_backward", "unfused", "xent", "xent_backward", "reg", "reg_backward", "windows", "slices", "device")


@pytest.mark.parametrize("route", ROUTES)
def test_chain_loss_route(route):
    # (a call is cut into slices of a multiple of 8 sequences: 16 sequences are the fewest that make two of them)
    n = 16 if route == "slices" else 4
    x, lengths, graphs, den = _loss_case(40, nseq=n)
    wts = _case_weights(n, 24, lengths)
    z = syn.make_input(*x.shape, seed=77) * 1.5 if route.startswith("xent") else None
    how = "fused_backward" if route.endswith("backward") else ("unfused" if route == "unfused" else "fused")
    graphs.set_time_windows(alignment_windows(viterbi_align(x, lengths, graphs), graphs.num_states, tolerance=2) if route == "windows" else None)
    try:
        if route == "slices":
            with _lib.option("chain_slices", "2"):
                _check_weighted("D40_" + route, how, den, x, lengths, graphs, wts)
        else:
            _check_weighted("D40_" + route, how, den, x, lengths, graphs, wts, z=z, reg=route.startswith("reg"), on_device=route == "device")
    finally:
        graphs.set_time_windows(None)


def test_unfused_route_with_every_term():
    x, lengths, graphs, den = _loss_case(40)
    z = syn.make_input(*x.shape, seed=77) * 1.5
    for which in ("u", "f", "both"):
        _check_weighted("D40_unfused_all_" + which, "unfused", den, x, lengths, graphs, _case_weights(4, 24, lengths, which), z=z, reg=True)


def test_second_backward_over_a_retained_graph():
    x, lengths, graphs, den = _loss_case(40)
    wts = _case_weights(4, 24, lengths)
    z = syn.make_input(*x.shape, seed=77) * 1.5
    with _lib.option("den_tseg", "0"):
        for route in ("fused", "fused_backward", "unfused"):
            off = _Run(route, den, x, lengths, graphs, None, reg=True)
            r = _Run(route, den, x, lengths, graphs, wts, reg=True, twice=True)
            assert same_bits(r.first.cpu(), r.gx) and same_bits(r.gx, np_weight_rows(off.gx, lengths, *wts)), route
        off = _Run("fused", den, x, lengths, graphs, None, z=z)
        r = _Run("fused", den, x, lengths, graphs, wts, z=z, twice=True)
        assert same_bits(r.first.cpu(), r.gx) and same_bits(r.gx, np_weight_rows(off.gx, lengths, *wts))


@pytest.mark.parametrize("route", ["fused_backward", "xent", "xent_backward", "unfused", "unfused_device"])
def test_averaged_under_utterance_weights_on_the_other_routes(route):
    """avg=True with N = sum u L where the normaliser meets the other backward code: overlap = False (the upstream gradient over a
    device N, or a host scale, into chain_loss_backward, then the rows), the xent branch, the unfused route's division by the
    weighted frames.  Reference: w * (the unweighted avg=False gradient of the same route) / N in float64.  These calls cannot be
    handed 'the same N without weights' through ChainLoss, and the occupancy kernels fold the scale into their per-frame
    normalisers, so no per-element ulp bound follows; the distance is held by the suite's own gradient metric and bound
    (tests/test_gpu_parity.py: max |a - b| / max |b| <= 1e-4) - a wrong or missing N is off by sum L / sum u L = 1.3 here."""
    x, lengths, graphs, den = _loss_case(40)
    u, f = _case_weights(4, 24, lengths)
    z = syn.make_input(*x.shape, seed=77) * 1.5 if route.startswith("xent") else None
    how = "fused_backward" if route.endswith("backward") else ("unfused" if route.startswith("unfused") else "fused")
    dev = route.endswith("device")
    with _lib.option("den_tseg", "0"):
        off = _Run(how, den, x, lengths, graphs, None, z=z)
        on = _Run(how, den, x, lengths, graphs, (u, f), avg=True, z=z, on_device=dev)
        per = _per_seq(den, x, lengths, graphs, z, unfused=how == "unfused")
    n = float((u.double() * lengths).sum())
    w = torch.from_numpy(row_weights(4, 24, u, f)).double()[:, :, None]
    for b, L in enumerate(lengths.tolist()):
        w[b, L:] = 1.0                                       # (rows beyond the lengths: zeros, untouched)
    pairs = [(on.gx, off.gx)] + ([(on.gz, off.gz)] if z is not None else [])
    for got, base in pairs:
        want = (w * base.double() / n).numpy()
        d = float(np.abs(got.double().numpy() - want).max() / np.abs(want).max())
        print("%s: %.2e" % (route, d))
        record_parity("weights_avg_route_" + route, grad=d / 1e-4)
        assert d <= 1e-4, d
    r = np_weighted_sums(u, lengths, per["den"], per["num"], per["xent"], 0.1 if z is not None else 0.0)
    assert abs(float(on.loss) - r["value"] / n) <= LOSS_REL * r["mag"] / n
    assert abs(float(on.out.weighted_frames) - n) <= SUM_REL * n


@pytest.mark.parametrize("D,route", [(44, "fused"), (48, "fused_backward")])
def test_up_cast_two_byte_output_is_rounded_once(D, route):
    """A bf16 network output that is up-cast for the call (rows of 44 pdfs are no multiple of 8; overlap = False): the gradient is
    fp32 until it is handed back, the weights multiply that, and the product is rounded to bf16 once.  The call on the fp32 value
    of the same output is the same computation and shows the fp32 gradient."""
    x, lengths, graphs, den = _loss_case(D)
    xh = x.to(torch.bfloat16)
    u, f = _case_weights(4, 24, lengths)
    with _lib.option("den_tseg", "0"):
        off32 = _Run(route, den, xh.float(), lengths, graphs, None)
        off = _Run(route, den, xh, lengths, graphs, None)
        on = _Run(route, den, xh, lengths, graphs, (u, f))
    assert off32.gx.dtype == torch.float32 and same_bits(off.gx, off32.gx.to(torch.bfloat16))       # (the premise)
    assert same_bits(on.gx, np_weight_rows(off32.gx, lengths, u, f).to(torch.bfloat16))


def test_sharded_chain_loss_in_a_world_of_one():
    x, lengths, graphs, den = _loss_case(40)
    u, f = _case_weights(4, 24, lengths)
    with _lib.option("den_tseg", "0"):
        ref = _Run("fused", den, x, lengths, graphs, (u, f), avg=True)
        xd = x.to(DEV).requires_grad_(True)
        crit = parallel.ShardedChainLoss(den, 1e-5, avg=True)
        loss = crit(xd, lengths, graphs, utt_weights=u, deriv_weights=f)
        loss.backward()
        torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(ref.loss)) <= 1e-5 * abs(float(ref.loss))
    assert abs(float(crit.last_stats[1]) - float((u * lengths).sum())) <= SUM_REL * float((u * lengths).sum())
    np.testing.assert_allclose(xd.grad.cpu().numpy(), ref.gx.numpy(), rtol=1e-5, atol=1e-7)
    for b, L in enumerate(lengths.tolist()):
        assert not bool(xd.grad[b, L:].any())
