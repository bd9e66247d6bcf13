"""Numerator posteriors as cross-entropy targets (include/pychain_hip.h: pychain_hip_xent; csrc/xent.hip) on the MI355X against
tests/xent_reference.np_xent: per-sequence objectives, the gradient of the xent output and the total loss, on every numerator
launch form of tests/num_cases.py (form_case over FORM_D and both sides of form_boundary_D), the largest graph of the tile
kernels, graphs on the general kernels (by state count, by row width, and a row too wide for LDS), a shared graph of 701
states under time windows with one infeasible sequence, and a C3-shaped batch (D = 3456, T = 1500) - each through the fused
speculative step, the fused step with overlap = False, the unfused route and numerator_xent alone.

The bound is measured, not chosen: the distance of the fp32 torch composition fed the float64 reference's gamma from np_xent
on the same case, plus the 1e-5 gamma itself is held to (xent_reference.fp32_distance); every figure goes through
helpers.record_parity."""
import numpy as np
import pytest
import torch

import num_cases as nc
from helpers import long_case, record_parity
from num_reference import np_num_fb
from pychain_amd import ChainGraphBatch, ChainLoss, ChainLossFunction, _lib, native, numerator_xent, synthetic as syn
from xent_reference import GAMMA_BOUND, check_xent, fp32_distance, np_xent

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
C = 0.1
FP32_ROUND = 2.0 ** -22            # two fp32 roundings of the total (the LF-MMI scalar, then the sum with the xent term)


def _boundary(which):
    return nc.form_boundary_D()[which]


def _wide_general_case():
    """A row of 30 000 pdfs: beyond the tile kernels (general numerator) AND beyond what the row kernel keeps in LDS."""
    D = 30000
    g = nc.all_final_graph(40, D)
    return syn.make_input(2, 12, D, seed=9), torch.tensor([9, 12]), ChainGraphBatch(g, 2), None


def _c3_case():
    case = long_case("c3_slice_num")               # 4 ragged utterances of up to 1500 frames, D = 3456, the C3 numerator graphs
    return case["x"], case["lengths"], case["num"], None


CASES = {}
for _D in nc.FORM_D:
    CASES["form_D%d" % _D] = (lambda D=_D: nc.form_case(D) + (None,))
CASES["form_tile_last"] = lambda: nc.form_case(_boundary(0)) + (None,)
CASES["form_general_first"] = lambda: nc.form_case(_boundary(1)) + (None,)
CASES["largest_tile"] = lambda: nc.largest_tile_case(nc.tile_boundary_H()[0]) + (None,)
CASES["general_by_states"] = lambda: nc.largest_tile_case(nc.tile_boundary_H()[1]) + (None,)
CASES["general_wide_row"] = _wide_general_case
CASES["shared701_windows"] = lambda: nc.shared701_case(True)
CASES["c3_shape"] = _c3_case
GENERAL = ("form_general_first", "general_by_states", "general_wide_row")


def _z(x, seed=77):
    B, T, D = x.shape
    return syn.make_input(B, T, D, seed=seed) * 1.5


def _den(D):
    return syn.make_den_graph(20, 60, D, seed=0)


class _Run(object):
    """One evaluation on the device: loss, per-sequence xent objectives, d loss / dz, d loss / dx, what the call reported."""

    def __init__(self, path, den, x, lengths, graphs, z, c, z_grad=True, lengths_dev=False):
        xd = x.to(DEV).requires_grad_(True)
        zd = None if z is None else z.to(DEV).requires_grad_(z_grad)
        L = lengths.to(DEV) if lengths_dev else lengths
        self.frames = float(lengths.sum())
        if path == "numerator_xent":
            o = numerator_xent(zd, xd, L, graphs)
            o.backward()
            self.loss, self.per_seq, self.gx = o.detach(), o.xent_objf_per_seq, xd.grad
            self.gz = zd.grad
            self.scale = 1.0
        else:
            crit = ChainLoss(den, 1e-5, avg=True, xent_regularize=c)
            crit.fused = path != "unfused"
            old = ChainLossFunction.overlap
            ChainLossFunction.overlap = path != "fused_backward"
            try:
                loss = crit(xd, L, graphs) if zd is None else crit(xd, L, graphs, xent_output=zd)
                loss.backward()
            finally:
                ChainLossFunction.overlap = old
            self.loss, self.gx = loss.detach(), xd.grad
            self.gz = None if zd is None else zd.grad
            self.xent_objf = getattr(loss, "xent_objf", None)
            self.per_seq = getattr(loss, "xent_objf_per_seq", None)
            self.totals, self.bad = loss.totals_all, loss.bad_count
            self.scale = -c / self.frames if c else 0.0
        torch.cuda.synchronize()

    def dz(self):
        return self.gz.float().cpu().numpy().astype(np.float64) / self.scale


def _same_statistics(a, b):
    """x.grad, bad_count and totals[1..3, 5..7] of two fused runs: bit-identical."""
    assert torch.equal(a.gx, b.gx)
    assert torch.equal(a.bad, b.bad)
    for i in (1, 2, 3, 5, 6, 7):
        assert torch.equal(a.totals[i], b.totals[i]) or (bool(torch.isnan(a.totals[i])) and bool(torch.isnan(b.totals[i]))), i


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_reference(name):
    x, lengths, graphs, w = CASES[name]()
    z = _z(x)
    D = x.shape[2]
    K = int(graphs.backward_transitions.shape[-2])
    general = not nc.on_tile_path(graphs.num_states, K, D)
    assert general == (name in GENERAL)
    graphs.set_time_windows(w)
    fb = np_num_fb(graphs, x, lengths, w)
    if w is not None:
        assert not bool(fb[2].all())                  # (one sequence without an admissible path)
    ref = np_xent(graphs, x, z, lengths, w, fb)
    own = fp32_distance(graphs, x, z, lengths, w, fb, ref)
    bound = (own[0] + GAMMA_BOUND, own[1] + GAMMA_BOUND)
    frames = float(lengths.sum())
    xent_ref = float(ref[0].sum())
    den = _den(D)
    calls = _lib.lib().pychain_hip_cpu_calls()
    worst = [0.0, 0.0, 0.0]
    for path in ("fused", "fused_backward", "unfused", "numerator_xent"):
        r = _Run(path, den, x, lengths, graphs, z, C)
        per_seq = r.per_seq.cpu().numpy() if r.per_seq is not None else None
        if per_seq is None:                            # (the unfused route reports the sum)
            per_seq = numerator_xent(z.to(DEV), x.to(DEV), lengths, graphs).xent_objf_per_seq.cpu().numpy()
        assert r.gz.dtype == torch.float32
        d = check_xent(per_seq, r.dz(), ref, lengths, fb[2], bound, "%s_%s" % (name, path))
        worst[0], worst[1] = max(worst[0], d[0]), max(worst[1], d[1])
        if path == "numerator_xent":
            assert abs(float(r.loss) - xent_ref) <= bound[0] * np.abs(ref[0]).sum()
            assert r.gx is None                        # gamma is a constant target
            continue
        off = _Run(path, den, x, lengths, graphs, None, C)
        assert torch.equal(r.gx, off.gx)               # nothing flows back to the chain output through the posteriors
        assert abs(float(r.xent_objf) - xent_ref / frames) <= bound[0] * np.abs(ref[0]).sum() / frames
        if np.isfinite(float(off.loss)):
            expect = float(off.loss) - C * xent_ref / frames
            d_t = abs(float(r.loss) - expect)
            assert d_t <= bound[0] * C * np.abs(ref[0]).sum() / frames + FP32_ROUND * (abs(float(off.loss)) + abs(expect)), (d_t, expect)
            worst[2] = max(worst[2], d_t / abs(expect))
        else:
            assert float(r.loss) == float(off.loss)
        if path != "unfused":
            _same_statistics(r, off)
            assert torch.equal(r.totals[0], r.totals[4]) and float(r.totals[4]) == float(r.loss)
            again = _Run(path, den, x, lengths, graphs, z, C)          # the same call gives the same bits
            assert torch.equal(again.gz, r.gz) and torch.equal(again.per_seq, r.per_seq) and torch.equal(again.loss, r.loss)
            assert torch.equal(again.gx, r.gx)
    assert _lib.lib().pychain_hip_cpu_calls() == calls                 # device tensors never reach the host twin
    # the device and the host twin agree within the same tolerance
    host = native.cpu_num_xent(graphs, x, lengths, z, windows=w)
    check_xent(per_seq, r.dz(), (host.objf.numpy().astype(np.float64), host.grad.numpy().astype(np.float64)), lengths, fb[2], bound,
               "%s_host_twin" % name)                                  # (r: the numerator_xent run, the last of the loop)
    graphs.set_time_windows(None)
    record_parity("xent_" + name, fp32_objf=own[0], fp32_grad=own[1], objf_rel=worst[0], grad_rel=worst[1], total_rel=worst[2])


@pytest.mark.parametrize("name", ["form_D48", "form_D4096", "form_D1001", "form_general_first", "shared701_windows"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_two_byte_rows_read_natively_give_the_bits_of_the_upcast(name, dtype):
    x, lengths, graphs, w = CASES[name]()
    graphs.set_time_windows(w)
    zh = _z(x).to(dtype)
    den = _den(x.shape[2])
    for path in ("fused", "numerator_xent"):
        a = _Run(path, den, x, lengths, graphs, zh, C)
        b = _Run(path, den, x, lengths, graphs, zh.float(), C)
        assert a.gz.dtype == dtype and b.gz.dtype == torch.float32
        assert torch.equal(a.per_seq, b.per_seq) and torch.equal(a.loss, b.loss)
        assert torch.equal(a.gz.view(torch.int16), b.gz.to(dtype).view(torch.int16))
        assert bool(a.gz.any())
    graphs.set_time_windows(None)


def test_without_a_gradient_for_the_xent_output_the_objectives_keep_their_bits():
    x, lengths, graphs, _ = CASES["form_D2052"]()
    z, den = _z(x), _den(2052)
    for path in ("fused", "fused_backward", "numerator_xent"):
        a = _Run(path, den, x, lengths, graphs, z, C)
        b = _Run(path, den, x, lengths, graphs, z, C, z_grad=False) if path != "numerator_xent" else None
        if b is not None:
            assert b.gz is None and torch.equal(a.per_seq, b.per_seq) and torch.equal(a.loss, b.loss) and torch.equal(a.gx, b.gx)
    r = native.num_xent(graphs.device_tensors(torch.device(DEV)), 1, graphs.num_states, x.to(DEV), lengths, z.to(DEV), with_grad=False)
    torch.cuda.synchronize()
    assert r.grad is None and torch.equal(r.objf, a.per_seq)


def test_lengths_on_the_device():
    """avg=True with device-resident lengths: the normaliser is read on the device by the row kernel too."""
    x, lengths, graphs, _ = CASES["form_D48"]()
    z, den = _z(x), _den(48)
    for path in ("fused", "fused_backward"):
        a = _Run(path, den, x, lengths, graphs, z, C)
        b = _Run(path, den, x, lengths, graphs, z, C, lengths_dev=True)
        assert torch.equal(a.per_seq, b.per_seq)
        assert abs(float(a.loss) - float(b.loss)) <= 4 * FP32_ROUND * abs(float(a.loss))
        assert float((a.gz - b.gz).abs().max()) <= 4 * FP32_ROUND * float(a.gz.abs().max())
        assert float((a.gx - b.gx).abs().max()) <= 4 * FP32_ROUND * float(a.gx.abs().max())


def test_num_compat_refuses():
    x, lengths, graphs, _ = CASES["form_D48"]()
    z, den = _z(x), _den(48)
    with _lib.option("num_compat", 1):
        for path in ("fused", "numerator_xent"):
            with pytest.raises(_lib.PychainHipError, match="num_compat"):
                _Run(path, den, x, lengths, graphs, z, C)
    _Run("fused", den, x, lengths, graphs, z, C)


def test_a_nan_in_a_live_row_reaches_that_sequence_only():
    x, lengths, graphs, _ = CASES["form_D48"]()
    z, den = _z(x), _den(48)
    clean = _Run("fused", den, x, lengths, graphs, z, C)
    zn = z.clone()
    zn[1, 20, 3] = float("nan")
    zn[2, 30, :] = float("nan")                        # beyond the 9 frames of sequence 2: never read
    for path in ("fused", "fused_backward", "numerator_xent"):
        r = _Run(path, den, x, lengths, graphs, zn, C)
        ps = r.per_seq.cpu()
        assert bool(torch.isnan(ps[1])) and torch.equal(ps[[0, 2]], clean.per_seq.cpu()[[0, 2]])
        assert bool(torch.isnan(r.loss))
        if path != "numerator_xent":
            _same_statistics(r, clean if path == "fused" else _Run(path, den, x, lengths, graphs, z, C))
        g = r.gz.cpu()
        assert bool(torch.isnan(g[1, 20]).all()) and not bool(torch.isnan(g[1, :20]).any()) and not bool(torch.isnan(g[[0, 2]]).any())
        assert not bool(g[2, 9:].any())


def test_a_sliced_call_gives_the_bits_of_the_whole():
    """option chain_slices: the row kernel runs slice by slice on the slices' own rows - same per-sequence bits."""
    lengths = torch.tensor([40, 33, 50, 12, 47, 50, 21, 8, 39, 44, 50, 17, 29, 36, 50, 5])
    D = 48
    graphs = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=20)
    x = syn.make_input(16, 50, D, seed=5)
    z, den = _z(x), _den(D)
    whole = _Run("fused", den, x, lengths, graphs, z, C)
    with _lib.option("chain_slices", 2):
        cut = _Run("fused", den, x, lengths, graphs, z, C)
    assert torch.equal(cut.per_seq, whole.per_seq) and torch.equal(cut.gz, whole.gz)
    assert abs(float(cut.loss) - float(whole.loss)) <= 4 * FP32_ROUND * abs(float(whole.loss))
    ref = np_xent(graphs, x, z, lengths)
    assert abs(float(cut.xent_objf) * float(lengths.sum()) - ref[0].sum()) <= 2e-5 * abs(ref[0].sum())
