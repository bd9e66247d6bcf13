"""What tests/test_num_arcs.py (CPU tensors: the host twin) and tests/test_gpu_num_arcs.py (the MI355X) both check of the
numerator's expected arc counts (include/pychain_hip.h: pychain_hip_num_arc_counts), as functions of the
device: the cases (the builders of tests/num_cases.py), their float64 references (tests/num_arcs_reference.py, computed once per
process and shared), the native calls, and the checks themselves.

BOUND = 1e-5 on max |d counts| / max |counts|, on the gradient by helpers.rel_err and on log P_b relatively: the project's
numerator bound (num_reference.check_numerator)."""
import numpy as np
import torch

import arc_counts_reference as ar
import num_arcs_reference as nr
import num_cases as nc
import smbr_reference as sref
from helpers import record_parity, rel_err
from pychain_amd import ChainGraph, ChainGraphBatch, _lib, den_log_partition, native, num_log_partition, synthetic as syn

BOUND = 1e-5
FORM_D = (4, 2052, 4096, 8408, 16388)            # one width per launch form <4,4,LD>, <1,8>, <4,8,LD>, <4,8>, <1,0>
_cases, _refs = {}, {}


def case(name):
    """(x, lengths, graphs, windows or None), made once and shared (do not edit in place)."""
    if name not in _cases:
        if name == "formtw4":
            c = nc.form_windows_case(4)
        elif name.startswith("form"):
            c = nc.form_case(int(name[4:])) + (None,)
        elif name == "shared701":
            c = nc.shared701_case(False) + (None,)
        elif name == "shared701_tw":
            c = nc.shared701_case(True)
        elif name == "ties":
            c = nc.ties_case() + (None,)
        elif name in ("tile_last", "tile_first"):
            c = nc.largest_tile_case(nc.tile_boundary_H()[0 if name == "tile_last" else 1]) + (None,)
        else:
            raise KeyError(name)
        _cases[name] = c
    return _cases[name]


def weights(name, kind):
    """None, "zeros", or "normal" = 0.5 N(0,1) from a fixed seed: float32 [B,K], K the batch's padded num_transitions."""
    if kind is None:
        return None
    x, _, graphs, _ = case(name)
    B, K = x.shape[0], nr.padded_K(graphs)
    if kind == "zeros":
        return torch.zeros(B, K)
    assert kind == "normal"
    return torch.from_numpy((0.5 * np.random.RandomState(4321 + len(name)).randn(B, K)).astype(np.float32))


def reference(name, wkind):
    key = (name, wkind)
    if key not in _refs:
        x, lengths, graphs, windows = case(name)
        _refs[key] = nr.np_num_arc_counts(graphs, x, lengths, weights(name, wkind), windows)
    return _refs[key]


def run(x, lengths, graphs, w=None, windows=None, with_grad=True, device="cpu"):
    """(objf_per_seq f64 [B], counts_per_seq f64 [B,K], grad f32 [B,T,D] or None, bad_count int32 [2]) of the native call"""
    x = x.to(device)
    if not x.is_cuda:
        return native.cpu_num_arc_counts(graphs, x, lengths, w, with_grad=with_grad, windows=windows)
    gt = graphs.device_tensors(x.device)
    return native.num_arc_counts(gt, 0 if graphs.shared_graph is not None else 1, graphs.num_states, x, lengths, w, with_grad=with_grad,
                                 windows=None if windows is None else windows.to(x.device))


def run_fb(x, lengths, graphs, windows=None, device="cpu"):
    """(objf f32 [B], grad f32 [B,T,D], bad int32 [1]) of pychain_hip_[cpu_]num_forward_backward_tw on the same inputs"""
    x = x.to(device)
    if not x.is_cuda:
        return native.cpu_forward_backward(graphs, x, lengths, grad_mode=_lib.GRAD_LINEAR, windows=windows)
    gt = graphs.device_tensors(x.device)
    return native.num_forward_backward(gt, 0 if graphs.shared_graph is not None else 1, graphs.num_states, x, lengths,
                                       grad_mode=_lib.GRAD_LINEAR, windows=None if windows is None else windows.to(x.device))


def run_case(name, wkind, device, **kw):
    x, lengths, graphs, windows = case(name)
    return run(x, lengths, graphs, weights(name, wkind), windows, device=device, **kw)


def run_with_full_windows(device):
    """shared701 with its weights: (without windows, under windows that admit every state at every time)"""
    x, lengths, graphs, _ = case("shared701")
    w = weights("shared701", "normal")
    return (run(x, lengths, graphs, w, None, device=device),
            run(x, lengths, graphs, w, nc.full_windows(x.shape[0], graphs.num_states), device=device))


def same_bits(a, b):
    """two float tensors bit for bit (a NaN equals itself)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    view = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def check(result, ref, lengths, graphs, name):
    """`result` of run() against `ref` of np_num_arc_counts: the sequences without a usable result (a row of exact zeros, the
    recursion's -inf), the others within BOUND, padding arcs exact zeros, the counts of a feasible sequence summing to its length.
    Returns the three distances."""
    objf, counts, grad, _ = result
    logp, rcounts, rgrad, feas = ref
    assert objf.dtype == counts.dtype == torch.float64
    o, c = objf.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(np.isfinite(o), feas)
    assert bool((o[~feas] == -np.inf).all())
    for b in np.nonzero(~feas)[0]:
        assert not c[b].any()
    L = np.asarray(lengths, dtype=np.float64)
    for b in range(len(L)):
        assert not c[b, nr.used_arcs(graphs, b):].any()                                   # padding arcs
    assert bool((np.abs(c.sum(1) - L)[feas] <= BOUND * L[feas]).all())
    d_c = nr.counts_distance(c[feas], rcounts[feas])
    d_o = float((np.abs(o[feas] - logp[feas]) / np.abs(logp[feas])).max())
    d_g = 0.0
    if grad is not None:
        assert grad.dtype == torch.float32
        g = grad.double().cpu().numpy()
        for b, n in enumerate(np.asarray(lengths).tolist()):
            assert not g[b, n:].any()
        for b in np.nonzero(~feas)[0]:
            assert not g[b].any()
        d_g = float(rel_err(g, rgrad))
    print("%s: counts %.3e gradient %.3e log P %.3e (bound %.0e)" % (name, d_c, d_g, d_o, BOUND))
    record_parity("num_arcs_" + name, counts=d_c, grad=d_g, logp=d_o, bound=BOUND)
    assert d_c <= BOUND and d_g <= BOUND and d_o <= BOUND, (d_c, d_g, d_o)
    return d_c, d_g, d_o


def check_case(name, wkind, device):
    x, lengths, graphs, _ = case(name)
    r = run_case(name, wkind, device)
    check(r, reference(name, wkind), lengths, graphs, "%s_%s_w%s" % (str(device)[:4], name, wkind))
    return r


def check_by_pdf(name, wkind, device):
    """Scattered by pdf, the counts are the sum over t of the gradient rows of the same call, and of
    pychain_hip_num_forward_backward_tw's (w = None)."""
    x, lengths, graphs, windows = case(name)
    objf, counts, grad, _ = run_case(name, wkind, device)
    B, T, D = x.shape
    c, g = counts.cpu().numpy(), grad.double().cpu().numpy()
    feas = np.isfinite(objf.cpu().numpy())
    by_pdf = np.zeros((B, D))
    for b in range(B):
        r = nr._forward_rows(graphs, b)
        n = nr.used_arcs(graphs, b)
        by_pdf[b] = np.bincount(r["ft"][:n, 2], weights=c[b, :n], minlength=D)
    d = nr.counts_distance(by_pdf[feas], g.sum(1)[feas])
    print("%s w=%s: counts by pdf against the summed gradient rows %.3e" % (name, wkind, d))
    assert d <= BOUND
    if wkind is None:
        g2 = run_fb(x, lengths, graphs, windows, device)[1].double().cpu().numpy()
        assert nr.counts_distance(by_pdf[feas], g2.sum(1)[feas]) <= BOUND


def check_identities(name, device):
    """w = None and w = zeros: objf, grad and bad_count[0] bit-identical to pychain_hip_num_forward_backward_tw; the fp64
    objective rounds to that call's float; two calls give the same bits."""
    x, lengths, graphs, windows = case(name)
    fo, fg, fbad = run_fb(x, lengths, graphs, windows, device)
    first = None
    for wkind in (None, "zeros"):
        objf, counts, grad, bad = run_case(name, wkind, device)
        assert same_bits(objf.float(), fo) and same_bits(grad, fg)
        assert int(bad[0]) == int(fbad[0]) and int(bad[1]) == 0
        if first is None:
            first = (objf, counts)
        else:
            assert same_bits(objf, first[0]) and same_bits(counts, first[1])
    again = run_case(name, "zeros", device)
    assert same_bits(again[0], first[0]) and same_bits(again[1], first[1]) and same_bits(again[2], fg)
    # without the gradient only the recursion's verdicts are counted, and the counts are the same bits
    objf, counts, grad, bad = run_case(name, None, device, with_grad=False)
    assert grad is None and same_bits(objf, first[0]) and same_bits(counts, first[1])
    assert int(bad[0]) == int((~np.isfinite(fo.cpu().numpy())).sum()) and int(bad[0]) <= int(fbad[0])


def check_bad_weights(name, device):
    """A NaN and a +inf weight count in bad_count[1], and the call equals the call with those weights set to 0."""
    x, lengths, graphs, windows = case(name)
    w = weights(name, "normal").clone()
    w0 = w.clone()
    w[0, 1], w[1, 0] = float("nan"), float("inf")
    w0[0, 1], w0[1, 0] = 0.0, 0.0
    r = run(x, lengths, graphs, w, windows, device=device)
    r0 = run(x, lengths, graphs, w0, windows, device=device)
    assert r[3].tolist()[1] == 2 and r0[3].tolist()[1] == 0 and int(r[3][0]) == int(r0[3][0])
    assert same_bits(r[0], r0[0]) and same_bits(r[1], r0[1]) and same_bits(r[2], r0[2])
    # a weight on a padding arc is not read
    n = min(nr.used_arcs(graphs, b) for b in range(x.shape[0]))
    if n < nr.padded_K(graphs):
        b = min(range(x.shape[0]), key=lambda i: nr.used_arcs(graphs, i))
        wp = w0.clone()
        wp[b, n:] = float("nan")
        rp = run(x, lengths, graphs, wp, windows, device=device)
        assert rp[3].tolist()[1] == 0 and same_bits(rp[1], r0[1]) and same_bits(rp[0], r0[0])


# ---- autograd ------------------------------------------------------------------------------------------------------------------------
def check_autograd(name, device, utt=None):
    """d num_log_partition / dw and / dx against the float64 autograd of the reference objective."""
    x, lengths, graphs, windows = case(name)
    graphs.set_time_windows(windows)
    try:
        w0 = weights(name, "normal")
        ref_lp, ref_gw, ref_gx = nr.torch_num_arc_counts(graphs, x, lengths, w0, windows, utt=utt)
        xd = x.to(device).requires_grad_(True)
        wd = w0.to(device).requires_grad_(True)
        out = num_log_partition(xd, lengths, graphs, wd, None if utt is None else torch.tensor(utt, dtype=torch.float32))
        assert out.dim() == 0 and out.dtype == torch.float32 and out.per_seq.dtype == torch.float64 and out.bad_count.numel() == 2
        (2.0 * out).backward(retain_graph=True)
        gw, gx = wd.grad.clone(), xd.grad.clone()
        assert gw.dtype == wd.dtype and gw.device == wd.device and gw.shape == wd.shape
        u = np.ones(len(ref_lp)) if utt is None else np.asarray(utt, dtype=np.float64)
        keep = np.isfinite(ref_lp) & (u != 0)
        want = float((ref_lp[keep] * u[keep]).sum())
        assert np.isfinite(float(out.detach())) and abs(float(out.detach()) - want) <= BOUND * abs(want)
        d_w = nr.counts_distance(gw.double().cpu().numpy() / 2.0, ref_gw)
        d_x = float(rel_err(gx.double().cpu().numpy() / 2.0, ref_gx))
        print("%s autograd on %s: d/dw %.3e d/dx %.3e" % (name, device, d_w, d_x))
        assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gx).all())
        assert d_w <= BOUND and d_x <= BOUND
        # a second backward finds the buffer gone and evaluates again (loss._recompute): the same gradient
        wd.grad, xd.grad = None, None
        (2.0 * out).backward()
        assert same_bits(wd.grad, gw) and same_bits(xd.grad, gx)
    finally:
        graphs.set_time_windows(None)


# ---- a parameter tied across both graphs ---------------------------------------------------------------------------------------------
def _tied_case(name):
    """smbr_reference.case(name)'s graph and network output with one left-to-right numerator per utterance (as many states as the
    utterance can traverse, four at most); the self-loop masks of both"""
    den, y, lengths = sref.case(name)[:3]
    D = y.shape[2]
    gs = [ChainGraph(syn.make_num_fst(min(4, int(L)), D, seed=50 + b), log_domain=True) for b, L in enumerate(lengths.tolist())]
    num = ChainGraphBatch(gs, max_num_transitions=max(g.num_transitions for g in gs), max_num_states=max(g.num_states for g in gs))
    ft = num.forward_transitions
    loops_num = (ft[..., 0] == ft[..., 1]).float()
    for b in range(len(gs)):
        loops_num[b, nr.used_arcs(num, b):] = 0.0
    dft = den.forward_transitions
    loops_den = (dft[:, 0] == dft[:, 1]).float()
    return den, num, y, lengths, loops_num, loops_den


def check_tied_scalar(name, device, coef=0.1, theta0=0.3):
    """d/d theta [num_log_partition(theta loops_num) - den_log_partition(theta loops_den)] against the composition of the two
    float64 references, within 2e-5 of the larger of the two terms (one bound for each)"""
    den, num, y, lengths, loops_num, loops_den = _tied_case(name)
    theta = torch.tensor(theta0, requires_grad=True)
    yd = y.to(device)
    obj = num_log_partition(yd, lengths, num, theta * loops_num.to(device)) - \
        den_log_partition(yd, lengths, den, theta * loops_den.to(device), coef).to(device)
    obj.backward()
    wn = (torch.tensor(theta0) * loops_num)
    wd = (torch.tensor(theta0) * loops_den)
    ref_num = nr.np_num_arc_counts(num, y, lengths, wn)
    assert bool(ref_num[3].all())
    t_num = float((ref_num[1] * loops_num.double().numpy()).sum())
    t_den = float((ar.batch(ar.counts, den, y, lengths, wd, coef)[1] * loops_den.double().numpy()[None, :]).sum())
    got, want = float(theta.grad), t_num - t_den
    print("%s on %s: d/dtheta %.9g, reference %.9g = %.9g - %.9g" % (name, device, got, want, t_num, t_den))
    assert t_num > 0 and t_den > 0
    assert abs(got - want) <= 2e-5 * max(abs(t_num), abs(t_den))
