"""Expected arc counts (include/pychain_hip.h: pychain_hip_den_arc_counts) written twice from the definition, for
the tests:

  counts(...)     the plain alpha' / beta' recursions over p exp(w) and the per-frame arc posteriors in numpy, in `dtype` (float64:
                  the reference the kernels are held to; float32 with the sum over time in float64: the rounding noise of one
                  operation order, which the tolerance rule reads)
  autograd(...)   log Z of tests/smbr_reference.autograd at lambda = 0 with p replaced by p exp(w), and d log Z / dw, d log Z / dy by
                  torch autograd in fp64: nothing hand-derived enters it

and the faults planted into the first (FAULTS) that show what the cases can see.  The model is the leaky HMM of den_general.hip:
v' = v + c leaky sum(v) forwards, u' = u + c sum(leaky u) backwards; leaky, initial and final probabilities are held fixed."""
import numpy as np
import torch

import smbr_reference as sref
from smbr_reference import BAR, COEFS, F32_SLACK, graph_arrays                 # noqa: F401  (the project's bound, one copy)

FAULTS = ("beta_unleaked", "neighbour_divisor", "no_w_in_recursion")

# name -> how it is made: the three shapes of smbr_reference.case; a graph of more than 2048 states (a recursion thread owns
# three) on two short sequences; one sequence of 1500 frames beside 400, 100 and 48 (24 count workgroups of 64 frames, the last
# one short; the sum over time); the graph of tests/test_gpu_smbr_general.py's `long_row` on rows of 4200 pdfs, more than the 4096
# elements the recursion threads hold in registers (four arcs carry pdfs beyond)
CASES = ("small", "wide", "degenerate", "states2100", "long", "long_row")
_OWN = {
    "states2100": dict(H=2100, K=9000, D=130, B=2, T=9, lengths=[9, 5], scale=2.0),
    "long": dict(H=300, K=1500, D=130, B=4, T=1500, lengths=[1500, 400, 100, 48], scale=2.0),
    "long_row": dict(H=37, K=150, D=4200, B=2, T=3, lengths=[3, 1], scale=2.0, graph_seed=3),
}
_made, _refs = {}, {}


def case(name):
    """(graph, y float32 [B,T,D], lengths) of a case, made once and shared (do not edit in place)."""
    if name not in _made:
        if name in _OWN:
            from pychain_amd import synthetic as syn
            c = _OWN[name]
            _made[name] = (syn.make_den_graph(c["H"], c["K"], c["D"], seed=c.get("graph_seed", 7)), syn.make_input(c["B"], c["T"], c["D"], seed=9, scale=c["scale"]),
                           torch.tensor(c["lengths"]))
        else:
            g, y, lengths, _, _ = sref.case(name)
            _made[name] = (g, y, lengths)
    return _made[name]


def weights(name, kind):
    """The arc log-weights of a case: None, or 0.5 N(0,1) from a fixed seed, float32 [K]."""
    if kind is None:
        return None
    K = case(name)[0].num_transitions
    return torch.from_numpy((0.5 * np.random.RandomState(1234 + len(name)).randn(K)).astype(np.float32))


def counts(arrays, y, w, coef, dtype=np.float64, fault=None):
    """One utterance: y [L,D], w [K] or None.  Returns (log Z, counts [K], gamma [L,D]) as float64 values of a computation carried
    out in `dtype`, the sums over time in float64."""
    src, dst, pdf, p, leaky, init, fin = arrays
    f = dtype
    K = p.shape[0]
    w = np.zeros(K) if w is None else np.asarray(w, dtype=np.float64)
    pw = (p.astype(f) * np.exp(w.astype(f))).astype(f)
    prec = p.astype(f) if fault == "no_w_in_recursion" else pw                 # what the recursions multiply by
    leaky, init, fin, c = leaky.astype(f), init.astype(f), fin.astype(f), f(coef)
    L, D = y.shape
    H = leaky.shape[0]
    x = np.exp(np.clip(y.astype(f), f(-30), f(30))).astype(f)

    def scatter(idx, v, n):
        out = np.zeros(n, dtype=f)
        np.add.at(out, idx, v)
        return out

    fleak = lambda v: (v + c * leaky * v.sum(dtype=f)).astype(f)
    bleak = lambda u: (u + c * (leaky * u).sum(dtype=f)).astype(f)
    al = np.zeros((L + 1, H), dtype=f)
    be = np.zeros((L + 1, H), dtype=f)
    braw = np.zeros((L + 1, H), dtype=f)
    s = init.sum(dtype=f)
    logz = np.log(np.float64(s))
    al[0] = fleak(init / s)
    for t in range(L):
        a = scatter(dst, al[t][src] * prec * x[t][pdf], H)
        s = a.sum(dtype=f)
        logz += np.log(np.float64(s))
        al[t + 1] = fleak(a / s)
    logz += np.log(np.float64((al[L] * fin).sum(dtype=f)))
    braw[L] = fin / fin.sum(dtype=f)
    be[L] = bleak(braw[L])
    for t in range(L - 1, -1, -1):
        b = scatter(src, prec * x[t][pdf] * be[t + 1][dst], H)
        braw[t] = b / b.sum(dtype=f)
        be[t] = bleak(braw[t])
    bsel = braw if fault == "beta_unleaked" else be
    raw = np.zeros((L, K), dtype=f)
    for t in range(L):
        raw[t] = al[t][src] * pw * x[t][pdf] * bsel[t + 1][dst]
    den = raw.sum(axis=1, dtype=f)
    if fault == "neighbour_divisor":
        den = np.roll(den, 1)
    post = (raw / den[:, None]).astype(f)
    cnt = post.sum(axis=0, dtype=np.float64)
    gamma = np.zeros((L, D))
    for t in range(L):
        np.add.at(gamma[t], pdf, post[t].astype(np.float64))
    return float(logz), cnt, gamma


def autograd(arrays, y, w, coef):
    """(log Z, d log Z / dw [K], d log Z / dy [L,D]) of one utterance by torch autograd, fp64."""
    src, dst, pdf, p, leaky, init, fin = arrays
    ti = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(torch.int64)
    td = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(torch.float64)
    src, dst, pdf, p, leaky, init, fin = ti(src), ti(dst), ti(pdf), td(p), td(leaky), td(init), td(fin)
    L = y.shape[0]
    yt = torch.from_numpy(np.clip(y.astype(np.float64), -30.0, 30.0)).requires_grad_(True)
    wt = (torch.zeros_like(p) if w is None else td(np.asarray(w, dtype=np.float64))).requires_grad_(True)
    pw = p * torch.exp(wt)
    xs = torch.exp(yt)
    a = init
    logz = torch.zeros((), dtype=torch.float64)
    for t in range(L):
        a = a + coef * leaky * a.sum()
        a = torch.zeros_like(init).index_add(0, dst, a[src] * pw * xs[t][pdf])
        s = a.sum()
        logz = logz + torch.log(s)
        a = a / s
    a = a + coef * leaky * a.sum()
    logz = logz + torch.log((a * fin).sum())
    gw, gy = torch.autograd.grad(logz, (wt, yt))
    return float(logz.detach()), gw.numpy(), gy.numpy()


def batch(fn, graph, y, lengths, w, coef, **kw):
    """`fn` (counts or autograd) over a batch: (log Z [B], counts_per_seq [B,K], gamma [B,T,D] - zero beyond a length), float64."""
    arrays = graph_arrays(graph)
    y = y.detach().double().numpy() if torch.is_tensor(y) else np.asarray(y, dtype=np.float64)
    w = w.detach().double().numpy() if torch.is_tensor(w) else w
    B, T, D = y.shape
    K = arrays[3].shape[0]
    Z, C, G = np.zeros(B), np.zeros((B, K)), np.zeros((B, T, D))
    for b in range(B):
        L = int(lengths[b])
        Z[b], C[b], G[b, :L] = fn(arrays, y[b, :L], w, coef, **kw)
    return Z, C, G


def dist(got, want):
    """max |d| / max |want|."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def value_dist(Z, want):
    """the largest relative error of log Z_b."""
    Z, want = np.asarray(Z, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(Z - want) / np.abs(want)).max())


def distances(got, ref):
    """(counts, gradient, log Z) distances of (Z, counts_per_seq or summed counts, gamma) triples."""
    return dist(got[1], ref[1]), dist(got[2], ref[2]), value_dist(got[0], ref[0])


def reference(name, coef, wkind):
    """((log Z [B], counts_per_seq [B,K], gamma [B,T,D]) by the fp64 recursions, (bound, the fp32 restatement's distance)) of a
    case: computed once per process.  The bound is smbr_reference.bound's rule: BAR, or twice the fp32 distance where that is
    beyond F32_SLACK."""
    key = (name, coef, wkind)
    if key not in _refs:
        g, y, lengths = case(name)
        w = weights(name, wkind)
        ref = batch(counts, g, y, lengths, w, coef)
        d = max(distances(batch(counts, g, y, lengths, w, coef, dtype=np.float32), ref))
        _refs[key] = (ref, ((2.0 * d if d > F32_SLACK else BAR), d))
    return _refs[key]
