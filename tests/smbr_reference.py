"""Lattice-free sMBR (include/pychain_hip.h: pychain_hip_smbr_*) written twice from the definition, for the tests:

  recursions(...)   the accuracy-weighted recursions of the design in numpy, in `dtype` (float64: the reference the kernels are
                    held to; float32: the rounding noise of one operation order, which the tolerance rule of the tests reads)
  autograd(...)     E = d log Z(x exp(lambda A)) / d lambda at lambda = 0 and its gradient by double-backward torch autograd in
                    fp64: nothing hand-derived enters it

and the faults planted into the first (FAULTS) that show what the test cases can see.  The model is the leaky HMM of
den_general.hip / oracle/forgetting.py: v' = v + c leaky sum(v) forwards, u' = u + c sum(leaky u) backwards."""
import numpy as np
import torch

FAULTS = ("abar_no_leak", "bbar_beta_unleaked", "no_a_q0")
BAR = 1e-5              # the project's bound for its fp32 kernels against fp64 (README.md, parity row)
F32_SLACK = 5e-6        # a case whose fp32 reference is further than this from fp64 gets twice that distance as its bound


COEFS = (0.1, 1e-5)
# the shapes both test files run: small; more states than the 1024 threads of a recursion workgroup (a thread owns two, H no
# multiple of 64, D no multiple of 4); a graph with a state nothing enters, a state nothing leaves and a pdf no arc carries
CASES = {
    "small": dict(H=37, K=150, D=23, B=4, T=17, lengths=[17, 9, 2, 1]),
    "wide": dict(H=1100, K=5000, D=130, B=2, T=12, lengths=[12, 7]),
    "degenerate": dict(H=12, K=40, D=9, B=3, T=7, lengths=[7, 4, 1]),
}
_made = {}


def degenerate_graph():
    """12 states: nothing enters state 0 (the start), nothing leaves state 11, no arc carries pdf 8."""
    from pychain_amd import synthetic as syn
    from pychain_amd.graph import ChainGraph
    from pychain_amd.simplefst import StdVectorFst
    H, K, D = 12, 40, 9
    ring = np.arange(1, 11)
    src = np.concatenate([[0, 0], ring, 1 + syn.randint(71, K - 14, 10), [3, 7]])
    dst = np.concatenate([[1, 5], 1 + ring % 10, 1 + syn.randint(72, K - 14, 10), [11, 11]])
    pdf = syn.randint(73, K, D - 1)
    lp = -2.1 + 2.0 * syn.uniform(74, K)
    order = np.argsort(src, kind="stable")
    fst = StdVectorFst.from_arrays(H, 0, src[order], dst[order], pdf[order], lp[order], np.zeros(H))
    return ChainGraph(fst, initial_mode="leaky", final_mode="ones", log_domain=False)


def case(name):
    """(graph, y float32 [B,T,D], lengths, pdfs int32 [B,T,2], probs float32 [B,T,2]) of CASES[name], made once and shared (do
    not edit in place).  The targets hold padding entries, a pdf repeated within a frame, and the LAST utterance has none."""
    if name not in _made:
        from pychain_amd import synthetic as syn
        c = CASES[name]
        B, T, D = c["B"], c["T"], c["D"]
        graph = degenerate_graph() if name == "degenerate" else syn.make_den_graph(c["H"], c["K"], D, seed=3)
        y = syn.make_input(B, T, D, seed=5)
        seed = 11 + len(name)
        pdfs = syn.randint(seed, B * T * 2, D).reshape(B, T, 2).astype(np.int32)
        probs = (0.05 + syn.uniform(seed + 1, B * T * 2)).reshape(B, T, 2).astype(np.float32)
        pdfs[:, 1::4, 1] = -1                              # padding behind a live entry
        pdfs[:, 2::5, 0] = -1                              # ... and in front of one
        pdfs[:, 0::3, 1] = pdfs[:, 0::3, 0]                # a pdf twice in a frame
        pdfs[B - 1] = -1                                   # an utterance without targets
        _made[name] = (graph, y, torch.tensor(c["lengths"]), torch.from_numpy(pdfs), torch.from_numpy(probs))
    return _made[name]


_refs = {}


def reference(name, coef):
    """(E [B], grad [B,T,D], closing [B]) of case `name` by the fp64 recursions, and the case's (bound, fp32 distance): computed
    once per process."""
    key = (name, coef)
    if key not in _refs:
        g, y, lengths, pdfs, probs = case(name)
        ref = batch(recursions, g, y, lengths, pdfs.numpy(), probs.numpy(), coef)
        _refs[key] = (ref, bound(g, y, lengths, pdfs.numpy(), probs.numpy(), coef, ref))
    return _refs[key]


def graph_arrays(g):
    """(src, dst, pdf, p, leaky, initial, final) of a probability-domain ChainGraph, float64."""
    ft = g.forward_transitions.numpy().astype(np.int64)
    f = lambda t: t.numpy().astype(np.float64)
    return ft[:, 0], ft[:, 1], ft[:, 2], f(g.forward_transition_probs), f(g.leaky_probs), f(g.initial_probs), f(g.final_probs)


def dense_accuracy(pdfs, probs, D):
    """A(t,n) [T,D] float64 of one utterance's sparse targets [T,K]: repeated pdfs add, pdf < 0 or >= D adds nothing."""
    T, K = pdfs.shape
    A = np.zeros((T, D))
    for t in range(T):
        for k in range(K):
            if 0 <= pdfs[t, k] < D:
                A[t, pdfs[t, k]] += float(probs[t, k])
    return A


def recursions(arrays, y, A, coef, dtype=np.float64, fault=None):
    """One utterance: y [L,D] (network output of the live frames), A [L,D].  Returns (E, grad [L,D], closing), float64 values of a
    computation carried out in `dtype`."""
    src, dst, pdf, p, leaky, init, fin = arrays
    f = dtype
    p, leaky, init, fin, c = p.astype(f), leaky.astype(f), init.astype(f), fin.astype(f), f(coef)
    L, D = y.shape
    H = leaky.shape[0]
    x = np.exp(np.clip(y.astype(f), f(-30), f(30))).astype(f)
    A = A.astype(f)

    def scatter(idx, v, n):
        out = np.zeros(n, dtype=f)
        np.add.at(out, idx, v)
        return out

    fleak = lambda v: (v + c * leaky * v.sum(dtype=f)).astype(f)
    bleak = lambda u: (u + c * (leaky * u).sum(dtype=f)).astype(f)
    # first-order pass: alpha', beta', occupancies, frame accuracies
    al = np.zeros((L + 1, H), dtype=f)
    be = np.zeros((L + 1, H), dtype=f)
    braw = np.zeros((L + 1, H), dtype=f)            # beta before its leak, same scale as be
    ta, tb = np.ones(L + 1, dtype=f), np.ones(L + 1, dtype=f)
    a = init / init.sum(dtype=f)
    al[0] = fleak(a)
    for t in range(L):
        a = scatter(dst, al[t][src] * p * x[t][pdf], H)
        ta[t + 1] = a.sum(dtype=f)
        al[t + 1] = fleak(a / ta[t + 1])
    tb[L] = fin.sum(dtype=f)
    braw[L] = fin / tb[L]
    be[L] = bleak(braw[L])
    for t in range(L - 1, -1, -1):
        b = scatter(src, p * x[t][pdf] * be[t + 1][dst], H)
        tb[t] = b.sum(dtype=f)
        braw[t] = b / tb[t]
        be[t] = bleak(braw[t])
    q0 = np.zeros((L, D), dtype=f)
    for t in range(L):
        q0[t] = scatter(pdf, p * al[t][src] * be[t + 1][dst], D)
    den = (x * q0).sum(axis=1, dtype=f)
    gamma = x * q0 / den[:, None]
    e = (gamma * A).sum(axis=1, dtype=f)
    ac = (A - e[:, None]).astype(f)                   # centred accuracies
    # accuracy-weighted pass, the normalisers of the first
    ab = np.zeros((L + 1, H), dtype=f)
    bb = np.zeros((L + 1, H), dtype=f)
    for t in range(L):
        v = scatter(dst, (ab[t][src] + ac[t][pdf] * al[t][src]) * p * x[t][pdf], H) / ta[t + 1]
        ab[t + 1] = v if fault == "abar_no_leak" else fleak(v)
    for t in range(L - 1, -1, -1):
        bsrc = braw[t + 1] if fault == "bbar_beta_unleaked" else be[t + 1]
        bb[t] = bleak(scatter(src, p * x[t][pdf] * (bb[t + 1][dst] + ac[t][pdf] * bsrc[dst]), H) / tb[t])
    grad = np.zeros((L, D), dtype=f)
    for t in range(L):
        q1 = scatter(pdf, p * (ab[t][src] * be[t + 1][dst] + al[t][src] * bb[t + 1][dst]), D)
        num = q1 if fault == "no_a_q0" else q1 + ac[t] * q0[t]
        grad[t] = x[t] * num / den[t]
    closing = (ab[L] * fin).sum(dtype=f) / (al[L] * fin).sum(dtype=f)
    return float(e.sum(dtype=np.float64)), grad.astype(np.float64), float(closing)


def autograd(arrays, y, A, coef):
    """E and dE/dy of one utterance through log Z alone, fp64."""
    src, dst, pdf, p, leaky, init, fin = arrays
    ti = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(torch.int64)
    td = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(torch.float64)
    src, dst, pdf, p, leaky, init, fin = ti(src), ti(dst), ti(pdf), td(p), td(leaky), td(init), td(fin)
    L = y.shape[0]
    yt = torch.from_numpy(np.clip(y.astype(np.float64), -30.0, 30.0)).requires_grad_(True)
    lam = torch.zeros((), dtype=torch.float64, requires_grad=True)
    xs = torch.exp(yt + lam * td(A))
    a = init
    logz = torch.zeros((), dtype=torch.float64)
    for t in range(L):
        a = a + coef * leaky * a.sum()
        a = torch.zeros_like(init).index_add(0, dst, a[src] * p * xs[t][pdf])
        s = a.sum()
        logz = logz + torch.log(s)
        a = a / s
    a = a + coef * leaky * a.sum()
    logz = logz + torch.log((a * fin).sum())
    E, = torch.autograd.grad(logz, lam, create_graph=True)
    g, = torch.autograd.grad(E, yt)
    return float(E.detach()), g.numpy()


def batch(fn, graph, y, lengths, pdfs, probs, coef, **kw):
    """`fn` (recursions or autograd) over a batch: (E [B] float64, grad [B,T,D] float64 - zero beyond a length -, extra [B])."""
    arrays = graph_arrays(graph)
    y = y.detach().double().numpy() if torch.is_tensor(y) else np.asarray(y, dtype=np.float64)
    pdfs, probs = np.asarray(pdfs), np.asarray(probs)
    B, T, D = y.shape
    E, G, X = np.zeros(B), np.zeros((B, T, D)), np.zeros(B)
    for b in range(B):
        L = int(lengths[b])
        r = fn(arrays, y[b, :L], dense_accuracy(pdfs[b, :L], probs[b, :L], D), coef, **kw)
        E[b], G[b, :L] = r[0], r[1]
        X[b] = r[2] if len(r) > 2 else 0.0
    return E, G, X


def grad_dist(g, want):
    """max |d grad| / max |grad| over the batch."""
    return float(np.abs(np.asarray(g, dtype=np.float64) - want).max() / np.abs(want).max())


def value_dist(E, want):
    """the largest relative error of E_b over the sequences whose reference is not zero."""
    E, want = np.asarray(E, dtype=np.float64), np.asarray(want)
    nz = want != 0
    return float((np.abs(E - want)[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0


def bound(graph, y, lengths, pdfs, probs, coef, ref=None):
    """The bound of a case against fp64 and the fp32 reference's own distance: BAR, or twice that distance where it is beyond
    F32_SLACK."""
    ref = ref or batch(recursions, graph, y, lengths, pdfs, probs, coef)
    e32, g32, _ = batch(recursions, graph, y, lengths, pdfs, probs, coef, dtype=np.float32)
    d = max(grad_dist(g32, ref[1]), value_dist(e32, ref[0]))
    return (2.0 * d if d > F32_SLACK else BAR), d
