"""Network outputs that look like a TRAINED model's, and a float64 emulator of the time-segmented denominator recursions
(DESIGN.md §3.13).  Plain numpy; nothing of the library's kernels is used here.

THE INPUTS.  synthetic.make_input is i.i.d. Gaussian: every pdf of a frame is about as likely as every other, so every state
of the denominator graph keeps a comparable share of the mass.  A trained output has one pdf per frame far above the rest,
follows a path through the graph for a few frames per arc, reaches the +-30 clamp, and now and then jumps somewhere the path
did not announce.  That is the regime in which the dynamic range of a state vector matters - the denominator runs in the
probability domain in fp32 -, and the regime in which a state that held 1e-6 of the mass can hold all of it two frames later.
  path_input     N(0,1) floor_sd - peak/2 everywhere, + 1.5 peak on the pdf of the arc a random walk from state 0 is on, each
                 arc held 1 + Poisson(hold) frames.  Values are PRE-clamp logs.
  clamp_input    the same with the peak of every arc drawn from (10, 70): in the frames of a 70 the floor is below -30 and the
                 path above +30 - both sides of the clamp are reached.
  surprise       x[frames, pdfs] = low.
  splice_surprise  the surprise that defeats a max-norm splice check (see below).

THE EMULATOR.  alpha_rows / beta_rows are the recursions of oracle/forgetting.py (chain-computation.h:124-153) in float64,
returning EVERY row as a distribution; spec_alpha / spec_beta start them `burn` frames outside a segment exactly where the
kernel does (den_lazy.inc.h: lazy_recursion): alpha segment [s, e) starts at row s - burn from the initial vector, its row s - 1
is the one the splice check sees, its rows s .. e - 1 are kept; beta segment [s, e) starts at row min(L, e + burn) from the
final vector, its row e + 1 is checked, its rows s + 1 .. e are kept.

TWO METRICS for "the speculated row agrees with the true one", both on rows normalised to sum 1:
  max_norm(p, q) = max_i |p_i - q_i| / max_i p_i                    the splice check up to ABI 27 (bound 4e-6)
  rel_norm(p, q) = max_i |q_i - p_i| / p_i   (0/0 = 0, x/0 = inf)    per state
A frame of either recursion is a nonnegative linear map followed by a positive scaling.  Such maps do not increase Hilbert's
projective distance log(max_i q_i/p_i) - log(min_i q_i/p_i), so rel_norm <= eps at the splice bounds every later row (and
every occupancy) to about 2 eps per element and splice of the chain (emulate_call).  max_norm is NOT contracted: a state with 1e-6 of the mass may be 50 % wrong
unseen, and decides the row once the network's peak moves onto its successors and off the heavy states' - splice_surprise
builds exactly that, and tests/test_peaky.py pins seeds for which it happens in float64.
"""
import numpy as np

OLD_SPLICE_TOL = 4e-6        # kSpliceTol of the max-norm check
CLAMP = 30.0


def graph_arrays(g):
    """The arcs of a probability-domain ChainGraph as float64 / int64 numpy arrays (+ arcs grouped by source state)."""
    ft = g.forward_transitions.numpy()
    src = ft[:, 0].astype(np.int64)
    H = int(g.num_states)
    order = np.argsort(src, kind="stable")
    first = np.searchsorted(src[order], np.arange(H + 1))
    return dict(src=src, dst=ft[:, 1].astype(np.int64), pdf=ft[:, 2].astype(np.int64),
                p=g.forward_transition_probs.numpy().astype(np.float64),
                leaky=g.leaky_probs.numpy().astype(np.float64),
                init=g.initial_probs.numpy().astype(np.float64), final=g.final_probs.numpy().astype(np.float64),
                H=H, by_src=order, first=first)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def path_input(G, T, D, seed, peak=10.0, hold=4, floor_sd=1.0, peaks=None):
    """(x [T, D] float32 pre-clamp logs, walk): walk = [(first frame, frames, arc, pdf)], the arcs a random walk from state 0
    takes (uniformly among the arcs leaving the state it is in).  `peaks`: the peak of every arc is drawn from this tuple."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((T, D)) * floor_sd
    walk, state, t = [], 0, 0
    while t < T:
        lo, hi = G["first"][state], G["first"][state + 1]
        k = int(G["by_src"][lo + rs.randint(hi - lo)])
        n = min(1 + int(rs.poisson(hold)), T - t)
        pk = float(peak if peaks is None else peaks[rs.randint(len(peaks))])
        x[t:t + n] -= pk / 2
        x[t:t + n, G["pdf"][k]] += 1.5 * pk
        walk.append((t, n, k, int(G["pdf"][k])))
        state, t = int(G["dst"][k]), t + n
    return x.astype(np.float32), walk


def clamp_input(G, T, D, seed, hold=4, floor_sd=1.0):
    """path_input whose arcs peak at 10 or at 70: under a 70 the floor (N(0,1) - 35) is below -30 and the path (+70) above +30."""
    return path_input(G, T, D, seed, hold=hold, floor_sd=floor_sd, peaks=(10.0, 70.0))


def surprise(x, frames, pdfs, low):
    """x[frames, pdfs] = low, in place; frames outside x are ignored."""
    fr = np.asarray([f for f in frames if 0 <= f < x.shape[0]], dtype=np.int64)
    if len(fr) and len(pdfs):
        x[np.ix_(fr, np.asarray(pdfs, dtype=np.int64))] = low
    return x


def arc_weights(G, x):
    """w[t, k] = p_k exp(clamp(x[t, pdf_k])) in float64."""
    return G["p"][None, :] * np.exp(np.clip(x.astype(np.float64), -CLAMP, CLAMP))[:, G["pdf"]]


def splice_surprise(G, x, coef, at, direction, seed, heavy=3, low=-25.0):
    """The jump nobody announced, placed where a splice check cannot see it.  alpha (direction 0), segment start `at`: the frames
    at - 1 .. at + 2 - the ones consumed AFTER row at - 1, the row that is checked - become N(0,1), and every pdf on an arc LEAVING
    the `heavy` heaviest states of the true row at - 1 becomes `low`: the mass those states hold goes nowhere, and the row is
    decided by states the check could not resolve.  beta (direction 1), segment end `at`: the mirror image - frames at - 3 .. at,
    consumed after row at + 1, and the arcs ENTERING the heaviest states of the true beta row at + 1.  In place."""
    T, D = x.shape
    rs = np.random.RandomState(seed)
    if direction == 0:
        frames = [at - 1, at, at + 1, at + 2]
        row = alpha_rows(G, arc_weights(G, x[:at - 1]), coef, 0, at - 1)[-1]
        ends = G["src"]
    else:
        frames = [at - 3, at - 2, at - 1, at]
        row = beta_rows(G, arc_weights(G, x), coef, T, at + 1)[0]
        ends = G["dst"]
    frames = [f for f in frames if 0 <= f < T]
    x[frames] = rs.standard_normal((len(frames), D)).astype(np.float32)
    top = np.argsort(-row, kind="stable")[:heavy]
    return surprise(x, frames, np.unique(G["pdf"][np.isin(ends, top)]), low)


# ---- the recursions, every row ---------------------------------------------------------------------------------------------
def alpha_rows(G, w, coef, t0, t1, a0=None):
    """Rows alpha(t0) .. alpha(t1), each normalised to sum 1, from alpha(t0) = a0 (default: the graph's initial vector).
    w: arc weights of the frames (w[t] is frame t of the sequence)."""
    a = (G["init"] if a0 is None else a0).astype(np.float64)
    out = np.empty((t1 - t0 + 1, G["H"]))
    out[0] = a / a.sum()
    for t in range(t0, t1):
        a = out[t - t0]
        ad = a + coef * G["leaky"]                        # alpha'(t) = alpha(t) + tot(t) coef leaky, tot = 1 here
        a = np.bincount(G["dst"], weights=ad[G["src"]] * w[t], minlength=G["H"])
        out[t - t0 + 1] = a / a.sum()
    return out


def beta_rows(G, w, coef, t1, t0, b0=None):
    """Rows beta(t0) .. beta(t1) (index t - t0), each normalised, from beta(t1) = b0 (default: the graph's final vector)."""
    b = (G["final"] if b0 is None else b0).astype(np.float64)
    out = np.empty((t1 - t0 + 1, G["H"]))
    out[t1 - t0] = b / b.sum()
    for t in range(t1 - 1, t0 - 1, -1):
        b = out[t + 1 - t0]
        bd = b + coef * (G["leaky"] * b).sum()            # beta'(t+1) = beta(t+1) + coef sum_i leaky_i beta(t+1, i)
        b = np.bincount(G["src"], weights=bd[G["dst"]] * w[t], minlength=G["H"])
        out[t - t0] = b / b.sum()
    return out


def segments(L, S):
    """[(s, e)] of a sequence of L frames cut in S (den_lazy.inc.h: seg_s, seg_e)."""
    return [((k * L) // S, L if k + 1 == S else ((k + 1) * L) // S) for k in range(S)]


def spec_alpha(G, w, coef, L, s, e, burn):
    """Speculated rows alpha(s - 1) .. alpha(e - 1) of segment [s, e), or None if the segment starts at the true start."""
    f0 = max(s - burn, 0)
    if f0 <= 0:
        return None
    return alpha_rows(G, w, coef, f0, e - 1)[s - 1 - f0:]


def spec_beta(G, w, coef, L, s, e, burn):
    """Speculated rows beta(s + 1) .. beta(e + 1) of segment [s, e), or None if it starts at the true end."""
    if e + burn >= L:
        return None
    return beta_rows(G, w, coef, e + burn, s + 1)[:e + 1 - s]


# ---- the two metrics -----------------------------------------------------------------------------------------------------
def max_norm(p, q):
    p, q = p / p.sum(), q / q.sum()
    return float(np.abs(p - q).max() / p.max())


def rel_norm(p, q):
    p, q = p / p.sum(), q / q.sum()
    both0 = (p == 0) & (q == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(both0, 0.0, np.abs(q - p) / p)
    return float(r.max())


def emulate_call(G, x, coef, L, S, burn):
    """Every splice of one sequence cut in S with burn-in `burn`: a list of dicts(dir, k, at, old, new, chain, inside,
    inside_new).  old / new: the mismatch at the checked row in both metrics AGAINST THE ROW THE KERNEL CHECKS IT WITH - the last row
    the neighbouring segment kept, which is itself speculated unless that neighbour started at the sequence's end (alpha: segment
    0; beta: the last segment).  inside / inside_new: the worst row the segment keeps against the UNCUT recursion, in both metrics.
    chain: the sum of dl = log((1 + new) / (1 - new)) over this splice and those between it and the sequence's end (inf where a
    new >= 1) - the projective distance from the uncut rows that the per-state checks along the chain allow."""
    if L < 2 * burn or S <= 1:
        return []
    w = arc_weights(G, x[:L])
    ta, tb = alpha_rows(G, w, coef, 0, L), beta_rows(G, w, coef, L, 0)
    segs = segments(L, S)
    dl = lambda eps: float(np.log((1 + eps) / (1 - eps))) if eps < 1 else np.inf
    out, fwd, bwd = [], [], []
    last, chain = ta[segs[0][1] - 1], 0.0                  # alpha: from segment 0 on; the row segment k - 1 kept last
    for k, (s, e) in list(enumerate(segs))[1:]:
        sp = spec_alpha(G, w, coef, L, s, e, burn)
        if sp is None:
            last, chain = ta[e - 1], 0.0
            continue
        tr = ta[s - 1:e]
        r = dict(dir=0, k=k, at=s, old=max_norm(last, sp[0]), new=rel_norm(last, sp[0]),
                 inside=max(max_norm(a, b) for a, b in zip(tr[1:], sp[1:])),
                 inside_new=max(rel_norm(a, b) for a, b in zip(tr[1:], sp[1:])))
        chain += dl(r["new"])
        r["chain"] = chain
        fwd.append(r)
        last = sp[-1]
    last, chain = tb[segs[-1][0] + 1], 0.0                 # beta: from the last segment down; row s + 1 of segment k + 1
    for k, (s, e) in list(enumerate(segs))[-2::-1]:
        sp = spec_beta(G, w, coef, L, s, e, burn)
        if sp is None:
            last, chain = tb[s + 1], 0.0
            continue
        tr = tb[s + 1:e + 2]
        r = dict(dir=1, k=k, at=e, old=max_norm(last, sp[-1]), new=rel_norm(last, sp[-1]),
                 inside=max(max_norm(a, b) for a, b in zip(tr[:-1], sp[:-1])),
                 inside_new=max(rel_norm(a, b) for a, b in zip(tr[:-1], sp[:-1])))
        chain += dl(r["new"])
        r["chain"] = chain
        bwd.append(r)
        last = sp[0]
    return fwd + bwd


def occupancies(G, w, coef, a, b):
    """gamma[t, pdf] of frames 0 .. L-1 from rows a[t] = alpha(t), b[t] = beta(t) (any scales): the arc posteriors
    alpha'(t, src) w(t, k) beta'(t+1, dst), normalised per frame, summed per pdf - the denominator's gradient."""
    L, D = w.shape[0], int(G["pdf"].max()) + 1
    out = np.zeros((L, D))
    for t in range(L):
        at, bt = a[t] / a[t].sum(), b[t + 1] / b[t + 1].sum()
        ad = at + coef * G["leaky"]
        bd = bt + coef * (G["leaky"] * bt).sum()
        g = ad[G["src"]] * w[t] * bd[G["dst"]]
        out[t] = np.bincount(G["pdf"], weights=g / g.sum(), minlength=D)
    return out


def cut_gradient_error(G, x, coef, L, S, burn):
    """max |gradient of the cut call - gradient of the uncut call| / max |uncut| in float64, with every speculated row KEPT (what a
    check that accepts every splice returns): the figure tests/test_gpu_tseg.py holds to 1e-5."""
    w = arc_weights(G, x[:L])
    ta, tb = alpha_rows(G, w, coef, 0, L), beta_rows(G, w, coef, L, 0)
    ca, cb = ta.copy(), tb.copy()
    for k, (s, e) in enumerate(segments(L, S)):
        sp = spec_alpha(G, w, coef, L, s, e, burn) if k > 0 else None
        if sp is not None:
            ca[s:e] = sp[1:]
        sp = spec_beta(G, w, coef, L, s, e, burn) if k + 1 < S else None
        if sp is not None:
            cb[s + 1:e + 1] = sp[:-1]
    gt, gc = occupancies(G, w, coef, ta, tb), occupancies(G, w, coef, ca, cb)
    return float(np.abs(gc - gt).max() / np.abs(gt).max())


# ---- the splice cases of tests/test_gpu_tseg.py (pinned by tests/test_peaky.py) -------------------------------------------
SPLICE_GRAPHS = {"LzDma": (300, 3000, 4100), "LzNarrowDma": (1100, 8000, 4096)}
SPLICE_T, SPLICE_LENGTHS, SPLICE_COEF = 400, (400, 399), 1e-5


def splice_seq1(G, D, seed1, peak=10.0, hold=4):
    return path_input(G, SPLICE_T, D, 1000 + seed1, peak=peak, hold=hold)[0]


def splice_seq0(G, D, S, direction, seed, peak=10.0, hold=4):
    """Sequence 0 of a splice case: path input with a splice_surprise at every segment start (direction 0) or end (direction 1)
    of the cut in S."""
    T = SPLICE_T
    x0, _ = path_input(G, T, D, seed, peak=peak, hold=hold)
    segs = segments(SPLICE_LENGTHS[0], S)
    ats = [s for (s, e) in segs[1:]] if direction == 0 else [e for (s, e) in segs[:-1]]
    # (each surprise is built on the input the earlier ones have already changed; beta's from the far end first: the true row
    # at a splice then no longer changes)
    for at in (ats if direction == 0 else ats[::-1]):
        splice_surprise(G, x0, SPLICE_COEF, at, direction, 7000 + seed + at)
    return x0


def splice_case(G, D, S, direction, seed, seed1):
    """x [2, T, D] float32: sequence 0 = splice_seq0(seed), sequence 1 = plain path input (seed1)."""
    return np.stack([splice_seq0(G, D, S, direction, seed), splice_seq1(G, D, seed1)])


# (graph, segments, burn-in, direction of the surprises) -> (seed of sequence 0, seed of sequence 1, the kept-row error and the
# gradient error the float64 emulation must show under an ACCEPTED max-norm check, (sequence, direction) of the splice whose segment
# keeps the worst row).  THE RULE OF THE SEARCH (tests/test_peaky.py asserts its outcome).  Seeds 0 .. 63 in order, sequence 0 (with
# the surprises) and sequence 1 (plain path input) apart.  A seed qualifies if every splice of its sequence is within 2e-6 in the
# max norm (half the old bound: the fp32 recursions must accept it too).  A qualifying seed MEETS THE TARGET if a kept row is
# >= 1e-3 off AND the cut gradient is >= 1.2e-5 from the uncut one - a row may be far off where the other direction gives it no
# weight (sequence 1, seed 47, burn-in 16 on the first graph: a row 2.7e-3 off, gradient 9e-6), and a call whose gradient stays
# inside 1e-5 cannot show the old check failing on the device.  Sequence 0: the first seed that meets the target with its worst row
# in the surprises' direction, else the first that meets it at all, and then sequence 1 is the first qualifying seed; else the
# qualifying seed with the largest kept-row error (among those with gradient >= 1.2e-5, if any), and sequence 1 by the same two
# steps.  The call's figures are the larger of its two sequences'.
# WHAT THE 64 SEEDS GIVE.  Burn-in 16, two segments: 1e-3 is reached on both graphs, by SEQUENCE 1 (plain path input: on LzDma its beta
# splice, on LzNarrowDma its alpha splice); no sequence 0 reaches it there (LzDma 3.4e-4 / 1.9e-4, LzNarrowDma 6e-6 / 1.4e-4).
# Burn-in 32: LzDma reaches 1e-3 with the surprises of sequence 0 (alpha 1.4e-3 in four segments; beta 1.8e-3 and 4.2e-3); LzNarrowDma
# does NOT - the largest found is 2.5e-4 (pinned at >= 1e-4), from alpha splices of either sequence.  A wrong BETA segment is thus
# pinned on LzDma only (2 segments at 16 and 32, 4 at 32); on LzNarrowDma no beta splice of the 64 seeds keeps a row 1e-4 off with a
# gradient beyond 1e-5, and its direction-1 calls are carried by sequence 1's alpha splice.  None: not pinned - no seed gives a call
# the old check accepts whole (4 segments at burn-in 16: twelve splices, each verifying three times in ten), or none whose gradient
# leaves 1e-5 (LzDma, 2 segments, burn-in 32, surprises at the start).  Such a call still runs on the device under the same
# either / or.
SPLICE_PINS = {
    ("LzDma", 2, 16, 0): (60, 39, 1e-3, 1e-4, (1, 1)), ("LzDma", 2, 16, 1): (57, 39, 1e-3, 1e-4, (1, 1)),
    ("LzDma", 4, 16, 0): (0, 0, None, None, None), ("LzDma", 4, 16, 1): (0, 0, None, None, None),
    ("LzDma", 2, 32, 0): (26, 61, None, None, None), ("LzDma", 2, 32, 1): (41, 0, 1e-3, 1.5e-5, (0, 1)),
    ("LzDma", 4, 32, 0): (5, 0, 1e-3, 5e-5, (0, 0)), ("LzDma", 4, 32, 1): (46, 0, 1e-3, 1e-4, (0, 1)),
    ("LzNarrowDma", 2, 16, 0): (40, 3, 1e-3, 1e-4, (1, 0)), ("LzNarrowDma", 2, 16, 1): (12, 3, 1e-3, 1e-4, (1, 0)),
    ("LzNarrowDma", 4, 16, 0): (0, 0, None, None, None), ("LzNarrowDma", 4, 16, 1): (0, 0, None, None, None),
    ("LzNarrowDma", 2, 32, 0): (49, 20, 1e-4, 3e-5, (1, 0)), ("LzNarrowDma", 2, 32, 1): (63, 20, 1e-4, 3e-5, (1, 0)),
    ("LzNarrowDma", 4, 32, 0): (31, 20, 1e-4, 3e-5, (0, 0)), ("LzNarrowDma", 4, 32, 1): (22, 20, 1e-4, 3e-5, (1, 0)),
    # burn-in 96 on the inputs of burn-in 32: in float64 the filter has forgotten its start there (every splice agrees to 1e-15 in
    # both metrics) - the calls of these inputs that a sound check may ACCEPT, and then must get right
    ("LzDma", 2, 96, 0): (26, 61, None, None, None), ("LzDma", 4, 96, 0): (5, 0, None, None, None),
    ("LzNarrowDma", 2, 96, 0): (49, 20, None, None, None), ("LzNarrowDma", 4, 96, 0): (31, 20, None, None, None),
}
_GRAPHS = {}


def splice_graph(name):
    """(ChainGraph, graph_arrays, D) of a splice graph, built once per process."""
    if name not in _GRAPHS:
        from pychain_amd import synthetic as syn
        H, K, D = SPLICE_GRAPHS[name]
        g = syn.make_den_graph(H, K, D)
        _GRAPHS[name] = (g, graph_arrays(g), D)
    return _GRAPHS[name]


def pinned_splice_case(name, S, burn, direction):
    seed, seed1 = SPLICE_PINS[(name, S, burn, direction)][:2]
    _, G, D = splice_graph(name)
    return splice_case(G, D, S, direction, seed, seed1)


# ---- the bar against the float64 oracle (README, fixture G6: the reference's own measured distance from fp64 + 1e-5) -------------
def oracle_bars(kind, x, lengths, *graphs, **kw):
    """(value, gradient) of the float64 oracle, the bars a device result is held to against them - the distance of the oracle's
    OWN float32 flavour from its float64 flavour on this very input, plus 1e-5, never above 1e-4 -, those two distances, and the
    float64 oracle's `ok`.  kind: "den" (graphs = the ChainGraphBatch) or "loss" (graphs = den graph, numerator batch)."""
    import torch
    import oracle as orc
    from helpers import rel_err
    res, ok = {}, True
    for fl in ("f32", "f64"):
        if kind == "den":
            xc = torch.as_tensor(x).float().clamp(-CLAMP, CLAMP).double().exp().float()
            o, g, ok = orc.den(graphs[0], xc, lengths, 1e-5, flavour=fl)
            o = o.sum()
        else:
            o, g = orc.chain_loss(x, lengths, graphs[0], graphs[1], 1e-5, avg=kw.get("avg", True), flavour=fl)
        res[fl] = (float(o), np.asarray(g, dtype=np.float64))
    (o32, g32), (o64, g64) = res["f32"], res["f64"]
    own_o, own_g = abs(o32 - o64) / abs(o64), rel_err(g32, g64)
    return o64, g64, min(own_o + 1e-5, 1e-4), min(own_g + 1e-5, 1e-4), (own_o, own_g), ok
