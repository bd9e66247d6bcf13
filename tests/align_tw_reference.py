"""A plain float64 reference of constrained re-alignment, written from include/pychain_hip.h (pychain_hip_align_tw) and from
nothing else in the tree, and the builders of the windows its tests use.

    adm(t,h) iff lo <= t <= hi, t in [0, L]
    s(0,h)   = initial(h)                                       if adm(0,h)   else -inf
    s(t+1,h) = max_k s(t,src_k) + (lp_k + x(t,pdf_k))           if adm(t+1,h) else -inf      (first k wins ties)
    score    = max over h with adm(L,h) of s(L,h) + final(h)                                  (lowest h wins ties)

The mask is a select after the max; an arc term counts towards the NaN score only if its destination is admissible at t+1, a
final term only if its state is admissible at L; no admissible path: score -inf and every row -1."""
import numpy as np
import torch

from num_reference import _graph_rows, np_viterbi
from pychain_amd import Alignment, alignment_windows


def np_viterbi_tw(graphs, x, lengths, windows):
    """(score[B] f64, states[B,T+1], pdfs[B,T], arc_ties[B], final_ties[B]) as num_reference.np_viterbi returns them, under
    `windows` (integers [B,H,2]; None: no windows)."""
    x = x.float().numpy()
    B, T, D = x.shape
    xc = np.clip(x, np.float32(-30), np.float32(30))             # (keeps a NaN, as torch.clamp does)
    w = None if windows is None else np.asarray(windows.numpy() if hasattr(windows, "numpy") else windows).astype(np.int64)
    score = np.zeros(B)
    states = np.full((B, T + 1), -1, dtype=np.int32)
    pdfs = np.full((B, T), -1, dtype=np.int64)
    arc_ties = np.zeros(B, dtype=np.int64)
    final_ties = np.zeros(B, dtype=np.int64)
    for b in range(B):
        r = _graph_rows(graphs, b)
        L, H = int(lengths[b]), r["bi"].shape[0]
        if w is None:
            adm = np.ones((L + 1, H), dtype=bool)
        else:
            t = np.arange(L + 1)[:, None]
            adm = (w[b, :, 0][None, :] <= t) & (t <= w[b, :, 1][None, :])
        lo, hi = r["bi"][:, 0], r["bi"][:, 1]
        has = np.nonzero(hi > lo)[0]
        ks = np.concatenate([np.arange(lo[h], hi[h]) for h in has]) if has.size else np.zeros(0, np.int64)
        starts = np.concatenate([[0], np.cumsum((hi - lo)[has])[:-1]]).astype(np.int64)
        seg = np.repeat(np.arange(has.size), (hi - lo)[has])
        dst = has[seg] if has.size else np.zeros(0, np.int64)    # (the state whose list the arc stands in)
        src, pdf, lp = r["bt"][ks, 0], r["bt"][ks, 2], r["lp"][ks]
        s = np.where(adm[0], r["init"], -np.inf)
        bk = np.zeros((L, H), dtype=np.int64)
        tie = np.zeros((L, H), dtype=bool)
        nan = False
        for t in range(L):
            te = s[src] + (lp + xc[b, t].astype(np.float64)[pdf])
            nan = nan or bool(np.isnan(te[adm[t + 1][dst]]).any())
            new = np.full(H, -np.inf)
            if has.size:
                m = np.maximum.reduceat(te, starts)
                at_max = te == m[seg]
                pos = np.where(at_max, np.arange(te.size), te.size)
                first = np.minimum(np.minimum.reduceat(pos, starts), te.size - 1)
                new[has] = m
                bk[t, has] = ks[first]
                tie[t, has] = np.add.reduceat(at_max.astype(np.int64), starts) > 1
            s = np.where(adm[t + 1], new, -np.inf)               # the select after the max
        e = s + r["fin"]
        nan = nan or bool(np.isnan(e[adm[L]]).any())
        e = np.where(adm[L], e, -np.inf)
        h = int(np.argmax(e)) if not nan else 0                  # (the first maximum: the lowest h)
        score[b] = np.nan if nan else e[h]
        if nan or not np.isfinite(score[b]):
            continue
        final_ties[b] = int((e == e[h]).sum() > 1)
        states[b, L] = h
        for t in range(L - 1, -1, -1):
            arc_ties[b] += int(tie[t, h])
            k = bk[t, h]
            pdfs[b, t] = r["bt"][k, 2]
            h = int(r["bt"][k, 0])
            states[b, t] = h
    return score, states, pdfs, arc_ties, final_ties


def reference_alignment(ref):
    """An Alignment (CPU tensors) of what np_viterbi / np_viterbi_tw returned: what alignment_windows reads."""
    score = torch.from_numpy(ref[0].copy())
    return Alignment(torch.from_numpy(ref[2].copy()), torch.from_numpy(ref[1].copy()), score, torch.isfinite(score))


def windows_around(ref, num_states, tau):
    return alignment_windows(reference_alignment(ref), num_states, tau)


def displaced_windows(x2, lengths, graphs, tau):
    """(int32 [B,H,2], the free alignment of x2): alignment_windows at tolerance `tau` around the unconstrained alignment of
    ANOTHER input x2 of the same shapes.  Feasible for any input - x2's path is admissible whatever x is - and in general
    not around the free best path of x."""
    other = np_viterbi(graphs, x2, lengths)
    assert bool(np.isfinite(other[0]).all())
    return windows_around(other, graphs.num_states, tau), other


def frames_differing(a, b, lengths):
    """Per sequence, the time indices t <= L at which the state rows of two results differ."""
    return [int((a[1][i, :int(L) + 1] != b[1][i, :int(L) + 1]).sum()) for i, L in enumerate(np.asarray(lengths).tolist())]


def admits(windows, ref, lengths):
    """True per sequence where every state of the path lies inside its window."""
    w = windows.numpy().astype(np.int64)
    out = []
    for b, L in enumerate(np.asarray(lengths).tolist()):
        st = ref[1][b, :L + 1].astype(np.int64)
        t = np.arange(L + 1)
        out.append(bool(((w[b, st, 0] <= t) & (t <= w[b, st, 1])).all()) if (st >= 0).all() else False)
    return out
