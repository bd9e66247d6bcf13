"""Plain float64 references of the numerator-graph operations, written from include/pychain_hip.h and from nothing else in
the tree: np_viterbi (pychain_hip_align: the association and the tie rules of the ABI, with counters of the ties the best path
met) and np_num_fb (pychain_hip_num_forward_backward[_tw]: a log-domain forward-backward in logaddexp arithmetic, with time
windows).  Both read the float32 input clamped to [-30, 30] and the float32 graph weights, widened to float64."""
import numpy as np
import torch

from helpers import rel_err


def _graph_rows(graphs, b):
    g = graphs.shared_graph if graphs.shared_graph is not None else None
    pick = (lambda n: getattr(g, n)) if g is not None else (lambda n: getattr(graphs, n)[b])
    return dict(bt=pick("backward_transitions").numpy().astype(np.int64), bi=pick("backward_transition_indices").numpy().astype(np.int64),
                lp=pick("backward_transition_probs").numpy().astype(np.float32).astype(np.float64),
                init=pick("initial_probs").numpy().astype(np.float32).astype(np.float64),
                fin=pick("final_probs").numpy().astype(np.float32).astype(np.float64))


def np_viterbi(graphs, x, lengths):
    """(score[B] f64, states[B,T+1], pdfs[B,T], arc_ties[B], final_ties[B]): s(t+1,h) = max_k s(t,src_k) + (lp_k + x(t,pdf_k)),
    first k wins ties; score = max_h s(L,h) + final(h), lowest h wins ties; NaN if an emitted column is NaN; rows -1 where
    there is no path.  arc_ties: frames of the returned path where more than one arc into the chosen state attained the
    maximum; final_ties: 1 where more than one state attained the final maximum (both 0 where there is no path)."""
    x = x.float().numpy()
    B, T, D = x.shape
    xc = np.clip(x, np.float32(-30), np.float32(30))             # (keeps a NaN, as torch.clamp does)
    score = np.zeros(B)
    states = np.full((B, T + 1), -1, dtype=np.int32)
    pdfs = np.full((B, T), -1, dtype=np.int64)
    arc_ties = np.zeros(B, dtype=np.int64)
    final_ties = np.zeros(B, dtype=np.int64)
    for b in range(B):
        r = _graph_rows(graphs, b)
        L, H = int(lengths[b]), r["bi"].shape[0]
        lo, hi = r["bi"][:, 0], r["bi"][:, 1]
        has = np.nonzero(hi > lo)[0]
        ks = np.concatenate([np.arange(lo[h], hi[h]) for h in has]) if has.size else np.zeros(0, np.int64)
        starts = np.concatenate([[0], np.cumsum((hi - lo)[has])[:-1]]).astype(np.int64)
        seg = np.repeat(np.arange(has.size), (hi - lo)[has])
        src, pdf, lp = r["bt"][ks, 0], r["bt"][ks, 2], r["lp"][ks]
        s = r["init"].copy()
        bk = np.zeros((L, H), dtype=np.int64)
        tie = np.zeros((L, H), dtype=bool)
        nan = False
        for t in range(L):
            te = s[src] + (lp + xc[b, t].astype(np.float64)[pdf])
            nan = nan or bool(np.isnan(te).any())
            new = np.full(H, -np.inf)
            if has.size:
                m = np.maximum.reduceat(te, starts)
                at_max = te == m[seg]
                pos = np.where(at_max, np.arange(te.size), te.size)
                first = np.minimum(np.minimum.reduceat(pos, starts), te.size - 1)
                new[has] = m
                bk[t, has] = ks[first]
                tie[t, has] = np.add.reduceat(at_max.astype(np.int64), starts) > 1
            s = new
        e = s + r["fin"]
        nan = nan or bool(np.isnan(e).any())
        h = int(np.argmax(e)) if not nan else 0
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


def _segments(key):
    """(order, starts, owners): a stable sort of the arcs by `key` and where each owner's run starts in it."""
    order = np.argsort(key, kind="stable")
    owners, starts = np.unique(key[order], return_index=True)
    return order, starts.astype(np.int64), owners


def np_num_fb(graphs, x, lengths, windows=None):
    """(logP[B] f64, grad[B,T,D] f64, feasible[B] bool) of the log-domain numerator of include/pychain_hip.h (ABI 19):
       alpha(0,h) = initial(h), alpha(t+1,h) = LogSum_k alpha(t,src_k) + lp_k + x(t,pdf_k), beta(L,h) = final(h),
       beta(t,h) = LogSum_k lp_k + x(t,pdf_k) + beta(t+1,dst_k), logP = LogSum_h alpha(L,h) + final(h),
       grad(t,n) = sum over the arcs k with pdf_k = n of exp(alpha(t,src_k) + lp_k + x(t,n) + beta(t+1,dst_k) - logP),
    every alpha(t,h) and beta(t,h), t = 0..L, replaced by -inf where t lies outside `windows`[b,h] = [lo, hi].  A sequence
    without an admissible path: logP = -inf, an all-zero gradient, feasible False."""
    x = x.float().numpy()
    B, T, D = x.shape
    xc = np.clip(x, np.float32(-30), np.float32(30)).astype(np.float64)
    w = None if windows is None else np.asarray(windows.numpy() if hasattr(windows, "numpy") else windows).astype(np.int64)
    logp = np.full(B, -np.inf)
    grad = np.zeros((B, T, D))
    for b in range(B):
        r = _graph_rows(graphs, b)
        L, H = int(lengths[b]), r["bi"].shape[0]
        lo, hi = r["bi"][:, 0], r["bi"][:, 1]
        has = np.nonzero(hi > lo)[0]
        if not has.size:
            continue
        ks = np.concatenate([np.arange(lo[h], hi[h]) for h in has])
        src, pdf, lp = r["bt"][ks, 0], r["bt"][ks, 2], r["lp"][ks]
        dst = np.repeat(has, (hi - lo)[has])                     # (the state whose list the arc stands in)
        assert np.array_equal(dst, r["bt"][ks, 1])
        od, sd, owd = _segments(dst)
        os_, ss, ows = _segments(src)
        if w is None:
            adm = np.ones((L + 1, H), dtype=bool)
        else:
            t = np.arange(L + 1)[:, None]
            adm = (w[b, :, 0][None, :] <= t) & (t <= w[b, :, 1][None, :])
        ninf = -np.inf
        alpha = np.full((L + 1, H), ninf)
        beta = np.full((L + 1, H), ninf)
        alpha[0] = np.where(adm[0], r["init"], ninf)
        for t in range(L):
            term = alpha[t][src] + lp + xc[b, t][pdf]
            row = np.full(H, ninf)
            row[owd] = np.logaddexp.reduceat(term[od], sd)
            alpha[t + 1] = np.where(adm[t + 1], row, ninf)
        lp_b = np.logaddexp.reduce(alpha[L] + r["fin"])
        if not np.isfinite(lp_b):
            continue
        beta[L] = np.where(adm[L], r["fin"], ninf)
        for t in range(L - 1, -1, -1):
            term = lp + xc[b, t][pdf] + beta[t + 1][dst]
            row = np.full(H, ninf)
            row[ows] = np.logaddexp.reduceat(term[os_], ss)
            beta[t] = np.where(adm[t], row, ninf)
            occ = np.exp(alpha[t][src] + lp + xc[b, t][pdf] + beta[t + 1][dst] - lp_b)
            grad[b, t] = np.bincount(pdf, weights=occ, minlength=D)
        logp[b] = lp_b
    return logp, grad, np.isfinite(logp)


# ---- what a result is held to -------------------------------------------------------------------------------------------------------
def check_alignment(score, states, pdfs, ok, bad, ref, lengths):
    """Bit-identical to np_viterbi: score words, states, pdfs, ok, the bad count; -1 beyond every length."""
    rs, rst, rpd = ref[:3]
    assert score.dtype == torch.float64 and states.dtype == torch.int32 and pdfs.dtype == torch.int64
    sc = score.numpy().copy()
    assert np.array_equal(sc.view(np.int64)[~np.isnan(rs)], rs.copy().view(np.int64)[~np.isnan(rs)])
    assert np.array_equal(np.isnan(sc), np.isnan(rs))
    assert np.array_equal(sc.view(np.int64)[np.isnan(rs)], np.full(int(np.isnan(rs).sum()), 0x7ff8000000000000, dtype=np.int64))
    assert np.array_equal(states.numpy(), rst)
    assert np.array_equal(pdfs.numpy(), rpd)
    assert np.array_equal(ok.numpy(), np.isfinite(rs))
    assert int(bad) == int((~np.isfinite(rs)).sum())
    for b, L in enumerate(np.asarray(lengths).tolist()):
        assert bool((pdfs[b, L:] == -1).all()) and bool((states[b, L + 1:] == -1).all())


def check_numerator(objf, grad, bad, ref, lengths, name=None):
    """Objective and gradient within 1e-5 of np_num_fb (README, "Numerical differences"); an infeasible sequence: -inf, a zero
    gradient.  `bad` None: not compared (the device counts failed checks, not sequences).  Returns the two distances."""
    logp, rgrad, feas = ref
    o = np.asarray(objf, dtype=np.float64)
    g = np.asarray(grad, dtype=np.float64)
    assert np.array_equal(np.isfinite(o), feas)
    assert bool((o[~feas] == -np.inf).all())
    for b in np.nonzero(~feas)[0]:
        assert not g[b].any()
    for b, L in enumerate(np.asarray(lengths).tolist()):
        assert not g[b, L:].any()
    if bad is not None:
        assert int(bad) == int((~feas).sum())
    d_o = float((np.abs(o[feas] - logp[feas]) / np.abs(logp[feas])).max())
    d_g = float(rel_err(g, rgrad))
    if name:
        print("%s: objective %.3e gradient %.3e" % (name, d_o, d_g))
    assert d_o <= 1e-5 and d_g <= 1e-5, (d_o, d_g)
    return d_o, d_g
