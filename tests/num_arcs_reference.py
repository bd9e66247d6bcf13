"""Float64 references of the numerator's expected arc counts, written from include/pychain_hip.h (pychain_hip_num_arc_counts)
and from nothing else in the tree: np_num_arc_counts in numpy logaddexp arithmetic and torch_num_objective, the same objective in
torch float64, whose autograd gives d/dw and d/dx.  Both walk the FORWARD arrays only (the library's backward copies have to find
their weights by the header's pairing rule; the references never need it), read the float32 input clamped to [-30, 30] and
fl32(lp + w) widened to float64 - so a distance to them is about the recursions and not about that one rounding - and take a
weight that is not finite as 0.  `fault` plants one of three mistakes into np_num_arc_counts (test_num_arcs.py shows that each
moves the counts by more than a hundred bounds)."""
import numpy as np
import torch

from num_reference import _segments

FAULTS = ("alpha_w", "beta_t", "share")      # w dropped from alpha only; beta(t) for beta(t+1); the neighbouring frame's share


def _forward_rows(graphs, b):
    g = graphs.shared_graph if graphs.shared_graph is not None else None
    pick = (lambda n: getattr(g, n)) if g is not None else (lambda n: getattr(graphs, n)[b])
    return dict(ft=pick("forward_transitions").numpy().astype(np.int64), fi=pick("forward_transition_indices").numpy().astype(np.int64),
                lp=pick("forward_transition_probs").numpy().astype(np.float32),
                init=pick("initial_probs").numpy().astype(np.float32).astype(np.float64),
                fin=pick("final_probs").numpy().astype(np.float32).astype(np.float64))


def padded_K(graphs):
    return int(graphs.forward_transitions.shape[-2])


def used_arcs(graphs, b):
    """The sequence's used arcs are k < this: the largest forward_transition_indices[h][1]."""
    return int(_forward_rows(graphs, b)["fi"][:, 1].max())


def _weights(w, B, K):
    if w is None:
        return np.zeros((B, K), dtype=np.float32)
    w = np.asarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w).astype(np.float32)
    assert w.shape == (B, K)
    return np.where(np.isfinite(w), w, np.float32(0))


def _arcs(r):
    lo, hi = r["fi"][:, 0], r["fi"][:, 1]
    has = np.nonzero(hi > lo)[0]
    ks = np.concatenate([np.arange(lo[h], hi[h]) for h in has]) if has.size else np.zeros(0, np.int64)
    return ks, r["ft"][ks, 0], r["ft"][ks, 1], r["ft"][ks, 2]


def _admissible(windows, b, L, H):
    if windows is None:
        return np.ones((L + 1, H), dtype=bool)
    w = np.asarray(windows.numpy() if hasattr(windows, "numpy") else windows).astype(np.int64)
    t = np.arange(L + 1)[:, None]
    return (w[b, :, 0][None, :] <= t) & (t <= w[b, :, 1][None, :])


def np_num_arc_counts(graphs, x, lengths, w=None, windows=None, fault=None):
    """(logP[B] f64, counts[B,K] f64, grad[B,T,D] f64, feasible[B]):
       alpha(0,h) = initial(h), alpha(t+1,h) = LogSum_{k into h} alpha(t,src_k) + lpw_k + x(t,pdf_k), beta(L,h) = final(h),
       beta(t,h) = LogSum_{k out of h} lpw_k + x(t,pdf_k) + beta(t+1,dst_k), logP = LogSum_h alpha(L,h) + final(h),
       counts(k) = sum_{t<L} exp(alpha(t,src_k) + lpw_k + x(t,pdf_k) + beta(t+1,dst_k) - logP),  lpw = fl32(lp + w),
    every alpha(t,h), beta(t,h) -inf where t lies outside windows[b,h]; grad(t,n) = the frame's posteriors summed by pdf.
    A sequence without a finite logP: its logP, zero counts and gradient, feasible False."""
    assert fault in (None,) + FAULTS
    x = x.float().numpy()
    B, T, D = x.shape
    K = padded_K(graphs)
    xc = np.clip(x, np.float32(-30), np.float32(30)).astype(np.float64)
    wz = _weights(w, B, K)
    logp = np.full(B, -np.inf)
    counts = np.zeros((B, K))
    grad = np.zeros((B, T, D))
    ninf = -np.inf
    for b in range(B):
        r = _forward_rows(graphs, b)
        L, H = int(lengths[b]), r["fi"].shape[0]
        ks, src, dst, pdf = _arcs(r)
        if not ks.size:
            continue
        lpw = (r["lp"][ks] + wz[b, ks]).astype(np.float32).astype(np.float64)          # fl32(lp + w), widened
        lp_alpha = r["lp"][ks].astype(np.float64) if fault == "alpha_w" else lpw
        od, sd, owd = _segments(dst)
        os_, ss, ows = _segments(src)
        adm = _admissible(windows, b, L, H)
        alpha = np.full((L + 1, H), ninf)
        beta = np.full((L + 1, H), ninf)
        alpha[0] = np.where(adm[0], r["init"], ninf)
        with np.errstate(invalid="ignore"):
            for t in range(L):
                term = alpha[t][src] + lp_alpha + xc[b, t][pdf]
                row = np.full(H, ninf)
                row[owd] = np.logaddexp.reduceat(term[od], sd)
                alpha[t + 1] = np.where(adm[t + 1], row, ninf)
            lp_b = np.logaddexp.reduce(alpha[L] + r["fin"])
            logp[b] = lp_b
            if not np.isfinite(lp_b):
                continue
            beta[L] = np.where(adm[L], r["fin"], ninf)
            share = np.full((L, ks.size), ninf)                                          # r_k(t) = term_k - beta(t,src_k)
            for t in range(L - 1, -1, -1):
                term = lpw + xc[b, t][pdf] + beta[t + 1][dst]
                row = np.full(H, ninf)
                row[ows] = np.logaddexp.reduceat(term[os_], ss)
                beta[t] = np.where(adm[t], row, ninf)
                share[t] = np.where(np.isfinite(beta[t][src]), term - np.where(np.isfinite(beta[t][src]), beta[t][src], 0.0), ninf)
            for t in range(L):
                if fault == "beta_t":
                    post = np.exp(alpha[t][src] + lpw + xc[b, t][pdf] + beta[t][dst] - lp_b)
                elif fault == "share":
                    post = np.exp(alpha[t][src] + beta[t][src] - lp_b + share[min(t + 1, L - 1)])
                else:
                    post = np.exp(alpha[t][src] + lpw + xc[b, t][pdf] + beta[t + 1][dst] - lp_b)
                post = np.where(np.isnan(post), 0.0, post)                               # (-inf - -inf: a state that cannot be reached)
                counts[b, ks] += post
                grad[b, t] = np.bincount(pdf, weights=post, minlength=D)
    return logp, counts, grad, np.isfinite(logp)


def _seg_logsumexp(term, owner, H):
    """LogSum of `term` by `owner` into [H] (torch float64, differentiable; -inf for an owner without a finite term)."""
    ninf = torch.full((H,), -float("inf"), dtype=torch.float64)
    m = ninf.scatter_reduce(0, owner, term.detach(), reduce="amax", include_self=True)
    ms = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(torch.isfinite(term), torch.exp(torch.where(torch.isfinite(term), term, torch.zeros_like(term)) - ms[owner]),
                    torch.zeros_like(term))
    s = torch.zeros(H, dtype=torch.float64).index_add(0, owner, e)
    pos = s > 0
    return torch.where(pos, ms + torch.log(torch.where(pos, s, torch.ones_like(s))), ninf)


def torch_num_objective(graphs, x, lengths, w=None, windows=None):
    """(logP [B] torch float64, x64, w64): the objective of np_num_arc_counts as a function of the leaves x64 [B,T,D] and w64 [B,K]
    (float64 copies of the float32 inputs).  The clamp and the rounding fl32(lp + w) are applied to the VALUES and not
    differentiated - d logP_b / d w64 are the counts, d logP_b / d x64 the gradient of np_num_arc_counts."""
    B, T, D = x.shape
    K = padded_K(graphs)
    x64 = x.detach().double().clone().requires_grad_(True)
    w64 = torch.from_numpy(_weights(w, B, K)).double().requires_grad_(True)
    xc = x64 + (torch.clamp(x.detach().float(), -30, 30).double() - x64).detach()
    out = []
    for b in range(B):
        r = _forward_rows(graphs, b)
        L, H = int(lengths[b]), r["fi"].shape[0]
        ks, src, dst, pdf = (torch.from_numpy(np.ascontiguousarray(v)) for v in _arcs(r))
        lp32 = torch.from_numpy(r["lp"])[ks]
        exact = lp32.double() + w64[b, ks]
        lpw = exact + ((lp32 + w64[b, ks].detach().float()).double() - exact).detach()        # the value fl32(lp + w), slope 1 in w
        adm = torch.from_numpy(_admissible(windows, b, L, H))
        ninf = torch.full((H,), -float("inf"), dtype=torch.float64)
        a = torch.where(adm[0], torch.from_numpy(r["init"]), ninf)
        for t in range(L):
            a = torch.where(adm[t + 1], _seg_logsumexp(a[src] + lpw + xc[b, t][pdf], dst, H), ninf)
        e = a + torch.from_numpy(r["fin"])
        fe = torch.isfinite(e)
        if not bool(fe.any()):
            out.append(torch.tensor(-float("inf"), dtype=torch.float64))
            continue
        out.append(torch.logsumexp(e[fe], 0))
    return torch.stack(out), x64, w64


def torch_num_arc_counts(graphs, x, lengths, w=None, windows=None, utt=None):
    """(logP[B], counts[B,K], grad[B,T,D]) as numpy float64 by autograd of sum_b u_b logP_b over the feasible sequences
    (u = `utt` or ones): rows of an infeasible sequence are zeros."""
    lp, x64, w64 = torch_num_objective(graphs, x, lengths, w, windows)
    feas = torch.isfinite(lp.detach())
    u = torch.ones(len(lp), dtype=torch.float64) if utt is None else torch.as_tensor(utt).double()
    if bool(feas.any()):
        (lp[feas] * u[feas]).sum().backward()
    gz = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return lp.detach().numpy(), gz(w64), gz(x64)


def counts_distance(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())
