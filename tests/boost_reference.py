"""The boosted objective (LF-bMMI; include/pychain_hip.h: pychain_hip_boost_rows) restated in plain float64 from
its definition, the bound the row pass is held to, and the inputs both test files share.

THE DEFINITION.  a(b,t,n) is the reference posterior of pdf n at frame t: the DENSE sum of the sparse boost targets.  The
denominator is evaluated on
    e64 = exp(clamp(x, -30, 30) - boost * a)                                       (float64)
by the float64 flavour of the oracle (oracle/oracle.py: den takes rows that are already exp'd - its interface carries them as
float32, one rounding of 2^-24 per element, far inside the bar), and
    loss = sum_b u_b (den_b(e64) - num_b [- c xent_b] [+ regularisers_b]) / N,     N = sum_b u_b L_b under avg
    d loss / dx = (gamma_den(e64) - q) / N         posterior supervision (q: the dense sum of the numerator's targets)
                = (gamma_den(e64) - gamma_num(x)) / N   graph numerators
Neither the clamp nor a is differentiated.  The ChainLoss comparisons use the library's fp64 bar, 1e-5 on the relative value and
on max |d grad| / max |grad|.

THE BOUND OF THE PASS IS DERIVED, NOT CHOSEN.  An element no entry addresses is E = exp(clamp(x)) as the denominator kernels
form it: compared BIT FOR BIT.  An addressed element is e = fl32(E * F) with the very E the call stored elsewhere in that form
(recomputed from the same x by the same instructions) and F the factor; against E * exp(-boost * qd) in float64, qd formed in
fp32 as the header says (ascending k), two things are rounded:
  the factor's exp   u = fl32(boost qd) and t = fl32(-u fp32(log2 e)) each round once, and fp32(log2 e) is itself a rounded
                     constant: the exponent is off by at most 3 * 2^-24 |boost qd| relatively, i.e. the factor by
                     exp(3 * 2^-24 boost qd) - 1 <= 3 * 2^-24 boost qd (1 + 2^-20) for the arguments here; the exp2 itself (v_exp_f32
                     on the device, exp2f on the host) is good to one ulp, 2^-23 relative;
  one multiply       2^-24 relative.
Their sum, times (1 + 2^-20) for the second-order terms, times |ref|; plus 2^-126 absolute where the product leaves the normal
range (v_exp_f32 may flush).  The tests print the fraction of this bound they measure.
"""
import numpy as np
import torch

import post_reference as pr

BAR = 1e-5
DTYPES = pr.DTYPES
NATIVE_B, NATIVE_T, NATIVE_LENGTHS = pr.NATIVE_B, pr.NATIVE_T, pr.NATIVE_LENGTHS
NATIVE_DS, NATIVE_KS = pr.NATIVE_DS, pr.NATIVE_KS
SENTINEL = -777.25


def native_case(D, K, dname="float32"):
    """post_reference.native_case: x in +-40 (beyond the clamp) with exact +-30, NaN in all padding of x, pdfs' rows (an index far
    outside the row) and probs, a frame without entries, one pdf three times in a frame, ONE entry with pdf >= D."""
    return pr.native_case(D, K, dname, seed=23)


def merged_case(pdfs, probs):
    """The same targets with every repeated pdf of a frame merged into its first occurrence (qd by the fp32 rule, ascending k),
    the later occurrences turned into padding: the pass must give the same bits."""
    pdfs, probs = pdfs.clone(), probs.clone()
    B, T, K = pdfs.shape
    for b, L in enumerate(NATIVE_LENGTHS):
        for t in range(L):
            for k in range(K):
                d = int(pdfs[b, t, k])
                if d < 0:
                    continue
                qd = np.float32(probs[b, t, k])
                for j in range(k + 1, K):
                    if int(pdfs[b, t, j]) == d:
                        qd = np.float32(qd + np.float32(probs[b, t, j]))
                        pdfs[b, t, j] = -1
                probs[b, t, k] = float(qd)
    return pdfs, probs


def np_boost_rows(E, lengths, pdfs, probs, boost):
    """E [B,T,D]: exp(clamp(x)) as the library forms it (its own bits).  Returns (want float64 [B,T,D] = E, the addressed
    elements times exp(-boost qd); touched bool [B,T,D]; bound float64 [B,T,D]; bad)."""
    E = np.asarray(E, dtype=np.float64)
    B, T, D = E.shape
    K = pdfs.shape[2]
    want, touched, bound = E.copy(), np.zeros(E.shape, dtype=bool), np.zeros(E.shape)
    bad = 0
    bf = np.float32(boost)
    for b, L in enumerate(pr._len(lengths, T)):
        for t in range(L):
            qd = {}
            for k in range(K):
                d = int(pdfs[b, t, k])
                if d < 0:
                    continue
                if d >= D:
                    bad += 1
                    continue
                q = np.float32(probs[b, t, k])
                qd[d] = np.float32(qd[d] + q) if d in qd else q
            for d, v in qd.items():
                u = float(bf) * float(v)
                want[b, t, d] = E[b, t, d] * np.exp(-u)
                touched[b, t, d] = True
                bound[b, t, d] = abs(want[b, t, d]) * (3 * 2.0 ** -24 * abs(u) + 2.0 ** -23 + 2.0 ** -24) * (1 + 2.0 ** -20) + 2.0 ** -126
    return want, touched, bound, bad


# ---- through ChainLoss -------------------------------------------------------------------------------------------------------------
def dense(targets, lengths, D):
    """a(b,t,n): the float64 dense sum of sparse targets over the live frames (padding and pdf >= D contribute nothing)"""
    pdfs, probs = targets.pdfs.cpu(), targets.probs.cpu()
    B, T, K = pdfs.shape
    live = (torch.arange(T)[None, :] < torch.as_tensor(lengths).cpu()[:, None])[..., None]
    ok = (pdfs >= 0) & (pdfs < D) & live
    a = torch.zeros(B, T, D, dtype=torch.float64)
    a.scatter_add_(2, pdfs.clamp(0, D - 1).to(torch.int64), torch.where(ok, probs.double(), torch.zeros((), dtype=torch.float64)))
    return a


def reference(den_graph, x, lengths, supervision, boost_targets, boost, avg=True, u=None, f=None, reg=None, z=None,
              xent_targets=None, c=0.0):
    """(loss, d loss / dx [, d loss / dz]) as float64 numpy, from the definition above.  `x`: the fp32 value of the network
    output; `supervision`: PosteriorTargets or numerator graphs (a ChainGraphBatch); `boost_targets` None or boost 0: the
    unboosted objective."""
    import oracle as orc
    from pychain_amd import ChainGraphBatch, PosteriorTargets
    x64 = x.detach().cpu().double()
    B, T, D = x64.shape
    lengths = torch.as_tensor(lengths).cpu()
    live = (torch.arange(T)[None, :] < lengths[:, None]).double()
    xc = x64.clamp(-30.0, 30.0)
    arg = xc if boost_targets is None or boost == 0.0 else xc - float(boost) * dense(boost_targets, lengths, D)
    e64 = torch.where(live[..., None] > 0, arg.exp(), torch.ones((), dtype=torch.float64))
    den, gden, _ = orc.den(ChainGraphBatch(den_graph, B), e64, lengths, 1e-5, flavour="f64")
    term = torch.from_numpy(np.asarray(den, dtype=np.float64))
    grad = torch.from_numpy(np.asarray(gden, dtype=np.float64)) * live[..., None]
    if isinstance(supervision, PosteriorTargets):
        q = dense(supervision, lengths, D)
        term = term - (q * xc).sum(dim=(1, 2))
        grad = grad - q
    else:
        shared = getattr(supervision, "shared_graph", None) is not None
        num, lg, _ = orc.num(supervision, xc.float(), lengths, shared=shared, flavour="f64")
        term = term - torch.from_numpy(np.asarray(num, dtype=np.float64))
        grad = grad - torch.from_numpy(np.exp(np.asarray(lg, dtype=np.float64))) * live[..., None]
    if reg is not None:
        over = (x64.abs() - 30.0).clamp_min(0.0)
        term = term + ((0.5 * reg[0] * x64 ** 2 + reg[1] * over ** 2) * live[..., None]).sum(dim=(1, 2))
        grad = grad + (reg[0] * x64 + 2.0 * reg[1] * torch.sign(x64) * over) * live[..., None]
    zgrad = None
    if z is not None:
        z64 = z.detach().cpu().double()
        qz = dense(xent_targets, lengths, D)
        ls = torch.log_softmax(z64, dim=2)
        term = term - c * (qz * ls).sum(dim=(1, 2))
        zgrad = -c * (qz - qz.sum(dim=2, keepdim=True) * ls.exp()) * live[..., None]
    ud = torch.ones(B, dtype=torch.float64) if u is None else u.detach().cpu().double()
    n = float((ud * lengths).sum()) if avg else 1.0
    w = ud[:, None] * (torch.ones(B, T, dtype=torch.float64) if f is None else f.detach().cpu().double())
    loss = float(torch.where(ud != 0, ud * term, torch.zeros((), dtype=torch.float64)).sum()) / n
    out = (loss, (grad * w[..., None] / n).numpy())
    return out if z is None else out + ((zgrad * w[..., None] / n).numpy(),)


distances = pr.distances
bits = pr.bits
