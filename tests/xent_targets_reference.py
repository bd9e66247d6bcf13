"""Cross-entropy of a network output z against sparse targets (include/pychain_hip.h: pychain_hip_xent_targets) in plain numpy
float64, straight from the header's equations: per live frame, with qd the fp32 sum in ascending k of the frame's q whose pdf
is d (0 <= d < D; pdf < 0 skipped, pdf >= D skipped and counted),
    s = sum_d qd,   objective = sum_d qd z(d) - s logsumexp(z),   d / dz = qd - s softmax(z)
a live frame without a live entry: objective 0, a zero row, z not looked at; rows beyond a length: zeros.

The bound a result is held to is NOT a literal: `fp32_distance` measures how far the same composition in fp32 torch arithmetic
(log_softmax, a gather of the entries, the product with q, sums, and autograd's backward) lies from np_xent_targets on the case
at hand; the code under test may lie that far away plus 1e-5, the bar of the existing xent term (tests/xent_reference.py).
The objective is measured relative, per sequence; the gradient as max |d| / max |ref|.  A gradient stored in bf16 / fp16 is
rounded once more, by at most u |element| <= u max |ref|: the bound gains u (post_reference.U)."""
import numpy as np
import torch

from post_reference import U

BAR = 1e-5


def _len(lengths, T):
    return [min(max(int(l), 1), T) for l in np.asarray(lengths).tolist()]


def np_xent_targets(z, lengths, pdfs, probs):
    """z [B,T,D] (the fp32 value of every element), pdfs / probs [B,T,K].  Returns (objf [B] f64, dz [B,T,D] f64, bad, read [B,T]
    bool: the frames whose row of z the objective depends on, mag [B] = sum over the frames of sum_d |qd z(d)| + s |lse|: the
    size of the terms the objective is the difference of)."""
    z = np.asarray(z, dtype=np.float64)
    pdfs, probs = np.asarray(pdfs), np.asarray(probs, dtype=np.float32)
    B, T, D = z.shape
    K = pdfs.shape[2]
    objf, dz, bad, mag = np.zeros(B), np.zeros((B, T, D)), 0, np.zeros(B)
    read = np.zeros((B, T), dtype=bool)
    for b, L in enumerate(_len(lengths, T)):
        for t in range(L):
            qd = {}
            for k in range(K):
                d = int(pdfs[b, t, k])
                if d < 0:
                    continue
                if d >= D:
                    bad += 1
                    continue
                qd[d] = np.float32(qd[d] + probs[b, t, k]) if d in qd else probs[b, t, k]     # the fp32 sum, ascending k
            if not qd:
                continue
            read[b, t] = True
            zr = z[b, t]
            with np.errstate(invalid="ignore"):
                m = zr.max()
                lse = m + np.log(np.exp(zr - m).sum())
                s = float(sum(float(v) for v in qd.values()))
                objf[b] += sum(float(v) * zr[d] for d, v in qd.items()) - s * lse
                mag[b] += sum(abs(float(v) * zr[d]) for d, v in qd.items()) + s * abs(lse)
                dz[b, t] = -s * np.exp(zr - lse)
            for d, v in qd.items():
                dz[b, t, d] += float(v)
    return objf, dz, bad, read, mag


def torch_xent_per_seq(z, lengths, pdfs, probs, read=None):
    """The torch composition the kernel replaces, per sequence and differentiable in z (any float dtype, any device):
    log_softmax, gather of the entries, product, masked sum.  Rows the objective does not depend on (`read` False; default: the
    rows beyond a length) are replaced by zeros first - a NaN in them would reach the others through 0 * NaN."""
    B, T, D = z.shape
    dev = z.device
    live = torch.arange(T, device=dev)[None, :] < torch.as_tensor(lengths).to(dev).clamp(1, T)[:, None]
    keep = live if read is None else torch.as_tensor(read).to(dev)
    zz = torch.where(keep[..., None], z, torch.zeros((), dtype=z.dtype, device=dev))
    pdfs, probs = pdfs.to(dev), probs.to(dev)
    ok = (pdfs >= 0) & (pdfs < D) & live[..., None]
    lp = torch.gather(torch.log_softmax(zz, dim=-1), 2, pdfs.clamp(0, D - 1).to(torch.int64))
    q = torch.where(ok, probs.to(z.dtype), torch.zeros((), dtype=z.dtype, device=dev))
    return torch.where(ok, lp * q, torch.zeros((), dtype=z.dtype, device=dev)).sum(dim=(1, 2))


def distances(objf, dz, ref):
    """(max over the sequences with a non-zero reference objective of |o - ref| / |ref|, max |dz - ref| / max |ref|); dz None:
    the objective alone.  A reference objective of exactly 0 (D = 1: log_softmax is 0) has no relative distance: the value is
    then held to what the header's arithmetic allows - the dot product sum qd z is an fp32 number, within 2^-24 of the terms it
    adds up, and the objective is its difference from s * lse: 2^-23 * mag (np_xent_targets) covers both."""
    ro, rdz = ref[0], ref[1]
    o = np.asarray(objf, dtype=np.float64)
    live = ro != 0
    d_o = float((np.abs(o[live] - ro[live]) / np.abs(ro[live])).max()) if live.any() else 0.0
    if len(ref) > 4:
        assert (np.abs(o[~live]) <= 2.0 ** -23 * ref[4][~live]).all(), (o[~live], ref[4][~live])
    if dz is None:
        return d_o, 0.0
    d_g = float(np.abs(np.asarray(dz, dtype=np.float64) - rdz).max() / max(np.abs(rdz).max(), 1e-30))
    return d_o, d_g


def fp32_distance(z, lengths, pdfs, probs, ref):
    """The distance of the fp32 torch composition from np_xent_targets (`ref`) on this case: (objective, gradient)."""
    z32 = z.detach().float().clone().requires_grad_(True)
    per = torch_xent_per_seq(z32, lengths, pdfs, probs, read=ref[3])
    per.sum().backward()
    return distances(per.detach().numpy(), z32.grad.numpy(), ref)


def bound(own, dname="float32"):
    """(objective bound, gradient bound) of a case whose fp32 composition lies `own` away: + 1e-5, + u for a 2-byte gradient"""
    return own[0] + BAR, own[1] + BAR + U[dname]
