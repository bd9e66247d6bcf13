"""Reference of the utterance / derivative weights pass (include/pychain_hip.h: pychain_hip_weight_rows) and the bounds the
tests hold it to.  The rows are held BIT FOR BIT: the expectation is a single IEEE fp32 multiply and a single rounding to the
gradient's type, which numpy (fp32 multiply) and torch (round to nearest even in .to(dtype)) restate exactly - no tolerance is
chosen.  The sums are fp64 and rounded once; their bounds are derived the way tests/outreg_reference.py derives its own."""
import numpy as np
import torch

SUM_REL = 2.0 ** -23        # a weighted sum: fp64 accumulation (below n * 2^-53 of the sum of magnitudes) + one rounding to fp32
LOSS_REL = 2.0 ** -22       # the loss scalar: the same, scaled and divided in fp64, rounded once; a second rounding where the
                            # comparand is itself an fp32 value
TERM_REL = 2.0 ** -21       # loss.xent_objf / l2_term / out_of_range_term on the fused route: the weighted sum (SUM_REL = 2 * 2^-24),
                            # then fp32 steps of 2^-24 each - the coefficient cast to fp32 and its product, the host scale cast and
                            # its product, the device normaliser's own rounding and the division: 2 + 6 = 8 roundings of 2^-24
WEIGHT_VALUES = (0.0, 1.0, 0.5, 3.0, 0.3)


def draw_weights(B, T, seed, which):
    """(u [B] or None, f [B,T] or None) drawn from WEIGHT_VALUES; every value occurs among the rows' products."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(WEIGHT_VALUES)
    u = vals[torch.randint(0, len(vals), (B,), generator=g)] if which in ("u", "both") else None
    f = vals[torch.randint(0, len(vals), (B, T), generator=g)] if which in ("f", "both") else None
    if u is not None:
        u[:3] = torch.tensor([0.5, 1.0, 0.0])[:B]           # a scaled, an untouched and a dropped utterance
    if f is not None:
        f[0, : min(T, 5)] = vals[: min(T, 5)]
    return u, f


def row_weights(B, T, u=None, f=None):
    """w [B,T] float32 = fl32(u_b * f_bt), a missing factor is 1"""
    w = np.ones((B, T), dtype=np.float32)
    if u is not None:
        w = w * np.asarray(u, dtype=np.float32)[:, None]
    if f is not None:
        w = (w * np.asarray(f, dtype=np.float32)).astype(np.float32)
    return w


def np_weight_rows(grad, lengths, u=None, f=None):
    """What the pass leaves of `grad` (torch [B,T,D], fp32 / bf16 / fp16): widen to fp32, ONE fp32 multiply by w, round to the
    dtype; rows with w == 1 and rows t >= L keep their bits, rows with w == 0 become +0."""
    B, T, D = grad.shape
    w = row_weights(B, T, u, f)
    g32 = grad.float().numpy()                               # (exact)
    prod = (g32 * w[:, :, None]).astype(np.float32)          # one IEEE multiply
    out = torch.from_numpy(prod).to(grad.dtype)              # one rounding, to nearest even
    keep = np.zeros((B, T), dtype=bool)
    for b in range(B):
        L = int(min(max(int(lengths[b]), 1), T))
        keep[b, L:] = True
    keep |= w == 1.0
    zero = (w == 0.0) & ~keep
    out = torch.where(torch.from_numpy(keep)[:, :, None], grad, out)
    return torch.where(torch.from_numpy(zero)[:, :, None], torch.zeros_like(out), out)


def np_weighted_sums(u, lengths, den, num, xent=None, c=0.0, reg=None, l2=0.0, oor=0.0, T=None):
    """dict of float64: lf = sum u (den - num), sx = sum u xent, s2 = sum u R2, so = sum u RO, sl = sum u L, value = the weighted
    objective sum_b u_b term_b (unscaled), mag = sum_b |u_b| (|den_b| + |num_b| + ...) - what the roundings are relative to.  An
    utterance with u_b == 0 is skipped."""
    B = len(lengths)
    u = np.ones(B) if u is None else np.asarray(u, dtype=np.float64)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    r = dict(lf=0.0, sx=0.0, s2=0.0, so=0.0, sl=0.0, mag=0.0)
    for b in range(B):
        if u[b] == 0.0:
            continue
        L = int(lengths[b]) if T is None else int(min(max(int(lengths[b]), 1), T))
        r["lf"] += u[b] * (f64(den[b]) - f64(num[b]))
        r["mag"] += abs(u[b]) * (abs(f64(den[b])) + abs(f64(num[b])))
        r["sl"] += u[b] * L
        if xent is not None:
            r["sx"] += u[b] * f64(xent[b])
            r["mag"] += abs(u[b] * c * f64(xent[b]))
        if reg is not None:
            r["s2"] += u[b] * f64(reg[b][0])
            r["so"] += u[b] * f64(reg[b][1])
            r["mag"] += abs(u[b]) * (0.5 * l2 * f64(reg[b][0]) + oor * f64(reg[b][1]))
    r["value"] = r["lf"] - c * r["sx"] + 0.5 * l2 * r["s2"] + oor * r["so"]
    return r


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))
