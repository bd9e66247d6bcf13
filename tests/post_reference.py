"""Posterior-target supervision (include/pychain_hip.h: pychain_hip_post_targets, pychain_hip_topk_rows) restated in plain numpy
float64 from the header text alone, the bounds the tests hold the library to, and the inputs both test files share.

THE BOUNDS ARE DERIVED, NOT CHOSEN.
  objective   The library widens x and q to fp64 (every product exact), adds the n terms of a sequence in fp64 - each add within
              2^-53 of the running sum, which never exceeds sum |q clamp(x)| - and rounds once to fp32 (2^-24 |ref|):
                  2^-24 |ref| + n 2^-53 sum |q clamp(x)|
  gradient    fp32: ONE correctly rounded fma on the very operands the reference multiplies (s and qd are formed here in fp32
              exactly as the header says): 2^-24 |ref|.  2-byte: that value is then rounded to nearest even to bf16 / fp16,
              u |ref| (u = 2^-8 / 2^-11), and the fp32 rounding before it moves the result by at most 2^-24 (1 + u) |ref| <
              2^-23 |ref|: (u + 2^-23) |ref|, plus 2^-25 absolute where fp16 goes subnormal (spacing 2^-24).
  top-k       pdfs and un-normalised values: the same bits (a selection and an exact widening).  Normalised values: the fp32 sum
              in slot order and one IEEE division are restated here operation by operation, so they would agree to the bit; the
              bound allows one ulp, 2^-23 relative.
"""
import numpy as np
import torch

U = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
TOPK_REL = 2.0 ** -23
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def _len(lengths, T):
    return [min(max(int(l), 1), T) for l in np.asarray(lengths).tolist()]


def f32_scale(grad_scale, grad_scale_dev=None, norm=None):
    """s = grad_scale [* grad_scale_dev] [/ norm], formed in fp32"""
    s = np.float32(grad_scale)
    if grad_scale_dev is not None:
        s = np.float32(s * np.float32(grad_scale_dev))
    if norm is not None:
        s = np.float32(s / np.float32(norm))
    return s


def np_post_targets(x, lengths, pdfs, probs, grad=None, s=1.0):
    """x [B,T,D] (the fp32 value of every element), pdfs / probs [B,T,K].  Returns a dict: num [B] float64 (math.fsum: the exact
    sum, rounded once), mag [B] = sum |q clamp(x)|, terms [B], bad, and - `grad` given, the stored gradient's values - want
    [B,T,D] float64 = grad + s qd at the addressed elements and touched [B,T,D] bool."""
    import math
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    K = pdfs.shape[2]
    num, mag, terms = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int64)
    bad = 0
    want = None if grad is None else np.array(grad, dtype=np.float64)
    touched = np.zeros(x.shape, dtype=bool)
    sd = float(np.float32(s))
    for b, L in enumerate(_len(lengths, T)):
        parts = []
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
                parts.append(float(q) * float(np.clip(x[b, t, d], -30.0, 30.0)) if not np.isnan(x[b, t, d]) else float("nan"))
                qd[d] = np.float32(qd[d] + q) if d in qd else q              # the fp32 sum, ascending k
            if want is not None:
                for d, v in qd.items():
                    want[b, t, d] = want[b, t, d] + sd * float(v)
                    touched[b, t, d] = True
        num[b] = math.fsum(parts) if not any(np.isnan(p) for p in parts) else float("nan")
        mag[b] = math.fsum(abs(p) for p in parts if not np.isnan(p))
        terms[b] = len(parts)
    return dict(num=num, mag=mag, terms=terms, bad=bad, want=want, touched=touched)


def objf_bound(ref):
    return 2.0 ** -24 * np.abs(ref["num"]) + ref["terms"] * 2.0 ** -53 * ref["mag"]


def grad_bound(want, dname):
    u = U[dname]
    if u == 0.0:
        return 2.0 ** -24 * np.abs(want)
    return (u + 2.0 ** -23) * np.abs(want) + (2.0 ** -25 if dname == "float16" else 0.0)


def np_totals(den, ref, before, loss_scale=1.0, norm=None):
    """The totals contract over a pre-filled totals[8]: (expected float64 [8], the indices that keep their bits)."""
    S = float(np.sum(np.asarray(den, dtype=np.float64))) - float(np.sum(ref["num"]))
    out = np.array(before, dtype=np.float64)
    out[3] = S
    out[0] = out[4] = loss_scale * S / (1.0 if norm is None else float(np.float32(norm)))
    out[2] = out[2] + ref["bad"]
    return out, (1, 5, 6, 7)


def totals_bounds(want, ref):
    """(bound on totals[3], bound on totals[0]): the numerator sums' own error carried into S, one rounding to fp32 each"""
    e = float(np.nansum(objf_bound(ref)))
    scale = abs(want[0] / want[3]) if want[3] else 1.0
    return 2.0 ** -24 * abs(want[3]) + e, 2.0 ** -24 * abs(want[0]) + scale * e + 2.0 ** -52 * abs(want[0])


def np_topk(rows, lengths, K, floor=0.0, normalize=True):
    """(pdfs int32 [B,T,K], probs float32 [B,T,K]): per live frame the first K elements >= floor in the order value descending,
    index ascending (a NaN is never selected); with `normalize`, divided by their fp32 sum in slot order."""
    rows = np.asarray(rows, dtype=np.float32)
    B, T, D = rows.shape
    pdfs = np.full((B, T, K), -1, dtype=np.int32)
    probs = np.zeros((B, T, K), dtype=np.float32)
    fl = np.float32(floor)
    for b, L in enumerate(_len(lengths, T)):
        for t in range(L):
            r = rows[b, t]
            keep = [i for i in range(D) if r[i] >= fl]                       # (a NaN fails the comparison)
            keep.sort(key=lambda i: (-float(r[i]), i))
            keep = keep[:K]
            vals = [np.float32(r[i]) for i in keep]
            if normalize and keep:
                tot = np.float32(0.0)
                for v in vals:
                    tot = np.float32(tot + v)
                with np.errstate(divide="ignore", invalid="ignore"):
                    vals = [np.float32(v / tot) for v in vals]
            for j, (i, v) in enumerate(zip(keep, vals)):
                pdfs[b, t, j], probs[b, t, j] = i, v
    return pdfs, probs


def topk_values_ok(got, want, normalize):
    """un-normalised: the same bits; normalised: within TOPK_REL (a frame whose selected values sum to zero divides by zero on
    both sides: a NaN where the reference has one)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if not normalize:
        return bool(np.array_equal(got.view(np.int32), want.view(np.int32)))
    with np.errstate(invalid="ignore"):
        return bool(((np.abs(got - want) <= TOPK_REL * np.abs(want)) | (np.isnan(got) & np.isnan(want)) | (got == want)).all())


# ---- the inputs of the native tests (both test files) ----------------------------------------------------------------------------
NATIVE_B, NATIVE_T = 3, 9
NATIVE_LENGTHS = [9, 1, 4]
NATIVE_DS = [1, 3, 8, 257, 3456]
NATIVE_KS = [1, 3, 4, 8, 33]


def native_case(D, K, dname="float32", seed=11):
    """x uniform in +-40 with exact +-30 in live rows (and referenced), a NaN in every padded row and every padded target, a frame
    whose entries are all -1, a frame with one pdf three times (as often as K allows), ONE entry with pdf >= D.  Returns (x in
    `dname`, lengths int64 [B], pdfs int32 [B,T,K], probs float32 [B,T,K])."""
    B, T = NATIVE_B, NATIVE_T
    g = torch.Generator().manual_seed(seed + 131 * D + K)
    x = (torch.rand(B, T, D, generator=g) * 80.0 - 40.0).float()
    pdfs = torch.randint(0, D, (B, T, K), generator=g).to(torch.int32)
    pdfs[torch.rand(B, T, K, generator=g) < 0.2] = -1
    probs = torch.rand(B, T, K, generator=g).float()
    x[0, 0, 0], x[0, 0, D - 1] = 30.0, -30.0
    pdfs[0, 0, 0] = 0
    if K > 1:
        pdfs[0, 0, 1] = D - 1
    pdfs[0, 1, :] = -1                                        # a frame without entries
    pdfs[0, 2, :min(K, 3)] = D // 2                           # one pdf three times
    pdfs[0, 3, 0] = D                                         # the one bad entry
    lengths = torch.tensor(NATIVE_LENGTHS, dtype=torch.int64)
    for b, L in enumerate(NATIVE_LENGTHS):
        x[b, L:] = float("nan")
        probs[b, L:] = float("nan")
        pdfs[b, L:] = 2 ** 30                                 # (never read: would address far outside the row)
    return x.to(DTYPES[dname]), lengths, pdfs, probs


def grad_pattern(shape, dname):
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 251.0) * 0.01 - 1.0).reshape(shape).to(DTYPES[dname])


def topk_case(D, dname="float32", seed=5):
    """Rows with ties (values on a coarse grid, so equal values are frequent), NaNs in live rows, values below zero; NaN in every
    padded row."""
    B, T = NATIVE_B, NATIVE_T
    g = torch.Generator().manual_seed(seed + D)
    rows = (torch.randint(-4, 13, (B, T, D), generator=g).float() / 16.0)
    rows[torch.rand(B, T, D, generator=g) < 0.1] = float("nan")
    rows[0, 0, :] = 0.25                                       # a whole row of equal values: the lowest indices win
    if D > 2:
        rows[0, 4, :] = -1.0                                   # nothing at or above a floor of 0
    lengths = torch.tensor(NATIVE_LENGTHS, dtype=torch.int64)
    for b, L in enumerate(NATIVE_LENGTHS):
        rows[b, L:] = float("nan")
    return rows.to(DTYPES[dname]), lengths


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def straight_through_clamp(x):
    """clamp(x, -30, 30) in value with the gradient of x: the library does not differentiate its clamp"""
    return x + (x.clamp(-30.0, 30.0) - x).detach()


def torch_numerator_per_seq(x, lengths, pdfs, probs):
    """The torch composition of the numerator, per sequence and differentiable in x: gather, multiply, mask, sum."""
    B, T, D = x.shape
    live = (torch.arange(T, device=x.device)[None, :] < torch.as_tensor(lengths).to(x.device)[:, None])[..., None]
    ok = (pdfs >= 0) & (pdfs < D) & live
    idx = pdfs.clamp(0, D - 1).to(torch.int64)
    vals = torch.gather(straight_through_clamp(x), 2, idx)
    q = torch.where(ok, probs.to(x.dtype), torch.zeros((), dtype=x.dtype, device=x.device))
    return torch.where(ok, vals * q, torch.zeros((), dtype=x.dtype, device=x.device)).sum(dim=(1, 2))


def composition(den_graph, x, lengths, targets, avg=True, u=None, f=None, reg=None, dtype=torch.float64):
    """(loss, d loss / dx as numpy float64) by the torch composition the feature replaces, on x's device: ChainFunction on the
    denominator, a gathered q * clamp(x), the regularisers written out, autograd's add; the weights applied to the rows of the
    un-weighted gradient and to the per-sequence terms."""
    from pychain_amd import ChainFunction, ChainGraphBatch
    B, T = x.size(0), x.size(1)
    dev = x.device
    lengths = torch.as_tensor(lengths).cpu()
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    den = ChainFunction.apply(xx, lengths, ChainGraphBatch(den_graph, B), 1e-5)
    num = torch_numerator_per_seq(xx, lengths, targets.pdfs.to(dev), targets.probs.to(dev))
    live = (torch.arange(T)[None, :] < lengths[:, None]).to(device=dev, dtype=dtype)
    term = -num
    if reg is not None:
        sq = 0.5 * reg[0] * xx ** 2 + reg[1] * (xx.abs() - 30.0).clamp_min(0.0) ** 2
        term = term + torch.where(live[..., None] > 0, sq, torch.zeros((), dtype=dtype, device=dev)).sum(dim=(1, 2))
    ud = torch.ones(B, dtype=torch.float64) if u is None else u.detach().cpu().double()
    n = float((ud * lengths).sum()) if avg else 1.0
    (den + term.sum()).backward()                                   # the un-weighted gradient, row by row
    w = ud[:, None] * (torch.ones(B, T, dtype=torch.float64) if f is None else f.detach().cpu().double())
    grad = xx.grad.detach().cpu().double() * w[..., None] / n
    per_seq = den._objf_per_seq.detach().cpu().double() + term.detach().cpu().double()
    value = float(torch.where(ud != 0, ud * per_seq, torch.zeros(())).sum()) / n
    return value, grad.numpy()


def distances(loss, grad, want_loss, want_grad):
    """(|d loss| / |loss|, max |d grad| / max |grad|): the library's two parity figures"""
    grad = np.asarray(grad, dtype=np.float64)
    return abs(float(loss) - want_loss) / abs(want_loss), float(np.abs(grad - want_grad).max() / np.abs(want_grad).max())
