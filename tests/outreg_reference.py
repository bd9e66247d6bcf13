"""Float64 reference of the output regularisers (include/pychain_hip.h: pychain_hip_output_reg): output L2 and the out-of-range
penalty over the live frames of the network output, and the bounds the tests hold the kernels to - derived from the number
formats and from the operation sequence csrc/outreg.hip writes down, not from what the kernels give."""
import numpy as np

LIMIT = 30.0
SUM_REL = 2.0 ** -23        # a per-sequence sum or a total: fp64 accumulation (below n * 2^-53) + at most two roundings to fp32
LOSS_REL = 2.0 ** -22       # the loss scalar: the LF-MMI scalar rounded, then the sum with the term rounded
U32 = 2.0 ** -24


def term_rel(avg):
    """Relative bound of `loss.l2_term` / `loss.out_of_range_term` against 0.5 l2 sum R2 [/ n] and oor sum RO [/ n] in float64:
    every step is one fp32 rounding of 2^-24 - the total of the sums (two: SUM_REL), the coefficient (0.5 l2 [* host scale] or
    oor, a Python float) cast to fp32, the product, and with `avg` the division by the frame count - 4 or 5 roundings, plus one
    for the fp64 accumulation and the second-order terms."""
    return (6 if avg else 5) * U32


K_ROUNDINGS = 8             # 7 fp32 roundings of the gradient term's operation sequence (two for s, l2 x, e, the fma, the product,
                            # the add) plus one
U_HALF = {"bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
F16_SUBNORMAL = 2.0 ** -25  # half the spacing of fp16 subnormals


def np_outreg(x, lengths, l2, oor):
    """(R2 [B], RO [B], term [B,T,D], loss term) in float64: R2_b = sum of x^2 and RO_b = sum of max(|x| - 30, 0)^2 over the live
    frames t < L_b, term = l2 x + 2 oor sign(x) max(|x| - 30, 0) on live frames and exactly 0 beyond them, loss term =
    0.5 l2 sum R2 + oor sum RO (un-averaged).  Frames beyond a length are not read."""
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    R2, RO, term = np.zeros(B), np.zeros(B), np.zeros((B, T, D))
    for b in range(B):
        L = int(min(max(int(lengths[b]), 1), T))
        v = x[b, :L]
        e = np.maximum(np.abs(v) - LIMIT, 0.0)
        e = np.where(np.isnan(v), np.nan, e)                 # (np.maximum keeps a NaN already; said aloud)
        R2[b], RO[b] = (v * v).sum(), (e * e).sum()
        term[b, :L] = l2 * v + 2.0 * oor * np.sign(v) * e
    return R2, RO, term, 0.5 * l2 * R2.sum() + oor * RO.sum()


def term_magnitude(x, lengths, l2, oor):
    """l2 |x| + 2 oor e(x) on live frames (0 beyond): what the roundings of the gradient term are relative to."""
    x = np.asarray(x, dtype=np.float64)
    m = np.zeros_like(x)
    for b in range(x.shape[0]):
        L = int(min(max(int(lengths[b]), 1), x.shape[1]))
        v = np.abs(x[b, :L])
        m[b, :L] = l2 * v + 2.0 * oor * np.maximum(v - LIMIT, 0.0)
    return m


def grad_bound(want, mag, s, dtype="float32"):
    """The bound on |got - want| for a gradient `want` = [stored g +] s * term (float64), element by element:
    fp32: 2^-24 |want| (the last rounding) + K * 2^-24 |s| (l2 |x| + 2 oor e); 2-byte gradients: u |want| (the rounding at the
    store) on top of the fp32 bound, and for fp16 an absolute 2^-25 where the result is subnormal."""
    b = U32 * np.abs(want) + K_ROUNDINGS * U32 * abs(s) * mag
    if dtype != "float32":
        b = b + U_HALF[dtype] * np.abs(want) + (F16_SUBNORMAL if dtype == "float16" else 0.0)
    return b


def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound (elements with a zero bound must agree exactly); <= 1 passes."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0
