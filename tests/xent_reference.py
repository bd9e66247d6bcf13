"""Plain float64 reference of the cross-entropy objective against the numerator posteriors (include/pychain_hip.h:
pychain_hip_xent), written from the header: gamma from tests/num_reference.np_num_fb, then per live frame
    objective = sum_d gamma z - s logsumexp(z),   d / dz = gamma - s softmax(z),   s = sum_d gamma
(terms with gamma = 0 left out of the dot product; a sequence without an admissible path: objective 0, zero rows).

The bound a result is held to is NOT a literal: `fp32_distance` measures how far the same composition in fp32 torch arithmetic
(log_softmax, product, sum and their autograd backward), fed the float64 reference's own gamma, lies from np_xent on the
case at hand; the code under test may lie that far away plus the 1e-5 the project holds gamma itself to (README,
"Numerical differences": the triangle rule)."""
import numpy as np
import torch

from helpers import rel_err
from num_reference import np_num_fb

GAMMA_BOUND = 1e-5


def np_xent(graphs, x, z, lengths, windows=None, fb=None):
    """(xent_objf[B] f64, dz[B,T,D] f64).  `fb`: np_num_fb's result for (graphs, x, lengths, windows), if the caller has it."""
    logp, gamma, feas = fb if fb is not None else np_num_fb(graphs, x, lengths, windows)
    z64 = z.detach().float().numpy().astype(np.float64)
    B, T, D = z64.shape
    objf = np.zeros(B)
    dz = np.zeros((B, T, D))
    for b in range(B):
        if not feas[b]:
            continue
        L = int(lengths[b])
        zr, g = z64[b, :L], gamma[b, :L]
        m = zr.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(zr - m).sum(axis=1, keepdims=True))
        s = g.sum(axis=1, keepdims=True)
        objf[b] = float((np.where(g > 0, g * zr, 0.0).sum(axis=1) - s[:, 0] * lse[:, 0]).sum())
        dz[b, :L] = g - s * np.exp(zr - lse)
    return objf, dz


def _distances(objf, dz, ref):
    """(max over the sequences with a non-zero reference objective of |o - ref| / |ref|, max |dz - ref| / max |ref|)."""
    ro, rdz = ref
    o = np.asarray(objf, dtype=np.float64)
    live = ro != 0
    d_o = float((np.abs(o[live] - ro[live]) / np.abs(ro[live])).max()) if live.any() else 0.0
    return d_o, float(rel_err(dz, rdz))


def fp32_distance(graphs, x, z, lengths, windows=None, fb=None, ref=None):
    """The distance of the fp32 torch composition fed the float64 reference's gamma from np_xent: (objective, gradient)."""
    fb = fb if fb is not None else np_num_fb(graphs, x, lengths, windows)
    ref = ref if ref is not None else np_xent(graphs, x, z, lengths, windows, fb)
    gamma32 = torch.from_numpy(fb[1].astype(np.float32))
    z32 = z.detach().float().clone().requires_grad_(True)
    per_frame = (gamma32 * torch.log_softmax(z32, dim=-1)).sum(-1)
    objf = torch.stack([per_frame[b, :int(lengths[b])].sum() for b in range(z32.shape[0])])
    objf.sum().backward()
    return _distances(objf.detach().numpy(), z32.grad.numpy(), ref)


def check_xent(objf, dz, ref, lengths, feasible, bound, name=None):
    """Objective and gradient within `bound` = (objective, gradient) of np_xent; zero rows beyond every length and for a
    sequence without an admissible path, whose objective is exactly 0.  Returns the two distances."""
    o = np.asarray(objf, dtype=np.float64)
    g = np.asarray(dz, dtype=np.float64)
    for b, L in enumerate(np.asarray(lengths).tolist()):
        assert not g[b, L:].any()
    for b in np.nonzero(~np.asarray(feasible))[0]:
        assert o[b] == 0.0 and not g[b].any()
    d_o, d_g = _distances(o, g, ref)
    if name:
        print("%s: xent objective %.3e (bound %.3e) gradient %.3e (bound %.3e)" % (name, d_o, bound[0], d_g, bound[1]))
    assert d_o <= bound[0] and d_g <= bound[1], (d_o, d_g, bound)
    return d_o, d_g
