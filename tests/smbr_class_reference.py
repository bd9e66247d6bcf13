"""Lattice-free sMBR with the accuracy by class (include/pychain_hip.h: pychain_hip_smbr_*_classes) for the tests:
the dense accuracy rows A(t,n) = Acls(t, cls[n]) built from the definition, handed to the two evaluations of tests/smbr_reference
(`recursions`, `autograd`: both take a dense A), over smbr_reference.CASES under three maps

  phones    cls[n] = 7 n // 20: uneven classes of two to three pdfs (the last may be short); the pdf no arc of `degenerate`
            carries, 8, shares class 2 with carried pdfs
  identity  the pdf-level quantities
  one       a single class: E_b = sum_t sum_k q_k, a zero gradient

and the faults planted into the rows (FAULTS) that show what the cases can see.  The targets are copies of the shared ones with,
in every third frame, two DIFFERENT pdfs of one `phones` class - their credit must add; they keep padding behind and in front of
a live entry, a pdf twice in a frame and an utterance without targets.

Tolerance: the rule of smbr_reference.bound with the class-level rows - 1e-5, or twice the fp32 numpy recursions' own distance
from fp64 where that is beyond 5e-6.  Gradient distances are relative to max |grad| of the fp64 reference; under `one`, whose
gradient is zero, to max |grad| of the pdf-level (identity) reference of the same targets."""
import numpy as np
import torch

import smbr_reference as sr

MAPS = ("phones", "identity", "one")
FAULTS = ("first_entry_only", "pdf_credit")
_made, _refs = {}, {}


def class_map(name, D):
    """int64 numpy [D]"""
    n = np.arange(D, dtype=np.int64)
    return {"phones": 7 * n // 20, "identity": n, "one": np.zeros(D, dtype=np.int64)}[name]


def classes(name, D):
    return torch.from_numpy(class_map(name, D)).to(torch.int32)


def case(name):
    """(graph, y, lengths, pdfs int32 [B,T,2], probs float32 [B,T,2]) as smbr_reference.case, the targets this file's own."""
    if name not in _made:
        g, y, lengths, pdfs, probs = sr.case(name)
        pdfs = pdfs.clone().numpy()
        D = y.size(2)
        ph = class_map("phones", D)
        B, T = pdfs.shape[:2]
        for b in range(B - 1):                                 # (the last utterance stays without targets)
            for t in range(1, T, 3):
                n = int(pdfs[b, t, 0])
                if n < 0:
                    continue                                   # (padding in front of a live entry stays)
                if n + 1 < D and ph[n + 1] == ph[n]:
                    m = n + 1
                elif n > 0 and ph[n - 1] == ph[n]:
                    m = n - 1
                else:                                          # a pdf alone in its class (the last, short class): its neighbours
                    n, m = n - 1, n - 2
                    pdfs[b, t, 0] = n
                assert m != n and ph[m] == ph[n]
                pdfs[b, t, 1] = m
        live = pdfs[:B - 1]
        assert (live[:, :, 1] < 0).any() and (live[:, :, 0] < 0).any() and (pdfs[B - 1] < 0).all()
        assert ((live[:, 0::3, 0] == live[:, 0::3, 1]) & (live[:, 0::3, 0] >= 0)).any()
        _made[name] = (g, y, lengths, torch.from_numpy(pdfs), probs.clone())
    return _made[name]


def dense_class_accuracy(pdfs, probs, cls, C, targets_are_classes=False, fault=None):
    """A(t,n) = Acls(t, cls[n]) [T,D] float64 of one utterance's sparse targets [T,K]: the q of a class add in ascending k; an id
    < 0, a pdf >= D or a class >= C adds nothing."""
    T, K = pdfs.shape
    D = cls.shape[0]
    if fault == "pdf_credit":                                   # pdf-level credit where class credit is due
        return sr.dense_accuracy(pdfs, probs, D)
    acl = np.zeros((T, C))
    for t in range(T):
        seen = set()
        for k in range(K):
            i = int(pdfs[t, k])
            if i < 0 or i >= (C if targets_are_classes else D):
                continue
            c = i if targets_are_classes else int(cls[i])
            if fault == "first_entry_only" and c in seen:       # the table made from the first entry of a class only
                continue
            seen.add(c)
            acl[t, c] += float(probs[t, k])
    return acl[:, cls]


def batch(fn, graph, y, lengths, pdfs, probs, cls, coef, targets_are_classes=False, fault=None, **kw):
    """`fn` (smbr_reference.recursions or .autograd) over a batch with the rows by class: (E [B], grad [B,T,D], extra [B])."""
    arrays = sr.graph_arrays(graph)
    y = y.detach().double().numpy() if torch.is_tensor(y) else np.asarray(y, dtype=np.float64)
    pdfs, probs, cls = np.asarray(pdfs), np.asarray(probs), np.asarray(cls, dtype=np.int64)
    C = int(cls.max()) + 1
    B, T, D = y.shape
    E, G, X = np.zeros(B), np.zeros((B, T, D)), np.zeros(B)
    for b in range(B):
        L = int(lengths[b])
        A = dense_class_accuracy(pdfs[b, :L], probs[b, :L], cls, C, targets_are_classes, fault)
        r = fn(arrays, y[b, :L], A, coef, **kw)
        E[b], G[b, :L] = r[0], r[1]
        X[b] = r[2] if len(r) > 2 else 0.0
    return E, G, X


def grad_dist(g, want, scale):
    """max |d grad| / scale over the batch."""
    return float(np.abs(np.asarray(g, dtype=np.float64) - want).max() / scale)


def reference(name, which, coef):
    """((E [B], grad [B,T,D], closing [B]), (bound, fp32 distance), scale) of case `name` under map `which` by the fp64 recursions,
    once per process.  `scale`: what gradient distances of this case are relative to (the module's docstring)."""
    key = (name, which, coef)
    if key not in _refs:
        g, y, lengths, pdfs, probs = case(name)
        cls = class_map(which, y.size(2))
        ref = batch(sr.recursions, g, y, lengths, pdfs.numpy(), probs.numpy(), cls, coef)
        scale = float(np.abs(ref[1]).max()) if which != "one" else reference(name, "identity", coef)[2]
        e32, g32, _ = batch(sr.recursions, g, y, lengths, pdfs.numpy(), probs.numpy(), cls, coef, dtype=np.float32)
        d = max(grad_dist(g32, ref[1], scale), sr.value_dist(e32, ref[0]))
        _refs[key] = (ref, ((2.0 * d if d > sr.F32_SLACK else sr.BAR), d), scale)
    return _refs[key]
