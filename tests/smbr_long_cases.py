"""Lattice-free sMBR at TRAINING lengths and on peaked rows, one definition for the CPU and the GPU tests
(tests/test_smbr_long.py, tests/test_gpu_smbr_long.py).  Every case of smbr_reference.CASES has T <= 17 and Gaussian rows; here:

  LONG_CASES   ladder   H=37, K=150, D=23, lengths [1500, 400, 100, 48], peaky.path_input: one call charts the growth with length
               clamp    the same graph, lengths [400, 123], peaky.clamp_input: rows beyond +-30 on both sides
               mid      H=300, K=3000, D=130, lengths [400, 57], path_input
               flat     H=37, one sequence of 1500 frames of synthetic.make_input rows, the targets of smbr_reference.case (two
                        entries a frame, padding, a pdf twice) without the empty utterance: peaks are not needed
    Sequence b of the first three: x, walk = maker(G, L_b, D, seed=20 + b); the targets have K = 1 and q = 1 on the pdf of the
    walk, the frames t % 5 == 0 redrawn from RandomState(3).randint(D); beyond L_b padding (-1) and zero rows.
  WIDE_CASES   more than 2048 states (three states per recursion thread, up to six per gradient thread), short
  MANY_CASES   more than 64 target entries a frame, with repeats and padding among them

`reference(name, form, coef)` is the fp64 evaluation (smbr_reference.recursions) of a case under a form - "pdf" (no map),
"identity", "phones" (smbr_class_reference.class_map) - with the bound of smbr_reference.bound, UNCHANGED: BAR, or twice the fp32
numpy recursions' own distance where that is beyond F32_SLACK.  `per_sequence` gives the same per sequence, each sequence with a
bound of its own by the same rule."""
import numpy as np
import torch

import peaky
import smbr_class_reference as cr
import smbr_reference as sr

COEFS = sr.COEFS
FORMS = ("pdf", "identity", "phones")
LONG_CASES = {
    "ladder": dict(H=37, K=150, D=23, lengths=[1500, 400, 100, 48], rows="path"),
    "clamp": dict(H=37, K=150, D=23, lengths=[400, 123], rows="clamp"),
    "mid": dict(H=300, K=3000, D=130, lengths=[400, 57], rows="path"),
    "flat": dict(H=37, K=150, D=23, lengths=[1500], rows="flat"),
}
# (graph seed 0: make_den_graph's default)
WIDE_CASES = {
    "wide3": dict(H=3000, K=9000, D=40, lengths=[6, 3], rows="flat", graph_seed=0, coef=0.1),            # K = 2, as `flat`
    # (path_input over 12 and 5 frames, the targets of the long cases: at [6, 3] the walk leaves no doubt and max |grad| is 5e-4)
    "wide3_peaked": dict(H=2100, K=7000, D=40, lengths=[12, 5], rows="path", graph_seed=0, coef=1e-5),
}
MANY_CASES = {
    "many70": dict(H=37, K=150, D=23, lengths=[9, 4], Kt=70),
    "many130": dict(H=200, K=1500, D=600, lengths=[9, 4], Kt=130),
}
_made, _refs, _seqs = {}, {}, {}


def _graph(c):
    from pychain_amd import synthetic as syn
    return syn.make_den_graph(c["H"], c["K"], c["D"], seed=c.get("graph_seed", 3))


def _case_targets(name, B, T, D):
    """the targets of smbr_reference.case (K = 2: padding behind and in front of a live entry, a pdf twice in a frame), every
    utterance with targets"""
    from pychain_amd import synthetic as syn
    seed = 11 + len(name)
    pdfs = syn.randint(seed, B * T * 2, D).reshape(B, T, 2).astype(np.int32)
    probs = (0.05 + syn.uniform(seed + 1, B * T * 2)).reshape(B, T, 2).astype(np.float32)
    pdfs[:, 1::4, 1] = -1
    pdfs[:, 2::5, 0] = -1
    pdfs[:, 0::3, 1] = pdfs[:, 0::3, 0]
    return pdfs, probs


def _walk_rows(c, graph):
    """(y [B,T,D] float32, the pdf of the walk per frame [B,T], -1 beyond a length)"""
    G = peaky.graph_arrays(graph)
    maker = {"path": peaky.path_input, "clamp": peaky.clamp_input}[c["rows"]]
    lengths, D = c["lengths"], c["D"]
    B, T = len(lengths), max(lengths)
    y, ali = np.zeros((B, T, D), dtype=np.float32), np.full((B, T), -1, dtype=np.int64)
    for b, L in enumerate(lengths):
        y[b, :L], walk = maker(G, L, D, seed=20 + b)
        for first, n, _, pdf in walk:
            ali[b, first:first + n] = pdf
    return y, ali


def case(name):
    """(graph, y float32 [B,T,D], lengths, pdfs int32 [B,T,K], probs float32 [B,T,K]) of a case of the three tables, made once
    and shared (do not edit in place)."""
    if name in _made:
        return _made[name]
    from pychain_amd import synthetic as syn
    c = LONG_CASES.get(name) or WIDE_CASES.get(name) or MANY_CASES[name]
    graph = _graph(c)
    lengths, D = c["lengths"], c["D"]
    B, T = len(lengths), max(lengths)
    if name in MANY_CASES:
        Kt = c["Kt"]
        y = syn.make_input(B, T, D, seed=5).numpy().copy()
        rs = np.random.RandomState(7 + Kt)
        pdfs = rs.randint(D, size=(B, T, Kt)).astype(np.int32)                  # (Kt > D on the small graph: every frame repeats)
        probs = (0.05 + rs.uniform(size=(B, T, Kt)) / Kt).astype(np.float32)
        pdfs[:, :, 3::7] = -1                                                   # padding among the live entries
        pdfs[:, :, 66] = pdfs[:, :, 1]                                          # a repeat across the 64 entries of a wave's chunk
        pdfs[:, 1::2, Kt - 1] = pdfs[:, 1::2, 0]                                # ... and of the first entry in the last
        pdfs[:, 2, 64:] = -1                                                    # a frame whose entries beyond 64 are all padding
    elif c["rows"] == "flat":
        y = syn.make_input(B, T, D, seed=5).numpy().copy()
        pdfs, probs = _case_targets(name, B, T, D)
    else:
        y, pdfs = _walk_rows(c, graph)
        for b, L in enumerate(lengths):
            rs = np.random.RandomState(3)
            for t in range(0, L, 5):
                pdfs[b, t] = rs.randint(D)
        pdfs = pdfs.astype(np.int32)[:, :, None]
        probs = np.ones(pdfs.shape, dtype=np.float32)
    for b, L in enumerate(lengths):
        y[b, L:], pdfs[b, L:], probs[b, L:] = 0.0, -1, 0.0
    _made[name] = (graph, torch.from_numpy(y), torch.tensor(lengths), torch.from_numpy(pdfs), torch.from_numpy(probs))
    return _made[name]


def class_map(form, D):
    return cr.class_map("identity" if form == "pdf" else form, D)


def classes(form, D):
    """what expected_accuracy takes as `classes` under a form: None for the pdf-level call"""
    return None if form == "pdf" else cr.classes(form, D)


def _evaluate(g, y, lengths, pdfs, probs, cls, coef):
    ref = cr.batch(sr.recursions, g, y, lengths, pdfs, probs, cls, coef)
    e32, g32, _ = cr.batch(sr.recursions, g, y, lengths, pdfs, probs, cls, coef, dtype=np.float32)
    scale = float(np.abs(ref[1]).max())
    d = max(cr.grad_dist(g32, ref[1], scale), sr.value_dist(e32, ref[0]))
    return ref, ((2.0 * d if d > sr.F32_SLACK else sr.BAR), d), scale


def reference(name, form, coef, y=None):
    """((E [B], grad [B,T,D], closing [B]), (bound, fp32 distance), scale = max |grad|) by the fp64 recursions, once per process
    (the pdf-level form and `identity` are one quantity and share theirs).  `y`: other rows than the case's (not cached)."""
    g, y0, lengths, pdfs, probs = case(name)
    cls = class_map(form, y0.size(2))
    if y is not None:
        return _evaluate(g, y, lengths, pdfs.numpy(), probs.numpy(), cls, coef)
    key = (name, "identity" if form == "pdf" else form, coef)
    if key not in _refs:
        _refs[key] = _evaluate(g, y0, lengths, pdfs.numpy(), probs.numpy(), cls, coef)
    return _refs[key]


def per_sequence(name, form, coef):
    """[(bound_b, fp32 distance_b, scale_b)] of the sequences of a case, each evaluated alone: the rule of `reference` with
    max |grad| of the sequence itself."""
    key = (name, "identity" if form == "pdf" else form, coef)
    if key not in _seqs:
        g, y, lengths, pdfs, probs = case(name)
        cls = class_map(form, y.size(2))
        out = []
        for b, L in enumerate(lengths.tolist()):
            _, bd, scale = _evaluate(g, y[b:b + 1, :L], [L], pdfs.numpy()[b:b + 1, :L], probs.numpy()[b:b + 1, :L], cls, coef)
            out.append((bd[0], bd[1], scale))
        _seqs[key] = out
    return _seqs[key]


def distances(E, grad, ref):
    """(value, gradient, row sums) of a result against ref = (E, grad, .): per sequence, each relative to the sequence's own
    max |grad| (the value: relative to E_b), and over the batch as smbr_reference measures them."""
    E, grad = np.asarray(E, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    scale = float(np.abs(ref[1]).max())
    whole = (sr.value_dist(E, ref[0]), cr.grad_dist(grad, ref[1], scale), float(np.abs(grad.sum(-1)).max() / scale))
    seqs = []
    for b in range(E.shape[0]):
        sb = float(np.abs(ref[1][b]).max())
        seqs.append((sr.value_dist(E[b:b + 1], ref[0][b:b + 1]), cr.grad_dist(grad[b], ref[1][b], sb), float(np.abs(grad[b].sum(-1)).max() / sb)))
    return whole, seqs
