"""The shapes of the general arc-count kernels (include/pychain_hip.h: pychain_hip_den_arc_counts_general) for
tests/test_arc_counts_general.py and tests/test_gpu_arc_counts_general.py: graphs and trees beyond the LDS form of
pychain_hip_den_arc_counts, and one small shape with more count items than the persistent count launch has workgroups.  The
references are arc_counts_reference's - the fp64 recursions, the fp32 restatement, the tolerance rule -, which this file only
calls: made once per process and shared (do not edit in place).

  pdfs_beyond    D = 20379 is the last the LDS form takes at H = 37; arcs carry pdfs far beyond the 4096 elements of a row a
                 recursion thread holds in registers                                                                     rows
  wide_tree      the benchmark graph's size on a tree of 17 500 pdfs                                                     rows
  states_beyond  more states than the rows form holds at any D; a recursion thread owns 20 or 21 states                  global
  both_beyond                                                                                                            global
  many_items     180 x ceil(130 / 64) = 540 count items > the 512 workgroups of the persistent count launch, so some workgroups
                 take a second item: a stale first-frame flag or a wrong partial row shows here; lengths 130, 129, 65, 64, 1, ...
                 put a short last run, a run of one frame and whole runs of padding among them                           lds
"""
import numpy as np
import torch

from arc_counts_reference import BAR, F32_SLACK, autograd, batch, counts, distances   # noqa: F401  (one copy of the rule)

AUTO, LDS, ROWS, GLOBAL = 0, 1, 2, 3
_MIXED = [130, 129, 65, 64, 1, 128, 100, 63, 2, 37]
SHAPES = {
    "pdfs_beyond": dict(H=37, K=150, D=20380, B=2, T=3, lengths=[3, 1], form=ROWS),
    "wide_tree": dict(H=3000, K=30000, D=17500, B=2, T=6, lengths=[6, 4], form=ROWS),
    "states_beyond": dict(H=20500, K=60000, D=130, B=2, T=5, lengths=[5, 2], form=GLOBAL),
    "both_beyond": dict(H=20500, K=60000, D=8408, B=1, T=3, lengths=[3], form=GLOBAL),
    "many_items": dict(H=37, K=150, D=23, B=180, T=130, lengths=_MIXED * 18, form=LDS),
}
BEYOND = ("pdfs_beyond", "wide_tree", "states_beyond", "both_beyond")
COUNT_WGS = 512                                    # csrc/arc_counts.hip: kArcCountMaxWgs
_made, _refs = {}, {}


def case(name):
    """(graph, y float32 [B,T,D], lengths) of a shape."""
    if name not in _made:
        from pychain_amd import synthetic as syn
        c = SHAPES[name]
        _made[name] = (syn.make_den_graph(c["H"], c["K"], c["D"], seed=3), syn.make_input(c["B"], c["T"], c["D"], seed=5, scale=2.0),
                       torch.tensor(c["lengths"]))
    return _made[name]


def weights(name, kind):
    """The arc log-weights of a shape: None, or 0.5 N(0,1) from a fixed seed, float32 [K]."""
    if kind is None:
        return None
    return torch.from_numpy((0.5 * np.random.RandomState(4321 + len(name)).randn(SHAPES[name]["K"])).astype(np.float32))


def reference(name, coef, wkind):
    """((log Z [B], counts_per_seq [B,K], gamma [B,T,D]) by the fp64 recursions, (bound, the fp32 restatement's distance)): the
    rule of arc_counts_reference.reference - BAR, or twice the fp32 distance where that is beyond F32_SLACK."""
    key = (name, coef, wkind)
    if key not in _refs:
        g, y, lengths = case(name)
        w = weights(name, wkind)
        ref = batch(counts, g, y, lengths, w, coef)
        d = max(distances(batch(counts, g, y, lengths, w, coef, dtype=np.float32), ref))
        _refs[key] = (ref, ((2.0 * d if d > F32_SLACK else BAR), d))
    return _refs[key]
