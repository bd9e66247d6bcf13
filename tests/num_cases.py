"""The cases tests/test_num_reference.py (host twin) and tests/test_gpu_align_forms.py / test_gpu_num_forms.py (device) run against
tests/num_reference.py: every launch form of align_kernel / num_fb_kernel by row width, dense length sweeps through the block
backtrace, the largest graph of the tile kernels, exact ties, and arbitrary time windows.  Every builder is deterministic and
returns CPU tensors: (x, lengths, graphs[, windows])."""
import numpy as np
import torch

from helpers import _rand_num_fst
from pychain_amd import ChainGraph, ChainGraphBatch, _lib, alignment_windows, viterbi_align, synthetic as syn
from pychain_amd.simplefst import StdVectorFst

BIG = 2 ** 31 - 1


def on_tile_path(H, K, D):
    """True where the shape runs on the tile kernels (not num_needs_general), read off the alignment workspace: uint16
    backpointers (2 B T H bytes) there, int32 ones (4 B T H) on the general kernel."""
    T = 1024
    return int(_lib.lib().pychain_hip_align_workspace_bytes(1, T, int(H), int(K), int(D))) < 4 * T * int(H)


def _bisect(pred, lo, hi):
    """(last value with pred, first without) between lo (pred holds) and hi (it does not)."""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


# ---- a. the form matrix: three small branching graphs, one of them with an odd number of states, ragged lengths -----------------
FORM_SIZES = (23, 40, 7)
FORM_LENGTHS = (41, 50, 9)
FORM_T = 50
FORM_D = (4, 48, 2048, 2052, 4096, 4100, 8408, 16384, 16388, 1001, 4095, 4097)
# the form of align_kernel / num_fb_kernel <VEC, XCH, LD> launch_align / launch_num_fb take for a row of D pdfs on the tile path
def form_of(D):
    if D % 4 == 0:
        return "<4,4,LD>" if D <= 2048 else "<4,8,LD>" if D <= 4096 else "<4,8>" if D <= 16384 else "<1,0>"
    return "<1,8>" if D <= 4096 else "<1,0>"


def form_graphs(D):
    """The three graphs over D pdfs; every one has an arc 0 -> 1 that emits the last column, D - 1."""
    rs = np.random.RandomState(D)
    fin = lambda H: {H - 1: 0.0, H - 2: -0.4}
    gs = []
    for h in FORM_SIZES:
        fst = _rand_num_fst(rs, h, h, D, fin)
        fst.add_arc(0, D, D, 1.1, 1)                               # (label = pdf + 1, weight = -log-prob)
        gs.append(ChainGraph(fst, log_domain=True))
    return ChainGraphBatch(gs, max_num_transitions=max(g.num_transitions for g in gs), max_num_states=max(g.num_states for g in gs))


def form_boundary_D():
    """(the widest row the form-matrix shape still runs on the tile kernels with, the first it does not)."""
    gb = form_graphs(4)
    H, K = gb.num_states, int(gb.backward_transitions.shape[-2])
    return _bisect(lambda D: on_tile_path(H, K, D), 16388, 65536)


def form_case(D, nan=False):
    """Network outputs of six times make_input's spread: some emitted values lie beyond +-30 (emitted_beyond_clamp).  `nan`:
    a NaN in column D - 1 of frame 20 of sequence 1."""
    graphs = form_graphs(D)
    x = syn.make_input(len(FORM_SIZES), FORM_T, D, seed=D % 1000 + 7) * 6.0
    if nan:
        x[1, 20, D - 1] = float("nan")
    return x, torch.tensor(FORM_LENGTHS), graphs


def emitted_beyond_clamp(x, lengths, graphs):
    """(values above 30, values below -30) among the x(t, pdf_k) the graphs' arcs read at t < L."""
    from num_reference import _graph_rows
    up = down = 0
    xn = x.float().numpy()
    for b in range(xn.shape[0]):
        r = _graph_rows(graphs, b)
        ks = np.concatenate([np.arange(lo, hi) for lo, hi in r["bi"] if hi > lo])
        v = xn[b, :int(lengths[b])][:, np.unique(r["bt"][ks, 2])]
        up += int((v > 30).sum())
        down += int((v < -30).sum())
    return up, down


# ---- b. backtrace sweeps: one shared graph with EVERY state final, lengths 1..B ----------------------------------------------------
SWEEPS = ((150, 250, 48), (701, 64, 48), (1500, 64, 48), (4000, 64, 48), (701, 64, 4100), (701, 64, 1001))    # (H, B = T, D)


def all_final_graph(H, D, seed=17):
    """_rand_num_fst(rs, H, H // 10, D) with small distinct final weights on every state: a path of any length exists."""
    rs = np.random.RandomState(seed + H)
    fin = lambda n: {h: -float(h + 1) / (4 * n) for h in range(n)}
    return ChainGraph(_rand_num_fst(rs, H, H // 10, D, fin), log_domain=True)


def sweep_case(H, B, D):
    g = all_final_graph(H, D)
    return syn.make_input(B, B, D, seed=H % 100 + 3), torch.arange(1, B + 1), ChainGraphBatch(g, B)


def single_frame_case():
    g = all_final_graph(150, 48)
    return syn.make_input(1, 1, 48, seed=5), torch.tensor([1]), ChainGraphBatch(g, 1)


# ---- c. the largest graph of the tile kernels ----------------------------------------------------------------------------------------
def tile_family_K(H):
    return 2 * H - 1 + H // 10                                      # arcs of _rand_num_fst(rs, H, H // 10, ...)


def tile_boundary_H(D=48):
    """(the last H of the all_final_graph family on the tile kernels, the first on the general ones)."""
    return _bisect(lambda H: on_tile_path(H, tile_family_K(H), D), 4000, 6000)


def largest_tile_case(H, D=48):
    g = all_final_graph(H, D)
    assert g.num_transitions == tile_family_K(H)
    return syn.make_input(4, 40, D, seed=23), torch.tensor([40, 33, 7, 1]), ChainGraphBatch(g, 4)


# ---- d. ties ---------------------------------------------------------------------------------------------------------------------------
TIE_STARTS = (1, 200, 600, 1100)
TIE_CHAIN = 10


def ties_case():
    """State 0 fans out into four identical 10-state chains that start at states 1, 200, 600 and 1100; every transition is two
    parallel arcs of one weight and two pdfs, the four last states are final with one weight; x in multiples of 0.25 with the
    columns of each pair equal: every sum is exact, every frame ties between the two arcs, the end between the four chains."""
    H, D = 1300, 48
    arcs = []
    for c in TIE_STARTS:
        arcs += [(0, c, 0, -0.5), (0, c, 1, -0.5)]
    for c in TIE_STARTS:
        for j in range(TIE_CHAIN):
            s = c + j
            arcs += [(s, s, 2 + 4 * j, -0.75), (s, s, 3 + 4 * j, -0.75)]
            if j + 1 < TIE_CHAIN:
                arcs += [(s, s + 1, 4 + 4 * j, -0.25), (s, s + 1, 5 + 4 * j, -0.25)]
    arcs.sort(key=lambda a: a[0])
    g = ChainGraph(StdVectorFst.from_arcs(H, 0, arcs, {c + TIE_CHAIN - 1: -0.5 for c in TIE_STARTS}), log_domain=True)
    x = torch.round(syn.make_input(3, 40, D, seed=31) * 4.0) / 4.0
    x[..., 1::2] = x[..., 0::2]
    return x, torch.tensor([40, 10, 23]), ChainGraphBatch(g, 3)


# ---- e. arbitrary time windows --------------------------------------------------------------------------------------------------------
def perturbed_windows(x, lengths, graphs, seed, infeasible):
    """int32 [B, H, 2]: the windows of the host twin's alignment at tolerance 2, then per state one of: left alone, shrunk by a
    frame, shifted by a frame, emptied (hi < lo), lo = -1, hi = 2^31 - 1.  Shrinking and shifting stay within the tolerance
    and only states the alignment never visits are emptied, so every sequence keeps its aligned path - but `infeasible`, whose
    visited states (the start state among them) are emptied too."""
    ali = viterbi_align(x, lengths, graphs)
    assert bool(ali.ok.all())
    H = graphs.num_states
    w = alignment_windows(ali, H, 2).numpy().astype(np.int64)
    B = w.shape[0]
    rs = np.random.RandomState(seed)
    L = np.asarray(lengths).astype(np.int64)[:, None]
    lo, hi = w[..., 0].copy(), w[..., 1].copy()
    visited = hi >= lo
    op = rs.randint(0, 6, size=(B, H))
    side = rs.randint(0, 2, size=(B, H)).astype(bool)
    can_lo, can_hi = visited & (lo > 0), visited & (hi < L)          # (the tolerance was not cut off at 0 / at L on that side)
    shrink = op == 1
    lo += (shrink & can_lo).astype(np.int64)
    hi -= (shrink & can_hi).astype(np.int64)
    right = (op == 2) & side & can_lo
    lo += right.astype(np.int64); hi += right.astype(np.int64)
    left = (op == 2) & ~side & can_hi
    lo -= left.astype(np.int64); hi -= left.astype(np.int64)
    empty = (op == 3) & ~visited
    empty[infeasible] |= visited[infeasible] & ((op[infeasible] == 3) | (np.arange(H) == 0))
    elo = rs.randint(0, int(L.max()) + 1, size=(B, H))
    lo = np.where(empty, elo, lo)
    hi = np.where(empty, elo - 1 - rs.randint(0, 3, size=(B, H)), hi)
    lo = np.where((op == 4) & ~empty, -1, lo)
    hi = np.where((op == 5) & ~empty, BIG, hi)
    return torch.from_numpy(np.stack([lo, hi], axis=-1).astype(np.int32))


def full_windows(B, H, lo=-1, hi=BIG):
    w = torch.empty(B, H, 2, dtype=torch.int32)
    w[..., 0], w[..., 1] = lo, hi
    return w


def form_windows_case(D):
    """The form-matrix batch with perturbed windows; sequence 1 (neither first nor last) is infeasible."""
    x, lengths, graphs = form_case(D)
    return x, lengths, graphs, perturbed_windows(x, lengths, graphs, seed=D + 1, infeasible=1)


def shared701_case(windows=True):
    """Four sequences of up to 120 frames over one all-final graph of 701 states; sequence 2 is infeasible under the windows."""
    g = all_final_graph(701, 48)
    x, lengths, graphs = syn.make_input(4, 120, 48, seed=41), torch.tensor([120, 97, 110, 64]), ChainGraphBatch(g, 4)
    if not windows:
        return x, lengths, graphs
    return x, lengths, graphs, perturbed_windows(x, lengths, graphs, seed=701, infeasible=2)
