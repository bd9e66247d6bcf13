"""The leaky-HMM term of the denominator at coefficients where a fault in it shows (tests/test_leaky.py on the CPU,
tests/test_gpu_leaky.py on the device).

Every other denominator test runs at coefficient 1e-5, where all a kernel does per state with the leaky term is of order 1e-5 of
the result - below the bounds.  What the kernels do themselves in that term: states on several lanes (csrc/plan.cpp: the first
part carries leaky(i) and initial(i), only the first part takes beta's constant, the others are marked in the sign bit of
beta's leaky probability), the one-gather form (its occupancy pass reads a(t+1,.) WITHOUT the leaky term), one-word states
(alpha gathers a / (coef leaky)), cl0 = coef leaky in registers in the two-barrier kernel, the pair and the general kernels'
own arithmetic.  This file holds: the graphs in two variants, the table of kernel forms with the name each must report, and the
planted faults - wrappers around plan_emulator.parse / tile_rows that never touch the emulator's own path."""
import contextlib

import numpy as np
import torch

import plan_emulator as emu
from pychain_amd import synthetic as syn
from pychain_amd.graph import ChainGraph

COEF = 0.1                                  # the coefficient of every case; the default forms also run at COEFS_MORE
COEFS_MORE = (1e-2, 0.5)
VARIANTS = ("leaky_ones", "fst_final")

# ---- graphs ---------------------------------------------------------------------------------------------------------
# name -> (builder of the ("leaky", "ones") graph, pdfs)
def _hubs(**kw):
    from test_plan import _hub_graph
    return _hub_graph(**kw)[0]


BASE = {
    "c3": (lambda: syn.make_den_graph(3000, 30000, 3456, seed=0), 3456),          # the benchmark graph
    "c2": (lambda: syn.make_den_graph(200, 2000, 1000), 1000),                    # four-wave workgroups
    "g4100": (lambda: syn.make_den_graph(300, 3000, 4100), 4100),                 # rows beyond 4096 pdfs: den_gamma_kernel
    "small_hubs": (lambda: _hubs(seed=6, H=200, D=300, extra=1500, hubs=3, fan=45), 300),
    "hubs": (lambda: _hubs(), 600),
    "structured": (lambda: syn.make_structured_den_graph(), 3456),                # pdf by state: one gather per arc
    "structured_small": (lambda: syn.make_structured_den_graph(90, 5, 1000), 1000),
}
_FINAL_SEED = 4242


def make_graph(name, variant):
    """A NEW graph object (nothing cached on it).  "leaky_ones": as the suite builds its denominators; "fst_final": a one-hot
    start (initial_mode="fst") and non-uniform final probabilities, uniform(seed, H) with every third state at 0 - built
    through ChainGraph.from_tensors, so every plan compiled from it sees them."""
    return as_variant(BASE[name][0](), variant)


def as_variant(g, variant):
    """`g` itself for "leaky_ones"; for "fst_final" a new graph over copies of its arcs (`g` may have a cached plan: not edited)."""
    if variant == "leaky_ones":
        return g
    assert variant == "fst_final"
    H = g.num_states
    final = syn.uniform(_FINAL_SEED, H)
    final[::3] = 0.0
    init = torch.zeros(H, dtype=g.initial_probs.dtype)
    init[g.start_state] = 1.0
    return ChainGraph.from_tensors(
        g.forward_transitions.clone(), g.forward_transition_probs.clone(), g.forward_transition_indices.clone(),
        g.backward_transitions.clone(), g.backward_transition_probs.clone(), g.backward_transition_indices.clone(),
        torch.from_numpy(final).to(g.final_probs.dtype), init, g.leaky_probs.clone(), start_state=g.start_state, log_domain=False)


def num_pdfs(name):
    return BASE[name][1]


# ---- kernel forms -----------------------------------------------------------------------------------------------------
LAZY_DMA = "den_recursion_lazy_kernel<dma>"
LAZY_SMALL = "den_recursion_lazy_kernel<small>"
LAZY_REGS = "den_recursion_lazy_kernel"
LAZY_SG = "den_recursion_lazy_kernel<dma; one gather per arc>"
LAZY_XF = "den_recursion_lazy_kernel<dma; one gather per arc; crossing>"
LAZY_Q = "den_recursion_lazy_kernel<dma; one-word states>"
TWO_BARRIER = "den_recursion_kernel"
PAIR = "den_recursion_pair_kernel"
GENERAL = "den_general_recursion_kernel"

# shapes: B = 5 (odd: the pair kernel gets a lone sequence)
LENGTHS = [61, 54, 40, 2, 1]
LENGTHS_TSEG = [420, 413, 280, 3, 1]         # two segments of 210 frames that start 96 frames outside themselves
TSEG = {"den_tseg": 2, "den_tburn": 96}


class Form(object):
    """One kernel form on one graph: the options that select it, the recursion (and occupancy) kernel name the query must
    report under those options, whether the call is cut into time segments, and whether the plan is a general one."""

    def __init__(self, graph, key, opts, rec, occ=None, tseg=False, general=False, coefs=(COEF,), lengths=None, rows_ahead=False):
        self.graph, self.key, self.opts, self.rec, self.occ = graph, key, dict(opts), rec, occ
        self.tseg, self.general, self.coefs, self.rows_ahead = tseg, general, coefs, rows_ahead
        self.lengths = list(lengths or (LENGTHS_TSEG if tseg else LENGTHS))

    @property
    def id(self):
        return "%s-%s" % (self.graph, self.key)

    def input(self, device="cpu"):
        """(x [5, T, D], lengths) of the form's calls - one input per (graph, lengths), whatever the form and the variant."""
        x = syn.make_input(len(self.lengths), max(self.lengths), num_pdfs(self.graph), seed=71 + sorted(BASE).index(self.graph), device=device)
        return x, torch.tensor(self.lengths)


_ALL = (COEF,) + COEFS_MORE
# (plans with beta positions that take no constant - small_hubs, hubs - are not for the pair kernel, whose normalise pass gives
# every position c(t): csrc/den_lazy.hip: pair_shape_ok.  Option den_pair = 1 then selects the one-sequence kernels, and that is
# the name pinned here; the pair kernel itself runs on the C3 graph.)
FORMS = [
    Form("c3", "default", {"den_tseg": 0}, LAZY_DMA, "den_gamma2_kernel", coefs=_ALL),
    Form("c3", "rows_through_registers", {"den_dma": 0, "den_tseg": 0}, LAZY_REGS),
    # (rows are exp'd ahead of the recursions from 64 frames on - den_policy.hip: den_would_exp_rows_ahead - so this form's longest
    # sequence has 77 frames, not 61; the test asks the library whether the call uses the row buffer)
    Form("c3", "rows_expd_ahead", {"den_dma": 3, "den_tseg": 0}, LAZY_DMA, lengths=[77, 54, 40, 2, 1], rows_ahead=True),
    Form("c3", "two_barrier", {"den_lazy": 0}, TWO_BARRIER),
    Form("c3", "pair", {"den_pair": 1}, PAIR),
    Form("c3", "pair_lazy0", {"den_pair": 1, "den_lazy": 0}, PAIR),
    Form("c3", "one_word_states", {"den_q": 1, "den_tseg": 0}, LAZY_Q),
    Form("c3", "time_segments", TSEG, LAZY_DMA, tseg=True),
    Form("c2", "small", {}, LAZY_SMALL),
    Form("c2", "general", {}, GENERAL, general=True),
    Form("g4100", "gamma_kernel", {"den_tseg": 0}, LAZY_DMA, "den_gamma_kernel"),
    Form("g4100", "segments1", {"den_segments": 1, "den_tseg": 0}, LAZY_DMA, "den_gamma_kernel"),
    Form("g4100", "segments3", {"den_segments": 3, "den_tseg": 0}, LAZY_DMA, "den_gamma_kernel"),
    Form("small_hubs", "default", {}, LAZY_SMALL),
    Form("small_hubs", "rows_through_registers", {"den_dma": 0}, LAZY_REGS),
    Form("small_hubs", "two_barrier", {"den_lazy": 0}, TWO_BARRIER),
    Form("small_hubs", "pair", {"den_pair": 1}, LAZY_SMALL),
    Form("small_hubs", "pair_lazy0", {"den_pair": 1, "den_lazy": 0}, TWO_BARRIER),
    Form("hubs", "default", {"den_tseg": 0}, LAZY_DMA, coefs=_ALL),
    Form("hubs", "rows_through_registers", {"den_dma": 0, "den_tseg": 0}, LAZY_REGS),
    Form("hubs", "two_barrier", {"den_lazy": 0}, TWO_BARRIER),
    Form("hubs", "pair", {"den_pair": 1, "den_tseg": 0}, LAZY_DMA),
    Form("hubs", "pair_lazy0", {"den_pair": 1, "den_lazy": 0}, TWO_BARRIER),
    Form("hubs", "time_segments", TSEG, LAZY_DMA, tseg=True),
    Form("structured", "one_gather", {"den_tseg": 0}, LAZY_SG),
    Form("structured", "sg0", {"den_sg": 0, "den_tseg": 0}, LAZY_DMA),
    # (the crossing takes sequences of at least 4 x 24 + 8 frames - den_lazy.hip: xf_shape_ok - and the name query answers for long
    # ones: the uncut crossing runs on the lengths of the time-segment cases)
    Form("structured", "crossing", {"den_cross": 1, "den_tseg": 0}, LAZY_XF, lengths=LENGTHS_TSEG),
    Form("structured", "time_segments", TSEG, LAZY_SG, tseg=True),
]
SPLIT_GRAPHS = ("small_hubs", "hubs", "structured")       # plans with states on several lanes


# ---- planted faults ---------------------------------------------------------------------------------------------------
def alpha_parts(hd):
    """[(first alpha position, [further alpha positions])] of the states a plan put on several alpha positions.  A pdf-by-state
    plan lists them (extra_a, b2a).  Otherwise: whoever gathers a state gathers every part of it, so the parts of a state are the
    positions gathered with the same multiset of (pdf, probability); the first is the one that carries the leaky probability."""
    if hd["pdf_by_state"]:
        groups = {}
        for pb, pa in hd["extra_a"]:
            groups.setdefault(int(hd["b2a"][pb]), []).append(int(pa))
        return sorted(groups.items())
    t = hd["alpha"]
    cols = {}
    for w in range(t["nwaves"]):
        first, ng, row, _ = t["waves"][w]
        for g in range(first, first + ng):
            base, ns = t["groups"][g]
            for j in range(ns):
                idx, p = t["idx"][row + j], t["p"][row + j]
                for lane in np.nonzero(p != 0)[0]:
                    cols.setdefault(int(idx[lane] & 0xffff), []).append((int(idx[lane] >> 16), float(p[lane])))
            row += ns
    by_sig = {}
    for pos, arcs in cols.items():
        by_sig.setdefault(tuple(sorted(arcs)), []).append(pos)
    out = []
    for members in by_sig.values():
        if len(members) > 1:
            firsts = [m for m in members if hd["leaky_a"][m] > 0]
            assert len(firsts) == 1, "a state's leaky probability sits on exactly one of its alpha positions"
            out.append((firsts[0], sorted(m for m in members if m != firsts[0])))
    return sorted(out)


def _fault_a(hd, coef):
    """every beta position of a state takes the constant c(t)"""
    hd["takes_c"][hd["no_const"]] = True


def _fault_b(hd, coef):
    """the no-constant flag (the sign bit of beta's leaky probability on the device) leaks into sum_i leaky_i beta_i"""
    hd["leaky_b"][hd["no_const"]] *= -1.0


def _fault_c(hd, coef):
    """every alpha part of a state carries its leaky probability"""
    for first, more in alpha_parts(hd):
        hd["leaky_a"][more] = hd["leaky_a"][first]


def _fault_d(hd, coef):
    """every alpha part of a state carries its initial probability"""
    for first, more in alpha_parts(hd):
        hd["init_a"][more] = hd["init_a"][first]


def _fault_e(hd, coef):
    """one-gather form: the occupancy pass reads the stored row WITH the leaky term (in planted(): tile_rows)"""


def _fault_f(hd, coef):
    """beta runs with coefficient 1e-5 whatever the call's (its only use of the coefficient is coef * leaky_b)"""
    hd["leaky_b"] *= np.float32(1e-5 / coef)


FAULTS = {"a": _fault_a, "b": _fault_b, "c": _fault_c, "d": _fault_d, "e": _fault_e, "f": _fault_f}


def fault_applies(fault, hd, sg):
    """(a), (b): the plan has beta positions without the constant; (c): states on several alpha positions; (d): one of them
    with an initial probability; (e): the one-gather form; (f): always."""
    if fault in "ab":
        return hd["split_b"] > 0
    if fault == "c":
        return len(alpha_parts(hd)) > 0
    if fault == "d":
        return any(hd["init_a"][first] > 0 for first, _ in alpha_parts(hd))
    return sg if fault == "e" else True


@contextlib.contextmanager
def planted(fault, coef):
    """plan_emulator.den_forward_backward with one fault planted, for the duration of the block: the parsed plan is edited on
    its way out of parse(); fault (e) turns the row the one-gather occupancy tile reads, a(t+1,.) before the leaky term (any
    scale), into the stored a'(t+1,.) = a / sum(a) + coef leaky."""
    real_parse, real_rows = emu.parse, emu.tile_rows
    seen = {}

    def parse(blob):
        hd = real_parse(blob)
        FAULTS[fault](hd, coef)
        seen["hd"] = hd
        return hd

    def tile_rows(t, U, V, nout, dtype):
        if fault == "e" and t is seen["hd"].get("gamma_sg"):
            U = U / U.sum() + coef * seen["hd"]["leaky_a"].astype(dtype)
        return real_rows(t, U, V, nout, dtype)
    emu.parse, emu.tile_rows = parse, tile_rows
    try:
        yield
    finally:
        emu.parse, emu.tile_rows = real_parse, real_rows


def emulate(blob, x, lengths, coef, sg=False, fault=None):
    if fault is None:
        return emu.den_forward_backward(blob, x, lengths, coef, sg=sg)
    with planted(fault, coef):
        return emu.den_forward_backward(blob, x, lengths, coef, sg=sg)
