"""Every denominator form on network outputs that look like a TRAINED model's (tests/peaky.py): one pdf per frame far above the
rest, a path through the graph held a few frames per arc, a jump nobody announced, values beyond the +-30 clamp on both sides.
Every other denominator test draws i.i.d. Gaussians, where every state keeps a comparable share of the mass; here a state
vector spans the whole range the probability-domain fp32 recursions have (chain-computation.cc:113-207, 247-342).

Each form at its smallest shape, selected the way the suite already selects it and checked by the kernel name the library
reports; B = 3 with lengths (T, 2, 1).  Objective and gradient against the float64 oracle under the oracle's own
fp32-to-fp64 distance on the same input + 1e-5, at most 1e-4 (README: fixture G6's rule) - computed here, on the CPU; the 5 %
invariant must not fire (`bad` == 0; the oracle's `ok` is the witness that the input is healthy); exact zeros in the padding.
Forms the suite holds bit-identical on Gaussian input stay bit-identical here (the streamed schedule - the default - against the
gated and the single one there, at T = 130)."""
import numpy as np
import pytest
import torch

import peaky as pk
from helpers import rel_err, record_parity
from pychain_amd import ChainFunction, ChainGraph, ChainGraphBatch, ChainLoss, _lib, _plan, native, synthetic as syn
from pychain_amd.simplefst import StdVectorFst

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
KINDS = ("path", "surprise", "clamp")
LAZY, DMA = "den_recursion_lazy_kernel", "den_recursion_lazy_kernel<dma>"
NARROW = ("rnd", 1100, 8000, 4096)
DENSE = ("rnd", 1100, 18000, 4096)        # 32 slot-rows per wave: what two sequences per workgroup and one-word states need
STRUCT = ("sg", 600, 6, 3456)

FORMS = [
    # id, graph, T, options, recursion kernel, occupancy kernel (None: not pinned)
    ("small-C1", ("rnd", 20, 60, 40), 97, {}, LAZY + "<small>", None),
    ("small-C2", ("rnd", 200, 2000, 1000), 97, {}, LAZY + "<small>", None),
    ("dma-LzDma", ("rnd", 300, 3000, 4100), 97, {}, DMA, "den_gamma_kernel"),
    ("dma-LzNarrowDma", NARROW, 97, {}, DMA, "den_gamma2_kernel"),      # (the default call: den_gamma2_kernel, streamed occupancies)
    ("rows-through-registers", NARROW, 97, {"den_dma": 0}, LAZY, None),
    ("two-barrier", NARROW, 97, {"den_lazy": 0, "den_dma": 0}, "den_recursion_kernel", None),
    ("pair", DENSE, 97, {"den_pair": 1}, "den_recursion_pair_kernel", None),
    ("one-gather", STRUCT, 97, {}, LAZY + "<dma; one gather per arc>", None),
    ("crossing", STRUCT, 130, {"den_cross": 1}, LAZY + "<dma; one gather per arc; crossing>", None),   # (two halves from 104 frames on)
    ("one-word-states", DENSE, 97, {"den_q": 1, "den_tseg": 0}, LAZY + "<dma; one-word states>", None),
    ("general-plan", ("general", 200, 2000, 1000), 97, {}, "den_general_recursion_kernel", None),
    ("gamma16", NARROW, 97, {"gamma16": 1}, DMA, "den_gamma_kernel"),
    ("D-not-a-multiple-of-4", ("rnd", 300, 3000, 4098), 97, {}, DMA, "den_gamma_kernel"),
    ("gated", NARROW, 130, {"den_segments": 3}, DMA, None),
    ("single", NARROW, 130, {"den_segments": 1}, DMA, None),
]
_cache = {}


def _graph(spec, monkeypatch=None):
    kind = spec[0]
    if kind == "general":
        # (a forced general plan: the knob is read when the plan is compiled, and plans are cached on the graph object)
        monkeypatch.setenv("PYCHAIN_PLAN_GENERAL", "1")
        return syn.make_den_graph(*spec[1:]), spec[3]
    if spec not in _cache:
        _cache[spec] = syn.make_structured_den_graph(*spec[1:]) if kind == "sg" else syn.make_den_graph(*spec[1:])
    return _cache[spec], spec[3]


def _input(spec, T, kind):
    """(x [B, T, D] float32 on the host, lengths, the walks): built once per (graph, T, kind)."""
    key = ("x", spec[1:], T, kind)
    if key not in _cache:
        g = syn.make_structured_den_graph(*spec[1:]) if spec[0] == "sg" else syn.make_den_graph(*spec[1:])
        G, D = pk.graph_arrays(g), spec[3]
        xs, walks = [], []
        for b in range(B):
            if kind == "clamp":
                x, w = pk.clamp_input(G, T, D, seed=40 + b)
            else:
                x, w = pk.path_input(G, T, D, seed=40 + b, peak=10.0, hold=4)
            if kind == "surprise" and b == 0:
                pk.splice_surprise(G, x, 1e-5, T // 2, 0, seed=9)
            xs.append(x); walks.append(w)
        _cache[key] = (torch.from_numpy(np.stack(xs)), torch.tensor([T, 2, 1]), walks)
    return _cache[key]


def _oracle(spec, T, kind, den):
    key = ("o", spec[1:], T, kind)
    if key not in _cache:
        x, L, _ = _input(spec, T, kind)
        _cache[key] = pk.oracle_bars("den", x, L, ChainGraphBatch(den, B))
    return _cache[key]


def _call(den, x, L, **opts):
    xx = x.clone().requires_grad_(True)
    ctx = [_lib.option(k, v) for k, v in opts.items()]
    for c in ctx:
        c.__enter__()
    try:
        plan = _plan.graph_plan(den, x.size(2), torch.device(DEV))
        names = _lib.den_kernel_names(plan.slot_rows, plan.num_states, x.size(2), x.size(0))
        o = ChainFunction.apply(xx, L, ChainGraphBatch(den, x.size(0)), 1e-5)
        o.backward()
        torch.cuda.synchronize()
    finally:
        for c in reversed(ctx):
            c.__exit__()
    return float(o.detach()), xx.grad, int(ChainFunction.last_bad_count.sum()), names


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_every_denominator_form_on_peaked_outputs(form, kind, monkeypatch):
    fid, spec, T, opts, rec, occ = form
    den, D = _graph(spec, monkeypatch)
    x_cpu, L, _ = _input(spec, T, kind)
    ro, rg, bar_o, bar_g, own, ok = _oracle(spec, T, kind, den)
    assert ok                                                              # a healthy input: the reference's own `ok`
    o, g, bad, names = _call(den, x_cpu.to(DEV), L, **opts)
    eo, eg = abs(o - ro) / abs(ro), rel_err(g.cpu().numpy(), rg)
    print("peaky", fid, kind, names, "objf %.3g (bar %.3g) grad %.3g (bar %.3g); the oracle's fp32 from its fp64: %.3g / %.3g"
          % (eo, bar_o, eg, bar_g, own[0], own[1]))
    record_parity("peaky_%s_%s" % (fid, kind), objf=eo, grad_vs_f64=eg, bar_objf=bar_o, bar_grad=bar_g)
    assert names[0] == rec and (occ is None or names[1] == occ), names
    assert bad == 0
    assert eo <= bar_o and eg <= bar_g
    assert bool((g[1, 2:] == 0).all()) and bool((g[2, 1:] == 0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_forms_that_are_bit_identical_stay_so_on_peaked_outputs(kind):
    """Two sequences per workgroup against the two-barrier kernel it restates; the occupancy schedules among themselves; rows
    exp'd ahead of the recursions against rows they exp themselves; rows by LDS-direct loads against rows through registers.  And
    the two occupancy kernels against each other (another summation order: equal to rounding, 1e-5 like every pair of forms)."""
    den, D = _graph(NARROW)
    x_cpu, L, _ = _input(NARROW, 130, kind)
    x = x_cpu.to(DEV)
    o, g, bad, _ = _call(den, x, L)
    for opts in ({"den_segments": 3}, {"den_segments": 1}, {"den_dma": 0}):
        o2, g2, bad2, _ = _call(den, x, L, **opts)
        assert bad == 0 and bad2 == 0 and o2 == o and torch.equal(g2, g), opts
    dense, _ = _graph(DENSE)
    xd = _input(DENSE, 130, kind)[0].to(DEV)
    o1, g1, _, n1 = _call(dense, xd, L, den_lazy=0, den_pair=0)
    o2, g2, _, n2 = _call(dense, xd, L, den_lazy=0, den_pair=1)
    assert n1[0] == "den_recursion_kernel" and n2[0] == "den_recursion_pair_kernel" and o1 == o2 and torch.equal(g1, g2)
    o1, g1, _, _ = _call(den, x, L, den_dma=2)
    o2, g2, _, _ = _call(den, x, L, den_dma=3)
    assert o1 == o2 and torch.equal(g1, g2)
    plan = _plan.graph_plan(den, D, torch.device(DEV))
    ahead = {}
    for v in (2, 3):                                                       # ... and the two calls were the two forms
        with _lib.option("den_dma", v):
            ahead[v] = _lib.lib().pychain_hip_den_uses_row_buffer(plan.stride, plan.slot_rows, plan.num_states, D, B, 130, 0)
    assert ahead == {2: 0, 3: 1}, ahead
    o2, g2, _, n2 = _call(den, x, L, gamma16=1)
    e = rel_err(g2.cpu().numpy(), g.cpu().numpy())
    print("peaky gamma16 against gamma2", kind, "%.3g" % e)
    assert n2[1] == "den_gamma_kernel" and o2 == o and e <= 1e-5


def _path_numerator(walk, L):
    """The left-to-right graph of the path the peaks follow: state i loops on the pdf of the walk's i-th arc and leaves on it."""
    segs = [(t, n, pdf) for (t, n, _, pdf) in walk if t < L]
    arcs = []
    for i, (t, n, pdf) in enumerate(segs):
        if min(n, L - t) > 1:
            arcs.append((i, i, pdf, -0.7))
        arcs.append((i, i + 1, pdf, -0.7))
    return ChainGraph(StdVectorFst.from_arcs(len(segs) + 1, 0, arcs, {len(segs): 0.0}), log_domain=True)


@pytest.mark.parametrize("kind", ("path", "clamp"))
def test_fused_loss_of_a_converged_model(kind):
    """What a converged model sees: the numerator graph of every utterance IS the path its output peaks on, so denominator and
    numerator occupancies nearly cancel and the gradient is what is left.  Fused ChainLoss against the float64 oracle (the same
    rule for the bar; rel_err divides by max |grad|, which is small here - the distances are printed and recorded); bf16 rows are
    the up-cast rows bit for bit."""
    spec, T = ("rnd", 200, 2000, 1000), 97
    den, D = _graph(spec)
    x_cpu, _, walks = _input(spec, T, kind)
    L = torch.tensor([T, 60, 2])
    gs = [_path_numerator(walks[b], int(L[b])) for b in range(B)]
    num = ChainGraphBatch(gs, max_num_transitions=max(g.num_transitions for g in gs), max_num_states=max(g.num_states for g in gs))

    def step(x):
        xx = x.clone().requires_grad_(True)
        loss = ChainLoss(den, 1e-5, avg=True)(xx, L, num)
        loss.backward()
        torch.cuda.synchronize()
        assert int(loss.bad_count.sum()) == 0
        return float(loss.detach()), xx.grad
    rl, rg, bar_l, bar_g, own, _ = pk.oracle_bars("loss", x_cpu, L, den, num)
    l, g = step(x_cpu.to(DEV))
    el, eg = abs(l - rl) / abs(rl), rel_err(g.cpu().numpy(), rg)
    print("peaky fused", kind, "loss %.6g (f64 %.6g): %.3g (bar %.3g); grad %.3g (bar %.3g) with max |grad| %.3g; the oracle's fp32 from its "
          "fp64: %.3g / %.3g" % (l, rl, el, bar_l, eg, bar_g, np.abs(rg).max(), own[0], own[1]))
    record_parity("peaky_fused_%s" % kind, loss=el, grad_vs_f64=eg, bar_loss=bar_l, bar_grad=bar_g, max_grad=np.abs(rg).max())
    assert el <= bar_l and eg <= bar_g
    assert bool((g[1, 60:] == 0).all()) and bool((g[2, 2:] == 0).all())
    xh = x_cpu.to(DEV).to(torch.bfloat16)
    outs = []
    for flag in (True, False):                                             # 2-byte rows in the kernels / up-cast by the caller
        native.HALF_ROWS = flag
        try:
            outs.append(step(xh))
        finally:
            native.HALF_ROWS = True
    (l1, h1), (l0, h0) = outs
    assert h1.dtype == torch.bfloat16 and l1 == l0 and torch.equal(h1, h0)
