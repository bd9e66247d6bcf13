"""The leaky-HMM term of the denominator, on the CPU: the inputs of tests/test_gpu_leaky.py are sensitive to the term (the
reference moves with the coefficient; faults planted in the emulator move its gradient by ten times the device bound), the
emulator itself - what the kernels compute from a compiled plan - stays the fp64 oracle's at coefficients 0.1 and 0.5 in both
graph variants, and so do the library's host twins.  tests/leaky_cases.py holds the cases and the planted faults.

Why the coefficient matters.  Gradient rel_err of the faulted emulator against the unfaulted one, fp64, measured with the
inputs below, ("leaky", "ones") graphs (every figure is recorded again by the tests):

  planted fault                                                 | coef 1e-5 | coef 0.1
  (a) every beta position takes the constant       small_hubs   |  8.1e-7   | 5.9e-3
                                                   hubs         |  1.2e-7   | 1.2e-3
  (b) the flag's sign in the leaky-weighted sum    small_hubs   |  4.3e-6   | 2.2e-2
                                                   hubs         |  2.7e-6   | 2.6e-2
  (c) every alpha part carries the leaky prob.     small_hubs   |  3.4e-7   | 3.2e-3
                                                   hubs         |  2.7e-7   | 8.4e-3
  (e) one-gather occupancy reads a' instead of a   structured   |  1.1e-5   | 8.9e-2
  (f) beta runs with 1e-5 whatever the call's      every graph  |  0        | 0.1 .. 0.17

At 1e-5 all of them sit under the 2e-5 of the device test of split plans: the suite could not see them.  Two limits of that
statement, both measured here: (e) grows with the peakiness of the network output - N(0,1) x 2 over 80 frames (the input of
test_structured_phone_lm_like_graph_vs_oracle) gives 1.8e-4 at 1e-5 - so the sensitivity case of the structured graph uses
N(0,1) x 1; and with a one-hot start on _hub_graph (whose start state leads down a chain of states with one arc each) beta's
constant decides the first frames even at 1e-5: (b) is 1.1e-2 there, so the blind spot is asserted on the ("leaky", "ones")
graphs, which is what the suite ran.
(d) - every alpha part carries the initial probability.  With a one-hot start it cannot move the gradient at all: the start row
is normalised, all of it sits on one state either way, and only the objective moves, by log(parts) (2.6e-2, 4.3e-2 of it, at
any coefficient).  With the leaky start the gradient moves: 3.7e-8 -> 3.0e-4 (small_hubs) and 6.3e-7 -> 6.0e-3 (hubs) from 1e-5
to 0.1 - what starts on those hubs reaches the gradient through beta's constant - and 8e-2 / 6e-2 on the structured graph,
whatever the coefficient.  Both are asserted."""
import numpy as np
import pytest
import torch

import leaky_cases as lc
import oracle as orc
from helpers import record_parity, rel_err
from pychain_amd import ChainFunction, ChainGraphBatch, _lib, synthetic as syn
from test_plan import _blob

# graph, frames, one-gather form, scale of the N(0,1) network output
SENSITIVITY = [("small_hubs", 14, False, 2.0), ("hubs", 9, False, 2.0), ("structured_small", 12, True, 1.0)]
_seen_faults = {}


def _objf_err(o, o0):
    return float(np.abs(np.asarray(o) - np.asarray(o0)).max() / np.abs(np.asarray(o0)).max())


@pytest.mark.parametrize("variant", lc.VARIANTS)
@pytest.mark.parametrize("name,T,sg,scale", SENSITIVITY, ids=[c[0] for c in SENSITIVITY])
def test_planted_faults_move_the_emulated_gradient(name, T, sg, scale, variant):
    """A condition on the inputs, not a measurement of the kernels: at coefficient 0.1 every planted fault that applies to the
    plan moves the emulator's gradient by at least 1e-4 - ten times the bound of the device tests - and at 1e-5, on the graphs
    the suite ran, (a), (b), (c) and (e) stay under 2e-5 (the module's docstring has the table and the two exceptions)."""
    g, D = lc.make_graph(name, variant), lc.num_pdfs(name)
    blob = _blob(g, D)
    import plan_emulator as emu
    hd = emu.parse(blob)
    x = syn.make_input(2, T, D, seed=21, scale=scale).numpy()
    L = np.array([T, T - 3])
    applies = [f for f in sorted(lc.FAULTS) if lc.fault_applies(f, hd, sg)]
    _seen_faults[(name, variant)] = applies
    assert "f" in applies and (("a" in applies and "b" in applies and "c" in applies and "d" in applies) if not sg else ("c" in applies and "e" in applies))
    for coef in (lc.COEF, 1e-5):
        o0, g0 = lc.emulate(blob, x, L, coef, sg=sg)
        for f in applies:
            o, gr = lc.emulate(blob, x, L, coef, sg=sg, fault=f)
            eg, eo = rel_err(gr, g0), _objf_err(o, o0)
            print("fault", f, name, variant, "coef", coef, "grad %.3g objf %.3g" % (eg, eo))
            record_parity("leaky_fault_%s_%s_%s_%g" % (f, name, variant, coef), grad=eg, objf=eo)
            if coef == lc.COEF:
                if f == "d" and variant == "fst_final":
                    assert eo >= 1e-4 and eg <= 1e-12, (f, eo, eg)           # a one-hot start: the objective alone, by log(parts)
                else:
                    assert eg >= 1e-4, (f, name, variant, eg)
            elif variant == "leaky_ones" and f in "abce":
                assert eg < 2e-5, (f, name, variant, eg)                       # the blind spot of a suite that runs at 1e-5
            if f in "abf":
                assert eo <= 1e-12                                             # beta's faults never move the objective


def test_every_planted_fault_was_applied_somewhere():
    """(a), (b): the two hub graphs; (c): every graph; (d): the hub graphs, whose start state is on several alpha positions, and
    the structured graph with the leaky start; (e): the one-gather form; (f): everywhere."""
    for name, T, sg, scale in SENSITIVITY:
        for variant in lc.VARIANTS:
            if (name, variant) not in _seen_faults:
                import plan_emulator as emu
                hd = emu.parse(_blob(lc.make_graph(name, variant), lc.num_pdfs(name)))
                _seen_faults[(name, variant)] = [f for f in sorted(lc.FAULTS) if lc.fault_applies(f, hd, sg)]
    assert set("".join("".join(v) for v in _seen_faults.values())) == set("abcdef")
    assert "d" in _seen_faults[("hubs", "fst_final")] and "d" in _seen_faults[("small_hubs", "fst_final")]


def test_alpha_parts_found_from_the_tiles_are_the_ones_the_plan_lists():
    """alpha_parts() of a plan without the crossing's tables goes by who gathers what (arcs with random probabilities: no two
    states are gathered alike).  It finds every further alpha position - the gathered positions without a leaky probability,
    every state of these graphs having one - once, and a pdf-by-state plan's own list has the same shape."""
    import plan_emulator as emu
    for name in ("small_hubs", "hubs", "structured_small"):
        hd = emu.parse(_blob(lc.make_graph(name, "leaky_ones"), lc.num_pdfs(name)))
        parts = lc.alpha_parts(hd)
        further = sorted(p for _, more in parts for p in more)
        gathered = set((hd["alpha"]["idx"][hd["alpha"]["p"] != 0] & 0xffff).tolist())
        assert len(parts) > 0 and set(further) <= gathered and len(set(further)) == len(further)
        if not hd["pdf_by_state"]:              # (two states of the structured graph have no leaky probability themselves)
            assert further == sorted(p for p in gathered if hd["leaky_a"][p] == 0), name
        for first, more in parts:
            assert hd["leaky_a"][first] > 0 and not hd["leaky_a"][more].any() and not hd["init_a"][more].any()


# ---- the reference moves with the coefficient -------------------------------------------------------------------------
_REF_CASES = sorted({(f.graph, tuple(f.lengths), c) for f in lc.FORMS for c in f.coefs})


@pytest.fixture(scope="module")
def oracle_at():
    cache = {}

    def get(graph, variant, lengths, coef):
        key = (graph, variant, lengths, coef)
        if key not in cache:
            g = cache.setdefault(("g", graph, variant), lc.make_graph(graph, variant))
            form = next(f for f in lc.FORMS if f.graph == graph and tuple(f.lengths) == lengths)
            x, L = cache.setdefault(("x", graph, lengths), form.input())
            cache[key] = orc.chain_function(x, L, ChainGraphBatch(g, len(lengths)), coef, flavour="f64")
        return cache[key]
    return get


@pytest.mark.parametrize("variant", lc.VARIANTS)
@pytest.mark.parametrize("graph,lengths,coef", _REF_CASES, ids=["%s-T%d-%g" % (g, max(l), c) for g, l, c in _REF_CASES])
def test_the_reference_moves_with_the_coefficient(oracle_at, graph, lengths, coef, variant):
    """Every (graph, lengths, coefficient) of the device table: the fp64 oracle's gradient at that coefficient is at least 1e-2
    from its gradient at 1e-5 - a kernel that ignored the call's coefficient could not pass a 1e-5 bound."""
    o, g = oracle_at(graph, variant, lengths, coef)
    o5, g5 = oracle_at(graph, variant, lengths, 1e-5)
    e = rel_err(g, g5)
    record_parity("leaky_reference_%s_%s_T%d_%g_vs_1e-5" % (graph, variant, max(lengths), coef), grad=e, objf=abs(o - o5) / abs(o5))
    assert e >= 1e-2, (graph, variant, coef, e)


# ---- the emulator, unfaulted ------------------------------------------------------------------------------------------
def _emulator_case(case):
    if case == "small_hubs":
        return lc.make_graph("small_hubs", "leaky_ones"), 300, 14, False
    if case == "hubs":
        return lc.make_graph("hubs", "leaky_ones"), 600, 9, False
    if case == "structured":
        return lc.make_graph("structured", "leaky_ones"), 3456, 5, True
    from helpers import random_hub_graph
    g, D = random_hub_graph(int(case[len("random"):]))
    return g, D, 7, False


@pytest.mark.parametrize("variant", lc.VARIANTS)
@pytest.mark.parametrize("case", ["small_hubs", "hubs", "structured", "random0", "random1", "random2", "random3"])
def test_emulated_kernels_at_large_coefficients(case, variant):
    """Coefficients 0.1 and 0.5, both graph variants, plans with states on several lanes: what the kernels compute from the plan
    (the emulator, fp64; the structured graph in its one-gather form too) is what they compute with every state on one lane
    (1e-11) and what the fp64 oracle gives (2e-6 / 1e-5: the bounds of test_plan.test_states_on_several_lanes)."""
    base, D, T, sg = _emulator_case(case)
    g = lc.as_variant(base, variant)
    blob = _blob(g, D)
    with _lib.option("plan_split", "0"):
        blob0 = _blob(g, D)
    x = syn.make_input(2, T, D, seed=21).numpy()
    L = np.array([T, T - 3])
    for coef in (0.1, 0.5):
        objf0, grad0 = lc.emulate(blob0, x, L, coef)
        ro, rg, ok = orc.den(ChainGraphBatch(g, 2), np.exp(np.clip(x, -30, 30)), L, coef, flavour="f64")
        assert ok
        for use_sg in ([False, True] if sg else [False]):
            objf, grad = lc.emulate(blob, x, L, coef, sg=use_sg)
            e0, e = rel_err(grad, grad0), rel_err(grad, rg)
            record_parity("leaky_emulator_%s_%s_sg%d_%g" % (case, variant, use_sg, coef), grad_vs_one_lane=e0, grad_vs_f64=e,
                          objf_vs_f64=abs(objf.sum() - ro.sum()) / abs(ro.sum()))
            assert np.abs(objf - objf0).max() <= 1e-11 * np.abs(objf0).max() and e0 <= 1e-11, (case, coef, e0)
            assert abs(objf.sum() - ro.sum()) <= 2e-6 * abs(ro.sum()) and e <= 1e-5, (case, coef, e)


# ---- the host twins ---------------------------------------------------------------------------------------------------
TWIN_LENGTHS = [61, 54, 40, 3, 2, 1]


@pytest.mark.parametrize("variant", lc.VARIANTS)
@pytest.mark.parametrize("graph", ["c2", "small_hubs"])
def test_host_twins_at_large_coefficients(graph, variant):
    """ChainFunction on CPU tensors (pychain_hip_cpu_*) at coefficients 1e-2, 0.1 and 0.5 against the fp64 oracle, 1e-5 for the
    objective and the gradient; the rows beyond each length are exactly zero."""
    g, D = lc.make_graph(graph, variant), lc.num_pdfs(graph)
    B, T = len(TWIN_LENGTHS), max(TWIN_LENGTHS)
    L = torch.tensor(TWIN_LENGTHS)
    x = syn.make_input(B, T, D, seed=37)
    for coef in (1e-2, 0.1, 0.5):
        xx = x.clone().requires_grad_(True)
        before = _lib.lib().pychain_hip_cpu_calls()
        o = ChainFunction.apply(xx, L, ChainGraphBatch(g, B), coef)
        o.backward()
        assert _lib.lib().pychain_hip_cpu_calls() == before + 1 and int(ChainFunction.last_bad_count.sum()) == 0
        ro, rg = orc.chain_function(x, L, ChainGraphBatch(g, B), coef, flavour="f64")
        grad = xx.grad.numpy()
        eo, eg = abs(float(o.detach()) - ro) / abs(ro), rel_err(grad, rg)
        print("host twin", graph, variant, coef, "objf %.3g grad %.3g" % (eo, eg))
        record_parity("leaky_host_twin_%s_%s_%g" % (graph, variant, coef), objf=eo, grad=eg, bound=1e-5)
        assert eo <= 1e-5 and eg <= 1e-5, (graph, variant, coef, eo, eg)
        for b, n in enumerate(TWIN_LENGTHS):
            assert not grad[b, n:].any()
