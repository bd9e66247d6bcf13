"""tests/peaky.py pinned on the CPU: the reference alone, never the library's kernels.  What the GPU tests of the splice check
rely on (tests/test_gpu_tseg.py) is PROVED here in float64: for every pinned case the max-norm criterion of ABI <= 27 accepts
every splice of the call, a row the segment keeps is >= 1e-3 (where no seed of 64 reaches that: >= 1e-4, the parity bar)
from the true one, and the call's gradient leaves the 1e-5 a cut call is held to; the per-state criterion sees it, and what it bounds stays bounded inside the segment."""
import numpy as np
import pytest

import peaky as pk


def _emulate(name, S, burn, direction):
    _, G, D = pk.splice_graph(name)
    x = pk.pinned_splice_case(name, S, burn, direction)
    return [pk.emulate_call(G, x[b], pk.SPLICE_COEF, L, S, burn) for b, L in enumerate(pk.SPLICE_LENGTHS)]


@pytest.mark.parametrize("name,S,burn,direction", sorted(k for k, v in pk.SPLICE_PINS.items() if v[2] is not None))
def test_pinned_inputs_defeat_the_max_norm_splice_check_in_float64(name, S, burn, direction):
    r0, r1 = _emulate(name, S, burn, direction)
    _, _, want_row, want_grad, carrier = pk.SPLICE_PINS[(name, S, burn, direction)]
    assert len(r0) == len(r1) == 2 * (S - 1)                       # every inner start and end of both sequences is speculated
    old = max(r["old"] for r in r0 + r1)
    _, G, D = pk.splice_graph(name)
    x = pk.pinned_splice_case(name, S, burn, direction)
    grad = max(pk.cut_gradient_error(G, x[b], pk.SPLICE_COEF, L, S, burn) for b, L in enumerate(pk.SPLICE_LENGTHS))
    worst = max(((b, r) for b, rs in enumerate((r0, r1)) for r in rs), key=lambda br: br[1]["inside"])
    inside = worst[1]["inside"]
    print(name, S, burn, direction, "max norm at the splices %.3g, worst kept row %.3g (sequence %d, direction %d), cut gradient from the "
          "uncut one %.3g, per state at that splice %.3g" % (old, inside, worst[0], worst[1]["dir"], grad, worst[1]["new"]))
    assert old <= pk.OLD_SPLICE_TOL / 2                            # accepted, with room for the fp32 recursions' own 5e-7
    assert inside >= want_row and grad >= want_grad                # ... and wrong: 1e-5 is what a cut call is held to
    assert (worst[0], worst[1]["dir"]) == carrier                  # which splice it is: a beta pin IS a wrong beta segment
    # every splice with a row that far off inside is far from verifying per state: the new criterion rejects the call
    bad = [r for r in r0 + r1 if r["inside"] >= want_row]
    assert bad and all(r["new"] > 1e-4 for r in bad)


def test_which_pins_hold_the_issues_bar_and_which_cover_beta():
    """The figures the comment at SPLICE_PINS states: kept rows 1e-3 off at burn-in 16 on BOTH graphs and at 32 on the first; a
    wrong beta segment pinned on the first graph only."""
    pins = {k: v for k, v in pk.SPLICE_PINS.items() if v[2] is not None}
    at = lambda name, burn: [v[2] for k, v in pins.items() if k[0] == name and k[2] == burn]
    assert at("LzDma", 16) == [1e-3, 1e-3] and at("LzNarrowDma", 16) == [1e-3, 1e-3] and at("LzDma", 32) == [1e-3] * 3
    assert at("LzNarrowDma", 32) == [1e-4] * 4
    assert sorted(k for k, v in pins.items() if v[4][1] == 1) == [("LzDma", 2, 16, 0), ("LzDma", 2, 16, 1), ("LzDma", 2, 32, 1), ("LzDma", 4, 32, 1)]


@pytest.mark.parametrize("name", sorted(pk.SPLICE_GRAPHS))
def test_per_state_agreement_does_not_grow_inside_a_segment(name):
    """Hilbert's projective distance is not increased by a frame of either recursion, and it is a metric: a segment's kept rows
    are within the SUM of dl = log((1 + eps) / (1 - eps)) over its own splice and the splices between it and the sequence's end
    (the row it is checked against is the neighbour's, itself speculated) - e^sum - 1 per state.  On the pinned cases' splices,
    two and four segments, both directions, whatever eps they happen to have (the max norm, measured beside it, grows by factors
    of 1e3 ... 1e5)."""
    seen = chained = grew = 0
    for (n, S, burn, direction), pin in sorted(pk.SPLICE_PINS.items()):
        if n != name or pin[2] is None:
            continue
        for r in sum(_emulate(n, S, burn, direction), []):
            if r["chain"] < 1.0:
                assert r["inside_new"] <= np.expm1(r["chain"]) * (1 + 1e-9) + 1e-13, r
                seen += 1
                chained += (r["k"] > 1) if r["dir"] == 0 else (r["k"] < S - 2)
            grew += r["inside"] > 100 * r["old"]
    assert seen >= 8 and chained >= 2 and grew >= 1


@pytest.mark.parametrize("name,S", [(n, S) for n in sorted(pk.SPLICE_GRAPHS) for S in (2, 4)])
def test_at_96_frames_the_filter_has_forgotten_on_these_inputs(name, S):
    r0, r1 = _emulate(name, S, 96, 0)
    assert len(r0) == len(r1) == 2 * (S - 1)
    assert max(max(r["old"], r["new"], r["inside"], r["inside_new"]) for r in r0 + r1) <= 1e-12


def test_metrics_and_inputs():
    p = np.array([0.5, 0.5 - 1e-6, 1e-6, 0.0])
    q = np.array([0.5, 0.5 - 1.5e-6, 1.5e-6, 0.0])
    assert pk.max_norm(p, q) == pytest.approx(1e-6, rel=1e-3)      # the max norm cannot see a light state that is 50 % off
    assert pk.rel_norm(p, q) == pytest.approx(0.5, rel=1e-3)       # per state: seen; zero in both rows compares equal
    assert pk.rel_norm(p, p * 7.0) == 0.0 and pk.max_norm(p, p * 7.0) == 0.0        # the scale is free
    assert pk.rel_norm(p, np.array([0.5, 0.5, 0.0, 0.0])) == pytest.approx(1.0)     # a zero in the speculated row only
    assert pk.rel_norm(np.array([0.5, 0.5, 0.0, 0.0]), p) == np.inf                 # a zero in the true row only
    _, G, D = pk.splice_graph("LzDma")
    x, walk = pk.path_input(G, 97, D, seed=3)
    assert x.dtype == np.float32 and x.shape == (97, D) and sum(n for _, n, _, _ in walk) == 97
    state = 0
    for t, n, k, pdf in walk:                                      # the peaks follow arcs of the graph, from state 0 on
        assert G["src"][k] == state and G["pdf"][k] == pdf and (x[t:t + n].argmax(axis=1) == pdf).all()
        assert x[t:t + n, pdf].min() > 5.0
        state = G["dst"][k]
    xc, _ = pk.clamp_input(G, 97, D, seed=3)
    assert xc.max() > 30.0 and xc.min() < -30.0 and (np.sort(xc, axis=1)[:, -2] < -30.0).any() and (xc.max(axis=1) < 30.0).any()
    y = pk.surprise(x.copy(), [5, 6, 200], [1, 2], -25.0)
    assert (y[5:7, 1:3] == -25.0).all() and (y[7] == x[7]).all()
    # alpha_rows / beta_rows are oracle/forgetting.py's recursions, every row kept
    import forgetting as fg
    w = pk.arc_weights(G, x)
    Gf = fg.graph_arrays(pk.splice_graph("LzDma")[0])
    a = pk.alpha_rows(G, w, 1e-5, 0, 40)
    b = pk.beta_rows(G, w, 1e-5, 97, 50)
    assert np.allclose(a[-1], fg.alpha_run(Gf, w, Gf["leaky"], 1e-5, 0, 40), rtol=1e-12, atol=0)
    assert np.allclose(b[0], fg.beta_run(Gf, w, np.ones(G["H"]), 1e-5, 97, 50), rtol=1e-12, atol=0)
    assert np.allclose(a.sum(axis=1), 1.0) and np.allclose(b.sum(axis=1), 1.0)
