"""The denominator kernels at leaky-HMM coefficients where their own work in the leaky term shows: 0.1 for every kernel form,
1e-2 and 0.5 for the default forms (every other device test runs at 1e-5, where that work is of order 1e-5 of the result:
tests/test_leaky.py has the measurements).  tests/leaky_cases.py holds the table: graphs in two variants - ("leaky", "ones")
and a one-hot start with non-uniform final probabilities -, the options of each form and the kernel name it must report.

Every case: the form runs under its own name; nothing is `bad`; objective and gradient within 1e-5 of the fp64 oracle AT THAT
COEFFICIENT (the project's bound for the kernels against fp64: tests/test_gpu_q.py); gradient rows beyond each length exactly
zero, every live frame's occupancies sum to 1 within 1e-5; a plan with states on several lanes also within 2e-5 of the same
graph compiled with every state on one lane.  Every measured distance is recorded (helpers.record_parity, "leaky_...")."""
import numpy as np
import pytest
import torch

import leaky_cases as lc
import oracle as orc
from helpers import record_parity, rel_err
from pychain_amd import ChainFunction, ChainGraphBatch, ChainLoss, _lib, _plan, native, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Options(object):
    def __init__(self, opts):
        self.ctx = [_lib.option(k, v) for k, v in opts.items()]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__()
        return False


class _World(object):
    """Graphs, plans, inputs and oracle results of the module, each made once."""

    def __init__(self):
        self.cache = {}

    def graph(self, name, variant, general=False):
        key = ("graph", name, variant, general)
        if key not in self.cache:
            self.cache[key] = lc.make_graph(name, variant)         # (a new object per plan format: plans are cached on the graph)
        return self.cache[key]

    def plan(self, name, variant, one_lane=False, general=False):
        g = self.graph(name, variant, general)
        with _Options({"plan_split": "0"} if one_lane else {}):
            return _plan.graph_plan(g, lc.num_pdfs(name), torch.device(DEV))

    def input(self, form):
        key = ("x", form.graph, tuple(form.lengths))
        if key not in self.cache:
            x, L = form.input(DEV)
            self.cache[key] = (x, L, x.cpu())
        return self.cache[key]

    def oracle(self, form, variant, coef, flavour="f64"):
        key = ("oracle", form.graph, variant, tuple(form.lengths), coef, flavour)
        if key not in self.cache:
            x, L, x_cpu = self.input(form)
            self.cache[key] = orc.chain_function(x_cpu, L, ChainGraphBatch(self.graph(form.graph, variant), len(form.lengths)), coef, flavour=flavour)
        return self.cache[key]

    def one_lane(self, form, variant, coef):
        """the call on the same graph compiled with every state on one lane (default kernels, uncut)"""
        key = ("one_lane", form.graph, variant, tuple(form.lengths), coef)
        if key not in self.cache:
            x, L, _ = self.input(form)
            plan0 = self.plan(form.graph, variant, one_lane=True)
            assert plan0.num_states == self.graph(form.graph, variant).num_states
            self.cache[key] = _den(plan0, x, L, coef, {"den_tseg": 0})
        return self.cache[key]


@pytest.fixture(scope="module")
def world():
    return _World()


def _den(plan, x, L, coef, opts):
    with _Options(opts):
        objf, grad, bad, tot = native.den_forward_backward(plan, x, L, coef, totals=True)
        torch.cuda.synchronize()
    return objf.double().cpu(), grad, int(bad), tot.cpu()


def _check_rows(grad, lengths):
    """rows beyond each length exactly zero; every live frame's occupancies sum to 1 (fp64 sum of the fp32 row)"""
    g = grad.float().cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lengths):
        assert not g[b, n:].any(), b
        worst = max(worst, float(np.abs(g[b, :n].astype(np.float64).sum(-1) - 1.0).max()))
    assert worst <= 1e-5, worst
    return g, worst


@pytest.mark.parametrize("variant", lc.VARIANTS)
@pytest.mark.parametrize("form", lc.FORMS, ids=[f.id for f in lc.FORMS])
def test_every_kernel_form_at_large_coefficients(world, monkeypatch, form, variant):
    D = lc.num_pdfs(form.graph)
    B = len(form.lengths)
    if form.general:
        monkeypatch.setenv("PYCHAIN_PLAN_GENERAL", "1")
    plan = world.plan(form.graph, variant, general=form.general)
    x, L, _ = world.input(form)
    # 1. the form runs: the name query under the call's options (it answers for long sequences and coefficient 1e-5: the forms that
    # depend on the length have lengths that take them - leaky_cases.FORMS -, the one that depends on the coefficient has a test below)
    with _Options(form.opts):
        rec, occ = _lib.den_kernel_names(plan.slot_rows, plan.num_states, D, B)
        rows_ahead = _lib.lib().pychain_hip_den_uses_row_buffer(plan.stride, plan.slot_rows, plan.num_states, D, B, max(form.lengths), 0)
    assert rec == form.rec and (form.occ is None or occ == form.occ), (form.id, rec, occ)
    assert bool(rows_ahead) == form.rows_ahead, form.id
    if form.graph in lc.SPLIT_GRAPHS:
        assert plan.num_states > world.graph(form.graph, variant).num_states              # states on several lanes
    for coef in form.coefs:
        objf, grad, bad, tot = _den(plan, x, L, coef, form.opts)
        assert bad == 0, (form.id, coef)                                                   # 2.
        assert int(tot[6]) == (2 if form.tseg else 1), (form.id, int(tot[6]))
        g, row_sum = _check_rows(grad, form.lengths)                                       # 4.
        ro, rg = world.oracle(form, variant, coef)                                         # 3.
        eo, eg = abs(float(objf.sum()) - ro) / abs(ro), rel_err(g, rg)
        measured = dict(objf_vs_f64=eo, grad_vs_f64=eg, row_sum=row_sum, bound=1e-5)
        if form.tseg:
            # cut against uncut, as tests/test_gpu_tseg.py: nothing missed and within 1e-6, or rows missed and the uncut call's bits
            o1, g1, bad1, tot1 = _den(plan, x, L, coef, {"den_tseg": 0})
            assert bad1 == 0 and int(tot1[6]) == 1
            measured.update(missed=int(tot[5]), objf_vs_uncut=float((objf - o1).abs().max() / o1.abs().max()), grad_vs_uncut=rel_err(g, g1.cpu().numpy()))
            if int(tot[5]) == 0:
                assert measured["objf_vs_uncut"] <= 1e-6 and measured["grad_vs_uncut"] <= 1e-6, (form.id, measured)
            else:
                assert torch.equal(objf, o1) and torch.equal(grad, g1), form.id
        if form.graph in lc.SPLIT_GRAPHS:                                                  # 5.
            o0, g0, bad0, _ = world.one_lane(form, variant, coef)
            measured.update(objf_vs_one_lane=abs(float(objf.sum() - o0.sum())) / abs(float(o0.sum())), grad_vs_one_lane=rel_err(g, g0.cpu().numpy()))
        print("leaky", form.id, variant, coef, measured)
        record_parity("leaky_%s_%s_%s_%g" % (form.graph, form.key, variant, coef), **measured)
        assert eo <= 1e-5 and eg <= 1e-5, (form.id, variant, coef, eo, eg)
        if form.graph in lc.SPLIT_GRAPHS:
            assert bad0 == 0 and measured["objf_vs_one_lane"] <= 2e-5 and measured["grad_vs_one_lane"] <= 2e-5, (form.id, measured)


@pytest.mark.parametrize("coef", [1e-7, 1e-9])
def test_one_word_states_at_the_edges_of_the_coefficient_window(world, coef):
    """Option den_q on the C3 graph, ("leaky", "ones").  The one-word form takes coefficients in [1e-8, 1] (den_lazy.hip:
    q_shape_ok: 1 / (coef leaky) stays below 1e20).  pychain_hip_den_kernel_names has no coefficient argument and ANSWERS FOR 1e-5:
    it reports the one-word kernel for this plan whatever the call's coefficient will be.  At 1e-9 the call is not eligible and runs
    the default kernels - their result bit for bit; at 1e-7 it is, and is held to the fp64 oracle (1e-5), nothing `bad`.  Nothing
    a query sizes - workspace, row buffer, stored rows - depends on the form."""
    form = next(f for f in lc.FORMS if f.id == "c3-one_word_states")
    plan = world.plan("c3", "leaky_ones")
    x, L, _ = world.input(form)
    with _Options(form.opts):
        assert _lib.den_kernel_names(plan.slot_rows, plan.num_states, 3456, len(form.lengths))[0] == lc.LAZY_Q
    objf, grad, bad, tot = _den(plan, x, L, coef, form.opts)
    o0, g0, bad0, _ = _den(plan, x, L, coef, {"den_q": 0, "den_tseg": 0})
    assert bad == 0 and bad0 == 0
    g, row_sum = _check_rows(grad, form.lengths)
    ro, rg = world.oracle(form, "leaky_ones", coef)
    eo, eg = abs(float(objf.sum()) - ro) / abs(ro), rel_err(g, rg)
    same = torch.equal(objf, o0) and torch.equal(grad, g0)
    print("leaky one-word states", coef, "objf %.3g grad %.3g same bits as the default kernels: %s" % (eo, eg, same))
    record_parity("leaky_c3_one_word_states_leaky_ones_%g" % coef, objf_vs_f64=eo, grad_vs_f64=eg, row_sum=row_sum, same_bits_as_default=float(same), bound=1e-5)
    if coef < 1e-8:
        assert same
    assert eo <= 1e-5 and eg <= 1e-5, (coef, eo, eg)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_chain_loss_at_coefficient_0_1(world, dtype):
    """ChainLoss(den, 0.1) on the C3 graph with ragged numerators, against the fp64 oracle's chain loss at 1e-5.  bf16 network
    output as tests/test_gpu_half.py holds it: the 2-byte rows read as they are give the bits of the rows up-cast on the host
    side of the ABI, whose fp32 arithmetic is the one held to 1e-5 - with the gradient rounded to bf16 where it is written
    (2^-8 of the largest entry)."""
    den = world.graph("c3", "leaky_ones")
    lens = [61, 54, 40, 4]
    L = torch.tensor(lens)
    x = syn.make_input(4, 61, 3456, seed=83, device=DEV).to(dtype)
    num = syn.make_num_graphs(lens, 3456, seed=100)

    def step():
        xx = x.clone().requires_grad_(True)
        loss = ChainLoss(den, lc.COEF, avg=True)(xx, L, num)
        loss.backward()
        torch.cuda.synchronize()
        assert int(ChainFunction.last_bad_count.sum()) == 0
        return float(loss.detach()), xx.grad
    loss, grad = step()
    rl, rg = orc.chain_loss(x.float().cpu(), L, den, num, lc.COEF, avg=True, flavour="f64")
    eo, eg = abs(loss - float(rl)) / abs(float(rl)), rel_err(grad.float().cpu().numpy(), rg)
    print("leaky fused loss", dtype, "loss %.3g grad %.3g" % (eo, eg))
    record_parity("leaky_c3_fused_loss_%s_0.1" % ("bf16" if dtype == torch.bfloat16 else "fp32"), loss_vs_f64=eo, grad_vs_f64=eg, bound=1e-5)
    assert grad.dtype == dtype and bool((grad[1, 54:] == 0).all()) and bool((grad[3, 4:] == 0).all())
    if dtype == torch.float32:
        assert eo <= 1e-5 and eg <= 1e-5, (eo, eg)
        return
    native.HALF_ROWS = False
    try:
        loss_up, grad_up = step()
    finally:
        native.HALF_ROWS = True
    assert loss == loss_up and torch.equal(grad, grad_up)
    assert eo <= 1e-5 and eg <= 2.0 ** -8 + 1e-5, (eo, eg)
