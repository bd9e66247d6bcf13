"""Plans of the edge-colouring slot-order solver (csrc/plan.cpp) under every kernel form that reads a plan's slot stream:
the fused loss and the denominator alone against the fp64 oracle, and bit for bit between the forms the suite holds to that.
A wrong slot order shows in the first frame, so the shapes are tiny: B = 3, lengths 40 / 7 / 1."""
import numpy as np
import pytest
import torch

import oracle as orc
from helpers import rel_err
from pychain_amd import ChainFunction, ChainGraphBatch, ChainLoss, _lib, _plan, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [40, 7, 1]
TOL = 1e-5                                          # objective and gradient against fp64, as tests/test_gpu_parity.py

GRAPHS = {"h1500": (1500, 15000, 1728, 1),          # sixteen-wave recursion workgroups
          "c2": (200, 2000, 1000, 0)}               # fits the four-wave map (den_lazy.inc.h: LzSmall)
FORMS = {"default": {}, "den_dma0": {"den_dma": 0}, "den_lazy0": {"den_lazy": 0}, "den_pair1": {"den_pair": 1},
         "gamma16": {"gamma16": 1}}

_cases, _outs = {}, {}


def _case(gname):
    """Graph, inputs and the fp64 references of a graph: computed once, shared by every form."""
    if gname not in _cases:
        H, K, D, seed = GRAPHS[gname]
        den = syn.make_den_graph(H, K, D, seed=seed)
        L = torch.tensor(LENGTHS)
        x = syn.make_input(len(LENGTHS), max(LENGTHS), D, seed=41)
        numg = syn.make_num_graphs(LENGTHS, D, seed=500)
        hint = _plan.plan_info(_plan.build_plan_blob(*[getattr(den, n) for n in _plan._NAMES], D))["slot_rows"]
        assert ((hint >> 29) & 1) == (1 if gname == "c2" else 0)             # the four-wave tiles: C2 carries them, the other does not
        rl, rg = orc.chain_loss(x, L, den, numg, 1e-5, avg=False, flavour="f64")
        ro, rog = orc.chain_function(x, L, ChainGraphBatch(den, len(LENGTHS)), flavour="f64")
        _cases[gname] = dict(den=den, D=D, L=L, x=x.to(DEV), numg=numg, loss=float(rl), loss_grad=rg, objf=float(ro), objf_grad=rog)
    return _cases[gname]


def _run(gname, form):
    if (gname, form) not in _outs:
        c = _case(gname)
        opts = FORMS[form]
        ctx = [_lib.option(k, v) for k, v in opts.items()]
        for m in ctx:
            m.__enter__()
        try:
            xx = c["x"].clone().requires_grad_(True)
            loss = ChainLoss(c["den"], 1e-5, avg=False)(xx, c["L"], c["numg"])
            loss.backward()
            assert int(loss.bad_count.sum().item()) == 0
            xd = c["x"].clone().requires_grad_(True)
            objf = ChainFunction.apply(xd, c["L"], ChainGraphBatch(c["den"], len(LENGTHS)), 1e-5)
            objf.backward()
            assert int(ChainFunction.last_bad_count.item()) == 0
            torch.cuda.synchronize()
            _outs[(gname, form)] = (loss.detach().clone(), xx.grad.clone(), objf.detach().clone(), xd.grad.clone())
        finally:
            for m in reversed(ctx):
                m.__exit__(None, None, None)
    return _outs[(gname, form)]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("gname", sorted(GRAPHS))
def test_every_kernel_form_reads_the_new_plans_right(gname, form):
    """Fused loss and denominator alone, objective and gradient, within 1e-5 of the fp64 evaluation; nothing past a
    sequence's length."""
    c = _case(gname)
    loss, lg, objf, og = _run(gname, form)
    lg, og = lg.cpu().numpy(), og.cpu().numpy()
    e = (abs(float(loss) - c["loss"]) / abs(c["loss"]), rel_err(lg, c["loss_grad"]),
         abs(float(objf) - c["objf"]) / abs(c["objf"]), rel_err(og, c["objf_grad"]))
    print("%s %s: loss %.2e grad %.2e | den objf %.2e grad %.2e" % ((gname, form) + e))
    assert max(e) <= TOL, e
    for b, n in enumerate(LENGTHS):
        assert np.all(lg[b, n:] == 0) and np.all(og[b, n:] == 0)


@pytest.mark.parametrize("gname", sorted(GRAPHS))
def test_forms_the_suite_holds_bit_identical_stay_so(gname):
    """The one-frame occupancy kernel (gamma16) gives the bits of the default form (tests/test_gpu_parity.py), and two
    sequences per recursion workgroup (den_pair) those of the two-barrier recursion it restates (den_lazy = 0:
    tests/test_gpu_pair.py) - on the new plans too."""
    for form, ref_form in (("gamma16", "default"), ("den_pair1", "den_lazy0")):
        for a, b in zip(_run(gname, ref_form), _run(gname, form)):
            assert torch.equal(a, b), form
