"""Numerator posteriors as cross-entropy targets (include/pychain_hip.h: pychain_hip_xent) on CPU tensors: the host twin and the
unfused ChainLoss(xent_regularize=c) against tests/xent_reference.np_xent and against the torch float64 composition
-(gamma * log_softmax(z)).sum() through autograd; per-sequence and shared graphs, ragged lengths in arbitrary order, with and
without alignment time windows, one sequence whose windows admit no path; the chain output's gradient bit-identical with
and without the term; xent_output=None and c = 0 are today's call; a 2-rank gloo ShardedChainLoss.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import num_cases as nc
from helpers import record_parity
from num_reference import np_num_fb
from pychain_amd import (ChainGraphBatch, ChainLoss, _lib, alignment_windows, native, numerator_xent, parallel, viterbi_align,
                         synthetic as syn)
from xent_reference import GAMMA_BOUND, check_xent, fp32_distance, np_xent

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 0.1
D = 40
LENGTHS = torch.tensor([37, 50, 9, 44])                    # ragged, in no order
DEN = syn.make_den_graph(20, 60, D, seed=0)


def _z(B, T, seed=77, scale=3.0):
    return syn.make_input(B, T, D, seed=seed) * (scale / 2.0)


def _per_seq_case():
    graphs = syn.make_num_graphs(LENGTHS.tolist(), D, seed=100, max_states=12)
    return syn.make_input(4, 50, D, seed=5), LENGTHS, graphs


def _shared_case():
    g = nc.all_final_graph(150, D)
    return syn.make_input(4, 50, D, seed=6), LENGTHS, ChainGraphBatch(g, 4)


CASES = {"per_seq": _per_seq_case, "shared": _shared_case}


def _windows(x, lengths, graphs, kind):
    """None; the tolerance-2 windows of the host alignment; the same perturbed, sequence 1 without an admissible path."""
    if kind == "free":
        return None
    if kind == "tau2":
        return alignment_windows(viterbi_align(x, lengths, graphs), graphs.num_states, tolerance=2)
    return nc.perturbed_windows(x, lengths, graphs, seed=11, infeasible=1)


@pytest.mark.parametrize("kind", ["free", "tau2", "infeasible"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_host_twin_matches_reference(case, kind):
    x, lengths, graphs = CASES[case]()
    z = _z(*x.shape[:2])
    w = _windows(x, lengths, graphs, kind)
    fb = np_num_fb(graphs, x, lengths, w)
    assert bool(fb[2].all()) == (kind != "infeasible") and (kind != "infeasible" or not fb[2][1])
    ref = np_xent(graphs, x, z, lengths, w, fb)
    own = fp32_distance(graphs, x, z, lengths, w, fb, ref)
    res = native.cpu_num_xent(graphs, x, lengths, z, with_grad=True, windows=w)
    name = "xent_cpu_%s_%s" % (case, kind)
    d = check_xent(res.objf.numpy(), res.grad.numpy(), ref, lengths, fb[2], (own[0] + GAMMA_BOUND, own[1] + GAMMA_BOUND), name)
    record_parity(name, fp32_objf=own[0], fp32_grad=own[1], objf_rel=d[0], grad_rel=d[1])
    assert abs(float(res.totals[1]) - ref[0].sum()) <= (own[0] + GAMMA_BOUND) * np.abs(ref[0]).sum()
    # the form without the store: the same objectives, bit for bit
    res2 = native.cpu_num_xent(graphs, x, lengths, z, with_grad=False, windows=w)
    assert res2.grad is None and torch.equal(res2.objf, res.objf)


def _loss(x, lengths, graphs, z=None, c=0.0, avg=True, **kw):
    xx = x.clone().requires_grad_(True)
    zz = None if z is None else z.clone().requires_grad_(True)
    crit = ChainLoss(DEN, 1e-5, avg=avg, xent_regularize=c) if (c or kw.get("pass_c")) else ChainLoss(DEN, 1e-5, avg=avg)
    loss = crit(xx, lengths, graphs) if zz is None else crit(xx, lengths, graphs, xent_output=zz)
    loss.backward()
    out = loss.detach()
    out.xent_objf = getattr(loss, "xent_objf", None)
    return out, xx.grad, None if zz is None else zz.grad


@pytest.mark.parametrize("kind", ["free", "tau2", "infeasible"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_unfused_chain_loss_on_cpu(case, kind):
    x, lengths, graphs = CASES[case]()
    z = _z(*x.shape[:2], seed=78)
    w = _windows(x, lengths, graphs, kind)
    graphs.set_time_windows(w)
    fb = np_num_fb(graphs, x, lengths, w)
    ref = np_xent(graphs, x, z, lengths, w, fb)
    own = fp32_distance(graphs, x, z, lengths, w, fb, ref)
    bound = (own[0] + GAMMA_BOUND, own[1] + GAMMA_BOUND)
    frames = float(lengths.sum())
    loss0, gx0, _ = _loss(x, lengths, graphs)
    loss, gx, gz = _loss(x, lengths, graphs, z, C)
    # the chain output's gradient does not see the term: bit-identical
    assert torch.equal(gx, gx0)
    # xent_output=None and c = 0: today's call, bit for bit
    for other in (_loss(x, lengths, graphs, None, C), _loss(x, lengths, graphs, z, 0.0, pass_c=True)):
        assert torch.equal(other[0].detach(), loss0.detach()) and torch.equal(other[1], gx0) and other[2] is None
    # the total and the logged objective
    xent_ref = float(ref[0].sum()) / frames
    assert abs(float(loss.xent_objf) - xent_ref) <= bound[0] * np.abs(ref[0]).sum() / frames
    if np.isfinite(float(loss0)):
        expect = float(loss0) - C * xent_ref
        assert abs(float(loss) - expect) <= bound[0] * (abs(float(loss0)) + C * abs(xent_ref)) + 1e-6 * abs(expect)
    # dz = -c / frames * (gamma - s softmax): against np_xent ...
    dz = gz.numpy().astype(np.float64) * (-frames / C)
    per_seq = numerator_xent(z, x, lengths, graphs).xent_objf_per_seq.numpy()
    check_xent(per_seq, dz, ref, lengths, fb[2], bound, "xent_cpu_loss_%s_%s" % (case, kind))
    # ... and against autograd through the torch float64 composition fed the reference's gamma
    z64 = z.double().clone().requires_grad_(True)
    live = torch.zeros(z.shape[:2], dtype=torch.float64)
    for b, L in enumerate(lengths.tolist()):
        live[b, :L] = 1.0
    comp = -(torch.from_numpy(fb[1]) * torch.log_softmax(z64, -1) * live[..., None]).sum()
    comp.backward()
    want = z64.grad.numpy() * (C / frames)
    assert np.abs(gz.numpy() - want).max() <= bound[1] * np.abs(want).max()
    graphs.set_time_windows(None)


def test_infeasible_sequence_contributes_nothing():
    x, lengths, graphs = _per_seq_case()
    z = _z(4, 50, seed=79)
    w = nc.perturbed_windows(x, lengths, graphs, seed=11, infeasible=1)
    res = native.cpu_num_xent(graphs, x, lengths, z, windows=w)
    assert float(res.objf[1]) == 0.0 and not bool(res.grad[1].any())
    assert bool((res.objf[[0, 2, 3]] < 0).all())
    for b, L in enumerate(lengths.tolist()):
        assert not bool(res.grad[b, L:].any()) and bool(res.grad[b, :L].any()) == (b != 1)
    # without the infeasible sequence's windows it contributes again
    w2 = w.clone()
    w2[1, :, 0], w2[1, :, 1] = -1, nc.BIG
    assert float(native.cpu_num_xent(graphs, x, lengths, z, windows=w2).objf[1]) < 0.0


def test_numerator_xent_is_differentiable_in_the_xent_output_only_and_recomputes():
    x, lengths, graphs = _per_seq_case()
    xx = x.clone().requires_grad_(True)
    zz = _z(4, 50, seed=80).requires_grad_(True)
    o = numerator_xent(zz, xx, lengths, graphs)
    assert o.dim() == 0 and o.xent_objf_per_seq.shape == (4,)
    (3.0 * o).backward(retain_graph=True)
    assert xx.grad is None
    first = zz.grad.clone()
    zz.grad = None
    (3.0 * o).backward()                                  # a second backward over the retained graph evaluates again
    assert torch.equal(zz.grad, first)
    ref = np_xent(graphs, x, zz.detach(), lengths)
    assert abs(float(o) - ref[0].sum()) <= 2e-5 * abs(ref[0].sum())
    assert np.abs(first.numpy() / 3.0 - ref[1]).max() <= 2e-5 * np.abs(ref[1]).max()
    # an in-place edit between the two backward calls is refused, as for the LF-MMI gradient
    zz2 = zz.detach().clone().requires_grad_(True)
    zin = zz2 * 1.0
    o2 = numerator_xent(zin, x, lengths, graphs)
    o2.backward(retain_graph=True)
    with torch.no_grad():
        zin.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        o2.backward()


def test_a_nan_row_makes_that_sequence_nan_only():
    x, lengths, graphs = _per_seq_case()
    z = _z(4, 50, seed=81)
    z[2, 3, 7] = float("nan")
    res = native.cpu_num_xent(graphs, x, lengths, z)
    assert np.isnan(float(res.objf[2])) and bool(torch.isfinite(res.objf[[0, 1, 3]]).all())
    z[2, 3, 7] = 0.0
    z[0, 40, :] = float("nan")                              # beyond the length of sequence 0: not read
    assert bool(torch.isfinite(native.cpu_num_xent(graphs, x, lengths, z).objf).all())


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 20
    for name in ("pychain_hip_num_forward_backward_xent", "pychain_hip_chain_loss_forward_xent", "pychain_hip_chain_loss_forward_backward_xent",
                 "pychain_hip_cpu_num_forward_backward_xent", "pychain_hip_xent_workspace_bytes"):
        assert name in header and hasattr(_lib.lib(), name)
    # the struct of the binding has the layout of the header's: field names in order
    fields = re.search(r"typedef struct pychain_hip_xent \{(.*?)\} pychain_hip_xent;", header, re.S).group(1)
    names = [re.search(r"(\w+);", line).group(1) for line in fields.strip().splitlines()]
    assert names == [n for n, _ in _lib.Xent._fields_]
    # the workspaces of a call are as large with xent as without; only the xent workspace knows about the general fallback
    L = _lib.lib()
    gb = nc.form_graphs(4)
    H, K = gb.num_states, int(gb.backward_transitions.shape[-2])
    small = L.pychain_hip_xent_workspace_bytes(4, 50, H, K, 48)
    Dg = nc.form_boundary_D()[1]
    assert small < 8 * 4 * 50 + 4096
    assert L.pychain_hip_xent_workspace_bytes(4, 50, H, K, Dg) >= 4 * 4 * 50 * Dg


def test_null_xent_is_the_call_without_it():
    """pychain_hip_cpu_num_forward_backward_xent(..., NULL) = pychain_hip_cpu_num_forward_backward_tw: same bits."""
    x, lengths, graphs = _per_seq_case()
    a = native.cpu_forward_backward(graphs, x, lengths)
    ts, stride = native._cpu_graph(graphs, False)
    B, T, _ = x.shape
    H, K = int(ts[1].shape[-2]), int(ts[0].shape[-2])
    objf, grad, bad = torch.empty(B), torch.empty(B, T, D), torch.zeros(1, dtype=torch.int32)
    lc = lengths.to(torch.int64)
    _lib.check(_lib.lib().pychain_hip_cpu_num_forward_backward_xent(
        *[t.data_ptr() for t in ts], stride, x.data_ptr(), lc.data_ptr(), B, T, D, H, K, _lib.GRAD_LINEAR, 1.0,
        objf.data_ptr(), grad.data_ptr(), bad.data_ptr(), 0, None, None), "xent")
    assert torch.equal(objf, a[0]) and torch.equal(grad, a[1]) and torch.equal(bad, a[2])


# ---- a 2-rank gloo ShardedChainLoss equals the one-process loss and gradient (tests/test_parallel.py's pattern) ---------------
def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, lengths, graphs = _per_seq_case()
        z = _z(4, 50, seed=82)
        xs, ls, gs, idx = parallel.shard_batch(x, lengths, graphs, world, rank)
        zs = z.index_select(0, idx).clone().requires_grad_(True)
        xs = xs.clone().requires_grad_(True)
        loss = parallel.ShardedChainLoss(DEN, 1e-5, avg=True, xent_regularize=C)(xs, ls, gs, xent_output=zs)
        loss.backward()
        out[rank] = (float(loss), idx.tolist(), xs.grad.numpy(), zs.grad.numpy())
    finally:
        dist.destroy_process_group()


def test_sharded_loss_matches_single_process():
    world, port = 2, 30731 + os.getpid() % 1000
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    x, lengths, graphs = _per_seq_case()
    z = _z(4, 50, seed=82)
    loss, gx, gz = _loss(x, lengths, graphs, z, C)
    for r in range(world):
        l, idx, sgx, sgz = out[r]
        assert abs(l - float(loss)) <= 1e-5 * abs(float(loss))
        np.testing.assert_allclose(sgx, gx.numpy()[idx], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(sgz, gz.numpy()[idx], rtol=1e-5, atol=1e-7)
