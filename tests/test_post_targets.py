"""Posterior-target supervision (include/pychain_hip.h: pychain_hip_post_targets, pychain_hip_topk_rows) on CPU tensors: the host
twins against tests/post_reference at the shapes the GPU tests use; posterior_numerator and ChainLoss(x, lengths, targets)
against the torch composition they replace (ChainFunction on the denominator, a gathered q * clamp(x), autograd's add), value and
gradient, alone and with weights and regularisers; a second backward; validation; a 2-rank gloo ShardedChainLoss; ABI 23.
No GPU.  The bounds are post_reference's; the ChainLoss comparisons use the library's fp64 bar, 1e-5 on the value and on
max |d grad| / max |grad|."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import post_reference as pr
from helpers import record_parity
from pychain_amd import (ChainLoss, PosteriorTargets, _lib, native, occupancies, parallel,
                         posterior_numerator, posterior_targets, synthetic as syn)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5
D = 40
LENGTHS = torch.tensor([37, 40, 9, 33])                    # ragged, in no order
DEN = syn.make_den_graph(20, 60, D, seed=0)
L2, OOR = 5e-4, 0.01


# ---- the twins against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", pr.NATIVE_KS)
@pytest.mark.parametrize("Dx", pr.NATIVE_DS)
def test_host_twin_matches_reference(Dx, K):
    x, lengths, pdfs, probs = pr.native_case(Dx, K)
    ref0 = pr.np_post_targets(x.numpy(), lengths, pdfs.numpy(), probs.numpy())
    num, bad = native.cpu_post_targets(x, lengths, pdfs, probs)                       # the objective only
    assert int(bad) == 1 == ref0["bad"]
    d_obj = float((np.abs(num.numpy().astype(np.float64) - ref0["num"]) / np.maximum(pr.objf_bound(ref0), 1e-300)).max())
    assert d_obj <= 1.0, d_obj
    pat = pr.grad_pattern(x.shape, "float32")
    worst = 0.0
    for gsd, norm in ((None, None), (1.5, None), (None, 7.0), (1.5, 7.0)):
        s = pr.f32_scale(-0.25, gsd, norm)
        ref = pr.np_post_targets(x.numpy(), lengths, pdfs.numpy(), probs.numpy(), grad=pat.numpy(), s=s)
        g = pat.clone()
        den = torch.tensor([-3.5, 2.25, -1.0])
        totals = torch.arange(8, dtype=torch.float32) + 0.5
        num2, bad2 = native.cpu_post_targets(x, lengths, pdfs, probs, grad=g, grad_scale=-0.25, grad_scale_dev=gsd, norm=norm,
                                             den_objf=den, loss_scale=0.5, totals=totals)
        assert torch.equal(num2, num) and int(bad2) == 1
        t = ref["touched"]
        r = float((np.abs(g.numpy().astype(np.float64) - ref["want"])[t] / pr.grad_bound(ref["want"], "float32")[t].clip(1e-300)).max())
        worst = max(worst, r)
        assert r <= 1.0, r
        assert np.array_equal(pr.bits(g).numpy()[~t], pr.bits(pat).numpy()[~t])       # untouched elements keep their bits
        want, keep = pr.np_totals(den.numpy(), ref, np.arange(8) + 0.5, 0.5, norm)
        tot = totals.numpy().astype(np.float64)
        b3, b0 = pr.totals_bounds(want, ref)
        assert abs(tot[3] - want[3]) <= b3 and abs(tot[0] - want[0]) <= b0 and tot[0] == tot[4]
        assert tot[2] == want[2] and all(tot[i] == i + 0.5 for i in keep)
    record_parity("post_cpu_D%d_K%d" % (Dx, K), objf=d_obj, grad=worst)


def test_a_nan_in_a_referenced_live_element_reaches_that_sequence_only():
    x, lengths, pdfs, probs = pr.native_case(8, 4)
    clean, _ = native.cpu_post_targets(x, lengths, pdfs, probs)
    d = int(pdfs[2, 1][pdfs[2, 1] >= 0][0]) if bool((pdfs[2, 1] >= 0).any()) else None
    if d is None:
        pdfs[2, 1, 0], d = 3, 3
    x[2, 1, d] = float("nan")
    num, _ = native.cpu_post_targets(x, lengths, pdfs, probs)
    assert bool(torch.isnan(num[2])) and torch.equal(num[:2], clean[:2])


@pytest.mark.parametrize("Dx", pr.NATIVE_DS)
def test_host_topk_matches_reference(Dx):
    rows, lengths = pr.topk_case(Dx)
    for K in sorted({1, min(3, Dx), min(8, Dx), min(Dx, 64)}):
        for floor, normalize in ((0.0, True), (0.0, False), (0.3, True), (float("-inf"), False)):
            want_p, want_v = pr.np_topk(rows.numpy(), lengths, K, floor, normalize)
            got_p, got_v = native.cpu_topk_rows(rows, lengths, K, floor, normalize)
            assert np.array_equal(got_p.numpy(), want_p), (K, floor, normalize)
            assert pr.topk_values_ok(got_v.numpy(), want_v, normalize), (K, floor, normalize)
    # ties: a whole row of equal values gives the lowest indices, in order; a row below the floor stays empty
    p, v = native.cpu_topk_rows(rows, lengths, min(Dx, 3), 0.0, False)
    assert p[0, 0].tolist() == list(range(min(Dx, 3)))
    if Dx > 2:
        assert p[0, 4].tolist() == [-1] * 3 and v[0, 4].tolist() == [0.0] * 3
    assert bool((p[1, 1:] == -1).all()) and bool((v[1, 1:] == 0).all())                # padded frames are written -1 / 0


# ---- through the Python interface ------------------------------------------------------------------------------------------------
def _case(k=6, seed=5):
    x = syn.make_input(4, 40, D, seed=seed)
    teacher = syn.make_input(4, 40, D, seed=seed + 50) * 1.5
    targets = posterior_targets(teacher, LENGTHS, DEN, k)
    return x, LENGTHS, targets


def _composition(x, lengths, targets, avg=True, u=None, f=None, reg=None):
    return pr.composition(DEN, x, lengths, targets, avg, u, f, reg)


_distances = pr.distances


def test_posterior_numerator_matches_the_torch_composition():
    x, lengths, targets = _case()
    xx = x.clone().requires_grad_(True)
    out = posterior_numerator(xx, lengths, targets)
    assert out.dim() == 0 and tuple(out.objf_per_seq.shape) == (4,)
    (2.0 * out).backward(retain_graph=True)
    first = xx.grad.clone()
    xx.grad = None
    (2.0 * out).backward()                                           # a second backward over the retained graph evaluates again
    assert torch.equal(xx.grad, first)
    x64 = x.double().clone().requires_grad_(True)
    per = pr.torch_numerator_per_seq(x64, lengths, targets.pdfs, targets.probs)
    (2.0 * per.sum()).backward()
    d = _distances(out.detach(), first.numpy(), float(per.detach().sum()), x64.grad.numpy())
    assert np.abs(out.objf_per_seq.numpy() - per.detach().numpy()).max() <= BAR * np.abs(per.detach().numpy()).max()
    record_parity("post_cpu_numerator", loss=d[0], grad=d[1])
    assert max(d) <= BAR, d


@pytest.mark.parametrize("avg", [True, False])
def test_chain_loss_on_cpu_matches_the_torch_composition(avg):
    x, lengths, targets = _case()
    xx = x.clone().requires_grad_(True)
    loss = ChainLoss(DEN, 1e-5, avg=avg)(xx, lengths, targets)
    loss.backward(retain_graph=True)
    first = xx.grad.clone()
    xx.grad = None
    loss.backward()
    assert torch.equal(xx.grad, first)                               # a second backward
    d = _distances(loss.detach(), first.numpy(), *_composition(x, lengths, targets, avg))
    record_parity("post_cpu_loss_avg%d" % avg, loss=d[0], grad=d[1])
    assert max(d) <= BAR, d
    for b, L in enumerate(lengths.tolist()):
        assert not bool(first[b, L:].any())


def test_chain_loss_on_cpu_with_weights_and_regularisers():
    x, lengths, targets = _case()
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.05
    x = torch.where(far, torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0, x)
    u = torch.tensor([1.0, 0.5, 0.0, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    f[0, :5], f[1, 3] = 1.0, 0.0
    xx = x.clone().requires_grad_(True)
    crit = ChainLoss(DEN, 1e-5, avg=True, output_l2_regularize=L2, out_of_range_regularize=OOR)
    loss = crit(xx, lengths, targets, utt_weights=u, deriv_weights=f)
    loss.backward()
    d = _distances(loss.detach(), xx.grad.numpy(), *_composition(x, lengths, targets, True, u, f, (L2, OOR)))
    record_parity("post_cpu_loss_weights_reg", loss=d[0], grad=d[1])
    assert max(d) <= BAR, d
    assert not bool(xx.grad[2].any())                                # the utterance of weight 0
    assert abs(float(loss.weighted_frames) - float((u * lengths).sum())) <= 1e-6 * float((u * lengths).sum())
    assert hasattr(loss, "l2_term") and hasattr(loss, "out_of_range_term")


def test_posterior_targets_with_k_equal_d_reproduce_the_occupancies():
    x = syn.make_input(2, 12, 8, seed=2)
    den = syn.make_den_graph(5, 14, 8, seed=1)
    lengths = torch.tensor([12, 7])
    occ = occupancies(x, lengths, den)
    t = posterior_targets(x, lengths, den, 8, normalize=False)
    dense = torch.zeros(2, 12, 8)
    ok = t.pdfs >= 0
    dense.scatter_add_(2, t.pdfs.clamp_min(0).to(torch.int64), torch.where(ok, t.probs, torch.zeros(())))
    assert torch.equal(dense, torch.where(occ >= 0, occ, torch.zeros(())).float())
    # the student at the teacher's own output: the gradient gamma_den(student) - gamma_den(teacher) vanishes
    xx = x.clone().requires_grad_(True)
    ChainLoss(den, 1e-5, avg=False)(xx, lengths, t).backward()
    assert float(xx.grad.abs().max()) <= BAR * float(occ.abs().max())


def test_validation_errors():
    x, lengths, targets = _case()
    pd, q = targets.pdfs, targets.probs
    with pytest.raises(ValueError):
        PosteriorTargets(pd[:, :, :2], q)                            # shapes differ
    with pytest.raises(ValueError):
        PosteriorTargets(pd[0], q[0])                                # not [B,T,K]
    with pytest.raises(ValueError):
        PosteriorTargets(pd.float(), q)                              # pdfs must be integers
    bad = q.clone()
    bad[0, 0, 0] = -0.5
    with pytest.raises(ValueError):
        PosteriorTargets(pd, bad)
    bad[0, 0, 0] = float("nan")
    with pytest.raises(ValueError):
        PosteriorTargets(pd, bad)
    big = pd.clone()
    big[1, 2, 0] = D
    with pytest.raises(ValueError):
        ChainLoss(DEN, 1e-5)(x, lengths, PosteriorTargets(big, q))   # pdf >= D on host tensors
    with pytest.raises(ValueError):
        posterior_numerator(x, lengths, PosteriorTargets(big, q))
    with pytest.raises(ValueError):
        ChainLoss(DEN, 1e-5)(x[:, :30], torch.tensor([30, 30, 9, 30]), targets)      # T differs
    with pytest.raises(ValueError):
        ChainLoss(DEN, 1e-5, xent_regularize=0.1)(x, lengths, targets, xent_output=x.clone())
    for k in (0, D + 1, 65):
        with pytest.raises(ValueError):
            PosteriorTargets.from_dense(torch.rand(4, 40, 80 if k == 65 else D), lengths, k)
    # the C ABI: K out of range for top-k, K < 1 or a missing pointer for the targets
    L = _lib.lib()
    rows, lc = torch.rand(2, 3, 4), torch.tensor([3, 2])
    op, ov = torch.empty(2, 3, 5, dtype=torch.int32), torch.empty(2, 3, 5)
    for k in (0, 5):
        assert L.pychain_hip_cpu_topk_rows(rows.data_ptr(), lc.data_ptr(), 2, 3, 4, k, 0.0, 1, op.data_ptr(), ov.data_ptr(), 1) == -1
    num, badc = torch.empty(2), torch.zeros(1, dtype=torch.int32)
    call = lambda k, totals: L.pychain_hip_cpu_post_targets(rows.data_ptr(), lc.data_ptr(), 2, 3, 4, op.data_ptr(), ov.data_ptr(), k, None, 1.0,
                                                            None, None, None, num.data_ptr(), badc.data_ptr(), 1.0, totals, 1)
    assert call(0, None) == -1 and call(5, torch.zeros(8).data_ptr()) == -1            # (totals without den_objf_per_seq)


def test_targets_move_select_and_cache():
    _, _, targets = _case()
    assert targets.batch_size == 4 and targets.pdfs.dtype == torch.int32 and targets.probs.dtype == torch.float32
    assert targets.to("cpu") is targets
    sel = targets.index_select(torch.tensor([2, 0]))
    assert sel.batch_size == 2 and torch.equal(sel.pdfs, targets.pdfs[[2, 0]]) and torch.equal(sel.probs, targets.probs[[2, 0]])
    t64 = PosteriorTargets(targets.pdfs.to(torch.int64), targets.probs.double())
    assert t64.pdfs.dtype == torch.int32 and t64.probs.dtype == torch.float32


# ---- a 2-rank gloo ShardedChainLoss equals the one-process loss and gradient (tests/test_weights.py's pattern) -----------------
def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, lengths, targets = _case()
        xs, ls, ts, idx = parallel.shard_batch(x, lengths, targets, world, rank)
        assert isinstance(ts, PosteriorTargets) and ts.batch_size == idx.numel()
        xs = xs.clone().requires_grad_(True)
        loss = parallel.ShardedChainLoss(DEN, 1e-5, avg=True)(xs, ls, ts)
        loss.backward()
        out[rank] = (float(loss), idx.tolist(), xs.grad.numpy())
    finally:
        dist.destroy_process_group()


def test_sharded_loss_matches_single_process():
    world, port = 2, 32741 + os.getpid() % 1000
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    x, lengths, targets = _case()
    xx = x.clone().requires_grad_(True)
    loss = ChainLoss(DEN, 1e-5, avg=True)(xx, lengths, targets)
    loss.backward()
    for r in range(world):
        l, idx, sgx = out[r]
        assert abs(l - float(loss)) <= BAR * abs(float(loss))
        assert np.abs(sgx - xx.grad.numpy()[idx]).max() <= BAR * float(xx.grad.abs().max())


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 23
    for name in ("pychain_hip_post_targets", "pychain_hip_post_targets_workspace_bytes", "pychain_hip_cpu_post_targets",
                 "pychain_hip_topk_rows", "pychain_hip_cpu_topk_rows"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    L = _lib.lib()
    assert L.pychain_hip_post_targets_workspace_bytes(0, 5) == 0 and L.pychain_hip_post_targets_workspace_bytes(4, 0) == 0
    assert 12 * 64 * 1500 + 12 * 64 <= L.pychain_hip_post_targets_workspace_bytes(64, 1500) <= 12 * 64 * 1500 + 12 * 64 + 1024
    import pychain
    assert pychain.PosteriorTargets is PosteriorTargets and pychain.posterior_targets is posterior_targets
    assert pychain.posterior_numerator is posterior_numerator and pychain.occupancies is occupancies
