"""Output L2 and the out-of-range penalty (include/pychain_hip.h: pychain_hip_output_reg) on CPU tensors: the host twin and
output_regularizer against tests/outreg_reference.np_outreg and against torch autograd of the float64 composition;
ChainLoss(output_l2_regularize=, out_of_range_regularize=) equals its own loss without the terms plus the reference term; zero
coefficients are today's call, bit for bit; a 2-rank gloo ShardedChainLoss; ABI 21.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import record_parity
from outreg_reference import LOSS_REL, SUM_REL, grad_bound, np_outreg, term_magnitude, term_rel, worst_ratio
from pychain_amd import ChainLoss, _lib, native, output_regularizer, parallel, synthetic as syn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, OOR = 5e-4, 0.01
D = 40
LENGTHS = torch.tensor([37, 50, 9, 44])                    # ragged, in no order
DEN = syn.make_den_graph(20, 60, D, seed=0)


def _x(B, T, Dx, seed=3):
    """Uniform in +-40 (both signs beyond the clamp), with exact +-30 and a -0.0 in live rows."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, T, Dx, generator=g) * 80.0 - 40.0).float()
    x[0, 0, 0], x[0, 0, Dx - 1], x[0, 0, Dx // 2] = 30.0, -30.0, -0.0
    return x


def _case():
    graphs = syn.make_num_graphs(LENGTHS.tolist(), D, seed=100, max_states=12)
    x = syn.make_input(4, 50, D, seed=5)
    big = _x(4, 50, D)
    x = torch.where(torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.1, big, x)   # a tenth of it far out
    return x, LENGTHS, graphs


def _check_sums(per_seq, totals, ref, l2, oor, scale=1.0):
    R2, RO, _, loss = ref
    assert (np.abs(per_seq[:, 0].astype(np.float64) - R2) <= SUM_REL * R2).all()
    assert (np.abs(per_seq[:, 1].astype(np.float64) - RO) <= SUM_REL * RO).all()
    assert abs(float(totals[1]) - R2.sum()) <= SUM_REL * R2.sum() and abs(float(totals[2]) - RO.sum()) <= SUM_REL * RO.sum()
    assert abs(float(totals[0]) - scale * loss) <= SUM_REL * abs(scale * loss)


@pytest.mark.parametrize("Dx", [1, 7, 40])
def test_host_twin_matches_reference(Dx):
    x = _x(4, 24, Dx)
    lengths = torch.tensor([24, 1, 23, 2])
    x[1, 5, :] = float("nan")                               # beyond the one frame of sequence 1: never read
    ref = np_outreg(x.numpy(), lengths, L2, OOR)
    mag = term_magnitude(x.numpy(), lengths, L2, OOR)
    res = native.cpu_output_reg(x, lengths, L2, OOR, grad_scale=0.25, loss_scale=0.5)
    _check_sums(res.per_seq.numpy(), res.totals.numpy(), ref, L2, OOR, 0.5)
    r_lin = worst_ratio(res.grad.numpy(), 0.25 * ref[2], grad_bound(0.25 * ref[2], mag, 0.25))
    assert r_lin <= 1.0
    for b, L in enumerate(lengths.tolist()):
        assert not bool(res.grad[b, L:].any())
    # ACCUM over a known pattern: live rows get the term, rows beyond the lengths keep their bits
    pat = torch.arange(x.numel(), dtype=torch.float32).reshape(x.shape).mul_(1e-3).sub_(1.0)
    g = pat.clone()
    res2 = native.cpu_output_reg(x, lengths, L2, OOR, grad=g, grad_mode=_lib.GRAD_ACCUM, grad_scale=0.25)
    assert res2.grad is g and torch.equal(res2.per_seq, res.per_seq)
    want = pat.numpy().astype(np.float64) + 0.25 * ref[2]
    r_acc = worst_ratio(g.numpy(), want, grad_bound(want, mag, 0.25))
    assert r_acc <= 1.0
    for b, L in enumerate(lengths.tolist()):
        assert torch.equal(g[b, L:], pat[b, L:])
    # the objective-only form: the same sums, bit for bit
    res3 = native.cpu_output_reg(x, lengths, L2, OOR, with_grad=False)
    assert res3.grad is None and torch.equal(res3.per_seq, res.per_seq)
    record_parity("outreg_cpu_D%d" % Dx, linear=r_lin, accum=r_acc)


def test_output_regularizer_gradient_matches_autograd_of_the_float64_composition():
    x = _x(4, 24, 7, seed=4)
    lengths = torch.tensor([24, 1, 23, 2])
    xx = x.clone().requires_grad_(True)
    out = output_regularizer(xx, lengths, l2=L2, out_of_range=OOR)
    assert out.dim() == 0
    (3.0 * out).backward(retain_graph=True)
    first = xx.grad.clone()
    xx.grad = None
    (3.0 * out).backward()                                   # a second backward over the retained graph evaluates again
    assert torch.equal(xx.grad, first)
    x64 = x.double().clone().requires_grad_(True)
    live = torch.zeros(x.shape[:2], dtype=torch.float64)
    for b, L in enumerate(lengths.tolist()):
        live[b, :L] = 1.0
    comp = (0.5 * L2 * (x64 ** 2) + OOR * (x64.abs() - 30.0).clamp_min(0.0) ** 2) * live[..., None]
    comp = comp.sum()
    comp.backward()
    ref = np_outreg(x.numpy(), lengths, L2, OOR)
    assert abs(float(comp.detach()) - ref[3]) <= 1e-12 * ref[3] and np.abs(x64.grad.numpy() - ref[2]).max() <= 1e-12
    comp = float(comp.detach())
    assert abs(float(out.detach()) - comp) <= SUM_REL * comp
    assert abs(float(out.l2_term) + float(out.out_of_range_term) - comp) <= term_rel(False) * comp    # (un-averaged)
    want = 3.0 * x64.grad.numpy()
    mag = term_magnitude(x.numpy(), lengths, L2, OOR)
    assert worst_ratio(first.numpy(), want, grad_bound(want, mag, 1.0) + 2.0 ** -24 * np.abs(want)) <= 1.0   # (+ the rescale by 3)


def test_a_nan_in_a_live_row_reaches_that_sequence_only():
    x = _x(4, 24, 7, seed=6)
    lengths = torch.tensor([24, 1, 23, 2])
    clean = native.cpu_output_reg(x, lengths, L2, OOR)
    x[2, 3, 5] = float("nan")
    x[0, 4, 1] = float("inf")
    res = native.cpu_output_reg(x, lengths, L2, OOR)
    assert bool(torch.isnan(res.per_seq[2]).all()) and torch.equal(res.per_seq[[1, 3]], clean.per_seq[[1, 3]])
    assert bool(torch.isinf(res.per_seq[0]).all()) and bool(torch.isnan(res.totals[0]))


def _loss(x, lengths, graphs, avg=True, **kw):
    xx = x.clone().requires_grad_(True)
    loss = ChainLoss(DEN, 1e-5, avg=avg, **kw)(xx, lengths, graphs)
    loss.backward()
    out = loss.detach()
    for n in ("l2_term", "out_of_range_term"):
        if hasattr(loss, n):
            setattr(out, n, getattr(loss, n))
    return out, xx.grad


@pytest.mark.parametrize("avg", [True, False])
def test_chain_loss_on_cpu_is_its_own_loss_plus_the_reference_term(avg):
    x, lengths, graphs = _case()
    ref = np_outreg(x.numpy(), lengths, L2, OOR)
    n = float(lengths.sum()) if avg else 1.0
    loss0, g0 = _loss(x, lengths, graphs, avg)
    loss, g = _loss(x, lengths, graphs, avg, output_l2_regularize=L2, out_of_range_regularize=OOR)
    expect = float(loss0) + ref[3] / n
    assert abs(float(loss) - expect) <= LOSS_REL * (abs(float(loss0)) + abs(expect))
    assert abs(float(loss.l2_term) - 0.5 * L2 * ref[0].sum() / n) <= term_rel(avg) * 0.5 * L2 * ref[0].sum() / n
    assert abs(float(loss.out_of_range_term) - OOR * ref[1].sum() / n) <= term_rel(avg) * OOR * ref[1].sum() / n
    want = g0.numpy().astype(np.float64) + ref[2] / n
    mag = term_magnitude(x.numpy(), lengths, L2, OOR)
    # (the loss without the terms reads x through a view of its own, so x receives two gradients - the one without the terms
    # and the term - and x.grad is their sum rounded once: the fp32 bound of the kernel's own ACCUM form holds for this route too)
    bound = grad_bound(want, mag, 1.0 / n)
    r = worst_ratio(g.numpy(), want, bound)
    record_parity("outreg_cpu_loss_avg%d" % avg, grad=r)
    assert r <= 1.0
    for b, L in enumerate(lengths.tolist()):
        assert not bool(g[b, L:].any())


def test_zero_coefficients_are_the_loss_without_the_arguments():
    x, lengths, graphs = _case()
    loss0, g0 = _loss(x, lengths, graphs)
    loss, g = _loss(x, lengths, graphs, output_l2_regularize=0.0, out_of_range_regularize=0.0)
    assert torch.equal(loss.detach(), loss0.detach()) and torch.equal(g, g0) and not hasattr(loss, "l2_term")


def test_negative_coefficients_raise():
    for kw in (dict(output_l2_regularize=-1e-3), dict(out_of_range_regularize=-1.0)):
        with pytest.raises(ValueError):
            ChainLoss(DEN, 1e-5, **kw)
    x = _x(2, 3, 4)
    with pytest.raises(ValueError):
        output_regularizer(x, torch.tensor([3, 2]), l2=-1.0)
    with pytest.raises(ValueError):
        output_regularizer(x, torch.tensor([3, 2]), out_of_range=-1.0)
    # the C ABI: negative coefficients or limit, or a mode that is neither ACCUM nor LINEAR
    per, lc = torch.empty(2, 2), torch.tensor([3, 2])
    for l2, oor, lim, mode in ((-1.0, 0.0, 30.0, _lib.GRAD_LINEAR), (0.0, -1.0, 30.0, _lib.GRAD_LINEAR), (0.0, 0.0, -30.0, _lib.GRAD_LINEAR),
                               (0.0, 0.0, 30.0, _lib.GRAD_LOG), (float("nan"), 0.0, 30.0, _lib.GRAD_LINEAR)):
        rc = _lib.lib().pychain_hip_cpu_output_reg(x.data_ptr(), lc.data_ptr(), 2, 3, 4, l2, oor, lim, mode, None, 1.0, None, None,
                                                   per.data_ptr(), 1.0, None, None, 1)
        assert rc == -1


# ---- a 2-rank gloo ShardedChainLoss equals the one-process loss and gradient (tests/test_parallel.py's pattern) ---------------
def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, lengths, graphs = _case()
        xs, ls, gs, idx = parallel.shard_batch(x, lengths, graphs, world, rank)
        xs = xs.clone().requires_grad_(True)
        crit = parallel.ShardedChainLoss(DEN, 1e-5, avg=True, output_l2_regularize=L2, out_of_range_regularize=OOR)
        loss = crit(xs, ls, gs)
        loss.backward()
        out[rank] = (float(loss), idx.tolist(), xs.grad.numpy())
    finally:
        dist.destroy_process_group()


def test_sharded_loss_matches_single_process():
    world, port = 2, 31731 + os.getpid() % 1000
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    x, lengths, graphs = _case()
    loss, gx = _loss(x, lengths, graphs, output_l2_regularize=L2, out_of_range_regularize=OOR)
    loss0, _ = _loss(x, lengths, graphs)
    assert abs(float(loss) - float(loss0)) > 1e-3 * abs(float(loss0))          # (the terms are there to be seen)
    for r in range(world):
        l, idx, sgx = out[r]
        assert abs(l - float(loss)) <= 1e-5 * abs(float(loss))
        np.testing.assert_allclose(sgx, gx.numpy()[idx], rtol=1e-5, atol=1e-7)


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 21
    for name in ("pychain_hip_output_reg", "pychain_hip_output_reg_workspace_bytes", "pychain_hip_cpu_output_reg"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    L = _lib.lib()
    assert L.pychain_hip_output_reg_workspace_bytes(0, 5) == 0 and L.pychain_hip_output_reg_workspace_bytes(4, 0) == 0
    assert 16 * 64 * 1500 + 16 * 64 <= L.pychain_hip_output_reg_workspace_bytes(64, 1500) <= 16 * 64 * 1500 + 16 * 64 + 512
    import pychain
    assert pychain.output_regularizer is output_regularizer


def test_header_compiles_as_c(tmp_path):
    # gcc, or the C compiler of the ROCm toolchain the library itself is built with: one of them is always here
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("gcc") or shutil.which("cc") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cc is not None, "no C compiler: neither gcc nor cc on PATH, nor %s" % rocm_clang
    src = tmp_path / "h.c"
    src.write_text('#include "pychain_hip.h"\n'
                   'static size_t (*ws)(int, int) = pychain_hip_output_reg_workspace_bytes;\n'
                   'static int (*dev)(const void*, int, const int64_t*, int, int, int, float, float, float, int, void*, float, const float*,\n'
                   '                  const float*, float*, float, float*, float*, void*, size_t, void*) = pychain_hip_output_reg;\n'
                   'static int (*host)(const float*, const int64_t*, int, int, int, float, float, float, int, float*, float, const float*,\n'
                   '                   const float*, float*, float, float*, float*, int) = pychain_hip_cpu_output_reg;\n'
                   'int main(void) { return ws == 0 || dev == 0 || host == 0 || PYCHAIN_HIP_ABI_VERSION < 21; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True, text=True)
