"""Utterance weights and per-frame derivative weights (include/pychain_hip.h: pychain_hip_weight_rows) on CPU tensors: the host
twin against tests/weights_reference.np_weight_rows bit for bit, ChainLoss(...)(x, lengths, graphs, utt_weights=, deriv_weights=)
against its own unweighted call, integer weights against a batch that lists the utterance twice, an utterance of weight zero
whose objectives are not finite, validation, a gloo ShardedChainLoss; ABI 22.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pychain_amd import ChainGraphBatch, ChainLoss, _lib, native, parallel, synthetic as syn, weight_rows
from weights_reference import LOSS_REL, SUM_REL, TERM_REL, draw_weights, np_weight_rows, np_weighted_sums, row_weights, same_bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 3, 7
LENGTHS = torch.tensor([7, 4, 1])
D = 8
DEN = syn.make_den_graph(10, 30, D, seed=0)


def _pattern(shape):
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 251.0) * 0.01 - 1.0).reshape(shape)


@pytest.mark.parametrize("which", ["u", "f", "both"])
@pytest.mark.parametrize("Dx", [1, 3, 4, 7, 8])
def test_host_twin_equals_the_reference_bit_for_bit(Dx, which):
    u, f = draw_weights(B, T, 11 + Dx, which)
    g0 = _pattern((B, T, Dx))
    g0[1, 5, :] = float("nan")                               # beyond the four frames of sequence 1: never touched
    g = g0.clone()
    assert native.cpu_weight_rows(g, LENGTHS, u, f) is None
    assert same_bits(g, np_weight_rows(g0, LENGTHS, u, f))
    w = row_weights(B, T, u, f)
    assert (w[0, :7] != 1).any() and bool(torch.isnan(g[1, 5]).all())


def _case(lengths=LENGTHS, seed=5):
    graphs = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=8)
    return syn.make_input(len(lengths), int(lengths.max()), D, seed=seed), lengths, graphs


def _run(x, lengths, graphs, avg=False, crit_kw=None, z=None, **kw):
    xx = x.clone().requires_grad_(True)
    zz = None if z is None else z.clone().requires_grad_(True)
    loss = ChainLoss(DEN, 1e-5, avg=avg, **(crit_kw or {}))(xx, lengths, graphs, xent_output=zz, **kw)
    loss.backward()
    return loss, xx.grad, None if zz is None else zz.grad


def _per_seq(x, lengths, graphs):
    """the unweighted call's per-sequence objectives: (den [B], num [B]) of the two host twins"""
    den = native.cpu_forward_backward(ChainGraphBatch(DEN, x.size(0)), x, lengths, 1e-5)[0]
    num = native.cpu_forward_backward(graphs, x, lengths)[0]
    return den.numpy(), num.numpy()


@pytest.mark.parametrize("which", ["u", "f", "both"])
def test_chain_loss_on_cpu_tensors(which):
    x, lengths, graphs = _case()
    u, f = draw_weights(B, T, 3, which)
    if u is not None:
        u[2] = 0.3                                           # (no dropped utterance here: every objective is finite anyway)
    loss0, g0, _ = _run(x, lengths, graphs)
    loss, g, _ = _run(x, lengths, graphs, utt_weights=u, deriv_weights=f)
    assert same_bits(g, np_weight_rows(g0, lengths, u, f))   # fl32(w * the gradient of the same call without weights)
    den, num = _per_seq(x, lengths, graphs)
    ref = np_weighted_sums(u, lengths, den, num)
    print("loss %r, fp64 weighted sum %r" % (float(loss.detach()), ref["value"]))
    assert abs(float(loss.detach()) - ref["value"]) <= LOSS_REL * ref["mag"]
    assert abs(float(loss.weighted_frames) - ref["sl"]) <= SUM_REL * ref["sl"]
    if u is None:
        assert torch.equal(loss.detach(), loss0.detach())    # derivative weights change no sum
    assert loss.totals is None


def test_integer_weights_are_the_utterance_listed_twice():
    lengths = torch.tensor([7, 4, 1])
    twice = torch.tensor([7, 7, 4, 1])
    graphs2 = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=8)
    x = syn.make_input(3, 7, D, seed=5)
    graphs = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=8)
    idx = torch.tensor([0, 0, 1, 2])
    x2 = x.index_select(0, idx)
    g4 = ChainGraphBatch.__new__(ChainGraphBatch)
    g4.__dict__.update(graphs2.__dict__)
    g4._device_cache = {}
    g4.reorder(idx)
    g4.batch_size = 4
    loss2, gx2, _ = _run(x2, twice, g4, avg=True)
    loss, gx, _ = _run(x, lengths, graphs, avg=True, utt_weights=torch.tensor([2, 1, 1]))       # (integers: converted)
    den, num = _per_seq(x2, twice, g4)
    mag = float(np.abs(den).sum() + np.abs(num).sum()) / float(twice.sum())
    print("weighted %r, listed twice %r" % (float(loss.detach()), float(loss2.detach())))
    assert abs(float(loss.detach()) - float(loss2.detach())) <= LOSS_REL * mag
    assert same_bits(gx2[0], gx2[1]) and same_bits(gx[0], 2.0 * gx2[0])     # (the host twins evaluate each sequence on its own)
    assert same_bits(gx[1:], gx2[2:])
    assert float(loss.weighted_frames) == float(twice.sum())


def test_weight_zero_utterance_with_objectives_that_are_not_finite():
    u = torch.tensor([0.5, 0.0, 2.0, 0.0])
    lengths = torch.tensor([5, 3, 2, 4])
    den = torch.tensor([10.0, float("-inf"), -3.0, 1.0])
    num = torch.tensor([4.0, 2.0, -5.0, float("nan")])
    xent = torch.tensor([-7.0, float("nan"), -1.0, float("-inf")])
    reg = torch.tensor([[3.0, 1.0], [float("inf"), 2.0], [5.0, 0.5], [float("nan"), float("nan")]])
    totals = torch.arange(8, dtype=torch.float32) + 0.5
    w = native.cpu_weight_rows(None, lengths, u, None, shape=(4, 5, 2), den_objf=den, num_objf=num, xent_objf=xent, xent_coef=-0.1,
                               reg_per_seq=reg, l2=0.2, oor=0.3, loss_scale=0.25, norm=torch.tensor([4.0]), totals=totals)
    ref = np_weighted_sums(u, lengths, den.numpy(), num.numpy(), xent.numpy(), 0.1, reg.numpy(), 0.2, 0.3)
    assert bool(torch.isfinite(totals).all()) and bool(torch.isfinite(w).all())
    for got, want in zip(w.tolist(), (ref["lf"], ref["sx"], ref["s2"], ref["so"], ref["sl"])):
        assert abs(got - want) <= SUM_REL * abs(want)
    full = 0.25 * ref["value"] / 4.0
    assert abs(float(totals[0]) - full) <= LOSS_REL * 0.25 * ref["mag"] / 4.0 and float(totals[0]) == float(totals[4])
    assert float(totals[1]) == ref["sl"] == 6.5 and abs(float(totals[3]) - ref["lf"]) <= SUM_REL * abs(ref["lf"])
    assert totals[[2, 5, 6, 7]].tolist() == [2.5, 5.5, 6.5, 7.5]
    # through ChainLoss: a dropped utterance's rows are zeros, the others' are the weighted rows, the loss is the others' sum
    x, lengths, graphs = _case()
    _, g0, _ = _run(x, lengths, graphs)
    loss, g, _ = _run(x, lengths, graphs, utt_weights=torch.tensor([1.0, 0.0, 1.0]))
    dn, nm = _per_seq(x, lengths, graphs)
    want = float(dn[0]) - float(nm[0]) + float(dn[2]) - float(nm[2])
    assert not bool(g[1].any()) and same_bits(g[[0, 2]], g0[[0, 2]])
    assert abs(float(loss.detach()) - want) <= LOSS_REL * float(np.abs(dn[[0, 2]]).sum() + np.abs(nm[[0, 2]]).sum())


def test_derivative_weights_change_no_sum():
    x, lengths, graphs = _case()
    f = torch.ones(B, T)
    f[:, 0] = 0.0
    f[0, 6] = 0.0
    for avg in (False, True):
        loss0, g0, _ = _run(x, lengths, graphs, avg=avg)
        loss, g, _ = _run(x, lengths, graphs, avg=avg, deriv_weights=f)
        assert torch.equal(loss.detach(), loss0.detach())
        assert float(loss.weighted_frames) == float(lengths.sum())
        assert not bool(g[:, 0].any()) and not bool(g[0, 6].any()) and same_bits(g[:, 1:6], g0[:, 1:6])
    # the native level, derivative weights only: with the totals given the sums are those of u = 1 - totals[1] is the frame
    # count exactly, [2] and [5..7] keep their bits -, and a NaN in a zero-weight row is gone
    totals = torch.arange(8, dtype=torch.float32) + 0.5
    g = torch.full((B, T, 3), float("nan"))
    den, num = torch.tensor([10.0, -3.5, 2.0]), torch.tensor([4.0, 2.25, -1.0])
    w = native.cpu_weight_rows(g, lengths, None, torch.zeros(B, T), den_objf=den, num_objf=num, totals=totals)
    assert float(totals[1]) == float(w[4]) == float(lengths.sum()) and totals[[2, 5, 6, 7]].tolist() == [2.5, 5.5, 6.5, 7.5]
    assert float(totals[0]) == float(totals[3]) == float(totals[4]) == float(w[0]) == 6.0 - 5.75 + 3.0
    for b, L in enumerate(lengths.tolist()):
        assert not bool(g[b, :L].any()) and bool(torch.isnan(g[b, L:]).all())


def test_xent_branch_and_regularisers_are_weighted():
    x, lengths, graphs = _case()
    z = syn.make_input(B, T, D, seed=77) * 1.5
    u, f = draw_weights(B, T, 3, "both")
    u[2] = 0.3
    kw = dict(xent_regularize=0.1, output_l2_regularize=5e-4, out_of_range_regularize=0.01)
    loss0, g0, gz0 = _run(x, lengths, graphs, crit_kw=kw, z=z)
    loss, g, gz = _run(x, lengths, graphs, crit_kw=kw, z=z, utt_weights=u, deriv_weights=f)
    assert same_bits(g, np_weight_rows(g0, lengths, u, f)) and same_bits(gz, np_weight_rows(gz0, lengths, u, f))
    den, num = _per_seq(x, lengths, graphs)
    xent = native.cpu_num_xent(graphs, x, lengths, z, with_grad=False).objf.numpy()
    reg = native.cpu_output_reg(x, lengths, 5e-4, 0.01, with_grad=False).per_seq.numpy()
    ref = np_weighted_sums(u, lengths, den, num, xent, 0.1, reg, 5e-4, 0.01)
    assert abs(float(loss.detach()) - ref["value"]) <= LOSS_REL * ref["mag"]
    assert abs(float(loss.xent_objf) - ref["sx"]) <= SUM_REL * abs(ref["sx"])
    assert abs(float(loss.l2_term) - 0.5 * 5e-4 * ref["s2"]) <= TERM_REL * 0.5 * 5e-4 * ref["s2"]
    assert abs(float(loss.out_of_range_term) - 0.01 * ref["so"]) <= TERM_REL * 0.01 * ref["so"]


def test_weight_rows_is_identity_with_a_scaled_backward():
    x = _pattern((B, T, 5)).requires_grad_(True)
    u, f = draw_weights(B, T, 9, "both")
    y = weight_rows(x, (u, f), LENGTHS)
    assert torch.equal(y.detach(), x.detach())
    up = _pattern((B, T, 5)) * 0.5 + 0.3
    y.backward(up)
    assert same_bits(x.grad, np_weight_rows(up, LENGTHS, u, f))
    x.grad = None
    weight_rows(x, u).sum().backward()                       # a [B] tensor: utterance weights, every frame live
    assert same_bits(x.grad, np_weight_rows(torch.ones(B, T, 5), [T] * B, u, None))


def test_validation_errors():
    x, lengths, graphs = _case()
    crit = ChainLoss(DEN, 1e-5, avg=True)
    for kw in (dict(utt_weights=torch.ones(B + 1)), dict(deriv_weights=torch.ones(B, T + 1)), dict(deriv_weights=torch.ones(B)),
               dict(utt_weights=torch.tensor([1.0, -1.0, 1.0])), dict(utt_weights=torch.tensor([1.0, float("nan"), 1.0])),
               dict(deriv_weights=torch.full((B, T), float("inf"))), dict(deriv_weights=-torch.ones(B, T)),
               dict(utt_weights=torch.zeros(B))):
        with pytest.raises(ValueError):
            crit(x, lengths, graphs, **kw)
    ChainLoss(DEN, 1e-5, avg=False)(x, lengths, graphs, utt_weights=torch.zeros(B))      # (all zero without avg: a zero loss)
    with pytest.raises(ValueError):
        weight_rows(x, torch.ones(B + 2))
    # the C ABI: no weights at all, bad sizes, sums without the objectives
    g, lc, u = torch.zeros(B, T, D), lengths.to(torch.int64), torch.ones(B)
    L = _lib.lib()
    call = lambda grad, uu, bb, den, tot: L.pychain_hip_cpu_weight_rows(grad, lc.data_ptr(), bb, T, D, uu, None, den, None, None, 0.0, None,
                                                                        0.0, 0.0, 1.0, None, tot, None, 1)
    tot = torch.zeros(8)
    assert call(g.data_ptr(), None, B, None, None) == -1 and call(g.data_ptr(), u.data_ptr(), 0, None, None) == -1
    assert call(None, u.data_ptr(), B, None, None) == -1 and call(None, u.data_ptr(), B, None, tot.data_ptr()) == -1
    assert call(g.data_ptr(), u.data_ptr(), B, None, None) == 0


# ---- a gloo ShardedChainLoss with weights equals the one-process weighted loss (tests/test_outreg.py's pattern) ---------------
S_LENGTHS = torch.tensor([7, 4, 1, 6])


def _sharded_case():
    x, lengths, graphs = _case(S_LENGTHS)
    u = torch.tensor([0.5, 3.0, 0.3, 1.0])
    f = torch.ones(4, 7)
    f[:, 0] = 0.0
    return x, lengths, graphs, u, f


def test_sharded_loss_refuses_all_zero_weights_in_a_world_of_one():
    x, lengths, graphs = _case()
    with pytest.raises(ValueError):
        parallel.ShardedChainLoss(DEN, 1e-5, avg=True)(x, lengths, graphs, utt_weights=torch.zeros(B))
    parallel.ShardedChainLoss(DEN, 1e-5, avg=False)(x, lengths, graphs, utt_weights=torch.zeros(B))


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, lengths, graphs, u, f = _sharded_case()
        xs, ls, gs, idx = parallel.shard_batch(x, lengths, graphs, world, rank)
        xs = xs.clone().requires_grad_(True)
        crit = parallel.ShardedChainLoss(DEN, 1e-5, avg=True)
        loss = crit(xs, ls, gs, utt_weights=u[idx], deriv_weights=f[idx])
        loss.backward()
        out[rank] = (float(loss), idx.tolist(), xs.grad.numpy(), float(crit.last_stats[1]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_loss_matches_single_process(world):
    port = 32741 + os.getpid() % 1000 + world
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    x, lengths, graphs, u, f = _sharded_case()
    loss, gx, _ = _run(x, lengths, graphs, avg=True, utt_weights=u, deriv_weights=f)
    loss0, _, _ = _run(x, lengths, graphs, avg=True)
    assert abs(float(loss.detach()) - float(loss0.detach())) > 1e-3 * abs(float(loss0.detach()))          # (the weights are there to be seen)
    for r in range(world):
        l, idx, sgx, frames = out[r]
        assert abs(l - float(loss)) <= 1e-5 * abs(float(loss))
        assert abs(frames - float((u * lengths).sum())) <= 1e-5 * frames
        np.testing.assert_allclose(sgx, gx.numpy()[idx], rtol=1e-5, atol=1e-7)


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as fh:
        header = fh.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 22
    for name in ("pychain_hip_weight_rows", "pychain_hip_cpu_weight_rows"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    import pychain
    assert pychain.weight_rows is weight_rows


def test_header_compiles_as_c(tmp_path):
    # gcc, or the C compiler of the ROCm toolchain the library itself is built with: one of them is always here
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("gcc") or shutil.which("cc") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cc is not None, "no C compiler: neither gcc nor cc on PATH, nor %s" % rocm_clang
    src = tmp_path / "h.c"
    src.write_text('#include "pychain_hip.h"\n'
                   'static int (*dev)(void*, int, const int64_t*, int, int, int, const float*, const float*, const float*, const float*,\n'
                   '                  const float*, float, const float*, float, float, float, const float*, float*, float*, void*)\n'
                   '    = pychain_hip_weight_rows;\n'
                   'static int (*host)(float*, const int64_t*, int, int, int, const float*, const float*, const float*, const float*,\n'
                   '                   const float*, float, const float*, float, float, float, const float*, float*, float*, int)\n'
                   '    = pychain_hip_cpu_weight_rows;\n'
                   'int main(void) { return dev == 0 || host == 0 || PYCHAIN_HIP_ABI_VERSION < 22; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True, text=True)
