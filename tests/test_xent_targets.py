"""Cross-entropy against sparse targets (include/pychain_hip.h: pychain_hip_xent_targets, ABI 24) on CPU tensors: the host twin
against tests/xent_targets_reference on the inputs the GPU tests use; posterior_xent and PosteriorTargets.from_alignment against
the torch composition; ChainLoss(..., xent_output=z, xent_targets=t) on the unfused route against the composition, with
regularisers and weights; ShardedChainLoss in a world of one; ABI 24.  No GPU.  Bounds: xent_targets_reference's - the case's
own fp32 distance + 1e-5 for the twin, the library's fp64 bar (1e-5) for the comparisons with the fp64 composition."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import post_reference as pr
import xent_targets_reference as xr
from helpers import record_parity
from pychain_amd import (ChainGraphBatch, ChainLoss, PosteriorTargets, _lib, native, parallel, posterior_targets, posterior_xent,
                         synthetic as syn, viterbi_align)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = xr.BAR
D = 40
LENGTHS = torch.tensor([37, 40, 9, 33])
DEN = syn.make_den_graph(20, 60, D, seed=0)
L2, OOR = 5e-4, 0.01
C = 0.1
DS, KS = [1, 3, 8, 257], [1, 3, 8, 33]


# ---- the host twin against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("Dx", DS)
def test_host_twin_matches_reference(Dx, K):
    z, lengths, pdfs, probs = pr.native_case(Dx, K)
    ref = xr.np_xent_targets(z.numpy(), lengths, pdfs.numpy(), probs.numpy())
    assert ref[2] == 1 and not ref[3][0, 1]                            # one bad entry; a live frame without entries
    own = xr.fp32_distance(z, lengths, pdfs, probs, ref)
    bo, bg = xr.bound(own)
    res, bad = native.cpu_xent_targets(z, lengths, pdfs, probs)
    assert int(bad) == 1
    g = res.grad.numpy()
    for b, L in enumerate(lengths.tolist()):
        assert not g[b, L:].any()                                      # zeros beyond a length (the padding of z is NaN)
    assert not g[0, 1].any()
    d = xr.distances(res.objf.numpy(), g, ref)
    print("D%d K%d: objective %.3e (bound %.3e) gradient %.3e (bound %.3e)" % (Dx, K, d[0], bo, d[1], bg))
    record_parity("xent_targets_cpu_D%d_K%d" % (Dx, K), fp32_objf=own[0], fp32_grad=own[1], objf_rel=d[0], grad_rel=d[1])
    assert d[0] <= bo and d[1] <= bg, (d, bo, bg)
    # the form without the store: the same objectives; the scale: grad_scale * grad_scale_dev / norm
    res0, _ = native.cpu_xent_targets(z, lengths, pdfs, probs, with_grad=False)
    assert res0.grad is None and torch.equal(res0.objf, res.objf)
    res2, _ = native.cpu_xent_targets(z, lengths, pdfs, probs, grad_scale=-0.25, grad_scale_dev=1.5, norm=7.0)
    s = float(pr.f32_scale(-0.25, 1.5, 7.0))
    d2 = xr.distances(res2.objf.numpy(), res2.grad.numpy() / s, ref)
    assert torch.equal(res2.objf, res.objf) and d2[1] <= bg, d2


def test_a_frame_without_entries_does_not_read_its_row():
    z, lengths, pdfs, probs = pr.native_case(8, 3)
    clean, _ = native.cpu_xent_targets(z, lengths, pdfs, probs)
    z[0, 1, :] = float("nan")
    res, _ = native.cpu_xent_targets(z, lengths, pdfs, probs)
    assert torch.equal(res.objf, clean.objf) and torch.equal(res.grad, clean.grad) and not bool(res.grad[0, 1].any())


def test_a_nan_in_a_read_row_reaches_that_sequence_only():
    z, lengths, pdfs, probs = pr.native_case(8, 3)
    pdfs[2, 1, 0] = 3
    clean, _ = native.cpu_xent_targets(z, lengths, pdfs, probs)
    z[2, 1, 5] = float("nan")                                          # (not an addressed element: the log-sum-exp meets it)
    res, _ = native.cpu_xent_targets(z, lengths, pdfs, probs)
    assert bool(torch.isnan(res.objf[2])) and torch.equal(res.objf[:2], clean.objf[:2])
    assert torch.equal(res.grad[:2], clean.grad[:2]) and bool(torch.isnan(res.grad[2, 1]).all())
    assert not bool(torch.isnan(res.grad[2, 0]).any())


# ---- through the Python interface ------------------------------------------------------------------------------------------------
def _case(k=6, seed=5):
    x = syn.make_input(4, 40, D, seed=seed)
    teacher = syn.make_input(4, 40, D, seed=seed + 50) * 1.5
    targets = posterior_targets(teacher, LENGTHS, DEN, k)
    z = syn.make_input(4, 40, D, seed=seed + 70) * 1.5
    return x, z, LENGTHS, targets


def test_posterior_xent_matches_the_fp64_composition():
    _, z, lengths, targets = _case()
    zz = z.clone().requires_grad_(True)
    out = posterior_xent(zz, lengths, targets)
    assert out.dim() == 0 and tuple(out.xent_objf_per_seq.shape) == (4,) and int(out.bad_count) == 0
    (2.0 * out).backward(retain_graph=True)
    first = zz.grad.clone()
    zz.grad = None
    (2.0 * out).backward()                                             # a second backward over the retained graph evaluates again
    assert torch.equal(zz.grad, first)
    z64 = z.double().clone().requires_grad_(True)
    per = xr.torch_xent_per_seq(z64, lengths, targets.pdfs, targets.probs)
    (2.0 * per.sum()).backward()
    d = pr.distances(out.detach(), first.numpy(), float(per.detach().sum()), z64.grad.numpy())
    assert np.abs(out.xent_objf_per_seq.numpy() - per.detach().numpy()).max() <= BAR * np.abs(per.detach().numpy()).max()
    record_parity("xent_targets_cpu_posterior_xent", loss=d[0], grad=d[1])
    assert max(d) <= BAR, d
    with pytest.raises(RuntimeError):                                  # an edit in place between the two backward calls
        out2 = posterior_xent(zz, lengths, targets)
        out2.backward(retain_graph=True)
        with torch.no_grad():
            zz.add_(1.0)
        out2.backward()
    with pytest.raises(ValueError):
        posterior_xent(z, lengths, (targets.pdfs, targets.probs))
    zg = posterior_xent(z, lengths, targets)                           # no gradient wanted: the form without the store
    assert torch.equal(zg, out.detach())


def test_from_alignment_is_frame_cross_entropy():
    lengths = LENGTHS
    graphs = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=20)
    x, z, _, _ = _case()
    ali = viterbi_align(x, lengths, graphs)
    assert bool(ali.ok.all())
    ali = ali._replace(ok=torch.tensor([True, True, False, True]))     # an utterance that did not align: no targets
    t = PosteriorTargets.from_alignment(ali)
    assert tuple(t.pdfs.shape) == (4, 40, 1) and t.pdfs.dtype == torch.int32 and bool((t.probs == 1).all())
    assert bool((t.pdfs[2] == -1).all()) and bool((t.pdfs[0, 37:] == -1).all()) and bool((t.pdfs[0, :37, 0] == ali.pdfs[0, :37]).all())
    zz = z.clone().requires_grad_(True)
    out = posterior_xent(zz, lengths, t)
    out.backward()
    z64 = z.double().clone().requires_grad_(True)
    ce = -F.cross_entropy(z64.reshape(-1, D), t.pdfs.reshape(-1).to(torch.int64), ignore_index=-1, reduction="sum")
    ce.backward()
    d = pr.distances(out.detach(), zz.grad.numpy(), float(ce.detach()), z64.grad.numpy())
    assert max(d) <= BAR, d
    assert not bool(zz.grad[2].any())


def _composition(x, z, lengths, targets, avg, u=None, f=None, reg=None, c=C):
    """(loss, d loss / dx, d loss / dz) by the torch composition: post_reference.composition for the LF-MMI part, the fp64
    log_softmax + gather for the xent term, the weights applied to the rows and to the per-sequence terms."""
    value, gx = pr.composition(DEN, x, lengths, targets, avg, u, f, reg)
    B, T = x.size(0), x.size(1)
    z64 = z.detach().double().clone().requires_grad_(True)
    per = xr.torch_xent_per_seq(z64, lengths, targets.pdfs, targets.probs)
    per.sum().backward()
    ud = torch.ones(B, dtype=torch.float64) if u is None else u.double()
    n = float((ud * lengths).sum()) if avg else 1.0
    w = ud[:, None] * (torch.ones(B, T, dtype=torch.float64) if f is None else f.double())
    gz = -c * z64.grad * w[..., None] / n
    xent = float(torch.where(ud != 0, ud * per.detach(), torch.zeros(())).sum()) / n
    return value - c * xent, gx, gz.numpy(), xent


@pytest.mark.parametrize("avg", [True, False])
def test_chain_loss_on_cpu_matches_the_torch_composition(avg):
    x, z, lengths, targets = _case()
    far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.05
    x = torch.where(far, torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0, x)
    u = torch.tensor([1.0, 0.5, 0.0, 2.0])
    f = (torch.rand(4, 40, generator=torch.Generator().manual_seed(3)) * 1.5).float()
    f[0, :5], f[1, 3] = 1.0, 0.0
    for name, kw, reg in (("plain", {}, None), ("weights_reg", dict(utt_weights=u, deriv_weights=f), (L2, OOR))):
        xx, zz = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
        crit = ChainLoss(DEN, 1e-5, avg=avg, xent_regularize=C, output_l2_regularize=reg[0] if reg else 0.0,
                         out_of_range_regularize=reg[1] if reg else 0.0)
        loss = crit(xx, lengths, targets, xent_output=zz, xent_targets=targets, **kw)
        loss.backward(retain_graph=True)
        gx, gz = xx.grad.clone(), zz.grad.clone()
        xx.grad = zz.grad = None
        loss.backward()                                                # a second backward
        assert torch.equal(xx.grad, gx) and torch.equal(zz.grad, gz)
        want, wgx, wgz, wxent = _composition(x, z, lengths, targets, avg, kw.get("utt_weights"), kw.get("deriv_weights"), reg)
        d = pr.distances(loss.detach(), gx.numpy(), want, wgx)
        dz = float(np.abs(gz.numpy() - wgz).max() / np.abs(wgz).max())
        dxe = abs(float(loss.xent_objf) - wxent) / abs(wxent)
        record_parity("xent_targets_cpu_loss_%s_avg%d" % (name, avg), loss=d[0], grad=d[1], zgrad=dz, xent=dxe)
        assert max(d) <= BAR and dz <= BAR and dxe <= BAR, (d, dz, dxe)
        assert len(loss.bad_count) == 3                                # denominator, targets, xent targets
        # nothing flows back to the chain output through the term
        x2 = x.clone().requires_grad_(True)
        crit(x2, lengths, targets, **kw).backward()
        assert torch.equal(x2.grad, gx)


def test_xent_targets_argument_rules():
    x, z, lengths, targets = _case()
    graphs = syn.make_num_graphs(lengths.tolist(), D, seed=100, max_states=20)
    crit = ChainLoss(DEN, 1e-5, xent_regularize=C)
    with pytest.raises(ValueError):
        crit(x, lengths, graphs, xent_output=z, xent_targets=targets)  # graph numerators bring their own posteriors
    with pytest.raises(ValueError):
        crit(x, lengths, targets, xent_output=z)                       # (as before: no targets for the term)
    with pytest.raises(ValueError):
        crit(x, lengths, targets, xent_output=z, xent_targets=(targets.pdfs, targets.probs))
    with pytest.raises(ValueError):
        crit(x, lengths, targets, xent_output=z[:, :, :30], xent_targets=targets)
    # c == 0, or no xent_output: the call without the term, bit for bit
    for crit0, kw in ((ChainLoss(DEN, 1e-5, xent_regularize=0.0), dict(xent_output=z, xent_targets=targets)),
                      (crit, dict(xent_targets=targets))):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a = crit0(xa, lengths, targets, **kw)
        b = ChainLoss(DEN, 1e-5)(xb, lengths, targets)
        a.backward()
        b.backward()
        assert torch.equal(a, b) and torch.equal(xa.grad, xb.grad) and not hasattr(a, "xent_objf") and len(a.bad_count) == 2


def test_sharded_loss_in_a_world_of_one_equals_chain_loss():
    x, z, lengths, targets = _case()
    out = []
    for cls in (ChainLoss, parallel.ShardedChainLoss):
        xx, zz = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
        loss = cls(DEN, 1e-5, avg=True, xent_regularize=C)(xx, lengths, targets, xent_output=zz, xent_targets=targets)
        loss.backward()
        out.append((loss.detach(), xx.grad, zz.grad))
    (la, xa, za), (lb, xb, zb) = out
    assert abs(float(la) - float(lb)) <= BAR * abs(float(la))
    assert float((xa - xb).abs().max()) <= BAR * float(xa.abs().max()) and float((za - zb).abs().max()) <= BAR * float(za.abs().max())


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 24
    for name in ("pychain_hip_xent_targets", "pychain_hip_xent_targets_workspace_bytes", "pychain_hip_xent_add_totals",
                 "pychain_hip_cpu_xent_targets"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    L = _lib.lib()
    assert L.pychain_hip_xent_targets_workspace_bytes(0, 5) == 0 and L.pychain_hip_xent_targets_workspace_bytes(4, 0) == 0
    assert 12 * 64 * 1500 + 4 * 64 <= L.pychain_hip_xent_targets_workspace_bytes(64, 1500) <= 12 * 64 * 1500 + 4 * 64 + 1280
    z, lc = torch.rand(2, 3, 4), torch.tensor([3, 2])
    pd, q = torch.zeros(2, 3, 5, dtype=torch.int32), torch.ones(2, 3, 5)
    objf, badc = torch.empty(2), torch.zeros(1, dtype=torch.int32)
    call = lambda k, zp: L.pychain_hip_cpu_xent_targets(zp, lc.data_ptr(), 2, 3, 4, pd.data_ptr(), q.data_ptr(), k, None, 1.0, None, None,
                                                        objf.data_ptr(), badc.data_ptr(), 1)
    assert call(0, z.data_ptr()) == -1 and call(5, None) == -1 and call(5, z.data_ptr()) == 0
    import pychain
    assert pychain.posterior_xent is posterior_xent and pychain.PosteriorTargets.from_alignment


def test_header_compiles_as_c(tmp_path):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("gcc") or shutil.which("cc") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cc is not None, "no C compiler: neither gcc nor cc on PATH, nor %s" % rocm_clang
    src = tmp_path / "h.c"
    src.write_text('#include "pychain_hip.h"\n'
                   'static size_t (*ws)(int, int) = pychain_hip_xent_targets_workspace_bytes;\n'
                   'static int (*dev)(const void*, int, const int64_t*, int, int, int, const int32_t*, const float*, int, void*, float,\n'
                   '                  const float*, const float*, float*, int32_t*, void*, size_t, void*) = pychain_hip_xent_targets;\n'
                   'static int (*tot)(const float*, int, float, const float*, float, float*, float*, const int32_t*, void*) =\n'
                   '    pychain_hip_xent_add_totals;\n'
                   'static int (*host)(const float*, const int64_t*, int, int, int, const int32_t*, const float*, int, float*, float,\n'
                   '                   const float*, const float*, float*, int32_t*, int) = pychain_hip_cpu_xent_targets;\n'
                   'int main(void) { return ws == 0 || dev == 0 || tot == 0 || host == 0 || PYCHAIN_HIP_ABI_VERSION < 24; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True, text=True)
