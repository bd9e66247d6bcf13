"""Expected arc counts (include/pychain_hip.h: pychain_hip_den_arc_counts) on CPU tensors: the host twin against
the fp64 recursions of tests/arc_counts_reference and against torch autograd of log Z; the planted faults; sum_k c(b,k) = L_b; the
counts scattered by pdf equal the gradient summed over time; w = 0 is w = None; utterance weights; finite differences of
den_log_partition in w; the refusals; ABI 30.  No GPU.

Tolerance (arc_counts_reference.reference; the rule of smbr_reference.bound): 1e-5 on max |d counts| / max |counts|, on
max |d grad| / max |grad| and on the relative log Z_b, or twice the fp32 restatement's own distance where that is beyond 5e-6."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import arc_counts_reference as ar
from helpers import record_parity
from pychain_amd import ArcCounts, ChainGraphBatch, _lib, den_log_partition, expected_arc_counts, native, synthetic as syn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WKINDS = (None, "normal")


def _twin(name, coef, wkind=None, u=None, w=None, y=None):
    g, y0, lengths = ar.case(name)
    w = ar.weights(name, wkind) if w is None else w
    gt = native.smbr_graph(g, y0.size(2), torch.device("cpu"))
    return native.cpu_den_arc_counts(gt, g.num_states, y0 if y is None else y, lengths, coef, w, u, per_seq=True)


def _triple(r):
    return r[0].numpy(), r[2].numpy(), r[3].double().numpy()


@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("coef", ar.COEFS)
@pytest.mark.parametrize("name", ar.CASES)
def test_host_twin_against_fp64(name, coef, wkind):
    ref, (bound, d32) = ar.reference(name, coef, wkind)
    calls = _lib.lib().pychain_hip_cpu_calls()
    r = _twin(name, coef, wkind)
    assert _lib.lib().pychain_hip_cpu_calls() == calls + 1
    dc, dg, dz = ar.distances(_triple(r), ref)
    print("%s c=%g w=%s: counts %.3g grad %.3g logZ %.3g (fp32 restatement %.3g, bound %.3g)" % (name, coef, wkind, dc, dg, dz, d32, bound))
    record_parity("arc_counts_twin_%s_c%g_w%s" % (name, coef, wkind), counts=dc, grad=dg, logz=dz, f32_reference=d32, bound=bound)
    assert dc <= bound and dg <= bound and dz <= bound and r[4].tolist() == [0, 0]
    lengths = ar.case(name)[2]
    cps = r[2].numpy()
    assert np.abs(cps.sum(1) - lengths.numpy()).max() <= bound * float(lengths.max())          # sum_k c(b,k) = L_b
    assert ar.dist(r[1].numpy(), cps.sum(0)) <= 1e-12                                            # counts = the sum over sequences
    # the counts scattered by pdf equal the gradient summed over time
    pdf = ar.graph_arrays(ar.case(name)[0])[2]
    by_pdf = np.zeros((cps.shape[0], r[3].shape[2]))
    for b in range(cps.shape[0]):
        np.add.at(by_pdf[b], pdf, cps[b])
    assert ar.dist(r[3].double().numpy().sum(1), by_pdf) <= bound
    g = r[3].numpy()
    for b, L in enumerate(lengths.tolist()):
        assert not g[b, L:].any()
    if name == "degenerate":
        assert not g[:, :, 8].any()                                                              # the pdf no arc carries


@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("coef", ar.COEFS)
@pytest.mark.parametrize("name", ["small", "wide", "degenerate", "states2100"])
def test_fp64_recursions_and_twin_against_autograd(name, coef, wkind):
    g, y, lengths = ar.case(name)
    ref, (bound, _) = ar.reference(name, coef, wkind)
    auto = ar.batch(ar.autograd, g, y, lengths, ar.weights(name, wkind), coef)
    dref = ar.distances(ref, auto)
    dtwin = ar.distances(_triple(_twin(name, coef, wkind)), auto)
    print("%s c=%g w=%s: fp64 recursions against autograd %s, twin %s" % (name, coef, wkind, dref, dtwin))
    record_parity("arc_counts_autograd_%s_c%g_w%s" % (name, coef, wkind), ref_counts=dref[0], ref_grad=dref[1], ref_logz=dref[2],
                  twin_counts=dtwin[0], twin_grad=dtwin[1], twin_logz=dtwin[2])
    assert max(dref) <= 1e-12                                  # two fp64 computations of one quantity
    assert max(dtwin) <= bound


def test_long_sequence_against_autograd():
    g, y, lengths = ar.case("long")
    ref, _ = ar.reference("long", 0.1, "normal")
    auto = ar.batch(ar.autograd, g, y, lengths, ar.weights("long", "normal"), 0.1)
    assert max(ar.distances(ref, auto)) <= 1e-11               # (1500 frames of fp64 rounding)


@pytest.mark.parametrize("fault", ar.FAULTS)
def test_planted_faults_are_seen(fault):
    g, y, lengths = ar.case("small")
    ref, (bound, _) = ar.reference("small", 0.1, "normal")
    bad = ar.batch(ar.counts, g, y, lengths, ar.weights("small", "normal"), 0.1, fault=fault)
    d = ar.dist(bad[1], ref[1])
    print("%s: counts moved by %.3g = %.0f bounds" % (fault, d, d / bound))
    record_parity("arc_counts_fault_%s" % fault, counts=d, bound=bound)
    assert d > 100 * bound


def test_zero_weights_are_no_weights():
    K = ar.case("small")[0].num_transitions
    a, b = _twin("small", 0.1), _twin("small", 0.1, w=torch.zeros(K))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_utterance_weights():
    u = torch.tensor([1.0, 0.0, 2.0, 0.25])
    plain, weighted = _twin("small", 0.1, "normal"), _twin("small", 0.1, "normal", u=u)
    assert torch.equal(plain[0], weighted[0]) and torch.equal(plain[2], weighted[2])             # log Z_b, c(b,k): not weighted
    assert not weighted[3][1].any()                                                              # weight 0: exact zeros
    assert torch.equal(weighted[3][0], plain[3][0])
    want = (u.double()[:, None] * plain[2]).sum(0)
    assert ar.dist(weighted[1].numpy(), want.numpy()) <= 1e-12
    # a weight of 0 leaves the others' bits unchanged: the same call without that sequence's frames mattering
    y2 = ar.case("small")[1].clone()
    y2[1] = 0.0
    other = _twin("small", 0.1, "normal", u=u, y=y2)
    keep = [0, 2, 3]
    assert torch.equal(other[1], weighted[1]) and torch.equal(other[3][keep], weighted[3][keep]) and torch.equal(other[0][keep], weighted[0][keep])
    # a NaN in a live row: counted once, NaN, exact zeros into the counts
    y3 = ar.case("small")[1].clone()
    y3[1, 3, 5] = float("nan")
    bad = _twin("small", 0.1, "normal", y=y3, u=torch.tensor([1.0, 1.0, 2.0, 0.25]))
    assert bad[4].tolist() == [1, 0] and bool(torch.isnan(bad[0][1])) and not bad[2][1].any()
    assert torch.equal(bad[1], weighted[1]) and torch.equal(bad[0][keep], weighted[0][keep])


def test_finite_differences_in_the_weights():
    g, y, lengths = ar.case("small")
    ref, (bound, _) = ar.reference("small", 0.1, "normal")
    w = ar.weights("small", "normal").double()
    K = w.numel()
    # fp64, through the reference: central differences of sum_b log Z_b against the counts
    total = lambda wv: ar.batch(ar.counts, g, y, lengths, wv, 0.1)[0].sum()
    h = 1e-5
    ks = list(range(0, K, 7))
    fd = np.array([(total(w + h * torch.eye(K, dtype=torch.float64)[k]) - total(w - h * torch.eye(K, dtype=torch.float64)[k])) / (2 * h) for k in ks])
    want = ref[1].sum(0)
    assert np.abs(fd - want[ks]).max() <= 1e-8 * np.abs(want).max()       # (h^2 and 1e-16 / h, both below 1e-9)
    # fp32, through the twin: the analytic gradient of den_log_partition in w at the bound, and a directional difference
    wt = ar.weights("small", "normal").clone().requires_grad_(True)
    out = den_log_partition(y, lengths, g, wt, 0.1)
    out.backward()
    assert wt.grad.dtype == torch.float32 and ar.dist(wt.grad.numpy(), want) <= bound
    v = torch.from_numpy(np.sign(np.random.RandomState(5).randn(K)).astype(np.float32))
    hh = 1.0 / 64                                                          # (exact in fp32; the curvature term h^2 / 6 |v|^3 stays small)
    per = lambda wv: den_log_partition(y, lengths, g, wv, 0.1).per_seq.sum().item()
    fdir = (per(wt.detach() + hh * v) - per(wt.detach() - hh * v)) / (2 * hh)
    exact = (total(w + hh * v.double()) - total(w - hh * v.double())) / (2 * hh)
    assert abs(fdir - exact) <= bound * abs(ref[0].sum()) / hh            # log Z within the bound, divided by the step


def test_autograd_function_on_cpu_tensors():
    g, y, lengths = ar.case("small")
    ref, (bound, _) = ar.reference("small", 0.1, "normal")
    x = y.clone().requires_grad_(True)
    w = ar.weights("small", "normal").clone().requires_grad_(True)
    out = den_log_partition(x, lengths, ChainGraphBatch(g, 4), w, 0.1)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.per_seq.dtype == torch.float64 and out.bad_count.tolist() == [0, 0]
    assert ar.value_dist(out.per_seq.numpy(), ref[0]) <= bound
    (2.0 * out).backward(retain_graph=True)
    assert ar.dist(x.grad.double().numpy(), 2.0 * ref[2]) <= bound and ar.dist(w.grad.numpy(), 2.0 * ref[1].sum(0)) <= bound
    first = (x.grad.clone(), w.grad.clone())
    x.grad, w.grad = None, None
    (2.0 * out).backward()
    assert torch.equal(x.grad, first[0]) and torch.equal(w.grad, first[1])
    res = expected_arc_counts(y, lengths, g, 0.1, per_seq=True)
    assert isinstance(res, ArcCounts) and res.counts_per_seq.shape == (4, g.num_transitions) and not res.counts.requires_grad


def test_refusals():
    g, y, lengths = ar.case("small")
    K = g.num_transitions
    with pytest.raises(ValueError, match="one entry per arc"):
        expected_arc_counts(y, lengths, g, arc_log_weights=torch.zeros(K + 1))
    with pytest.raises(ValueError, match="float tensor"):
        expected_arc_counts(y, lengths, g, arc_log_weights=torch.zeros(K, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"shape \[4\]"):
        expected_arc_counts(y, lengths, g, utt_weights=torch.ones(3))
    with pytest.raises(ValueError, match="one denominator graph|ChainGraph"):
        expected_arc_counts(y, lengths, [g])
    with pytest.raises(ValueError, match="batch size"):
        expected_arc_counts(y, lengths, ChainGraphBatch(g, 3))
    with pytest.raises(ValueError, match="names pdf"):
        expected_arc_counts(y[:, :, :20], lengths, g)
    with pytest.raises(ValueError, match=r"\[B, T, D\]"):
        expected_arc_counts(y[0], lengths, g)
    # the C ABI: null pointers, sizes, the coefficient; the device entry point refuses a graph beyond the LDS before it launches
    L = _lib.lib()
    gt = native.smbr_graph(g, 23, torch.device("cpu"))
    lc = lengths.to(torch.int64)
    objf, counts, bad, grad = torch.zeros(4, dtype=torch.float64), torch.zeros(K, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 17, 23)
    host = lambda coef, B, cp: L.pychain_hip_cpu_den_arc_counts(
        *[t.data_ptr() for t in gt], 37, K, None, y.data_ptr(), lc.data_ptr(), B, 17, 23, coef, None, 1.0, None, grad.data_ptr(),
        objf.data_ptr(), cp, None, bad.data_ptr(), 1)
    assert host(0.0, 4, counts.data_ptr()) == -1 and host(1.0, 4, counts.data_ptr()) == -1 and host(0.1, 0, counts.data_ptr()) == -1
    assert host(0.1, 4, None) == -1 and host(0.1, 4, counts.data_ptr()) == 0
    need = L.pychain_hip_den_arc_counts_lds_bytes(37, 21000)
    assert need == (2 * 37 + 2 * 21000 + 64) * 4 + 256 and L.pychain_hip_den_arc_counts_lds_bytes(0, 5) == 0
    dev = L.pychain_hip_den_arc_counts(*[t.data_ptr() for t in gt], 37, K, None, y.data_ptr(), 0, lc.data_ptr(), 4, 17, 21000, 0.1, None, 1.0, None,
                                       None, objf.data_ptr(), counts.data_ptr(), None, bad.data_ptr(), grad.data_ptr(), 1, None)
    msg = L.pychain_hip_last_error().decode()
    assert dev == -2 and "37 states" in msg and "21000 pdfs" in msg and str(need) in msg and str(160 * 1024) in msg
    assert L.pychain_hip_den_arc_counts_workspace_bytes(0, 1, 1, 1) == 0
    nb = L.pychain_hip_den_arc_counts_workspace_bytes(64, 1500, 3000, 30000)
    assert 8 * 1501 * 3000 * 64 + 64 * 24 * 30000 * 8 <= nb <= 8 * 1501 * 3000 * 64 + 64 * 24 * 30000 * 8 + (1 << 20)


def test_abi_version_and_symbols():
    with open(os.path.join(REPO, "include", "pychain_hip.h")) as f:
        header = f.read()
    v = int(re.search(r"#define PYCHAIN_HIP_ABI_VERSION (\d+)", header).group(1))
    assert v == _lib.ABI_VERSION == _lib.lib().pychain_hip_abi_version() and v >= 30
    for name in ("pychain_hip_den_arc_counts_workspace_bytes", "pychain_hip_den_arc_counts_lds_bytes", "pychain_hip_den_arc_counts",
                 "pychain_hip_cpu_den_arc_counts"):
        assert name in header and hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    import pychain
    import pychain_amd
    assert pychain.expected_arc_counts is expected_arc_counts is pychain_amd.expected_arc_counts
    assert pychain.den_log_partition is den_log_partition
    from pychain_amd import build_ext
    assert "arc_counts.hip" in build_ext.SOURCES


def test_header_compiles_as_c(tmp_path):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("gcc") or shutil.which("cc") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cc is not None, "no C compiler: neither gcc nor cc on PATH, nor %s" % rocm_clang
    graph = ("const int32_t*, const int32_t*, const float*, const int32_t*, const int32_t*, const float*, const float*, const float*,\n"
             "    const float*, const int32_t*, const int32_t*, int, int, const float*, ")
    tail = "float, const float*, float, const float*, %s, double*, double*, double*, int32_t*, "
    src = tmp_path / "h.c"
    src.write_text('#include "pychain_hip.h"\n'
                   'static size_t (*ws)(int, int, int, int) = pychain_hip_den_arc_counts_workspace_bytes;\n'
                   'static size_t (*lds)(int, int) = pychain_hip_den_arc_counts_lds_bytes;\n'
                   'static int (*dev)(' + graph + 'const void*, int, const int64_t*, int, int, int,\n    ' + tail % "void*" +
                   'void*, size_t, void*) = pychain_hip_den_arc_counts;\n'
                   'static int (*host)(' + graph + 'const float*, const int64_t*, int, int, int,\n    ' + tail % "float*" +
                   'int) = pychain_hip_cpu_den_arc_counts;\n'
                   'int main(void) { return ws == 0 || lds == 0 || dev == 0 || host == 0 || PYCHAIN_HIP_ABI_VERSION < 30; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True, text=True)
