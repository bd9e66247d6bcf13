"""Tensor-level entry points over the C ABI: the drop-in for the reference's
`pychain_C` module (pytorch_binding/src/pychain.cc:131-135).

`forward_backward` / `forward_backward_log_domain` / `set_verbose_level` keep the
reference's positional signatures and return `[objf, grad, ok]`; the `den_*` /
`num_*` functions are what `pychain_amd.loss` calls (device-resident plans, fused
clamp/exp, per-sequence objf).
"""
import ctypes
import threading

import torch

from . import _lib, _plan

_ws_cache = {}          # (device, stream, tag) -> uint8 tensor, most recently used last
_ws_lock = threading.Lock()      # (criteria on several host threads share this module)
_WS_CACHE_ENTRIES = 8   # a training process uses 2 (den, num) per stream; more are streams that came and went


def _require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            "pychain_amd: %s must live on a HIP device (got %s): the HIP entry points have no CPU fallback "
            "(CPU tensors are served by cpu_forward_backward, never the other way round)." % (what, t.device))


# ---------------------------------------------------------------------------
# CPU tensors: the library's host twins (include/pychain_hip.h: pychain_hip_cpu_*; pychain_amd/csrc/cpu.cpp).  The reference
# computes on whatever device its input lives on (chain-computation.cc:40): so does this package - CPU tensors HERE, device
# tensors in the HIP kernels, and never one for the other (a device tensor that cannot reach the kernels raises).
# ---------------------------------------------------------------------------
CPU_THREADS = 0          # host threads the sequences of a minibatch are dealt to (0 = one per hardware thread)
_GRAPH_INT = ("forward_transitions", "forward_transition_indices", "backward_transitions", "backward_transition_indices")
_GRAPH6 = ["forward_transitions", "forward_transition_indices", "forward_transition_probs",
           "backward_transitions", "backward_transition_indices", "backward_transition_probs"]
_GRAPH8 = _GRAPH6 + ["initial_probs", "final_probs"]
_GRAPH_FORWARD = _GRAPH6[:3]


def _graph_ptrs(gt, names=_GRAPH8):
    """The graph pointers of a device entry point in ABI order, `gt` a dict of device graph tensors: all eight, or those of
    `names` (chain_loss_backward reads the forward transitions alone)."""
    return [gt[n].data_ptr() for n in names]


def _cpu_graph(graphs, with_leaky):
    """(tensors in ABI order, graph_batch_stride): one graph for every sequence (stride 0) or [B,...] tensors."""
    src, stride = (graphs.shared_graph, 0) if graphs.shared_graph is not None else (graphs, 1)
    names = _GRAPH6 + (["leaky_probs"] if with_leaky else []) + ["initial_probs", "final_probs"]
    ts = [getattr(src, n).to(torch.int32 if n in _GRAPH_INT else torch.float32).contiguous() for n in names]
    return ts, stride


def _host_lengths(lengths, B, T):
    """The int64 lengths a host twin reads: on the host, contiguous, checked."""
    lc = torch.as_tensor(lengths).to(torch.int64).cpu().contiguous()
    _check_lengths(lc, B, T)
    return lc


def _host_inputs(x, lengths):
    """(x as contiguous float32 [B,T,D], the int64 lengths on the host - checked): what every host twin reads."""
    xf = x.detach().to(torch.float32).contiguous()
    return xf, _host_lengths(lengths, xf.shape[0], xf.shape[1])


def cpu_forward_backward(graphs, x, lengths, leaky_coefficient=1e-5, input_is_exp=False, grad_mode=_lib.GRAD_LINEAR, clamp=True,
                         windows=None):
    """ChainFunction's computation on CPU tensors: (objf_per_seq[B], grad[B,T,D] fp32, bad_count int32[1]).  Denominator
    (probability-domain graphs) or numerator (log-domain graphs) by `graphs.log_domain`.  `clamp` False (numerator): the network
    output as it is - what pychain_C.forward_backward_log_domain computes on (the reference clamps in Python, loss.py:30).
    `windows` (numerator only): int [B, H, 2] alignment time windows (include/pychain_hip.h: pychain_hip_*_tw), None = none."""
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_forward_backward is for CPU tensors; device tensors run on the HIP kernels")
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    ts, stride = _cpu_graph(graphs, not graphs.log_domain)
    H, K = int(ts[1].shape[-2]), int(ts[0].shape[-2])
    objf = torch.empty(B, dtype=torch.float32)
    grad = torch.empty(B, T, D, dtype=torch.float32)
    bad = torch.zeros(1, dtype=torch.int32)
    L = _lib.lib()
    ptrs = [t.data_ptr() for t in ts]
    if not graphs.log_domain:
        _lib.check(L.pychain_hip_cpu_den_forward_backward(
            *ptrs, stride, xf.data_ptr(), int(bool(input_is_exp)), lc.data_ptr(), B, T, D, H, K,
            float(leaky_coefficient), 1.0, objf.data_ptr(), grad.data_ptr(), bad.data_ptr(), int(CPU_THREADS)),
            "pychain_hip_cpu_den_forward_backward")
    elif windows is None:
        _lib.check(L.pychain_hip_cpu_num_forward_backward(
            *ptrs, stride, xf.data_ptr(), lc.data_ptr(), B, T, D, H, K, int(grad_mode) | (0 if clamp else _lib.CPU_NO_CLAMP), 1.0,
            objf.data_ptr(), grad.data_ptr(), bad.data_ptr(), int(CPU_THREADS)), "pychain_hip_cpu_num_forward_backward")
    else:
        tw = _check_windows(windows.cpu(), B, H)
        _lib.check(L.pychain_hip_cpu_num_forward_backward_tw(
            *ptrs, stride, xf.data_ptr(), lc.data_ptr(), B, T, D, H, K, int(grad_mode) | (0 if clamp else _lib.CPU_NO_CLAMP), 1.0,
            objf.data_ptr(), grad.data_ptr(), bad.data_ptr(), int(CPU_THREADS), tw.data_ptr()),
            "pychain_hip_cpu_num_forward_backward_tw")
    return objf, grad, bad


def _check_windows(windows, B, H, device=None):
    """The int32 [B, H, 2] time windows a *_tw entry point reads (its kernels index them by sequence and state: checked here)."""
    if windows.dtype != torch.int32 or tuple(windows.shape) != (B, H, 2):
        raise ValueError("time windows must be int32 [%d, %d, 2], got %s %s" % (B, H, windows.dtype, tuple(windows.shape)))
    if device is not None and windows.device != device:
        raise ValueError("time windows live on %s, the call on %s" % (windows.device, device))
    return windows.contiguous()


def _workspace(nbytes, device, tag="a"):
    """Scratch for the stored trajectories, reused from call to call.  Keyed by the CALLER'S STREAM as well:
    calls on one stream are ordered, so the next one may overwrite what the previous one left; calls on
    two streams of one device run concurrently and must not share it.  (A replaced buffer goes back to the
    caching allocator, which hands it out again only in the stream order of its allocation.)"""
    key = (str(device), _stream(device), tag)
    with _ws_lock:
        ws = _ws_cache.pop(key, None)
        if ws is None or ws.numel() < nbytes:
            ws = None                      # (the old buffer goes back to the allocator before the larger one is asked for)
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws                # (re-)inserted last = most recently used
        while len(_ws_cache) > _WS_CACHE_ENTRIES:
            _ws_cache.pop(next(iter(_ws_cache)))       # least recently used: multi-GB buffers of streams no longer in use
    return ws


def release_workspaces():
    """Drop every cached workspace (several GB at C3 sizes) and the memoised plans / graph uploads of the
    pychain_C-compatible surface."""
    with _ws_lock:
        _ws_cache.clear()
        _compat_cache.clear()


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _dev_scalar(t, device):
    """An optional 0-dim scalar the kernels read on the device (a normaliser, an upstream gradient): None, or float32 on `device`."""
    return None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()


def _kernel_tensor(t):
    """`t` as a device entry point takes it: contiguous and starting on a 16-byte boundary (the entry points whose kernels read
    and write the rows 16 bytes at a time refuse any other pointer - include/pychain_hip.h; pychain_hip_smbr_forward_backward,
    pychain_hip_topk_rows and the time windows take any element-aligned start and do not come through here).  An aligned contiguous tensor
    comes back as it is, without a launch; a strided view, or a contiguous one whose offset into its buffer is no multiple of
    16 bytes (`y[1:]` at an odd T * D, one half of a wider layer's output), costs one copy of that tensor."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() & 15 else t


def _kernel_buffer(t):
    """(the buffer a kernel updates in place of the caller's contiguous `t`, what to call behind the launch): `t` itself and a
    no-op where it starts on a 16-byte boundary, else an aligned copy and the copy back into `t`."""
    if t is None or not t.data_ptr() & 15:
        return t, lambda: None
    k = t.clone()
    return k, lambda: t.copy_(k)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _lengths_dev(lengths, device):
    return torch.as_tensor(lengths).to(device=device, dtype=torch.int64, non_blocking=True).contiguous()


def _check_lengths(lengths, B, T):
    lc = torch.as_tensor(lengths)
    if lc.numel() != B:
        raise ValueError("sequence_lengths has %d entries for a batch of %d" % (lc.numel(), B))
    if not lc.is_cuda:   # cheap host-side validation only when it costs no sync
        if int(lc.min()) < 1 or int(lc.max()) > T:
            raise ValueError("sequence lengths must be in [1, %d]" % T)


# (Time segments - include/pychain_hip.h: totals[5..7], DESIGN.md §3.13: the burn-in controller that used to live here, fed by
# non-blocking copies of totals[5] whenever their event happened to have fired, is in the LIBRARY since ABI 16 - a device-
# resident state per plan, read and updated by the call's own kernels in stream order: pychain_amd/_plan.py attaches it, nothing
# on the host reads it, and the same run gives the same bits.)


HALF_ROWS = True        # False: bf16 / fp16 network outputs are up-cast on the host side of the ABI (the tests compare the two ways)
_DTYPE_CODE = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def _rows_as_given(x, native):
    """(tensor the kernels read, its PYCHAIN_HIP_* element code): a bf16 / fp16 network output goes to the kernels as it is
    where the call's kernel family takes 2-byte rows (`native`: the library's own answer, include/pychain_hip.h:
    pychain_hip_*_half_native) - no fp32 copy of [B,T,D], and the gradient comes back in the same type; otherwise it is
    up-cast here, once (general plans, the two-barrier recursion, rows that are not a multiple of 8 pdfs, ...)."""
    if x.dtype == torch.float32:
        return x, _lib.F32
    if HALF_ROWS and x.dtype in _DTYPE_CODE and native():
        return x, _DTYPE_CODE[x.dtype]
    return x.float(), _lib.F32


def den_forward_backward(plan, x, lengths, leaky_coefficient=1e-5, input_is_exp=False, grad_scale=1.0, totals=False):
    """Denominator on the GPU.  `plan`: _plan.DevicePlan.
    Returns (objf_per_seq[B], grad[B,T,D], bad_count[1]) and, `totals`, the device float[4] of
    include/pychain_hip.h (sum of the objectives, frames, bad count - from the call's last kernel, no extra launch)."""
    _require_device(x, "nnet_output")
    num_states = plan.num_states
    x = _kernel_tensor(x)
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    L = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        x, xcode = _rows_as_given(x, lambda: L.pychain_hip_den_half_native(plan.stride, plan.slot_rows, int(num_states), D, B, T))
        ld = _lengths_dev(lengths, dev)
        objf = torch.empty(B, dtype=torch.float32, device=dev)
        grad = torch.empty_like(x)                 # (in the type the kernels read: the gradient is rounded where it is written)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        tot = torch.empty(_lib.TOTALS, dtype=torch.float32, device=dev)
        # (the [B,T,D] buffer of the rows exp'd ahead only where this call will use it: ADVICE r4)
        full = L.pychain_hip_den_uses_row_buffer(plan.stride, plan.slot_rows, int(num_states), D, B, T, int(bool(input_is_exp)))
        nws = (L.pychain_hip_den_workspace_bytes if full else L.pychain_hip_den_workspace_min_bytes)(B, T, int(num_states), D)
        ws = _workspace(nws, dev, "den")
        _lib.check(L.pychain_hip_den_forward_backward(
            plan.blob.data_ptr(), plan.stride, plan.slot_rows, int(num_states), D, x.data_ptr(), xcode,
            int(bool(input_is_exp)),
            ld.data_ptr(), B, T, float(leaky_coefficient), float(grad_scale),
            objf.data_ptr(), grad.data_ptr(), bad.data_ptr(), tot.data_ptr(),
            ws.data_ptr(), ws.numel(), _stream(dev)),
            "pychain_hip_den_forward_backward")
    return (objf, grad, bad, tot) if totals else (objf, grad, bad)


def num_forward_backward(gt, graph_stride, num_states, x, lengths, grad_mode=_lib.GRAD_LINEAR,
                         grad_scale=1.0, grad_out=None, windows=None):
    """Numerator on the GPU.  `gt`: dict of device graph tensors; `windows`: int32 [B, H, 2] device time windows or None.
    Returns (objf_per_seq[B], grad[B,T,D], bad_count[1])."""
    _require_device(x, "nnet_output")
    x = _kernel_tensor(x)
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    K = gt["forward_transitions"].shape[1]
    L = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        x, xcode = _rows_as_given(x, lambda: L.pychain_hip_num_half_native(int(num_states), K, D))
        ld = _lengths_dev(lengths, dev)
        objf = torch.empty(B, dtype=torch.float32, device=dev)
        if grad_mode == _lib.GRAD_ACCUM:
            if grad_out is None:
                raise ValueError("GRAD_ACCUM needs grad_out")
            grad = grad_out
        else:
            grad = torch.empty(x.shape, dtype=torch.float32, device=dev)     # (this entry point's gradient is fp32 whatever it read)
        gk, put_back = _kernel_buffer(grad)              # (a caller's buffer off the 16-byte grid: updated through an aligned copy)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        nws = L.pychain_hip_num_workspace_bytes(B, T, int(num_states), K, D)
        ws = _workspace(nws, dev, "num")
        if windows is not None:
            windows = _check_windows(windows, B, int(num_states), dev)
        # (the widest entry point of the family; the narrower ones pass NULL on to it)
        _lib.check(L.pychain_hip_num_forward_backward_xent(
            *_graph_ptrs(gt), int(graph_stride),
            x.data_ptr(), xcode, ld.data_ptr(), B, T, D, int(num_states), K, int(grad_mode), float(grad_scale),
            objf.data_ptr(), gk.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev), _ptr(windows), None),
            "pychain_hip_num_forward_backward_xent")
        put_back()
    return objf, grad, bad


class XentResult(object):
    """What an *_xent entry point leaves (include/pychain_hip.h: pychain_hip_xent): objf [B] fp32, totals fp32[2] = [scaled sum,
    sum], grad [B,T,D] in z's dtype or None (the form without the store)."""
    __slots__ = ("objf", "totals", "grad")


def _xent_arg(z, shape, H, K, with_grad, grad_scale, loss_coef, res):
    """(the pychain_hip_xent of a device call, the tensors it points to - to be kept alive over the call).  `z` goes to the
    kernel in its own dtype (fp32 / bf16 / fp16) whatever the row width; the gradient comes back in the same dtype."""
    B, T, D = shape
    _require_device(z, "xent_output")
    if tuple(z.shape) != (B, T, D):
        raise ValueError("xent_output has shape %s, the chain output %s" % (tuple(z.shape), (B, T, D)))
    if z.dtype not in _DTYPE_CODE:
        raise ValueError("xent_output must be float32, bfloat16 or float16, got %s" % z.dtype)
    dev = z.device
    zc = _kernel_tensor(z.detach())
    res.objf = torch.empty(B, dtype=torch.float32, device=dev)
    res.totals = torch.empty(2, dtype=torch.float32, device=dev)
    res.grad = torch.empty_like(zc) if with_grad else None
    ws = _workspace(_lib.lib().pychain_hip_xent_workspace_bytes(B, T, int(H), int(K), D), dev, "xent")
    arg = _lib.Xent(zc.data_ptr(), _DTYPE_CODE[zc.dtype], res.grad.data_ptr() if with_grad else None, float(grad_scale), None,
                    float(loss_coef), res.objf.data_ptr(), res.totals.data_ptr(), ws.data_ptr(), ws.numel())
    return arg, (zc, ws)


def num_xent(gt, graph_stride, num_states, x, lengths, z, with_grad=True, windows=None):
    """The numerator posteriors of (x, graphs) as cross-entropy targets of z on the GPU: pychain_hip_num_forward_backward_xent
    without a dense numerator gradient.  Returns an XentResult (grad for an upstream gradient of 1)."""
    _require_device(x, "nnet_output")
    x = _kernel_tensor(x.detach())
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    K = gt["forward_transitions"].shape[1]
    L = _lib.lib()
    dev = x.device
    res = XentResult()
    with torch.cuda.device(dev):
        x, xcode = _rows_as_given(x, lambda: L.pychain_hip_num_half_native(int(num_states), K, D))
        ld = _lengths_dev(lengths, dev)
        objf = torch.empty(B, dtype=torch.float32, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(L.pychain_hip_num_workspace_bytes(B, T, int(num_states), K, D), dev, "num")
        if windows is not None:
            windows = _check_windows(windows, B, int(num_states), dev)
        arg, keep = _xent_arg(z, (B, T, D), num_states, K, with_grad, 1.0, 0.0, res)
        _lib.check(L.pychain_hip_num_forward_backward_xent(
            *_graph_ptrs(gt), int(graph_stride),
            x.data_ptr(), xcode, ld.data_ptr(), B, T, D, int(num_states), K, int(_lib.GRAD_LINEAR), 1.0,
            objf.data_ptr(), 0, bad.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev),
            _ptr(windows), ctypes.addressof(arg)), "pychain_hip_num_forward_backward_xent")
        del keep
    return res


def cpu_num_xent(graphs, x, lengths, z, with_grad=True, windows=None):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_num_forward_backward_xent), fp64 accumulation."""
    if x.is_cuda or z.is_cuda:
        raise RuntimeError("pychain_amd: cpu_num_xent is for CPU tensors; device tensors run on the HIP kernels")
    zf = z.detach().to(torch.float32).contiguous()
    if tuple(zf.shape) != tuple(x.shape):
        raise ValueError("xent_output has shape %s, the chain output %s" % (tuple(zf.shape), tuple(x.shape)))
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    ts, stride = _cpu_graph(graphs, False)
    H, K = int(ts[1].shape[-2]), int(ts[0].shape[-2])
    objf = torch.empty(B, dtype=torch.float32)
    grad = torch.empty(B, T, D, dtype=torch.float32)
    bad = torch.zeros(1, dtype=torch.int32)
    res = XentResult()
    res.objf = torch.empty(B, dtype=torch.float32)
    res.totals = torch.empty(2, dtype=torch.float32)
    res.grad = torch.empty(B, T, D, dtype=torch.float32) if with_grad else None
    tw = None if windows is None else _check_windows(windows.cpu(), B, H)
    arg = _lib.Xent(zf.data_ptr(), _lib.F32, res.grad.data_ptr() if with_grad else None, 1.0, None, 0.0, res.objf.data_ptr(),
                    res.totals.data_ptr(), None, 0)
    _lib.check(_lib.lib().pychain_hip_cpu_num_forward_backward_xent(
        *[t.data_ptr() for t in ts], stride, xf.data_ptr(), lc.data_ptr(), B, T, D, H, K, int(_lib.GRAD_LINEAR), 1.0,
        objf.data_ptr(), grad.data_ptr(), bad.data_ptr(), int(CPU_THREADS), 0 if tw is None else tw.data_ptr(),
        ctypes.addressof(arg)), "pychain_hip_cpu_num_forward_backward_xent")
    return res


def xent_targets(z, lengths, pdfs, probs, with_grad=True, grad_scale=1.0, grad_scale_dev=None, norm_dev=None):
    """Sparse targets as cross-entropy targets of z on the GPU (include/pychain_hip.h: pychain_hip_xent_targets), on the current
    stream: `z` ([B,T,D], fp32 / bf16 / fp16) goes to the kernel as it is; `pdfs` / `probs`: [B,T,K].  Returns (XentResult -
    objf [B], grad in z's dtype for the scale grad_scale [* grad_scale_dev] [/ norm_dev] or None, totals None until
    xent_add_totals fills them -, bad_count int32 [1])."""
    _require_device(z, "xent_output")
    if z.dtype not in _DTYPE_CODE:
        raise ValueError("xent_output must be float32, bfloat16 or float16, got %s" % z.dtype)
    zc = _kernel_tensor(z.detach())
    B, T, D = zc.shape
    _check_lengths(lengths, B, T)
    L = _lib.lib()
    dev = zc.device
    res = XentResult()
    with torch.cuda.device(dev):
        ld = _lengths_dev(lengths, dev)
        pd, pr = _target_args(pdfs, probs, B, T, dev)
        res.objf = torch.empty(B, dtype=torch.float32, device=dev)
        res.totals = None
        res.grad = torch.empty_like(zc) if with_grad else None
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        grad_scale_dev, norm_dev = _dev_scalar(grad_scale_dev, dev), _dev_scalar(norm_dev, dev)
        ws = _workspace(L.pychain_hip_xent_targets_workspace_bytes(B, T), dev, "xent_targets")
        _lib.check(L.pychain_hip_xent_targets(
            zc.data_ptr(), _DTYPE_CODE[zc.dtype], ld.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), _ptr(res.grad),
            float(grad_scale), _ptr(grad_scale_dev), _ptr(norm_dev), res.objf.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(),
            _stream(dev)), "pychain_hip_xent_targets")
    return res, bad


def xent_add_totals(res, bad=None, loss_scale=1.0, norm_dev=None, loss_coef=0.0, totals=None):
    """The totals step behind xent_targets (include/pychain_hip.h: pychain_hip_xent_add_totals), on the current stream:
    res.totals = fp32[2] = [loss_scale * S [/ norm_dev], S], S the sum of res.objf; `totals` (the device float[8] of the step, or
    None): [0] = [4] += loss_coef * res.totals[0], [2] += bad.  Returns `res`."""
    dev = res.objf.device
    with torch.cuda.device(dev):
        res.totals = torch.empty(2, dtype=torch.float32, device=dev)
        norm_dev = _dev_scalar(norm_dev, dev)
        _lib.check(_lib.lib().pychain_hip_xent_add_totals(
            res.objf.data_ptr(), int(res.objf.numel()), float(loss_scale), _ptr(norm_dev), float(loss_coef), res.totals.data_ptr(),
            _ptr(totals), _ptr(bad), _stream(dev)), "pychain_hip_xent_add_totals")
    return res


def cpu_xent_targets(z, lengths, pdfs, probs, with_grad=True, grad_scale=1.0, grad_scale_dev=None, norm=None):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_xent_targets), fp32 z, fp64 sums.  Returns (XentResult with
    totals = [S, S], bad_count int32 [1])."""
    if z.is_cuda:
        raise RuntimeError("pychain_amd: cpu_xent_targets is for CPU tensors; device tensors run on the HIP kernels")
    zf, lc = _host_inputs(z, lengths)
    B, T, D = zf.shape
    pd, pr = _target_args(pdfs, probs, B, T, torch.device("cpu"))
    cf = lambda t: None if t is None else torch.as_tensor(t).detach().to(torch.float32).contiguous()
    grad_scale_dev, norm = cf(grad_scale_dev), cf(norm)
    res = XentResult()
    res.objf = torch.empty(B, dtype=torch.float32)
    res.grad = torch.empty(B, T, D, dtype=torch.float32) if with_grad else None
    bad = torch.zeros(1, dtype=torch.int32)
    _lib.check(_lib.lib().pychain_hip_cpu_xent_targets(
        zf.data_ptr(), lc.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), _ptr(res.grad), float(grad_scale),
        _ptr(grad_scale_dev), _ptr(norm), res.objf.data_ptr(), bad.data_ptr(), int(CPU_THREADS)), "pychain_hip_cpu_xent_targets")
    S = res.objf.sum(dtype=torch.float64).to(torch.float32)
    res.totals = torch.stack([S, S])
    return res, bad


_CLAMP_LIMIT = 30.0        # the kernels' own clamp: the `limit` of the out-of-range penalty (pychain_hip_output_reg)


class RegResult(object):
    """What pychain_hip_output_reg leaves (include/pychain_hip.h): per_seq [B,2] fp32 = {R2_b, RO_b}, totals fp32[3] = [scaled term,
    sum R2, sum RO], grad [B,T,D] in x's dtype or None (the objective-only form, or the caller's own buffer in ACCUM)."""
    __slots__ = ("per_seq", "totals", "grad")


def output_reg(x, lengths, l2, oor, grad=None, grad_mode=_lib.GRAD_LINEAR, with_grad=True, grad_scale=1.0, grad_scale_dev=None,
               norm_dev=None, loss_scale=1.0, totals=None):
    """Output L2 and the out-of-range penalty on the GPU (include/pychain_hip.h: pychain_hip_output_reg), on the current stream.
    `x` goes to the kernel in its own dtype (fp32 / bf16 / fp16).  GRAD_ACCUM: `grad` (x's dtype and shape) += s * term over the
    live rows; GRAD_LINEAR: a fresh gradient buffer = s * term, zero rows beyond the lengths (`with_grad` False: the objective
    only).  s = grad_scale [* grad_scale_dev] [/ norm_dev], the two 0-dim device tensors read on the device.  `totals`: the
    device float[8] of a fused call on this stream - its [0] and [4] get the scaled term added.  Returns a RegResult."""
    _require_device(x, "nnet_output")
    if x.dtype not in _DTYPE_CODE:
        raise ValueError("nnet_output must be float32, bfloat16 or float16, got %s" % x.dtype)
    x = _kernel_tensor(x.detach())
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    L = _lib.lib()
    dev = x.device
    res = RegResult()
    with torch.cuda.device(dev):
        ld = _lengths_dev(lengths, dev)
        if grad_mode == _lib.GRAD_ACCUM:
            if grad is not None and (grad.dtype != x.dtype or tuple(grad.shape) != (B, T, D) or not grad.is_contiguous()
                                     or grad.device != dev):
                raise ValueError("GRAD_ACCUM needs a contiguous gradient of the network output's dtype, shape and device")
        elif grad_mode == _lib.GRAD_LINEAR:
            grad = torch.empty_like(x) if with_grad else None
        else:
            raise ValueError("output_reg: grad_mode must be GRAD_ACCUM or GRAD_LINEAR")
        res.per_seq = torch.empty(B, 2, dtype=torch.float32, device=dev)
        res.totals = torch.empty(3, dtype=torch.float32, device=dev)
        res.grad = grad
        grad, put_back = _kernel_buffer(grad)
        grad_scale_dev, norm_dev = _dev_scalar(grad_scale_dev, dev), _dev_scalar(norm_dev, dev)
        ws = _workspace(L.pychain_hip_output_reg_workspace_bytes(B, T), dev, "outreg")
        _lib.check(L.pychain_hip_output_reg(
            x.data_ptr(), _DTYPE_CODE[x.dtype], ld.data_ptr(), B, T, D, float(l2), float(oor), _CLAMP_LIMIT, int(grad_mode),
            _ptr(grad), float(grad_scale), _ptr(grad_scale_dev), _ptr(norm_dev), res.per_seq.data_ptr(), float(loss_scale),
            res.totals.data_ptr(), _ptr(totals), ws.data_ptr(), ws.numel(), _stream(dev)), "pychain_hip_output_reg")
        put_back()
    return res


def cpu_output_reg(x, lengths, l2, oor, grad=None, grad_mode=_lib.GRAD_LINEAR, with_grad=True, grad_scale=1.0, loss_scale=1.0):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_output_reg), fp32 rows, fp64 sums."""
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_output_reg is for CPU tensors; device tensors run on the HIP kernels")
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    res = RegResult()
    if grad_mode == _lib.GRAD_ACCUM:
        if grad is not None and (grad.dtype != torch.float32 or tuple(grad.shape) != (B, T, D) or not grad.is_contiguous()):
            raise ValueError("GRAD_ACCUM needs a contiguous float32 gradient of the network output's shape")
    elif grad_mode == _lib.GRAD_LINEAR:
        grad = torch.empty(B, T, D, dtype=torch.float32) if with_grad else None
    else:
        raise ValueError("cpu_output_reg: grad_mode must be GRAD_ACCUM or GRAD_LINEAR")
    res.per_seq = torch.empty(B, 2, dtype=torch.float32)
    res.totals = torch.empty(3, dtype=torch.float32)
    res.grad = grad
    _lib.check(_lib.lib().pychain_hip_cpu_output_reg(
        xf.data_ptr(), lc.data_ptr(), B, T, D, float(l2), float(oor), _CLAMP_LIMIT, int(grad_mode),
        None if grad is None else grad.data_ptr(), float(grad_scale), None, None, res.per_seq.data_ptr(), float(loss_scale),
        res.totals.data_ptr(), None, int(CPU_THREADS)), "pychain_hip_cpu_output_reg")
    return res


def _weight_args(u, f, B, T, device):
    """The float32 [B] / [B,T] weights an entry point reads, on `device` (None stays None)."""
    if u is None and f is None:
        raise ValueError("weight_rows: neither utterance weights nor derivative weights (a caller without weights makes no call)")
    if u is not None:
        u = u.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
        if tuple(u.shape) != (B,):
            raise ValueError("utterance weights must have shape [%d], got %s" % (B, tuple(u.shape)))
    if f is not None:
        f = f.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
        if tuple(f.shape) != (B, T):
            raise ValueError("derivative weights must have shape [%d, %d], got %s" % (B, T, tuple(f.shape)))
    return u, f


def weight_rows(grad, lengths, utt_weights=None, deriv_weights=None, shape=None, den_objf=None, num_objf=None, xent_objf=None,
                xent_coef=0.0, reg_per_seq=None, l2=0.0, oor=0.0, loss_scale=1.0, norm_dev=None, totals=None):
    """Utterance weights u [B] and derivative weights f [B,T] on the GPU (include/pychain_hip.h: pychain_hip_weight_rows), on the
    current stream.  `grad` ([B,T,D], fp32 / bf16 / fp16, contiguous) is scaled IN PLACE: per live row, w = u_b * f_bt; w == 1
    rows are not touched, w == 0 rows are stored as zeros without a load, the others get one multiply and one rounding.  `grad`
    None (`shape` = (B, T, D) then): the sums only.  `den_objf` / `num_objf` given: the weighted sums over the per-sequence
    arrays of a fused call - into `totals` (its device float[8]: [0] = [4] = the weighted loss, [1] = sum u L, [3] = sum u
    (den - num)) - and the returned float[5] {sum u (den - num), sum u xent, sum u R2, sum u RO, sum u L}; else None."""
    if grad is not None:
        _require_device(grad, "grad")
        if grad.dtype not in _DTYPE_CODE or grad.dim() != 3 or not grad.is_contiguous():
            raise ValueError("weight_rows: grad must be a contiguous [B,T,D] float32, bfloat16 or float16 tensor")
        shape = tuple(grad.shape)
    B, T, D = shape
    dev = grad.device if grad is not None else den_objf.device
    _check_lengths(lengths, B, T)
    weighted = None
    with torch.cuda.device(dev):
        ld = _lengths_dev(lengths, dev)
        u, f = _weight_args(utt_weights, deriv_weights, B, T, dev)
        if den_objf is not None:
            weighted = torch.empty(5, dtype=torch.float32, device=dev)
        norm_dev = _dev_scalar(norm_dev, dev)
        grad, put_back = _kernel_buffer(grad)
        _lib.check(_lib.lib().pychain_hip_weight_rows(
            _ptr(grad), _DTYPE_CODE[grad.dtype] if grad is not None else _lib.F32, ld.data_ptr(), B, T, D, _ptr(u), _ptr(f),
            _ptr(den_objf), _ptr(num_objf), _ptr(xent_objf), float(xent_coef), _ptr(reg_per_seq), float(l2), float(oor),
            float(loss_scale), _ptr(norm_dev), _ptr(totals), _ptr(weighted), _stream(dev)), "pychain_hip_weight_rows")
        put_back()
    return weighted


def cpu_weight_rows(grad, lengths, utt_weights=None, deriv_weights=None, shape=None, den_objf=None, num_objf=None, xent_objf=None,
                    xent_coef=0.0, reg_per_seq=None, l2=0.0, oor=0.0, loss_scale=1.0, norm=None, totals=None):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_weight_rows), a contiguous float32 `grad` scaled in place, the
    same single multiply and fp64 sums.  `norm`: None or a float32 tensor of one element the loss is divided by."""
    if grad is not None:
        if grad.is_cuda:
            raise RuntimeError("pychain_amd: cpu_weight_rows is for CPU tensors; device tensors run on the HIP kernels")
        if grad.dtype != torch.float32 or grad.dim() != 3 or not grad.is_contiguous():
            raise ValueError("cpu_weight_rows: grad must be a contiguous [B,T,D] float32 tensor")
        shape = tuple(grad.shape)
    B, T, D = shape
    lc = _host_lengths(lengths, B, T)
    u, f = _weight_args(utt_weights, deriv_weights, B, T, torch.device("cpu"))
    cf = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    den_objf, num_objf, xent_objf, reg_per_seq, norm = cf(den_objf), cf(num_objf), cf(xent_objf), cf(reg_per_seq), cf(norm)
    weighted = torch.empty(5, dtype=torch.float32) if den_objf is not None else None
    _lib.check(_lib.lib().pychain_hip_cpu_weight_rows(
        _ptr(grad), lc.data_ptr(), B, T, D, _ptr(u), _ptr(f), _ptr(den_objf), _ptr(num_objf), _ptr(xent_objf), float(xent_coef),
        _ptr(reg_per_seq), float(l2), float(oor), float(loss_scale), _ptr(norm), _ptr(totals), _ptr(weighted), int(CPU_THREADS)),
        "pychain_hip_cpu_weight_rows")
    return weighted


def _target_args(pdfs, probs, B, T, device):
    """The int32 / float32 [B,T,K] targets an entry point reads, on `device`."""
    if pdfs.dim() != 3 or tuple(pdfs.shape[:2]) != (B, T) or tuple(probs.shape) != tuple(pdfs.shape) or pdfs.shape[2] < 1:
        raise ValueError("posterior targets must be [%d, %d, K >= 1] pdfs and probs of one shape, got %s and %s"
                         % (B, T, tuple(pdfs.shape), tuple(probs.shape)))
    return (pdfs.detach().to(device=device, dtype=torch.int32).contiguous(),
            probs.detach().to(device=device, dtype=torch.float32).contiguous())


def post_targets(x, lengths, pdfs, probs, grad=None, grad_scale=1.0, grad_scale_dev=None, norm_dev=None, den_objf=None,
                 loss_scale=1.0, totals=None):
    """Sparse posterior targets as the numerator on the GPU (include/pychain_hip.h: pychain_hip_post_targets), on the current
    stream.  `x` ([B,T,D], fp32 / bf16 / fp16) goes to the kernel as it is; `pdfs` / `probs`: [B,T,K].  `grad` (x's dtype and
    shape, or None: the objective only) gets s * q added at the addressed elements, s = grad_scale [* grad_scale_dev]
    [/ norm_dev].  `totals` (with `den_objf` [B]): the device float[8] of the denominator call on this stream - [3] = sum den -
    sum num, [0] = [4] = loss_scale * that [/ norm_dev], [2] += the bad entries.  Returns (num_objf [B], bad_count int32 [1])."""
    _require_device(x, "nnet_output")
    if x.dtype not in _DTYPE_CODE:
        raise ValueError("nnet_output must be float32, bfloat16 or float16, got %s" % x.dtype)
    x = x.detach().contiguous()            # (read one element at a time, csrc/post.hip: any element-aligned start will do)
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    L = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        ld = _lengths_dev(lengths, dev)
        pd, pr = _target_args(pdfs, probs, B, T, dev)
        if grad is not None and (grad.dtype != x.dtype or tuple(grad.shape) != (B, T, D) or not grad.is_contiguous() or grad.device != dev):
            raise ValueError("post_targets needs a contiguous gradient of the network output's dtype, shape and device")
        if totals is not None and den_objf is None:
            raise ValueError("post_targets: totals need den_objf")
        num_objf = torch.empty(B, dtype=torch.float32, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        grad_scale_dev, norm_dev = _dev_scalar(grad_scale_dev, dev), _dev_scalar(norm_dev, dev)
        ws = _workspace(L.pychain_hip_post_targets_workspace_bytes(B, T), dev, "post")
        grad, put_back = _kernel_buffer(grad)
        _lib.check(L.pychain_hip_post_targets(
            x.data_ptr(), _DTYPE_CODE[x.dtype], ld.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), _ptr(grad),
            float(grad_scale), _ptr(grad_scale_dev), _ptr(norm_dev), _ptr(den_objf), num_objf.data_ptr(), bad.data_ptr(),
            float(loss_scale), _ptr(totals), ws.data_ptr(), ws.numel(), _stream(dev)), "pychain_hip_post_targets")
        put_back()
    return num_objf, bad


def cpu_post_targets(x, lengths, pdfs, probs, grad=None, grad_scale=1.0, grad_scale_dev=None, norm=None, den_objf=None,
                     loss_scale=1.0, totals=None):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_post_targets), fp32 rows, a contiguous float32 `grad` updated in
    place.  `grad_scale_dev` / `norm`: None or float32 tensors of one element."""
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_post_targets is for CPU tensors; device tensors run on the HIP kernels")
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    pd, pr = _target_args(pdfs, probs, B, T, torch.device("cpu"))
    if grad is not None and (grad.dtype != torch.float32 or tuple(grad.shape) != (B, T, D) or not grad.is_contiguous()):
        raise ValueError("cpu_post_targets needs a contiguous float32 gradient of the network output's shape")
    if totals is not None and den_objf is None:
        raise ValueError("cpu_post_targets: totals need den_objf")
    cf = lambda t: None if t is None else torch.as_tensor(t).detach().to(torch.float32).contiguous()
    grad_scale_dev, norm, den_objf = cf(grad_scale_dev), cf(norm), cf(den_objf)
    num_objf = torch.empty(B, dtype=torch.float32)
    bad = torch.zeros(1, dtype=torch.int32)
    _lib.check(_lib.lib().pychain_hip_cpu_post_targets(
        xf.data_ptr(), lc.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), _ptr(grad), float(grad_scale),
        _ptr(grad_scale_dev), _ptr(norm), _ptr(den_objf), num_objf.data_ptr(), bad.data_ptr(), float(loss_scale), _ptr(totals),
        int(CPU_THREADS)), "pychain_hip_cpu_post_targets")
    return num_objf, bad


def _check_boost(boost):
    boost = float(boost)
    if not (boost >= 0.0) or boost == float("inf"):
        raise ValueError("boost must be finite and not negative, got %r" % boost)
    return boost


def boost_rows(x, lengths, pdfs, probs, boost, out=None):
    """The rows of the boosted denominator on the GPU (include/pychain_hip.h: pychain_hip_boost_rows), on the current stream:
    e = exp(clamp(x)) over the live frames, the elements the frame's entries address scaled by exp(-boost * qd).  `x` ([B,T,D],
    fp32 / bf16 / fp16) goes to the kernel as it is; `pdfs` / `probs`: [B,T,K].  Returns (e float32 [B,T,D] - rows beyond a
    length are not written -, bad_count int32 [1]).  `out` None: e is a view of the cached workspace of the caller's stream (key
    "boost") - the next boost_rows on that stream overwrites it, so it goes straight into den_forward_backward(...,
    input_is_exp=True)."""
    _require_device(x, "nnet_output")
    if x.dtype not in _DTYPE_CODE:
        raise ValueError("nnet_output must be float32, bfloat16 or float16, got %s" % x.dtype)
    boost = _check_boost(boost)
    x = _kernel_tensor(x.detach())
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    dev = x.device
    with torch.cuda.device(dev):
        ld = _lengths_dev(lengths, dev)
        pd, pr = _target_args(pdfs, probs, B, T, dev)
        if out is None:
            n = B * T * D
            out = _workspace(4 * n, dev, "boost")[:4 * n].view(torch.float32).view(B, T, D)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, T, D) or not out.is_contiguous() or out.device != dev:
            raise ValueError("boost_rows: out must be a contiguous float32 tensor of the network output's shape and device")
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        ek, put_back = _kernel_buffer(out)
        _lib.check(_lib.lib().pychain_hip_boost_rows(
            x.data_ptr(), _DTYPE_CODE[x.dtype], ld.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), boost,
            ek.data_ptr(), bad.data_ptr(), _stream(dev)), "pychain_hip_boost_rows")
        put_back()
    return out, bad


def cpu_boost_rows(x, lengths, pdfs, probs, boost, out=None):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_boost_rows), fp32 rows.  `out` None: a fresh buffer."""
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_boost_rows is for CPU tensors; device tensors run on the HIP kernels")
    boost = _check_boost(boost)
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    pd, pr = _target_args(pdfs, probs, B, T, torch.device("cpu"))
    if out is None:
        out = torch.empty(B, T, D, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, T, D) or not out.is_contiguous() or out.is_cuda:
        raise ValueError("cpu_boost_rows: out must be a contiguous float32 CPU tensor of the network output's shape")
    bad = torch.zeros(1, dtype=torch.int32)
    _lib.check(_lib.lib().pychain_hip_cpu_boost_rows(
        xf.data_ptr(), lc.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), boost, out.data_ptr(),
        bad.data_ptr(), int(CPU_THREADS)), "pychain_hip_cpu_boost_rows")
    return out, bad


_SMBR_GRAPH = _GRAPH6 + ["leaky_probs", "initial_probs", "final_probs"]


def smbr_graph(graph, D, device):
    """The tensors of a denominator ChainGraph that the sMBR entry points read (include/pychain_hip.h: pychain_hip_smbr_*), on
    `device`, in ABI order: the nine of the reference layout, then the arcs by pdf - pdf_arcs int32 [K], the ids of the forward
    arcs in a stable sort by pdf, and pdf_index int32 [D + 1].  Built once per (graph tensors, D, device) and cached on the graph;
    checked here, on the host: every state below H, every pdf below D."""
    ts = [getattr(graph, n) for n in _SMBR_GRAPH]
    key = ("smbr", str(device), int(D)) + tuple((t.data_ptr(), t._version) for t in ts)
    hit = graph._plan_cache.get(key)
    if hit is None:
        ft = graph.forward_transitions.to(torch.int64)
        H = int(graph.num_states)
        if int(ft[:, :2].min()) < 0 or int(ft[:, :2].max()) >= H or int(ft[:, 2].min()) < 0:
            raise ValueError("denominator graph: an arc names a state outside [0, %d) or a negative pdf" % H)
        if int(ft[:, 2].max()) >= D:
            raise ValueError("denominator graph names pdf %d, the network output has %d" % (int(ft[:, 2].max()), D))
        order = torch.sort(ft[:, 2], stable=True)[1]
        index = torch.zeros(D + 1, dtype=torch.int64)
        index[1:] = torch.cumsum(torch.bincount(ft[:, 2], minlength=D), 0)
        host = [t.to(torch.int32 if n in _GRAPH_INT else torch.float32).contiguous() for n, t in zip(_SMBR_GRAPH, ts)]
        host += [order.to(torch.int32).contiguous(), index.to(torch.int32).contiguous()]
        hit = [t.to(device) for t in host]
        for k in [k for k in graph._plan_cache if k[:1] == ("smbr",) and k[1:3] == key[1:3]]:
            del graph._plan_cache[k]
        graph._plan_cache[key] = hit
    return hit


_smbr_classes_cache = {}


def smbr_classes(classes, D, device):
    """(the map pdf -> class as a contiguous int32 tensor [D] on `device`, C = max + 1) of `classes`, an integer tensor [D] without
    a negative entry: checked on the host and uploaded once per (tensor, D, device) - cached until the tensor is replaced or
    edited in place, one map per device (as smbr_graph caches the graph's tensors)."""
    if not torch.is_tensor(classes):
        classes = torch.as_tensor(classes)
    key = (id(classes), classes.data_ptr(), classes._version, int(D))
    hit = _smbr_classes_cache.get(str(device))
    if hit is None or hit[0] != key or hit[1] is not classes:
        if classes.is_floating_point() or classes.is_complex() or classes.dtype == torch.bool:
            raise ValueError("classes must be an integer tensor, got %s" % classes.dtype)
        if classes.dim() != 1 or classes.numel() != D:
            raise ValueError("classes must be [D] = [%d], one class per pdf, got %s" % (D, list(classes.shape)))
        lo, hi = int(classes.min()), int(classes.max())
        if lo < 0:
            raise ValueError("classes holds a negative entry (%d)" % lo)
        if hi >= 2 ** 31 - 1:
            raise ValueError("classes names class %d: beyond int32" % hi)
        # (an aligned copy, 4 D bytes once per map: an int32 map already on `device` that is a contiguous view off the 16-byte grid
        # would come back as that view, and the accuracy pass picks its 16-byte or its element form - other fp64 sum orders, other
        # last bits - by the map's start.  One form serves a (D, gamma) whatever view the caller passed; the key stays the caller's.)
        hit = (key, classes, _kernel_tensor(classes.detach().to(device=device, dtype=torch.int32)), hi + 1)
        _smbr_classes_cache[str(device)] = hit
    return hit[2], hit[3]


def _classes_args(classes, num_classes, targets_are_classes, D, device, who):
    """The three trailing arguments of the *_classes entry points; `classes` None: the pdf-level call."""
    if classes is None:
        if targets_are_classes:
            raise ValueError("%s: targets_are_classes needs classes" % who)
        return None
    if classes.dtype != torch.int32 or tuple(classes.shape) != (D,) or classes.device != device or not classes.is_contiguous():
        raise ValueError("%s: classes must be a contiguous int32 tensor [D] on the network output's device (native.smbr_classes)" % who)
    if int(num_classes) < 1:
        raise ValueError("%s: num_classes must be at least 1, got %s" % (who, num_classes))
    return classes, int(num_classes), int(bool(targets_are_classes))


SMBR_FORMS = {"lds": _lib.SMBR_LDS, "auto": _lib.SMBR_AUTO, "rows": _lib.SMBR_ROWS, "global": _lib.SMBR_GLOBAL}


def smbr_form_code(form, who="smbr"):
    """PYCHAIN_HIP_SMBR_* of `form` ("lds", "auto", "rows", "global"); ValueError for anything else."""
    if not isinstance(form, str) or form not in SMBR_FORMS:
        raise ValueError("%s: the kernels must be one of %s, got %r" % (who, ", ".join(repr(k) for k in SMBR_FORMS), form))
    return SMBR_FORMS[form]


def smbr(gt, num_states, x, lengths, gamma, pdfs, probs, leaky_coefficient=1e-5, grad_scale=1.0, grad_scale_dev=None, *,
         classes=None, num_classes=0, targets_are_classes=False, form="lds"):
    """Lattice-free sMBR on the GPU (include/pychain_hip.h: pychain_hip_smbr_frame_accuracy, then pychain_hip_smbr_forward_backward),
    on the current stream.  `gt`: smbr_graph(...); `x` ([B,T,D], fp32 / bf16 / fp16) goes to the kernels as it is; `gamma`: the
    denominator's occupancies of x, float32 [B,T,D]; `pdfs` / `probs`: [B,T,K].  Returns (acc_per_seq float64 [B], grad in x's
    dtype, bad_count int32 [2], closing float32 [B], frame_acc float32 [B,T] - beyond a length not written).  With `classes`
    (smbr_classes(...): int32 [D] on the device) and `num_classes` the accuracy is by class (the *_classes entry points);
    `targets_are_classes`: the ids of `pdfs` are classes already.  `form`: "lds" - the two entry points above, which refuse a
    graph and tree beyond the LDS of a CU -, or "auto", "rows", "global": pychain_hip_smbr_forward_backward_general with that
    form (any H, D, C; the bits of "lds" wherever both run)."""
    _require_device(x, "nnet_output")
    form_code = smbr_form_code(form)
    if x.dtype not in _DTYPE_CODE:
        raise ValueError("nnet_output must be float32, bfloat16 or float16, got %s" % x.dtype)
    # (x is read one element at a time - include/pychain_hip.h: pychain_hip_smbr_forward_backward, "any element-aligned start";
    # csrc/smbr.hip: row_load1 - so a contiguous view off the 16-byte grid goes to the kernels as it is, 2-byte rows at a 2-byte
    # offset included: no copy.  tests/test_gpu_layouts.py sends such views.  gamma and grad are this package's own, aligned.)
    x = x.detach().contiguous()
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    L = _lib.lib()
    dev = x.device
    H, K = int(num_states), int(gt[0].shape[0])
    with torch.cuda.device(dev):
        if gamma.dtype != torch.float32 or tuple(gamma.shape) != (B, T, D) or gamma.device != dev:
            raise ValueError("smbr: gamma must be a float32 tensor of the network output's shape and device")
        gamma = gamma.contiguous()
        ld = _lengths_dev(lengths, dev)
        pd, pr = _target_args(pdfs, probs, B, T, dev)
        frame_acc = torch.empty(B, T, dtype=torch.float32, device=dev)
        acc = torch.empty(B, dtype=torch.float64, device=dev)
        closing = torch.empty(B, dtype=torch.float32, device=dev)
        bad = torch.empty(2, dtype=torch.int32, device=dev)
        grad = torch.empty_like(x)
        grad_scale_dev = _dev_scalar(grad_scale_dev, dev)
        cls = _classes_args(classes, num_classes, targets_are_classes, D, dev, "smbr")
        acc_args = (gamma.data_ptr(), ld.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), frame_acc.data_ptr(),
                    acc.data_ptr(), bad.data_ptr(), _stream(dev))
        if cls is None:
            _lib.check(L.pychain_hip_smbr_frame_accuracy(*acc_args), "pychain_hip_smbr_frame_accuracy")
        else:
            wa = _workspace(L.pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(B, T), dev, "smbr_acc")
            _lib.check(L.pychain_hip_smbr_frame_accuracy_classes(*acc_args, cls[0].data_ptr(), cls[1], cls[2], wa.data_ptr(), wa.numel()),
                       "pychain_hip_smbr_frame_accuracy_classes")
        if form == "lds":
            ws = _workspace(L.pychain_hip_smbr_workspace_bytes(B, T, H), dev, "smbr")
        else:
            ws = _workspace(L.pychain_hip_smbr_general_workspace_bytes(B, T, H, D, cls[1] if cls else 0), dev, "smbr")
        args = (*[t.data_ptr() for t in gt], H, K, x.data_ptr(), _DTYPE_CODE[x.dtype], ld.data_ptr(), B, T, D,
                pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), frame_acc.data_ptr(), float(leaky_coefficient), float(grad_scale),
                _ptr(grad_scale_dev), grad.data_ptr(), acc.data_ptr(), closing.data_ptr(), bad.data_ptr(),
                ws.data_ptr(), ws.numel(), _stream(dev))
        if form != "lds":
            tail = (cls[0].data_ptr(), cls[1], cls[2]) if cls else (None, 0, 0)
            _lib.check(L.pychain_hip_smbr_forward_backward_general(*args, *tail, form_code), "pychain_hip_smbr_forward_backward_general")
        elif cls is None:
            _lib.check(L.pychain_hip_smbr_forward_backward(*args), "pychain_hip_smbr_forward_backward")
        else:
            _lib.check(L.pychain_hip_smbr_forward_backward_classes(*args, cls[0].data_ptr(), cls[1], cls[2]),
                       "pychain_hip_smbr_forward_backward_classes")
    return acc, grad, bad, closing, frame_acc


def cpu_smbr(gt, num_states, x, lengths, gamma, pdfs, probs, leaky_coefficient=1e-5, grad_scale=1.0, *,
             classes=None, num_classes=0, targets_are_classes=False, form="lds"):
    """The same on CPU tensors: the host twins (pychain_hip_cpu_smbr_*), fp32 rows and gradient.  `form` is checked and changes
    nothing: the one host twin has no size limit."""
    smbr_form_code(form, "cpu_smbr")
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_smbr is for CPU tensors; device tensors run on the HIP kernels")
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    H, K = int(num_states), int(gt[0].shape[0])
    gamma = gamma.detach().to(torch.float32).contiguous()
    if tuple(gamma.shape) != (B, T, D):
        raise ValueError("cpu_smbr: gamma must have the network output's shape")
    pd, pr = _target_args(pdfs, probs, B, T, torch.device("cpu"))
    frame_acc = torch.zeros(B, T, dtype=torch.float32)
    acc = torch.empty(B, dtype=torch.float64)
    closing = torch.empty(B, dtype=torch.float32)
    bad = torch.zeros(2, dtype=torch.int32)
    grad = torch.empty(B, T, D, dtype=torch.float32)
    L = _lib.lib()
    cls = _classes_args(classes, num_classes, targets_are_classes, D, torch.device("cpu"), "cpu_smbr")
    acc_args = (gamma.data_ptr(), lc.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]), frame_acc.data_ptr(),
                acc.data_ptr(), bad.data_ptr(), int(CPU_THREADS))
    args = (*[t.data_ptr() for t in gt], H, K, xf.data_ptr(), lc.data_ptr(), B, T, D, pd.data_ptr(), pr.data_ptr(), int(pd.shape[2]),
            frame_acc.data_ptr(), float(leaky_coefficient), float(grad_scale), None, grad.data_ptr(), acc.data_ptr(),
            closing.data_ptr(), bad.data_ptr(), int(CPU_THREADS))
    if cls is None:
        _lib.check(L.pychain_hip_cpu_smbr_frame_accuracy(*acc_args), "pychain_hip_cpu_smbr_frame_accuracy")
        _lib.check(L.pychain_hip_cpu_smbr_forward_backward(*args), "pychain_hip_cpu_smbr_forward_backward")
    else:
        tail = (cls[0].data_ptr(), cls[1], cls[2])
        _lib.check(L.pychain_hip_cpu_smbr_frame_accuracy_classes(*acc_args, *tail), "pychain_hip_cpu_smbr_frame_accuracy_classes")
        _lib.check(L.pychain_hip_cpu_smbr_forward_backward_classes(*args, *tail), "pychain_hip_cpu_smbr_forward_backward_classes")
    return acc, grad, bad, closing, frame_acc


def _arc_weight_args(arc_log_weights, utt_weights, K, B, device):
    """(arc_log_weights float32 [K], utt_weights float32 [B]) as the arc-count entry points read them, on `device`; None stays
    None.  Both are read one element at a time: a contiguous view off the 16-byte grid goes as it is."""
    w, u = arc_log_weights, utt_weights
    if w is not None:
        if not torch.is_tensor(w) or not w.is_floating_point():
            raise ValueError("arc_log_weights must be a float tensor [%d], got %s" % (K, getattr(w, "dtype", type(w))))
        if tuple(w.shape) != (K,):
            raise ValueError("arc_log_weights must have one entry per arc, [%d], got %s" % (K, list(w.shape)))
        w = w.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
    if u is not None:
        u = torch.as_tensor(u).detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
        if tuple(u.shape) != (B,):
            raise ValueError("utterance weights must have shape [%d], got %s" % (B, tuple(u.shape)))
    return w, u


def den_arc_counts(gt, num_states, x, lengths, leaky_coefficient=1e-5, arc_log_weights=None, utt_weights=None, with_grad=True,
                   grad_scale=1.0, grad_scale_dev=None, per_seq=False, *, form="lds"):
    """Expected arc counts of the denominator on the GPU (include/pychain_hip.h: pychain_hip_den_arc_counts), on the current
    stream.  `gt`: smbr_graph(...); `x` ([B,T,D], fp32 / bf16 / fp16) goes to the kernels as it is.  Returns (objf_per_seq
    float64 [B], counts float64 [K], counts_per_seq float64 [B,K] or None, grad in x's dtype or None, bad_count int32 [2]).
    `form`: "lds" - the entry point above, which refuses a graph and tree beyond the LDS of a CU -, or "auto", "rows", "global":
    pychain_hip_den_arc_counts_general with that form (any H, D; the bits of "lds" wherever both run)."""
    _require_device(x, "nnet_output")
    form_code = smbr_form_code(form, who="den_arc_counts")
    if x.dtype not in _DTYPE_CODE:
        raise ValueError("nnet_output must be float32, bfloat16 or float16, got %s" % x.dtype)
    x = x.detach().contiguous()
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    L = _lib.lib()
    dev = x.device
    H, K = int(num_states), int(gt[0].shape[0])
    with torch.cuda.device(dev):
        w, u = _arc_weight_args(arc_log_weights, utt_weights, K, B, dev)
        ld = _lengths_dev(lengths, dev)
        objf = torch.empty(B, dtype=torch.float64, device=dev)
        counts = torch.empty(K, dtype=torch.float64, device=dev)
        cps = torch.empty(B, K, dtype=torch.float64, device=dev) if per_seq else None
        grad = torch.empty_like(x) if with_grad else None
        bad = torch.empty(2, dtype=torch.int32, device=dev)
        grad_scale_dev = _dev_scalar(grad_scale_dev, dev)
        if form == "lds":
            ws = _workspace(L.pychain_hip_den_arc_counts_workspace_bytes(B, T, H, K), dev, "arcs")
        else:
            ws = _workspace(L.pychain_hip_den_arc_counts_general_workspace_bytes(B, T, H, K, D), dev, "arcs")
        args = (*[t.data_ptr() for t in gt], H, K, _ptr(w), x.data_ptr(), _DTYPE_CODE[x.dtype], ld.data_ptr(), B, T, D,
                float(leaky_coefficient), _ptr(u), float(grad_scale), _ptr(grad_scale_dev), _ptr(grad), objf.data_ptr(), counts.data_ptr(),
                _ptr(cps), bad.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        if form == "lds":
            _lib.check(L.pychain_hip_den_arc_counts(*args), "pychain_hip_den_arc_counts")
        else:
            _lib.check(L.pychain_hip_den_arc_counts_general(*args, form_code), "pychain_hip_den_arc_counts_general")
    return objf, counts, cps, grad, bad


def cpu_den_arc_counts(gt, num_states, x, lengths, leaky_coefficient=1e-5, arc_log_weights=None, utt_weights=None, with_grad=True,
                       grad_scale=1.0, per_seq=False, *, form="lds"):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_den_arc_counts), fp32 rows and gradient.  `form` is checked and
    changes nothing: the one host twin has no size limit."""
    smbr_form_code(form, "cpu_den_arc_counts")
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_den_arc_counts is for CPU tensors; device tensors run on the HIP kernels")
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    H, K = int(num_states), int(gt[0].shape[0])
    w, u = _arc_weight_args(arc_log_weights, utt_weights, K, B, torch.device("cpu"))
    objf = torch.empty(B, dtype=torch.float64)
    counts = torch.empty(K, dtype=torch.float64)
    cps = torch.empty(B, K, dtype=torch.float64) if per_seq else None
    grad = torch.empty(B, T, D, dtype=torch.float32) if with_grad else None
    bad = torch.zeros(2, dtype=torch.int32)
    _lib.check(_lib.lib().pychain_hip_cpu_den_arc_counts(
        *[t.data_ptr() for t in gt], H, K, _ptr(w), xf.data_ptr(), lc.data_ptr(), B, T, D, float(leaky_coefficient), _ptr(u),
        float(grad_scale), None, _ptr(grad), objf.data_ptr(), counts.data_ptr(), _ptr(cps), bad.data_ptr(), int(CPU_THREADS)),
        "pychain_hip_cpu_den_arc_counts")
    return objf, counts, cps, grad, bad


def _num_arc_weights(arc_log_weights, B, K, device):
    """arc_log_weights float32 [B,K] contiguous on `device` as the numerator's arc-count entry points read them (one element at
    a time: any element-aligned start); None stays None."""
    w = arc_log_weights
    if w is None:
        return None
    if not torch.is_tensor(w) or not w.is_floating_point():
        raise ValueError("arc_log_weights must be a float tensor [%d, %d], got %s" % (B, K, getattr(w, "dtype", type(w))))
    if tuple(w.shape) != (B, K):
        raise ValueError("arc_log_weights must have one entry per sequence and arc, [%d, %d], got %s" % (B, K, list(w.shape)))
    return w.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()


def num_arc_counts(gt, graph_stride, num_states, x, lengths, arc_log_weights=None, with_grad=False, grad_mode=_lib.GRAD_LINEAR,
                   grad_scale=1.0, grad_out=None, windows=None):
    """Expected arc counts of the numerator on the GPU (include/pychain_hip.h: pychain_hip_num_arc_counts), on the current stream,
    without a host synchronisation.  `gt`, `graph_stride`, `windows`: as num_forward_backward takes them; `arc_log_weights`:
    float [B,K] or None.  Returns (objf_per_seq float64 [B], counts_per_seq float64 [B,K], grad float32 [B,T,D] or None,
    bad_count int32 [2])."""
    _require_device(x, "nnet_output")
    x = _kernel_tensor(x)
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    K = gt["forward_transitions"].shape[1]
    L = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        w = _num_arc_weights(arc_log_weights, B, K, dev)
        x, xcode = _rows_as_given(x, lambda: L.pychain_hip_num_half_native(int(num_states), K, D))
        ld = _lengths_dev(lengths, dev)
        objf = torch.empty(B, dtype=torch.float64, device=dev)
        counts = torch.empty(B, K, dtype=torch.float64, device=dev)
        grad = None
        if grad_mode == _lib.GRAD_ACCUM:
            if grad_out is None:
                raise ValueError("GRAD_ACCUM needs grad_out")
            grad = grad_out
        elif with_grad:
            grad = torch.empty(x.shape, dtype=torch.float32, device=dev)
        gk, put_back = _kernel_buffer(grad)
        bad = torch.empty(2, dtype=torch.int32, device=dev)
        ws = _workspace(L.pychain_hip_num_arc_counts_workspace_bytes(B, T, int(num_states), K, D), dev, "num_arcs")
        if windows is not None:
            windows = _check_windows(windows, B, int(num_states), dev)
        _lib.check(L.pychain_hip_num_arc_counts(
            *_graph_ptrs(gt), int(graph_stride), x.data_ptr(), xcode, ld.data_ptr(), B, T, D, int(num_states), K, int(grad_mode),
            float(grad_scale), _ptr(w), objf.data_ptr(), _ptr(gk), counts.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(),
            _stream(dev), _ptr(windows)), "pychain_hip_num_arc_counts")
        put_back()
    return objf, counts, grad, bad


def cpu_num_arc_counts(graphs, x, lengths, arc_log_weights=None, with_grad=False, grad_mode=_lib.GRAD_LINEAR, grad_scale=1.0,
                       grad_out=None, windows=None):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_num_arc_counts).  `graphs`: the ChainGraphBatch."""
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_num_arc_counts is for CPU tensors; device tensors run on the HIP kernels")
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    ts, stride = _cpu_graph(graphs, False)
    H, K = int(ts[1].shape[-2]), int(ts[0].shape[-2])
    w = _num_arc_weights(arc_log_weights, B, K, torch.device("cpu"))
    objf = torch.empty(B, dtype=torch.float64)
    counts = torch.empty(B, K, dtype=torch.float64)
    grad = None
    if grad_mode == _lib.GRAD_ACCUM:
        if grad_out is None:
            raise ValueError("GRAD_ACCUM needs grad_out")
        grad = grad_out
    elif with_grad:
        grad = torch.empty(B, T, D, dtype=torch.float32)
    bad = torch.zeros(2, dtype=torch.int32)
    tw = None if windows is None else _check_windows(windows.cpu(), B, H)
    _lib.check(_lib.lib().pychain_hip_cpu_num_arc_counts(
        *[t.data_ptr() for t in ts], stride, xf.data_ptr(), lc.data_ptr(), B, T, D, H, K, int(grad_mode), float(grad_scale), _ptr(w),
        objf.data_ptr(), _ptr(grad), counts.data_ptr(), bad.data_ptr(), int(CPU_THREADS), _ptr(tw)), "pychain_hip_cpu_num_arc_counts")
    return objf, counts, grad, bad


def topk_rows(rows, lengths, k, floor=0.0, normalize=True):
    """Sparse targets out of dense posterior rows on the GPU (include/pychain_hip.h: pychain_hip_topk_rows), on the current
    stream: `rows` [B,T,D] in fp32 / bf16 / fp16 as it is.  Returns (pdfs int32 [B,T,k], probs float32 [B,T,k])."""
    _require_device(rows, "rows")
    if rows.dtype not in _DTYPE_CODE:
        raise ValueError("rows must be float32, bfloat16 or float16, got %s" % rows.dtype)
    rows = rows.detach().contiguous()      # (csrc/post.hip picks element-wise loads for a start off the 16-byte grid itself)
    B, T, D = rows.shape
    _check_lengths(lengths, B, T)
    dev = rows.device
    with torch.cuda.device(dev):
        ld = _lengths_dev(lengths, dev)
        pdfs = torch.empty(B, T, max(int(k), 0), dtype=torch.int32, device=dev)
        probs = torch.empty(B, T, max(int(k), 0), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().pychain_hip_topk_rows(
            rows.data_ptr(), _DTYPE_CODE[rows.dtype], ld.data_ptr(), B, T, D, int(k), float(floor), int(bool(normalize)),
            pdfs.data_ptr(), probs.data_ptr(), _stream(dev)), "pychain_hip_topk_rows")
    return pdfs, probs


def cpu_topk_rows(rows, lengths, k, floor=0.0, normalize=True):
    """The same on CPU tensors: the host twin (pychain_hip_cpu_topk_rows), fp32 rows."""
    if rows.is_cuda:
        raise RuntimeError("pychain_amd: cpu_topk_rows is for CPU tensors; device tensors run on the HIP kernels")
    rf, lc = _host_inputs(rows, lengths)
    B, T, D = rf.shape
    pdfs = torch.empty(B, T, max(int(k), 0), dtype=torch.int32)
    probs = torch.empty(B, T, max(int(k), 0), dtype=torch.float32)
    _lib.check(_lib.lib().pychain_hip_cpu_topk_rows(
        rf.data_ptr(), lc.data_ptr(), B, T, D, int(k), float(floor), int(bool(normalize)), pdfs.data_ptr(), probs.data_ptr(),
        int(CPU_THREADS)), "pychain_hip_cpu_topk_rows")
    return pdfs, probs


def align(gt, graph_stride, num_states, x, lengths, windows=None):
    """Viterbi alignment on the GPU (include/pychain_hip.h: pychain_hip_align).  `gt`: dict of device graph tensors; `windows`:
    int32 [B, H, 2] device time windows (pychain_hip_align_tw: the best path inside them) or None.
    Returns (score[B] float64, states[B,T+1] int32, pdfs[B,T] int64, bad_count[1] int32), all on x's device."""
    _require_device(x, "nnet_output")
    x = _kernel_tensor(x.detach())
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    K = gt["backward_transitions"].shape[1]
    L = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        x, xcode = _rows_as_given(x, lambda: L.pychain_hip_align_half_native(int(num_states), K, D))
        ld = _lengths_dev(lengths, dev)
        score = torch.empty(B, dtype=torch.float64, device=dev)
        states = torch.empty(B, T + 1, dtype=torch.int32, device=dev)
        pdfs = torch.empty(B, T, dtype=torch.int64, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(L.pychain_hip_align_workspace_bytes(B, T, int(num_states), K, D), dev, "align")
        if windows is not None:
            windows = _check_windows(windows, B, int(num_states), dev)
        _lib.check(L.pychain_hip_align_tw(
            *_graph_ptrs(gt), int(graph_stride),
            x.data_ptr(), xcode, ld.data_ptr(), B, T, D, int(num_states), K,
            score.data_ptr(), states.data_ptr(), pdfs.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev),
            _ptr(windows)), "pychain_hip_align_tw")
    return score, states, pdfs, bad


def cpu_align(graphs, x, lengths, windows=None):
    """Viterbi alignment on CPU tensors (the host twin, pychain_hip_cpu_align): same results, bit for bit, as `align` on the
    fp32 value of the same input.  `windows`: int32 [B, H, 2] time windows (pychain_hip_cpu_align_tw) or None.  Returns (score[B] float64, states[B,T+1] int32, pdfs[B,T] int64, bad_count[1] int32)."""
    if x.is_cuda:
        raise RuntimeError("pychain_amd: cpu_align is for CPU tensors; device tensors run on the HIP kernels")
    xf, lc = _host_inputs(x, lengths)
    B, T, D = xf.shape
    ts, stride = _cpu_graph(graphs, False)
    H, K = int(ts[1].shape[-2]), int(ts[0].shape[-2])
    score = torch.empty(B, dtype=torch.float64)
    states = torch.empty(B, T + 1, dtype=torch.int32)
    pdfs = torch.empty(B, T, dtype=torch.int64)
    bad = torch.zeros(1, dtype=torch.int32)
    tw = None if windows is None else _check_windows(windows.cpu(), B, H)
    _lib.check(_lib.lib().pychain_hip_cpu_align_tw(
        *[t.data_ptr() for t in ts], stride, xf.data_ptr(), lc.data_ptr(), B, T, D, H, K,
        score.data_ptr(), states.data_ptr(), pdfs.data_ptr(), bad.data_ptr(), int(CPU_THREADS), _ptr(tw)), "pychain_hip_cpu_align_tw")
    return score, states, pdfs, bad


def _chain_loss_args(plan, gt, graph_stride, num_states_num, x, lengths, leaky_coefficient, half_ok, windows):
    """What the two forms of the fused call share: the inputs as the kernels read them - checked -, the outputs both write and
    the arguments both begin with.  Returns (x, lengths on the device, den_objf [B], num_objf [B], bad_count [2], windows, K,
    the leading arguments: plan, leaky coefficient, numerator graphs, x, lengths, B, T, D)."""
    _require_device(x, "nnet_output")
    x = _kernel_tensor(x)
    B, T, D = x.shape
    _check_lengths(lengths, B, T)
    K = gt["forward_transitions"].shape[1]
    L = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        x, xcode = _rows_as_given(x, lambda: half_ok and L.pychain_hip_chain_loss_half_native(
            plan.stride, plan.slot_rows, plan.num_states, D, B, T, int(num_states_num), K))
        ld = _lengths_dev(lengths, dev)
        den_objf = torch.empty(B, dtype=torch.float32, device=dev)
        num_objf = torch.empty(B, dtype=torch.float32, device=dev)
        bad = torch.empty(2, dtype=torch.int32, device=dev)
    if windows is not None:
        windows = _check_windows(windows, B, int(num_states_num), dev)
    head = [plan.blob.data_ptr(), plan.stride, plan.slot_rows, plan.num_states, float(leaky_coefficient)] + _graph_ptrs(gt) + [
        int(graph_stride), int(num_states_num), K, x.data_ptr(), xcode, ld.data_ptr(), B, T, D]
    return x, ld, den_objf, num_objf, bad, windows, K, head


def chain_loss_forward_backward(plan, gt, graph_stride, num_states_num, x, lengths,
                                leaky_coefficient=1e-5, grad_scale=1.0, windows=None):
    """Fused ChainLoss: returns (den_objf[B], num_objf[B], grad[B,T,D] = grad_scale*(gamma_den - gamma_num),
    bad_count[2]).  The numerator recursion overlaps the denominator on a side stream.  `windows`: the numerator's device time
    windows (int32 [B, H, 2]) or None."""
    x, ld, den_objf, num_objf, bad, windows, K, head = _chain_loss_args(
        plan, gt, graph_stride, num_states_num, x, lengths, leaky_coefficient, True, windows)
    B, T, D = x.shape
    L = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        grad = torch.empty_like(x)
        dws = _workspace(L.pychain_hip_den_workspace_min_bytes(B, T, plan.num_states, D), dev, "den")   # (the fused loss never exp's rows ahead)
        nws = _workspace(L.pychain_hip_num_workspace_bytes(B, T, int(num_states_num), K, D), dev, "num")
        _lib.check(L.pychain_hip_chain_loss_forward_backward_xent(
            *head, float(grad_scale), den_objf.data_ptr(), num_objf.data_ptr(), grad.data_ptr(), bad.data_ptr(), 1.0, 0, 0,
            dws.data_ptr(), dws.numel(), nws.data_ptr(), nws.numel(), _stream(dev), _ptr(windows), None),
            "pychain_hip_chain_loss_forward_backward_xent")
    return den_objf, num_objf, grad, bad


class ChainLossState(object):
    """What `chain_loss_forward` leaves behind for `chain_loss_backward`: the stored
    trajectories (workspaces) and the handles of everything the occupancy passes read."""
    __slots__ = ("plan", "gt", "graph_stride", "num_states_num", "x", "lengths_dev", "den_ws", "num_ws", "shape",
                 "grad", "num_compat", "xent", "reg", "weighted")


def chain_loss_forward(plan, gt, graph_stride, num_states_num, x, lengths, leaky_coefficient=1e-5,
                       with_grad=False, grad_scale=1.0, loss_scale=1.0, norm_dev=None, half_ok=True, windows=None, xent=None):
    """Recursions (and, `with_grad`, the occupancy passes overlapped with them: state.grad =
    grad_scale * (gamma_den - gamma_num)).  Returns (den_objf[B], num_objf[B], bad_count[2], state, totals) with
    totals = device float[4] [(sum den - sum num) * loss_scale [/ norm_dev], frames, bad count, sum den - sum num]
    written by the call's last kernel (include/pychain_hip.h).  `windows`: the numerator's device time windows (int32
    [B, H, 2]) or None; chain_loss_backward reads the rows they shaped and needs them no more.
    `xent`: None, or (z, with_grad, c) - the numerator posteriors of the call as cross-entropy targets of z (include/pychain_hip.h:
    pychain_hip_xent): state.xent is then an XentResult (grad = -c * grad_scale [/ norm_dev] * d xent / dz, written by the same
    call), and totals[0] = totals[4] = the full loss, LF-MMI - c * xent, scaled alike."""
    # (`half_ok` False: a later chain_loss_backward on this state - it accumulates the numerator into an fp32 gradient)
    x, ld, den_objf, num_objf, bad, windows, K, head = _chain_loss_args(
        plan, gt, graph_stride, num_states_num, x, lengths, leaky_coefficient, half_ok, windows)
    B, T, D = x.shape
    L = _lib.lib()
    dev = x.device
    st = ChainLossState()
    with torch.cuda.device(dev):
        totals = torch.empty(_lib.TOTALS, dtype=torch.float32, device=dev)
        norm_dev = _dev_scalar(norm_dev, dev)
        # per-call workspaces (they must survive until backward); the caching allocator makes this cheap
        dws = torch.empty(L.pychain_hip_den_workspace_min_bytes(B, T, plan.num_states, D), dtype=torch.uint8, device=dev)
        nws = torch.empty(L.pychain_hip_num_workspace_bytes(B, T, int(num_states_num), K, D), dtype=torch.uint8,
                          device=dev)
        grad = torch.empty_like(x) if with_grad else None
        st.xent = arg = keep = st.reg = st.weighted = None
        if xent is not None:
            z, z_grad, c = xent
            st.xent = XentResult()
            arg, keep = _xent_arg(z, (B, T, D), num_states_num, K, z_grad, -float(c) * float(grad_scale), -float(c), st.xent)
        # (the widest entry point of the family; the narrower ones pass NULL on to it)
        _lib.check(L.pychain_hip_chain_loss_forward_xent(
            *head, den_objf.data_ptr(), num_objf.data_ptr(), _ptr(grad), float(grad_scale),
            bad.data_ptr(), float(loss_scale), _ptr(norm_dev), totals.data_ptr(),
            dws.data_ptr(), dws.numel(), nws.data_ptr(), nws.numel(), _stream(dev), _ptr(windows),
            None if arg is None else ctypes.addressof(arg)), "pychain_hip_chain_loss_forward_xent")
    st.grad = grad
    # (which numerator wrote the stored rows: backward runs on autograd's thread, where the caller's thread options do not reach)
    st.num_compat = _lib.get_option("num_compat") or "0"
    st.plan, st.gt, st.graph_stride, st.num_states_num = plan, gt, int(graph_stride), int(num_states_num)
    st.x, st.lengths_dev, st.den_ws, st.num_ws, st.shape = x, ld, dws, nws, (B, T, D, K)
    return den_objf, num_objf, bad, st, totals


def chain_loss_backward(st, grad_scale=1.0, grad_scale_dev=None):
    """Occupancy passes: grad[B,T,D] = grad_scale * grad_scale_dev * (gamma_den - gamma_num), written once.
    `grad_scale_dev`: optional 0-dim float32 device tensor (the upstream autograd gradient)."""
    B, T, D, K = st.shape
    L = _lib.lib()
    dev = st.x.device
    with torch.cuda.device(dev):
        grad = torch.empty_like(st.x)
        bad = torch.empty(2, dtype=torch.int32, device=dev)
        grad_scale_dev = _dev_scalar(grad_scale_dev, dev)
        with _lib.option("num_compat", st.num_compat):
            _lib.check(L.pychain_hip_chain_loss_backward(
                st.plan.blob.data_ptr(), st.plan.stride, st.plan.slot_rows, st.plan.num_states, *_graph_ptrs(st.gt, _GRAPH_FORWARD),
                st.graph_stride, st.num_states_num, K, st.x.data_ptr(), _DTYPE_CODE[st.x.dtype], st.lengths_dev.data_ptr(), B, T, D,
                float(grad_scale), _ptr(grad_scale_dev), grad.data_ptr(), bad.data_ptr(),
                st.den_ws.data_ptr(), st.den_ws.numel(), st.num_ws.data_ptr(), st.num_ws.numel(), _stream(dev)),
                "pychain_hip_chain_loss_backward")
    return grad, bad


def loss_total(den_objf, num_objf, scale=1.0, norm_dev=None):
    """(den_objf.sum() - num_objf.sum()) * scale [/ norm_dev] as a 0-dim device tensor, one launch
    (the scalar of ChainLoss.forward, loss.py:100-104)."""
    dev = den_objf.device
    out = torch.empty((), dtype=torch.float32, device=dev)
    norm_dev = _dev_scalar(norm_dev, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pychain_hip_loss_total(
            den_objf.data_ptr(), _ptr(num_objf), den_objf.numel(), float(scale), _ptr(norm_dev), out.data_ptr(), _stream(dev)),
            "pychain_hip_loss_total")
    return out


def totals_scalar(totals):
    """The call's scalar (totals[4], the second copy of totals[0]: include/pychain_hip.h) as a 0-dim tensor that is NOT an
    autograd view and shares no element with the statistics totals[:4]: a caller may `loss /= n` in place, as it may with
    the fresh tensor the reference returns (a view created inside a custom Function refuses in-place ops)."""
    return torch.empty((), dtype=totals.dtype, device=totals.device).set_(totals.untyped_storage(), totals.storage_offset() + 4, ())


def rescale_(t, scale_dev):
    """t *= scale_dev (0-dim device tensor), skipped on the device when the scalar is exactly 1."""
    scale_dev = _dev_scalar(scale_dev, t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().pychain_hip_rescale(t.data_ptr(), _DTYPE_CODE[t.dtype], t.numel(), scale_dev.data_ptr(), _stream(t.device)),
                   "pychain_hip_rescale")
    return t


# ---------------------------------------------------------------------------
# pychain_C-compatible surface (positional signatures of pychain.cc:26-41, :81-94)
# ---------------------------------------------------------------------------
def _check_contiguous(**named):
    """CHECK_CONTIGUOUS of pychain.cc:24,42-54,95-107: every tensor argument, RuntimeError with the
    reference's message.  One extension: the stride-0 batch views of `ChainGraphBatch(one_graph, B)`
    (the reference materialises them with .repeat, graph.py:104-119; here they are views of the single
    graph) count as contiguous when each row is - code that hands them on unchanged must keep working."""
    for n, t in named.items():
        if t.is_contiguous():
            continue
        if t.dim() >= 1 and t.stride(0) == 0 and t[0].is_contiguous():
            continue
        raise RuntimeError("%s must be contiguous" % n)


# The reference's loss.py calls pychain_C on EVERY training step with the same graph tensors.  Compiling the
# denominator plan (seconds for a C3-size graph) or re-uploading the numerator graphs per call would make
# that pattern ~1000x slower than the kernels, so both are memoised on what identifies the inputs:
# (data_ptr, _version, shape) of every tensor + pdf count + device.  A few entries, least recently used out.
_compat_cache = {}
_COMPAT_CACHE_ENTRIES = 8


def _tensors_key(tensors, extra):
    return tuple((t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride())) for t in tensors) + tuple(extra)


def _compat_cached(kind, tensors, extra, build):
    key = (kind,) + _tensors_key(tensors, extra)
    hit = _compat_cache.pop(key, None)
    if hit is None:
        hit = (build(), list(tensors))        # the tensors are kept alive: their data_ptr cannot be recycled
    _compat_cache[key] = hit                  # (re-)inserted last = most recently used
    while len(_compat_cache) > _COMPAT_CACHE_ENTRIES:
        _compat_cache.pop(next(iter(_compat_cache)))
    return hit[0]


class _RawGraphs(object):
    """The batched graph tensors of a pychain_C-style call as the object cpu_forward_backward reads."""
    shared_graph = None

    def __init__(self, named, log_domain):
        self.__dict__.update(named)
        self.log_domain = log_domain


def forward_backward(forward_transitions, forward_transition_indices, forward_transition_probs,
                     backward_transitions, backward_transition_indices, backward_transition_probs,
                     leaky_probs, initial_probs, final_probs, start_state, exp_nnet_output,
                     batch_sizes, sequence_lengths, num_states, leaky_hmm_coefficient=1.0e-05):
    """Same contract as `pychain_C.forward_backward`: pre-exponentiated input, returns
    [objf (0-dim), nnet_output_grad [B,T,D], ok (bool[1])]."""
    _check_contiguous(forward_transitions=forward_transitions, forward_transition_indices=forward_transition_indices,
                      forward_transition_probs=forward_transition_probs, backward_transitions=backward_transitions,
                      backward_transition_indices=backward_transition_indices,
                      backward_transition_probs=backward_transition_probs, leaky_probs=leaky_probs,
                      exp_nnet_output=exp_nnet_output, batch_sizes=batch_sizes, sequence_lengths=sequence_lengths,
                      initial_probs=initial_probs, final_probs=final_probs, start_state=start_state)
    names = _GRAPH6 + ["leaky_probs", "initial_probs", "final_probs"]
    vals = [forward_transitions, forward_transition_indices, forward_transition_probs,
            backward_transitions, backward_transition_indices, backward_transition_probs,
            leaky_probs, initial_probs, final_probs]
    if not exp_nnet_output.is_cuda:              # the reference's CPU path (chain-computation.cc:136-175,272-310): the host twin
        gb = _RawGraphs(dict(zip(names, vals)), log_domain=False)
        objf, grad, bad = cpu_forward_backward(gb, exp_nnet_output, sequence_lengths, leaky_hmm_coefficient, input_is_exp=True)
        return [objf.sum(), grad, bad == 0]
    D = exp_nnet_output.shape[2]
    dev = exp_nnet_output.device
    plan = _compat_cached("den", vals, (D, str(dev)), lambda: _plan.batch_plans(dict(zip(names, vals)), D, dev))
    objf, grad, bad = den_forward_backward(plan, exp_nnet_output, sequence_lengths,
                                           leaky_hmm_coefficient, input_is_exp=True)
    return [objf.sum(), grad, bad == 0]


def forward_backward_log_domain(forward_transitions, forward_transition_indices, forward_transition_probs,
                                backward_transitions, backward_transition_indices, backward_transition_probs,
                                initial_probs, final_probs, start_state, nnet_output,
                                batch_sizes, sequence_lengths, num_states):
    """Same contract as `pychain_C.forward_backward_log_domain`: returns
    [objf, log-grad [B,T,D] (-inf where zero), ok]."""
    _check_contiguous(forward_transitions=forward_transitions, forward_transition_indices=forward_transition_indices,
                      forward_transition_probs=forward_transition_probs, backward_transitions=backward_transitions,
                      backward_transition_indices=backward_transition_indices,
                      backward_transition_probs=backward_transition_probs, nnet_output=nnet_output,
                      batch_sizes=batch_sizes, sequence_lengths=sequence_lengths, initial_probs=initial_probs,
                      final_probs=final_probs, start_state=start_state)
    dev = nnet_output.device
    vals = [forward_transitions, forward_transition_indices, forward_transition_probs,
            backward_transitions, backward_transition_indices, backward_transition_probs,
            initial_probs, final_probs]
    if not nnet_output.is_cuda:                   # chain-log-domain-computation.cc:123-159,231-271: the host twin
        gb = _RawGraphs(dict(zip(_GRAPH8, vals)), log_domain=True)
        objf, lgrad, bad = cpu_forward_backward(gb, nnet_output, sequence_lengths, grad_mode=_lib.GRAD_LOG, clamp=False)
        return [objf.sum(), lgrad, bad == 0]
    gt = _compat_cached("num", vals, (str(dev),), lambda: {
        n: t.contiguous().to(dev) for n, t in zip(_GRAPH8, vals)})
    objf, lgrad, bad = num_forward_backward(gt, 1, num_states, nnet_output, sequence_lengths,
                                            grad_mode=_lib.GRAD_LOG)
    return [objf.sum(), lgrad, bad == 0]


def set_verbose_level(level):
    _lib.lib().pychain_hip_set_verbose_level(int(level))
