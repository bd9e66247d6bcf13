"""ctypes binding of libpychain_hip.so (include/pychain_hip.h).

There is NO fallback: if the shared library is missing, or a call is made with
tensors that are not on a HIP device, this raises.  The product path never
touches the CPU checker.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PYCHAIN_HIP_LIB") or os.path.join(_HERE, "libpychain_hip.so")  # env: kernel experiments only
ABI_VERSION = 32
TOTALS = 8            # floats of a `totals` buffer (include/pychain_hip.h: PYCHAIN_HIP_TOTALS)

GRAD_LOG, GRAD_LINEAR, GRAD_ACCUM = 0, 1, 2
CPU_NO_CLAMP = 0x100     # (host twin of the numerator only: include/pychain_hip.h)
F32, BF16, F16 = 0, 1, 2        # include/pychain_hip.h: PYCHAIN_HIP_F32 / _BF16 / _F16
SMBR_AUTO, SMBR_LDS, SMBR_ROWS, SMBR_GLOBAL = 0, 1, 2, 3     # include/pychain_hip.h: PYCHAIN_HIP_SMBR_*

_lib = None


class Xent(ctypes.Structure):
    """include/pychain_hip.h: pychain_hip_xent (the last argument of the *_xent entry points)."""
    _fields_ = [("z", ctypes.c_void_p), ("z_dtype", ctypes.c_int), ("xent_grad", ctypes.c_void_p), ("grad_scale", ctypes.c_float),
                ("grad_scale_dev", ctypes.c_void_p), ("loss_coef", ctypes.c_float), ("xent_objf_per_seq", ctypes.c_void_p),
                ("xent_totals", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


_vp, _i, _f, _sz, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_int64

# the argument groups the numerator, alignment and fused-loss entry points are made of (include/pychain_hip.h)
_GRAPHS = [_vp] * 8 + [_i]                       # ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride
_ROWS = [_vp, _i, _vp]                           # nnet_output, nnet_output_dtype, seq_lengths
_CPU_ROWS = [_vp, _vp]                           # (the host twins: fp32 rows)
_SIZES = [_i] * 5                                # B, T, D, H, K
_WS = [_vp, _sz]                                 # a workspace and its bytes
_DEN_PLAN = [_vp, _i64, _i, _i]                  # plans_dev, plan_stride_bytes, hint, den_H
_NUM_OUT = [_i, _f, _vp, _vp, _vp]               # grad_mode, grad_scale, objf_per_seq, grad, bad_count
_ALIGN_OUT = [_vp] * 4                           # score_per_seq, states, pdfs, bad_count
_NUM = _GRAPHS + _ROWS + _SIZES + _NUM_OUT + _WS + [_vp]                     # ..., stream
_ALIGN = _GRAPHS + _ROWS + _SIZES + _ALIGN_OUT + _WS + [_vp]
_CPU_NUM = _GRAPHS + _CPU_ROWS + _SIZES + _NUM_OUT + [_i]                    # ..., num_threads
_CPU_ALIGN = _GRAPHS + _CPU_ROWS + _SIZES + _ALIGN_OUT + [_i]
_FUSED_HEAD = _DEN_PLAN + [_f] + _GRAPHS + [_i, _i] + _ROWS + [_i] * 3       # plan, leaky, graphs, num_H, num_K, rows, B, T, D
_FUSED_TAIL = [_f, _vp, _vp] + _WS + _WS + [_vp]                             # loss_scale, loss_norm_dev, totals, den_ws, num_ws, stream
_FORWARD = _FUSED_HEAD + [_vp, _vp, _vp, _f, _vp] + _FUSED_TAIL              # den_objf, num_objf, grad, grad_scale, bad_count
_FORWARD_BACKWARD = _FUSED_HEAD + [_f] + [_vp] * 4 + _FUSED_TAIL             # grad_scale, den_objf, num_objf, grad, bad_count
_SMBR_GRAPH = [_vp] * 11 + [_i, _i]                                          # the nine graph tensors, pdf_arcs, pdf_index, H, K
_SMBR_CLASSES = [_vp, _i, _i]                                                # pdf_classes, num_classes, targets_are_classes
_SMBR_TAIL = [_vp, _vp, _i, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp]            # targets, K, frame_acc, coef, grad_scale[_dev], grad, acc, closing, bad
_ARC_TAIL = [_f, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]                          # coef, seq_weights, grad_scale[_dev], grad, objf, counts, counts_per_seq, bad

_NUM_ARC_OUT = [_i, _f, _vp, _vp, _vp, _vp, _vp]   # grad_mode, grad_scale, arc_log_weights, objf_per_seq, grad, counts_per_seq, bad_count

_SIGNATURES = {
    "pychain_hip_abi_version": (_i, []),
    "pychain_hip_last_error": (ctypes.c_char_p, []),
    "pychain_hip_set_verbose_level": (None, [_i]),
    "pychain_hip_get_verbose_level": (_i, []),
    "pychain_hip_set_den_phase_mask": (None, [_i]),
    "pychain_hip_set_den_lazy": (None, [_i]),
    "pychain_hip_den_kernel_names": (_i, [_i, _i, _i, _i, _i, ctypes.c_char_p, _sz]),
    "pychain_hip_set_option": (_i, [ctypes.c_char_p, ctypes.c_char_p]),
    "pychain_hip_set_thread_option": (_i, [ctypes.c_char_p, ctypes.c_char_p]),
    "pychain_hip_get_option": (_i, [ctypes.c_char_p, ctypes.c_char_p, _sz]),
    "pychain_hip_debug_launch_map": (_i, [_i, _i, _i, _i, _i, _vp, _i, _vp, _i]),
    "pychain_hip_debug_stream_rings": (_i, [_i, _vp, _i, _vp, _i]),
    "pychain_hip_debug_occupy": (_i, [_i, _i, _vp]),
    "pychain_hip_den_plan_build": (_i64, [_vp] * 9 + [_i, _i, _i, _vp, _sz]),
    "pychain_hip_den_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pychain_hip_den_workspace_min_bytes": (_sz, [_i, _i, _i, _i]),
    "pychain_hip_den_plan_info": (_i, [_vp, _sz, _vp]),
    "pychain_hip_den_uses_row_buffer": (_i, [_i64, _i, _i, _i, _i, _i, _i]),
    "pychain_hip_den_time_segments": (_i, [_i64, _i, _i, _i, _i, _i, _i]),
    "pychain_hip_den_forward_backward": (_i, [_vp, _i64, _i, _i, _i, _vp, _i, _i, _vp, _i, _i, _f, _f,
                                              _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pychain_hip_den_half_native": (_i, [_i64, _i, _i, _i, _i, _i]),
    "pychain_hip_num_half_native": (_i, [_i, _i, _i]),
    "pychain_hip_chain_loss_half_native": (_i, [_i64, _i, _i, _i, _i, _i, _i, _i]),
    "pychain_hip_chain_loss_slices": (_i, [_i64, _i, _i]),
    "pychain_hip_num_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "pychain_hip_num_forward_backward": (_i, _NUM),
    "pychain_hip_chain_loss_forward_backward": (_i, _FORWARD_BACKWARD),
    "pychain_hip_chain_loss_forward": (_i, _FORWARD),
    # (ABI 19: the same four with alignment time windows, one pointer more, last - include/pychain_hip.h)
    "pychain_hip_num_forward_backward_tw": (_i, _NUM + [_vp]),
    "pychain_hip_chain_loss_forward_backward_tw": (_i, _FORWARD_BACKWARD + [_vp]),
    "pychain_hip_chain_loss_forward_tw": (_i, _FORWARD + [_vp]),
    "pychain_hip_cpu_num_forward_backward_tw": (_i, _CPU_NUM + [_vp]),
    # (ABI 20: the same four with the numerator posteriors as cross-entropy targets, a pointer to a pychain_hip_xent more, last)
    "pychain_hip_xent_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "pychain_hip_num_forward_backward_xent": (_i, _NUM + [_vp, _vp]),
    "pychain_hip_chain_loss_forward_backward_xent": (_i, _FORWARD_BACKWARD + [_vp, _vp]),
    "pychain_hip_chain_loss_forward_xent": (_i, _FORWARD + [_vp, _vp]),
    "pychain_hip_cpu_num_forward_backward_xent": (_i, _CPU_NUM + [_vp, _vp]),
    # (ABI 21: output L2 and the out-of-range penalty over the network output itself)
    "pychain_hip_output_reg_workspace_bytes": (_sz, [_i, _i]),
    "pychain_hip_output_reg": (_i, [_vp, _i, _vp, _i, _i, _i, _f, _f, _f, _i, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, _sz, _vp]),
    "pychain_hip_cpu_output_reg": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _f, _i, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _i]),
    # (ABI 22: utterance weights and per-frame derivative weights over a gradient already written, and the weighted sums)
    "pychain_hip_weight_rows": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "pychain_hip_cpu_weight_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _f, _f, _f, _vp, _vp, _vp, _i]),
    # (ABI 23: sparse posterior targets as the numerator behind a denominator call, and the top-k rows that make them)
    "pychain_hip_post_targets_workspace_bytes": (_sz, [_i, _i]),
    "pychain_hip_post_targets": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _sz, _vp]),
    "pychain_hip_cpu_post_targets": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i]),
    "pychain_hip_topk_rows": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp]),
    "pychain_hip_cpu_topk_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, _i]),
    # (ABI 24: cross-entropy of a network output against sparse targets - posterior targets, alignments - and its totals step)
    "pychain_hip_xent_targets_workspace_bytes": (_sz, [_i, _i]),
    "pychain_hip_xent_targets": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pychain_hip_xent_add_totals": (_i, [_vp, _i, _f, _vp, _f, _vp, _vp, _vp, _vp]),
    "pychain_hip_cpu_xent_targets": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp, _i]),
    # (ABI 25: the rows of the boosted denominator - exp(clamp(x)) with the targeted elements scaled by exp(-boost * a))
    "pychain_hip_boost_rows": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "pychain_hip_cpu_boost_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _f, _vp, _vp, _i]),
    # (ABI 27: lattice-free sMBR - the frame accuracies under the denominator's occupancies, the accuracy-weighted recursions)
    "pychain_hip_smbr_workspace_bytes": (_sz, [_i, _i, _i]),
    "pychain_hip_smbr_frame_accuracy": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "pychain_hip_smbr_forward_backward": (_i, _SMBR_GRAPH + _ROWS + [_i] * 3 + _SMBR_TAIL + _WS + [_vp]),
    "pychain_hip_cpu_smbr_frame_accuracy": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i]),
    "pychain_hip_cpu_smbr_forward_backward": (_i, _SMBR_GRAPH + _CPU_ROWS + [_i] * 3 + _SMBR_TAIL + [_i]),
    # (ABI 28: the same with the accuracy by class - pdf_classes, num_classes, targets_are_classes more, last; the accuracy pass
    # then takes a workspace)
    "pychain_hip_smbr_frame_accuracy_classes_workspace_bytes": (_sz, [_i, _i]),
    "pychain_hip_smbr_lds_bytes": (_sz, [_i, _i, _i]),
    "pychain_hip_smbr_frame_accuracy_classes": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp] + _SMBR_CLASSES + _WS),
    "pychain_hip_smbr_forward_backward_classes": (_i, _SMBR_GRAPH + _ROWS + [_i] * 3 + _SMBR_TAIL + _WS + [_vp] + _SMBR_CLASSES),
    "pychain_hip_cpu_smbr_frame_accuracy_classes": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i] + _SMBR_CLASSES),
    "pychain_hip_cpu_smbr_forward_backward_classes": (_i, _SMBR_GRAPH + _CPU_ROWS + [_i] * 3 + _SMBR_TAIL + [_i] + _SMBR_CLASSES),
    "pychain_hip_smbr_form": (_i, [_i, _i, _i, _i]),
    "pychain_hip_smbr_general_lds_bytes": (_sz, [_i]),
    "pychain_hip_smbr_general_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "pychain_hip_smbr_forward_backward_general": (_i, _SMBR_GRAPH + _ROWS + [_i] * 3 + _SMBR_TAIL + _WS + [_vp] + _SMBR_CLASSES + [_i]),
    # (ABI 30: expected arc counts - the gradient of the denominator objective in the arc weights of its graph)
    "pychain_hip_den_arc_counts_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pychain_hip_den_arc_counts_lds_bytes": (_sz, [_i, _i]),
    "pychain_hip_den_arc_counts": (_i, _SMBR_GRAPH + [_vp] + _ROWS + [_i] * 3 + _ARC_TAIL + _WS + [_vp]),
    "pychain_hip_cpu_den_arc_counts": (_i, _SMBR_GRAPH + [_vp] + _CPU_ROWS + [_i] * 3 + _ARC_TAIL + [_i]),
    "pychain_hip_den_arc_counts_general_lds_bytes": (_sz, [_i]),
    "pychain_hip_den_arc_counts_form": (_i, [_i, _i, _i]),
    "pychain_hip_den_arc_counts_general_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "pychain_hip_den_arc_counts_general": (_i, _SMBR_GRAPH + [_vp] + _ROWS + [_i] * 3 + _ARC_TAIL + _WS + [_vp, _i]),
    # (ABI 32: expected arc counts of the numerator - the gradient of log P_b in per-sequence arc log-weights)
    "pychain_hip_num_arc_counts_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "pychain_hip_num_arc_counts": (_i, _GRAPHS + _ROWS + _SIZES + _NUM_ARC_OUT + _WS + [_vp, _vp]),      # ..., stream, time_windows
    "pychain_hip_cpu_num_arc_counts": (_i, _GRAPHS + _CPU_ROWS + _SIZES + _NUM_ARC_OUT + [_i, _vp]),   # ..., num_threads, time_windows
    "pychain_hip_cpu_calls": (ctypes.c_long, []),
    "pychain_hip_cpu_den_forward_backward": (_i, [_vp] * 9 + [_i, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _i]),
    "pychain_hip_cpu_num_forward_backward": (_i, _CPU_NUM),
    "pychain_hip_align_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "pychain_hip_align": (_i, _ALIGN),
    "pychain_hip_align_half_native": (_i, [_i, _i, _i]),
    "pychain_hip_cpu_align": (_i, _CPU_ALIGN),
    # (ABI 26: the same two under alignment time windows, one pointer more, last)
    "pychain_hip_align_tw": (_i, _ALIGN + [_vp]),
    "pychain_hip_cpu_align_tw": (_i, _CPU_ALIGN + [_vp]),
    "pychain_hip_den_tseg_state": (_i, [_vp, _vp]),
    "pychain_hip_den_tseg_state_bytes": (_sz, []),
    "pychain_hip_rescale": (_i, [_vp, _i, _sz, _vp, _vp]),
    "pychain_hip_loss_total": (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp]),
    "pychain_hip_chain_loss_backward": (_i, _DEN_PLAN + [_vp, _vp, _vp, _i, _i, _i] + _ROWS + [_i] * 3      # ft, fi, fp, stride, num_H, num_K
                                        + [_f, _vp, _vp, _vp] + _WS + _WS + [_vp]),     # grad_scale, grad_scale_dev, grad, bad_count
    "pychain_hip_batch_layout": (_i64, [_i, _i, _i, _i, _vp, _vp]),
    "pychain_hip_batch_pack": (_i, [_i, _i, _i, _i, _vp, _vp, _sz]),
    "pychain_hip_batch_reorder": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pychain_hip_batch_reorder_dev": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pychain_hip_fst_read": (_vp, [ctypes.c_char_p, _i64]),
    "pychain_hip_fst_from_arcs": (_vp, [ctypes.c_int32, ctypes.c_int32, _i64, _vp, _vp, _vp, _vp, _vp]),
    "pychain_hip_fst_free": (None, [_vp]),
    "pychain_hip_fst_write": (_i, [_vp, ctypes.c_char_p]),
    "pychain_hip_fst_num_states": (ctypes.c_int32, [_vp]),
    "pychain_hip_fst_start": (ctypes.c_int32, [_vp]),
    "pychain_hip_fst_num_arcs": (_i64, [_vp]),
    "pychain_hip_fst_to_tensors": (_i, [_vp, _i] + [_vp] * 7),
    "pychain_hip_fst_leaky_probs": (_i, [_vp, _vp]),
}
EXPORTS = tuple(_SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "pychain_amd: %s is missing. Build it with `python -m pychain_amd.build_ext` "
                "(needs hipcc; cross-compiles for gfx950 without a GPU). There is no CPU fallback."
                % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        v = l.pychain_hip_abi_version()
        if v != ABI_VERSION:
            raise ImportError("pychain_amd: libpychain_hip.so has ABI %d, expected %d" % (v, ABI_VERSION))
        _lib = l
        # tuning scripts set PYCHAIN_<OPTION> in the environment: read ONCE here, never on the call path
        for name in OPTIONS:
            v = os.environ.get("PYCHAIN_" + name.upper())
            if v:
                l.pychain_hip_set_option(name.encode(), v.encode())
    return _lib


OPTIONS = ("verbose", "den_phase_mask", "den_lazy", "den_dma", "den_segments", "den_pair", "gamma16", "debug_corrupt_row", "num_compat", "den_tseg", "den_tburn", "plan_split", "chain_slices", "den_sg", "den_cross", "den_q", "num_arcs_gather")

_thread_values = threading.local()       # what this thread's overrides currently are (for restoring)


def get_option(name):
    """The value of a library option in effect for the calling thread (None = unset)."""
    buf = ctypes.create_string_buffer(256)
    n = check(lib().pychain_hip_get_option(name.encode(), buf, 256), "pychain_hip_get_option")
    return buf.value.decode() if n > 0 else None


class option(object):
    """`with _lib.option("den_segments", 3): ...` - a test / tuning option of the library for the duration of a
    block, FOR THE CALLING THREAD ONLY (include/pychain_hip.h: pychain_hip_set_thread_option); the previous
    override - or the process-wide default, e.g. one taken from PYCHAIN_<NAME> at load time - is back afterwards."""

    def __init__(self, name, value=1):
        self.name, self.value = name, value

    def __enter__(self):
        d = _thread_values.__dict__.setdefault("v", {})
        self.prev = d.get(self.name)
        d[self.name] = str(self.value)
        check(lib().pychain_hip_set_thread_option(self.name.encode(), str(self.value).encode()),
              "pychain_hip_set_thread_option")
        return self

    def __exit__(self, *exc):
        d = _thread_values.__dict__.setdefault("v", {})
        if self.prev is None:
            d.pop(self.name, None)
            lib().pychain_hip_set_thread_option(self.name.encode(), None)
        else:
            d[self.name] = self.prev
            lib().pychain_hip_set_thread_option(self.name.encode(), self.prev.encode())
        return False


def den_kernel_names(slot_rows, num_states, num_pdfs, batch, plans_shared=True, fused=False):
    """("recursion kernel", "occupancy kernel") a denominator call of this shape would launch (`fused`: as part of a fused loss)."""
    buf = ctypes.create_string_buffer(128)
    check(lib().pychain_hip_den_kernel_names(int(slot_rows), int(num_states), int(num_pdfs), int(batch),
                                             int(bool(plans_shared)) | (2 if fused else 0), buf, 128), "pychain_hip_den_kernel_names")
    rec, occ = buf.value.decode().split(",")
    return rec, occ


class PychainHipError(RuntimeError):
    pass


def check(rc, what):
    if rc < 0:
        raise PychainHipError("%s failed (%d): %s" % (what, rc, lib().pychain_hip_last_error().decode()))
    return rc
