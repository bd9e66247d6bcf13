"""Views, slices and tensors off the 16-byte grid through every public entry point, device tensors on the HIP kernels: the
matrix of tests/layout_cases.py (what a case asserts, and which float64 reference each control is held to, is written there).
The HIP entry points whose kernels read and write rows 16 bytes at a time refuse a pointer that is not 16-byte aligned
(include/pychain_hip.h says so entry point by entry point: the denominator, the numerator, alignment, the xent, target, boost,
weight and regulariser passes), and a contiguous view with a storage offset is such a pointer - `y[1:]` at an odd T * D,
`buf[o:o + n].view(B, T, D)`, one head of a two-headed layer: the Python layer hands those kernels an aligned contiguous tensor in
its place (native._kernel_tensor), at the cost of one copy of that tensor, and leaves an aligned contiguous one exactly as it
is.  Three take an element-aligned pointer as it comes: pychain_hip_smbr_forward_backward[_classes] reads the network output one
element at a time (native.smbr passes a contiguous view on, 2-byte rows at 2 / 4 / 6-byte offsets included), pychain_hip_topk_rows
picks element loads for rows off the grid itself, and the time windows of the *_tw entry points are read by element.  The class
map of pychain_hip_smbr_frame_accuracy_classes is different: its pass has a 16-byte and an element form whose fp64 sums run in
another order, so native.smbr_classes always hands over an aligned map (test_a_class_map_off_the_grid_...).

Every entry was found bit-stable control against control (test_control_is_stable_and_meets_its_float64_reference asserts it on
every route), so every layout case is held to its control to the bit."""
import pytest
import torch

import layout_cases as lc
import layouts as ly
from helpers import record_parity
from pychain_amd import _lib, native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _controls():
    return [(e.name, m) for e in lc.ENTRIES for m in lc.entry_modes(e, DEV)]


@pytest.mark.parametrize("D,dname", lc.CONFIGS)
@pytest.mark.parametrize("name,mode", _controls())
def test_control_is_stable_and_meets_its_float64_reference(name, mode, D, dname):
    e = lc.BY_NAME[name]
    lc.inputs(D, dname)                                              # (made on the host, by the host twins: before the count)
    calls = _lib.lib().pychain_hip_cpu_calls()
    lc.fresh_is_stable(e, DEV, D, dname, mode)
    assert _lib.lib().pychain_hip_cpu_calls() == calls               # (the kernels, not the host twins)
    ctl = lc.control(e, DEV, D, dname, mode)
    assert ("per_seq" in ctl.values) == ("closing" in ctl.values) == (e.ref in lc.SMBR_REFS)       # (no other result carries the names)
    d = lc.check_reference(e, ctl, DEV, D, dname, mode, record=record_parity)
    print(name, mode, D, dname, d)


def _make(entry, cases):
    @pytest.mark.parametrize("D,dname", lc.CONFIGS)
    @pytest.mark.parametrize("mode,layout", cases)
    def test(mode, layout, D, dname):
        for lay, eq in lc.variants(entry, layout):
            res = lc.run(entry, DEV, D, dname, mode, lay, eq)
            lc.assert_same(res, lc.control(entry, DEV, D, dname, mode, eq), "%s %s %s" % (entry.name, mode, lay))
    test.__name__ = "test_" + entry.name
    return test


for _e in lc.ENTRIES:
    globals()["test_" + _e.name] = _make(_e, [(m, l) for n, m, l in lc.matrix(DEV) if n == _e.name])


@pytest.mark.parametrize("D,dname", lc.CONFIGS)
@pytest.mark.parametrize("mode", lc.GRAPH_MODES)
def test_two_heads_of_one_layer(mode, D, dname):
    """x = wide[..., :D], z = wide[..., D + 1:] of one leaf: wide.grad holds both gradients and a zero column between them"""
    loss, wide, ctl = lc.two_heads(DEV, D, dname, mode)
    # (autograd ADDS the two heads' gradients at the leaf: a -0 of a padded row meets the other head's +0 and becomes +0 - the
    # values are compared, which differs from the bits in the sign of a zero only)
    assert lc.same_bits(loss, ctl.values["loss"])
    assert torch.equal(wide[..., :D], ctl.grads["x"]["inside"]) and torch.equal(wide[..., D + 1:], ctl.grads["z"]["inside"])
    assert not bool(wide[..., D].any()) and wide.dtype == lc.DTYPES[dname]


@pytest.mark.parametrize("layout", ["offset_1", "offset_2", "offset_3", "batch_slice"])
@pytest.mark.parametrize("D,dname", [(41, "float32"), (40, "bfloat16")])
def test_a_callers_buffer_off_the_grid_is_updated_in_place(D, dname, layout):
    """native.weight_rows / output_reg (ACCUM) / post_targets / boost_rows / num_forward_backward (ACCUM) update a buffer of the
    caller's: one that is contiguous but starts off the 16-byte grid gets the bits an aligned one gets, and nothing around it
    is touched"""
    inp = lc.inputs(D, dname)
    dev = torch.device(DEV)
    x, lengths = inp.v["x"].to(dev), inp.lengths
    pd, pq, u, f = inp.v["pdfs"].to(dev), inp.v["probs"].to(dev), inp.v["u"].to(dev), inp.v["f"].to(dev)
    gt = inp.num.device_tensors(dev)
    passes = {
        "weight_rows": (inp.v["gy"], lambda g: native.weight_rows(g, lengths, u, f)),
        "output_reg": (inp.v["gy"], lambda g: native.output_reg(x, lengths, lc.L2, lc.OOR, grad=g, grad_mode=_lib.GRAD_ACCUM)),
        "post_targets": (inp.v["gy"], lambda g: native.post_targets(x, lengths, pd, pq, grad=g, grad_scale=-0.5)),
        "boost_rows": (torch.zeros(x.shape), lambda e: native.boost_rows(x, lengths, pd, pq, lc.BOOST, out=e)),
        "num_accum": (inp.v["gy"].float(), lambda g: native.num_forward_backward(gt, 1, inp.num.num_states, x, lengths,
                                                                                 grad_mode=_lib.GRAD_ACCUM, grad_scale=-1.0, grad_out=g)),
    }
    for name, (start, run) in passes.items():
        want = ly.LAYOUTS["fresh"](start.to(dev))
        got = ly.LAYOUTS[layout](start.to(dev))
        assert got.is_contiguous()
        run(want)
        run(got)
        torch.cuda.synchronize()
        assert lc.same_bits(got.cpu(), want.cpu()), (name, layout)
        assert ly.is_poison(ly.outside(got), got), (name, layout, "written outside the buffer")


@pytest.mark.parametrize("layout", ["offset_1", "offset_2", "offset_3", "head_hi"])
def test_a_class_map_off_the_grid_gives_the_bits_of_the_aligned_map(layout):
    """D = 40, fp32: the class accuracy pass reads gamma and the map 16 bytes at a time where both start on the grid and one
    element at a time otherwise, and the two forms sum a frame's products in fp64 in another order (csrc/smbr.hip:
    launch_smbr_frame_acc).  An int32 device map that is a contiguous view 4 / 8 / 12 bytes off the grid must not pick another form
    than the aligned map of the control: the same bits in per_seq, closing, bad_count and x.grad."""
    D, dname = 40, "float32"
    e = lc.BY_NAME["smbr_classes"]
    view = ly.LAYOUTS[layout](lc.inputs(D, dname).v["classes"].to(DEV))
    assert D % 4 == 0 and view.dtype == torch.int32 and view.is_cuda and view.is_contiguous() and view.data_ptr() % 16 != 0
    ctl = lc.control(e, DEV, D, dname)
    calls = _lib.lib().pychain_hip_cpu_calls()
    res = lc.run(e, DEV, D, dname, None, {"classes": layout})
    assert _lib.lib().pychain_hip_cpu_calls() == calls
    for k in ("per_seq", "closing", "bad_count", "loss"):
        assert lc.same_bits(res.values[k], ctl.values[k]), (layout, k, lc.bits(res.values[k]), lc.bits(ctl.values[k]))
    assert lc.same_bits(res.grads["x"]["inside"], ctl.grads["x"]["inside"]), (layout, "x.grad")
    assert native.smbr_classes(view, D, view.device)[0].data_ptr() % 16 == 0          # (how: the kernels are handed an aligned map)
