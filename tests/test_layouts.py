"""Views, slices and tensors off the 16-byte grid through every public entry point, CPU tensors on the host twins: the matrix
of tests/layout_cases.py (what a case asserts is written there) on a machine without a GPU, and the layout functions themselves
(tests/layouts.py).  The host twins have no alignment requirement: a failure here is a stride bug."""
import pytest
import torch

import layout_cases as lc
import layouts as ly
from helpers import record_parity

DEV = "cpu"
NEW = ("smbr_pdf", "smbr_pdf_host_targets", "smbr_loss_devlen", "smbr_classes", "smbr_classes_int64", "smbr_classes_host_map",
       "smbr_class_targets", "viterbi_windows_own", "viterbi_windows_explicit", "viterbi_windows_explicit_int64", "upstream_smbr")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64])
@pytest.mark.parametrize("shape", [(), (4,), (4, 23), (4, 23, 41), (4, 23, 40), (4, 7, 2)])
def test_the_layout_functions(shape, dtype):
    """every layout: the input's values, shape and dtype; is_contiguous() and data_ptr() % 16 as its name promises; everything
    else in the buffer is poison"""
    g = torch.Generator().manual_seed(len(shape))
    t = (torch.randn(shape, generator=g) * 3).to(dtype) if dtype.is_floating_point else torch.randint(0, 50, shape, generator=g).to(dtype)
    for name, make in ly.LAYOUTS.items():
        if not ly.applies(name, len(shape), True):
            continue
        if len(shape) == 0 and name != "fresh" and name not in ly.OFFSETS:
            continue
        src = t[..., :1].expand(shape).contiguous() if name == "expanded" else t
        v = make(src)
        assert v.shape == src.shape and v.dtype == src.dtype and v.device == src.device and torch.equal(v, src), name
        assert v.is_contiguous() == ly.is_contiguous(name, shape), name
        base = ly.base_of(v)
        assert base.data_ptr() % 16 == 0 and base.is_contiguous()
        assert v.data_ptr() % 16 == (ly.element_offset(name, shape) * src.element_size()) % 16, name
        assert (v.data_ptr() - base.data_ptr()) == v.storage_offset() * src.element_size()
        out = ly.outside(v)
        assert out.numel() == base.numel() - (src[..., :1].numel() if name == "expanded" else src.numel()), name
        assert ly.is_poison(out, src), name
        if name == "fresh":
            assert base is v and v.data_ptr() != t.data_ptr()
        elif name != "time_major":                    # (a transposed buffer has no element outside the view)
            assert out.numel() > 0
        if dtype.is_floating_point:
            leaf = make(src, leaf=True)
            assert ly.base_of(leaf).requires_grad and ly.base_of(leaf).is_leaf and torch.equal(leaf.detach(), src)
    # the byte offsets the offset layouts are there for
    if len(shape) == 3 and dtype in (torch.float32, torch.bfloat16):
        want = [4, 8, 12, 0] if dtype == torch.float32 else [2, 4, 6, 8]
        assert [ly.LAYOUTS[n](t).data_ptr() % 16 for n in ly.OFFSETS] == want
    if shape == (4, 23, 41) and dtype == torch.float32:
        assert ly.LAYOUTS["batch_slice"](t).data_ptr() % 16 == 12 and ly.LAYOUTS["head_hi"](t).storage_offset() % 2 == 0
    assert ly.LAYOUTS["expanded"](torch.ones(4, 23)).stride() == (3, 0) if len(shape) == 2 else True


def test_the_matrix_covers_every_entry_and_layout():
    names = {e.name for e in lc.ENTRIES if not e.gpu_only}
    seen = {}
    for name, mode, layout in lc.matrix(DEV):
        seen.setdefault(name, set()).add(layout)
    assert set(seen) == names
    for e in lc.ENTRIES:
        if e.gpu_only:
            continue
        for a in e.args:
            assert set(lc.arg_layouts(a)) <= seen[e.name], (e.name, a)
        for layout in seen[e.name]:
            assert lc.variants(e, layout), (e.name, layout)
    lay, eq = lc.variants(lc.BY_NAME["loss_all"], "everything")[0]
    assert len(set(lay.values())) == len(lay) == 4 and "fresh" not in lay.values()
    # sMBR, the class maps and windowed alignment: every listed argument in every layout of its dimensionality, one at a time,
    # and all of an entry's arguments at once, each in a layout of its own
    one_dim = ["offset_1", "offset_2", "offset_3", "offset_4", "batch_slice", "batch_step", "head_lo", "head_hi"]
    for a in lc.CLASS_MAPS + ("lengths",):
        assert lc.arg_layouts(a) == one_dim, a                         # (a map is never `expanded`)
    for a in ("x", "x_in", "pdfs", "probs", "cls_pdfs", "hpdfs", "hprobs", "windows", "windows64"):
        assert lc.arg_layouts(a) == lc.NON_FRESH[:-1] and lc.NON_FRESH[-1] == "expanded", a
    assert set(NEW) <= {e.name for e in lc.ENTRIES}
    for name in NEW:
        e = lc.BY_NAME[name]
        for a in e.args:
            for layout in lc.arg_layouts(a):
                assert [lay for lay, _ in lc.variants(e, layout) if lay == {a: layout}], (name, a, layout)
        if len(e.args) > 1:
            (lay, eq), = lc.variants(e, "everything")
            assert sorted(lay) == sorted(e.args) and len(set(lay.values())) == len(lay) and "fresh" not in lay.values() and not eq
            assert (name, e.modes[0], "everything") in lc.matrix(DEV) or e.gpu_only


def _record(name, **d):
    record_parity(name.replace("layouts_", "layouts_cpu_", 1), **d)


def _controls(dev):
    return [(e.name, m) for e in lc.ENTRIES if not (e.gpu_only and dev == "cpu") for m in lc.entry_modes(e, dev)]


@pytest.mark.parametrize("D,dname", lc.CONFIGS)
@pytest.mark.parametrize("name,mode", _controls(DEV))
def test_control_is_stable_and_meets_its_float64_reference(name, mode, D, dname):
    e = lc.BY_NAME[name]
    lc.fresh_is_stable(e, DEV, D, dname, mode)
    ctl = lc.control(e, DEV, D, dname, mode)
    assert ("per_seq" in ctl.values) == ("closing" in ctl.values) == (e.ref in lc.SMBR_REFS)       # (no other result carries the names)
    d = lc.check_reference(e, ctl, DEV, D, dname, mode, record=_record if name in NEW else None)
    print(name, mode, D, dname, d)


def _make(entry, dev, cases):
    @pytest.mark.parametrize("D,dname", lc.CONFIGS)
    @pytest.mark.parametrize("mode,layout", cases)
    def test(mode, layout, D, dname):
        for lay, eq in lc.variants(entry, layout):
            res = lc.run(entry, dev, D, dname, mode, lay, eq)
            lc.assert_same(res, lc.control(entry, dev, D, dname, mode, eq), "%s %s %s" % (entry.name, mode, lay))
    test.__name__ = "test_" + entry.name
    return test


for _e in lc.ENTRIES:
    _cases = [(m, l) for n, m, l in lc.matrix(DEV) if n == _e.name]
    if _cases:
        globals()["test_" + _e.name] = _make(_e, DEV, _cases)


@pytest.mark.parametrize("D,dname", lc.CONFIGS)
def test_two_heads_of_one_layer(D, dname):
    loss, wide, ctl = lc.two_heads(DEV, D, dname, None)
    # (autograd ADDS the two heads' gradients at the leaf: a -0 of a padded row meets the other head's +0 and becomes +0 - the
    # values are compared, which differs from the bits in the sign of a zero only)
    assert lc.same_bits(loss, ctl.values["loss"])
    assert torch.equal(wide[..., :D], ctl.grads["x"]["inside"]) and torch.equal(wide[..., D + 1:], ctl.grads["z"]["inside"])
    assert not bool(wide[..., D].any()) and wide.dtype == lc.DTYPES[dname]
