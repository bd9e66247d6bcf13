"""The tensors a training loop hands over, for the layout tests (tests/test_layouts.py, tests/test_gpu_layouts.py): views, slices
and tensors that do not start on a 16-byte boundary.

LAYOUTS maps a name to `make(t, leaf=False, poison=None) -> view`: a view with exactly the values, shape, dtype and device of
`t` that lives in a larger buffer, every element of the buffer outside the view being POISON - NaN for float tensors, and for
integer tensors `poison` (default: -7 for int32, the pdfs' and windows' type; 2^40, a huge length, for int64).  A call that reads
anything outside the view shows it.  `leaf` True: the BUFFER is the autograd leaf (requires_grad) and the view a differentiable
view of it - the gradient must land in the buffer, inside the view, and be exactly zero outside.  `base_of(view)` is the buffer.

  fresh         a contiguous clone: the control (its own buffer, nothing outside)
  offset_1..4   a flat buffer of numel + 8 elements viewed at that ELEMENT offset: contiguous, 4 / 8 / 12 / 16 bytes off for
                4-byte types (the last one aligned again), 2 / 4 / 6 / 8 for 2-byte types
  batch_slice   big[1:-1] of [B + 2, ...]: contiguous, off by one sequence
  batch_step    big[::2] of [2 B, ...]: not contiguous
  time_major    a contiguous [T, B, ...] buffer transposed (tensors of two or more dimensions)
  time_slice    big[:, 2:2 + T] of [B, T + 3, ...] (two or more dimensions)
  head_lo / _hi wide[..., :D] and wide[..., D + 1:] of [..., 2 D + 1]: the two heads of one layer, the odd gap giving the second
                an odd element offset
  expanded      stride 0 along the last dimension (offset 1 in a [..., 3] buffer): only for tensors whose values along it are
                equal - utterance weights that are all alike, frame weights constant over an utterance
"""
import torch

INT_POISON = {torch.int32: -7, torch.int64: 2 ** 40}


def poison_of(t, poison=None):
    if t.is_floating_point():
        return float("nan")
    return INT_POISON[t.dtype] if poison is None else poison


def _layout(alloc, view):
    """alloc(shape) -> the buffer's shape; view(buffer, shape) -> the view of `shape` in it"""
    def make(t, leaf=False, poison=None):
        shape = tuple(t.shape)
        buf = torch.full(alloc(shape), poison_of(t, poison), dtype=t.dtype, device=t.device)
        view(buf, shape).copy_(t.detach())
        if leaf:
            buf.requires_grad_(True)
        return view(buf, shape)
    return make


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _fresh(t, leaf=False, poison=None):
    c = t.detach().clone(memory_format=torch.contiguous_format)
    return c.requires_grad_(True) if leaf else c


def _offset(k):
    return _layout(lambda s: (_numel(s) + 8,), lambda b, s: b[k:k + _numel(s)].view(s))


def _expanded(t, leaf=False, poison=None):
    assert t.dim() >= 1 and bool((t == t[..., :1]).all()), "expanded: the values along the last dimension must be equal"
    buf = torch.full(tuple(t.shape[:-1]) + (3,), poison_of(t, poison), dtype=t.dtype, device=t.device)
    buf[..., 1:2] = t.detach()[..., :1]
    if leaf:
        buf.requires_grad_(True)
    return buf[..., 1:2].expand(t.shape)


LAYOUTS = {
    "fresh": _fresh,
    "offset_1": _offset(1), "offset_2": _offset(2), "offset_3": _offset(3), "offset_4": _offset(4),
    "batch_slice": _layout(lambda s: (s[0] + 2,) + s[1:], lambda b, s: b[1:-1]),
    "batch_step": _layout(lambda s: (2 * s[0],) + s[1:], lambda b, s: b[::2]),
    "time_major": _layout(lambda s: (s[1], s[0]) + s[2:], lambda b, s: b.transpose(0, 1)),
    "time_slice": _layout(lambda s: (s[0], s[1] + 3) + s[2:], lambda b, s: b[:, 2:2 + s[1]]),
    "head_lo": _layout(lambda s: s[:-1] + (2 * s[-1] + 1,), lambda b, s: b[..., :s[-1]]),
    "head_hi": _layout(lambda s: s[:-1] + (2 * s[-1] + 1,), lambda b, s: b[..., s[-1] + 1:]),
    "expanded": _expanded,
}
OFFSETS = ("offset_1", "offset_2", "offset_3", "offset_4")
MIN_DIM = {"time_major": 2, "time_slice": 2, "batch_slice": 1, "batch_step": 1, "head_lo": 1, "head_hi": 1, "expanded": 1}


def applies(name, dim, equal_values=False):
    """whether layout `name` exists for a tensor of `dim` dimensions (`equal_values`: one whose values may legitimately be
    equal along its last dimension - the only ones `expanded` is for)"""
    if name == "expanded" and not equal_values:
        return False
    return dim >= MIN_DIM.get(name, 0)


def base_of(view):
    """the buffer a layout's view lives in (`fresh`: the tensor itself)"""
    return view if view._base is None else view._base


def element_offset(name, shape):
    """the view's first element in its buffer, in elements"""
    if name in OFFSETS:
        return int(name[-1])
    if name == "batch_slice":
        return _numel(shape[1:])
    if name == "time_slice":
        return 2 * _numel(shape[2:])
    if name == "head_hi":
        return shape[-1] + 1
    if name == "expanded":
        return 1
    return 0


def is_contiguous(name, shape):
    """what torch's is_contiguous() gives for the view of a tensor of `shape`: dimensions of size 1 do not count"""
    if name in ("fresh", "batch_slice") or name in OFFSETS:
        return True
    if name == "batch_step":
        return shape[0] == 1
    if name == "time_major":
        return shape[0] == 1 or shape[1] == 1
    if name == "time_slice":
        return shape[0] == 1
    if name in ("head_lo", "head_hi"):
        return _numel(shape[:-1]) == 1
    if name == "expanded":
        return shape[-1] == 1
    raise KeyError(name)


def inside_mask(view):
    """bool [numel of the buffer]: the buffer's elements the view addresses"""
    base = base_of(view)
    idx = torch.arange(base.numel(), device=base.device).as_strided(view.shape, view.stride(), view.storage_offset())
    mark = torch.zeros(base.numel(), dtype=torch.bool, device=base.device)
    mark[idx.reshape(-1)] = True
    return mark


def outside(view):
    """the buffer's elements outside the view, flat (`fresh`: none)"""
    base = base_of(view)
    if base is view:
        return base.detach().reshape(-1)[:0]
    return base.detach().reshape(-1)[~inside_mask(view)]


def is_poison(values, like, poison=None):
    """every one of `values` is the poison of a tensor like `like`"""
    if like.is_floating_point():
        return bool(torch.isnan(values).all())
    return bool((values == poison_of(like, poison)).all())
