"""The matrix of the layout tests: every public entry point x every layout (tests/layouts.py) of each of its tensor arguments,
shared by tests/test_layouts.py (CPU tensors on the host twins) and tests/test_gpu_layouts.py (device tensors on the kernels).

WHAT A CASE ASSERTS.  The library normalises a tensor's layout before its kernels (or host twins) see it, so a call on a view
runs the same code on the same values and shapes as the call on a contiguous clone, the CONTROL (layout `fresh`): the loss,
every gradient and everything the returned tensor reports are compared with the control's TO THE BIT.  The buffer around a view
is poison (NaN / sentinels), the buffer is the autograd leaf: the outputs are finite, the gradient lands in the buffer inside
the view and is exactly zero outside it, in the buffer's dtype; a second backward over the retained graph gives the first one's
bits.  The control itself is held to the float64 reference its own feature test uses, at that test's bar (`check_reference`):
  ChainLoss, every route      boost_reference.reference (denominator by the oracle's f64 flavour, posterior / graph numerators,
                              regularisers, weights, xent targets; the xent term of graph numerators from xent_reference.np_xent,
                              a windowed numerator from num_reference.np_num_fb), bar boost_reference.BAR = 1e-5 on the relative
                              value and on max |d grad| / max |grad|
  ChainFunction, occupancies  the same two pieces, the same bar (num_reference.check_numerator)
  numerator_xent              xent_reference.np_xent, its measured fp32 distance + 1e-5
  posterior_xent              xent_targets_reference, its bound
  posterior_numerator         post_reference.np_post_targets, objf_bound / grad_bound
  output_regularizer          outreg_reference.np_outreg, SUM_REL / grad_bound
  boost_rows                  boost_reference.np_boost_rows, its derived bound
  weight_rows                 weights_reference.np_weight_rows, bit for bit
  from_dense, posterior_targets   post_reference.np_topk, the same pdfs, values within TOPK_REL
  viterbi_align               num_reference.np_viterbi, bit for bit
  viterbi_align under windows align_tw_reference.np_viterbi_tw, bit for bit (the batch's own windows, explicit int32 windows, explicit
                              int64 windows): the windows lie around the alignment of `x`, the input aligned is `z`, so the constraint
                              binds - asserted - and every sequence stays feasible
  expected_accuracy, SMBRLoss smbr_reference.batch(recursions) on the up-cast input: per_seq, the gradient, its row sums and `closing`
                              within smbr_reference.bound - 1e-5, or twice the fp32 numpy recursions' own distance where that is
                              beyond F32_SLACK; the loss of SMBRLoss is -sum E_b / sum L_b, an upstream gradient scales the gradient
  ... with `classes`          smbr_class_reference.batch(recursions) under the map `phones`, the same rule with the class-level rows;
                              class-id targets (to_classes) give the bits of the pdf-level targets' control as well
A gradient stored in bf16 / fp16 is rounded once or more per pass that touched it; the float64 comparison of GRADIENTS is made
for float32 network outputs (the 2-byte stores have their derived bounds in tests/test_gpu_half.py, test_gpu_post_targets.py,
test_gpu_weights.py, test_gpu_outreg.py), the loss of a 2-byte control is held to the bar like any other, and every 2-byte
layout case is held to its control to the bit.

THE sMBR INPUTS.  `x` has 5 % of its elements beyond the clamp; the fp32 reference's own distance from fp64 on exactly these
inputs is computed here, on the CPU, and recorded with every measured distance (`f32_reference`, `bound`).  A bound beyond 1e-4
would mean an input on which fp32 itself is poor: SEED_X is then to be changed, not the bound accepted (`smbr_bound` asserts it).
SEED_X = 5 (the seed the matrix has had from the start) keeps every config's fp32 distance below F32_SLACK, so every bound is 1e-5.

THE int64 WINDOWS.  `windows64` holds the windows of `windows` with every bound that cannot bind written beyond int32 - a lower
bound of 0 as -2^40, an upper bound at the sequence's length as 2^40: saturated to int32 they admit exactly what `windows` admits
(the reference reads them as int64), wrapped they would not.  The buffer around a view of them is poison beyond int32 too.
"""
import contextlib
import copy

import numpy as np
import torch

import align_tw_reference as atr
import boost_reference as br
import layouts as ly
import num_reference as nr
import outreg_reference as orf
import post_reference as pr
import smbr_class_reference as scr
import smbr_reference as sr
import weights_reference as wr
import xent_reference as xr
import xent_targets_reference as xtr
from pychain_amd import (ChainFunction, ChainGraphBatch, ChainLoss, ChainLossFunction, PosteriorTargets, SMBRLoss, alignment_windows,
                         boost_rows, expected_accuracy, native, numerator_xent, occupancies, output_regularizer, posterior_numerator,
                         posterior_targets, posterior_xent, viterbi_align, weight_rows, synthetic as syn)

B, T = 4, 23
LENGTHS = [23, 17, 9, 1]
# D = 41: T * D * 4 % 16 == 12 (a batch slice starts off the 16-byte grid; rows that are no multiple of 4: the scalar row forms);
# D = 42: T * D * 4 % 16 == 8; D = 40: the float4 forms and the native 2-byte rows (misalignment from the offset layouts)
CONFIGS = [(41, "float32"), (42, "float32"), (40, "float32"), (40, "bfloat16"), (40, "float16")]
DTYPES = pr.DTYPES
L2, OOR, XENT_C, BOOST, TOPK = 5e-4, 1e-2, 0.2, 1.0, 3
UPSTREAM = 0.37
COEF = 1e-5                     # the leaky-HMM coefficient of the sMBR entries (and, written out, of every other entry)
SEED_X = 5                      # (the module's docstring: THE sMBR INPUTS)
BEYOND_INT32 = 2 ** 40
_CACHE = {}


class Inputs(object):
    """The values of one (D, dtype): made once on the host, shared by every case, never changed."""

    def __init__(self, D, dname):
        self.D, self.dname, self.dtype = D, dname, DTYPES[dname]
        self.lengths = torch.tensor(LENGTHS, dtype=torch.int64)
        self.den = syn.make_den_graph(20, 60, D, seed=0)
        self.num = syn.make_num_graphs(LENGTHS, D, seed=100)
        x = syn.make_input(B, T, D, seed=SEED_X)
        far = torch.rand(x.shape, generator=torch.Generator().manual_seed(9)) < 0.05        # some elements beyond the clamp
        x = torch.where(far, torch.rand(x.shape, generator=torch.Generator().manual_seed(10)) * 80.0 - 40.0, x)
        v = dict(x=x.to(self.dtype), z=syn.make_input(B, T, D, seed=77).to(self.dtype),
                 gy=syn.make_input(B, T, D, seed=31, scale=1.0).to(self.dtype), g0=torch.tensor(UPSTREAM))
        v["post"] = torch.softmax(syn.make_input(B, T, D, seed=55) * 1.5, dim=-1).to(self.dtype)
        v["u"] = torch.tensor([1.0, 0.5, 0.25, 2.0])
        f = (torch.rand(B, T, generator=torch.Generator().manual_seed(3)) * 1.5).float()
        f[0, :5], f[1, 3] = 1.0, 0.0
        v["f"] = f
        v["u=eq"], v["f=eq"] = torch.full((B,), 0.5), f[:, 1:2].expand(B, T).contiguous()
        tg = posterior_targets(syn.make_input(B, T, D, seed=55) * 1.5, self.lengths, self.den, TOPK)
        v["pdfs"], v["probs"] = tg.pdfs, tg.probs
        ali = viterbi_align(v["x"], self.lengths, self.num)
        assert bool(ali.ok.all())
        bt = PosteriorTargets.from_alignment(ali)
        v["bt_pdfs"], v["bt_probs"] = bt.pdfs, bt.probs
        v["windows"] = alignment_windows(ali, self.num.num_states, tolerance=2)
        v["lengths"] = self.lengths
        # the same windows, every bound that cannot bind beyond int32 (the module's docstring: THE int64 WINDOWS)
        w64 = v["windows"].to(torch.int64)
        length = self.lengths.view(B, 1)
        w64[..., 0] = torch.where(w64[..., 0] <= 0, torch.full_like(w64[..., 0], -BEYOND_INT32), w64[..., 0])
        w64[..., 1] = torch.where(w64[..., 1] >= length, torch.full_like(w64[..., 1], BEYOND_INT32), w64[..., 1])
        assert int((w64.abs() == BEYOND_INT32).sum()) >= 2 * B
        v["windows64"] = w64
        v["classes64"] = torch.from_numpy(scr.class_map("phones", D))
        v["classes"] = v["classes64"].to(torch.int32)
        v["cls_pdfs"] = PosteriorTargets(tg.pdfs, tg.probs).to_classes(v["classes"]).pdfs
        assert v["cls_pdfs"].dtype == torch.int32 and v["cls_pdfs"].dim() == 3
        self.v = v
        self.xf, self.zf = v["x"].float(), v["z"].float()

    def value(self, name, eq=()):
        return self.v[name + "=eq" if name in eq else name]

    def targets(self, which="pdfs"):
        return PosteriorTargets(self.v[which], self.v[which.replace("pdfs", "probs")])


def inputs(D, dname):
    key = ("inputs", D, dname)
    if key not in _CACHE:
        _CACHE[key] = Inputs(D, dname)
    return _CACHE[key]


# ---- the arguments of an entry and the layouts each takes -------------------------------------------------------------------------
# name -> (dimensions, equal values legitimate, differentiable leaf, lives on the host whatever the call's device)
ARGS = {"x": (3, False, True, False), "z": (3, False, True, False), "x_in": (3, False, False, False), "gy": (3, False, False, False),
        "post": (3, False, False, False), "u": (1, True, False, False), "f": (2, True, False, False),
        "pdfs": (3, False, False, False), "probs": (3, False, False, False), "bt_pdfs": (3, False, False, False),
        "bt_probs": (3, False, False, False), "hpdfs": (3, False, False, True), "hprobs": (3, False, False, True),
        "windows": (3, False, False, False), "lengths": (1, False, False, False), "g0": (0, False, False, False),
        "windows64": (3, False, False, False), "cls_pdfs": (3, False, False, False), "classes": (1, False, False, False),
        "classes64": (1, False, False, False), "hclasses": (1, False, False, True)}
_VALUE_OF = {"x_in": "x", "hpdfs": "pdfs", "hprobs": "probs", "hclasses": "classes64"}
CLASS_MAPS = ("classes", "classes64", "hclasses")
NON_FRESH = [n for n in ly.LAYOUTS if n != "fresh"]


def arg_layouts(arg):
    dim, eq = ARGS[arg][:2]
    if dim == 0:
        return list(ly.OFFSETS)
    return [n for n in NON_FRESH if ly.applies(n, dim, eq)]


class Case(object):
    """One call: `t(name)` is the argument `name` on the call's device in the layout this case gives it."""

    def __init__(self, inp, dev, mode, lay, eq, values=None):
        self.inp, self.dev, self.mode, self.lay, self.eq = inp, dev, mode, dict(lay), tuple(eq)
        self.values = dict(_VALUE_OF, **(values or {}))       # (an entry may give an argument another of the inputs' values)
        self.views, self.leaves = {}, {}

    def t(self, name):
        if name not in self.views:
            dim, _, leaf, host = ARGS[name]
            val = self.inp.value(self.values.get(name, name), self.eq)
            val = val if host else val.to(self.dev)
            view = ly.LAYOUTS[self.lay.get(name, "fresh")](val, leaf=leaf)
            self.views[name] = view
            if leaf:
                self.leaves[name] = view
        return self.views[name]

    def lengths(self, devlen):
        """the lengths on the host as they are, or (`devlen`) on the call's device in this case's layout"""
        return self.t("lengths") if devlen else self.inp.lengths

    def num(self):
        return self.inp.num

    def targets(self, pdfs="pdfs", probs="probs"):
        """PosteriorTargets whose tensors are this case's views (assigned: the constructor would normalise them)"""
        tg = PosteriorTargets(self.inp.v["pdfs" if "bt" not in pdfs else "bt_pdfs"], self.inp.v["probs" if "bt" not in pdfs else "bt_probs"])
        tg.pdfs, tg.probs = self.t(pdfs), self.t(probs)
        return tg

    def crit(self, **kw):
        c = ChainLoss(self.inp.den, 1e-5, avg=True, **kw)
        c.fused = self.mode != "unfused"
        return c


def _loss_plain(c, devlen=False):
    return c.crit()(c.t("x"), c.lengths(devlen), c.num())


def _loss_all(c, devlen=False):
    crit = c.crit(xent_regularize=XENT_C, output_l2_regularize=L2, out_of_range_regularize=OOR)
    return crit(c.t("x"), c.lengths(devlen), c.num(), xent_output=c.t("z"), utt_weights=c.t("u"), deriv_weights=c.t("f"))


def _post_plain(c, p="pdfs", q="probs"):
    return c.crit()(c.t("x"), c.lengths(False), c.targets(p, q))


def _post_xent(c, p="pdfs", q="probs"):
    tg = c.targets(p, q)
    return c.crit(xent_regularize=XENT_C)(c.t("x"), c.lengths(False), tg, xent_output=c.t("z"), xent_targets=tg)


def _boost_post(c):
    return c.crit(boost=BOOST)(c.t("x"), c.lengths(False), c.targets())


def _boost_graph(c):
    return c.crit(boost=BOOST)(c.t("x"), c.lengths(False), c.num(), boost_targets=c.targets("bt_pdfs", "bt_probs"))


def _windows(c):
    num = copy.copy(c.inp.num)                       # (a batch of its own: the windows are set on the object)
    num._device_cache = dict(c.inp.num._device_cache)
    num.__dict__.pop("_tw_device", None)
    num.set_time_windows(c.t("windows"))
    return c.crit()(c.t("x"), c.lengths(False), num)


def _chain_den(c):
    return ChainFunction.apply(c.t("x"), c.lengths(False), ChainGraphBatch(c.inp.den, B), 1e-5)


def _chain_num(c):
    return ChainFunction.apply(c.t("x"), c.lengths(False), c.num())


def _occupancies(c):
    x = c.t("x_in")
    return dict(den=occupancies(x, c.lengths(False), c.inp.den), num=occupancies(x, c.lengths(False), c.num()))


def _posterior_targets(c):
    tg = posterior_targets(c.t("x_in"), c.lengths(False), c.inp.den, TOPK)
    return dict(pdfs=tg.pdfs, probs=tg.probs, occ=occupancies(c.t("x_in"), c.lengths(False), c.inp.den))


def _from_dense(c):
    tg = PosteriorTargets.from_dense(c.t("post"), c.lengths(False), TOPK)
    return dict(pdfs=tg.pdfs, probs=tg.probs)


def _numerator_xent(c):
    return numerator_xent(c.t("z"), c.t("x_in"), c.lengths(False), c.num())


def _posterior_xent(c):
    return posterior_xent(c.t("z"), c.lengths(False), c.targets())


def _posterior_numerator(c):
    return posterior_numerator(c.t("x"), c.lengths(False), c.targets())


def _output_regularizer(c):
    return output_regularizer(c.t("x"), c.lengths(False), L2, OOR)


def _boost_rows(c):
    return dict(e=boost_rows(c.t("x_in"), c.lengths(False), c.targets(), BOOST))


def _weight_rows(c):
    return weight_rows(c.t("x"), (c.t("u"), c.t("f")), c.lengths(False))


def _viterbi(c):
    ali = viterbi_align(c.t("x_in"), c.lengths(False), c.num())
    return dict(pdfs=ali.pdfs, states=ali.states, score=ali.score, ok=ali.ok)


def _smbr(c, p="pdfs", q="probs", classes=None, targets_are_classes=False):
    kw = {} if classes is None else dict(classes=c.t(classes), targets_are_classes=targets_are_classes)
    return expected_accuracy(c.t("x"), c.lengths(False), c.inp.den, c.targets(p, q), COEF, **kw)


def _smbr_loss(c):
    return SMBRLoss(ChainGraphBatch(c.inp.den, B), COEF, avg=True)(c.t("x"), c.lengths(True), c.targets())


def _viterbi_windows(c, windows="windows", own=False):
    if own:                                          # (a batch of its own, as _windows makes it)
        num = copy.copy(c.inp.num)
        num._device_cache = dict(c.inp.num._device_cache)
        num.__dict__.pop("_tw_device", None)
        num.set_time_windows(c.t(windows))
        ali = viterbi_align(c.t("x_in"), c.lengths(False), num, time_windows=True)
    else:
        ali = viterbi_align(c.t("x_in"), c.lengths(False), c.num(), time_windows=c.t(windows))
    return dict(pdfs=ali.pdfs, states=ali.states, score=ali.score, ok=ali.ok)


class Entry(object):
    def __init__(self, name, fn, args, ref, modes=(None,), gpu_only=False, gradient=None, kw=None, values=None):
        self.name, self.fn, self.args, self.ref, self.modes, self.gpu_only = name, fn, tuple(args), ref, tuple(modes), gpu_only
        self.gradient, self.kw, self.values = gradient, dict(kw or {}), dict(values or {})


GRAPH_MODES = ("fused", "no_overlap", "unfused")
ENTRIES = [
    Entry("loss_plain", _loss_plain, ["x"], "loss_plain", GRAPH_MODES),
    Entry("loss_plain_devlen", _loss_plain, ["x", "lengths"], "loss_plain", GRAPH_MODES, kw=dict(devlen=True)),
    Entry("loss_all", _loss_all, ["x", "z", "u", "f"], "loss_all", GRAPH_MODES),
    Entry("loss_all_devlen", _loss_all, ["x", "z", "u", "f", "lengths"], "loss_all", GRAPH_MODES, kw=dict(devlen=True)),
    Entry("post_plain", _post_plain, ["x", "pdfs", "probs"], "post_plain", ("fused", "unfused")),
    Entry("post_plain_host_targets", _post_plain, ["x", "hpdfs", "hprobs"], "post_plain", ("fused",), gpu_only=True,
          kw=dict(p="hpdfs", q="hprobs")),
    Entry("post_xent", _post_xent, ["x", "z", "pdfs", "probs"], "post_xent", ("fused", "unfused")),
    Entry("post_xent_host_targets", _post_xent, ["x", "z", "hpdfs", "hprobs"], "post_xent", ("fused",), gpu_only=True,
          kw=dict(p="hpdfs", q="hprobs")),
    Entry("boost_post", _boost_post, ["x", "pdfs", "probs"], "boost_post", ("fused",)),
    Entry("boost_graph", _boost_graph, ["x", "bt_pdfs", "bt_probs"], "boost_graph", ("fused",)),
    Entry("windows", _windows, ["x", "windows"], "windows", ("fused", "unfused")),
    Entry("chain_den", _chain_den, ["x"], "chain_den"),
    Entry("chain_num", _chain_num, ["x"], "chain_num"),
    Entry("occupancies", _occupancies, ["x_in"], "occupancies"),
    Entry("posterior_targets", _posterior_targets, ["x_in"], "posterior_targets"),
    Entry("from_dense", _from_dense, ["post"], "from_dense"),
    Entry("numerator_xent", _numerator_xent, ["z", "x_in"], "numerator_xent"),
    Entry("posterior_xent", _posterior_xent, ["z", "pdfs", "probs"], "posterior_xent"),
    Entry("posterior_numerator", _posterior_numerator, ["x", "pdfs", "probs"], "posterior_numerator"),
    Entry("output_regularizer", _output_regularizer, ["x"], "output_regularizer"),
    Entry("boost_rows", _boost_rows, ["x_in", "pdfs", "probs"], "boost_rows"),
    Entry("weight_rows", _weight_rows, ["gy", "u", "f"], "weight_rows", gradient="gy"),
    Entry("viterbi_align", _viterbi, ["x_in"], "viterbi_align"),
    # an upstream gradient other than 1, a 0-dim view at an element offset: read on the device by native.rescale_
    Entry("upstream_graph", _loss_plain, ["g0"], "loss_plain", ("fused", "no_overlap"), gradient="g0"),
    Entry("upstream_post", _post_plain, ["g0"], "post_plain", ("fused",), gradient="g0"),
    # lattice-free sMBR: x goes to its kernels as it is, 2-byte rows at 2 / 4 / 6-byte offsets included (native.smbr)
    Entry("smbr_pdf", _smbr, ["x", "pdfs", "probs"], "smbr_pdf"),
    Entry("smbr_pdf_host_targets", _smbr, ["x", "hpdfs", "hprobs"], "smbr_pdf", gpu_only=True, kw=dict(p="hpdfs", q="hprobs")),
    Entry("smbr_loss_devlen", _smbr_loss, ["x", "lengths"], "smbr_loss"),
    Entry("smbr_classes", _smbr, ["x", "pdfs", "probs", "classes"], "smbr_classes", kw=dict(classes="classes")),
    Entry("smbr_classes_int64", _smbr, ["classes64"], "smbr_classes", kw=dict(classes="classes64")),
    Entry("smbr_classes_host_map", _smbr, ["x", "hclasses"], "smbr_classes", gpu_only=True, kw=dict(classes="hclasses")),
    Entry("smbr_class_targets", _smbr, ["x", "cls_pdfs", "probs", "classes"], "smbr_class_targets",
          kw=dict(p="cls_pdfs", classes="classes", targets_are_classes=True)),
    # constrained re-alignment: `z` aligned inside the windows around the alignment of `x`
    Entry("viterbi_windows_own", _viterbi_windows, ["x_in", "windows"], "viterbi_windows", kw=dict(own=True), values=dict(x_in="z")),
    Entry("viterbi_windows_explicit", _viterbi_windows, ["x_in", "windows"], "viterbi_windows", values=dict(x_in="z")),
    Entry("viterbi_windows_explicit_int64", _viterbi_windows, ["windows64"], "viterbi_windows64", kw=dict(windows="windows64"),
          values=dict(x_in="z")),
    Entry("upstream_smbr", _smbr, ["g0"], "smbr_pdf", gradient="g0"),
]
SMBR_REFS = ("smbr_pdf", "smbr_loss", "smbr_classes", "smbr_class_targets")
BY_NAME = {e.name: e for e in ENTRIES}


def entry_modes(entry, dev):
    """the routes an entry is run on: device tensors take each of `modes`; CPU tensors have one route, the host twins"""
    return entry.modes if str(dev) != "cpu" else entry.modes[:1]


def matrix(dev):
    """[(entry name, mode, layout)]: every layout at least one of the entry's arguments takes, and "everything" - all of them in
    different layouts at once"""
    out = []
    for e in ENTRIES:
        if e.gpu_only and str(dev) == "cpu":
            continue
        names = [n for n in NON_FRESH if any(n in arg_layouts(a) for a in e.args)]
        for mode in entry_modes(e, dev):
            out += [(e.name, mode, n) for n in names + (["everything"] if len(e.args) > 1 else [])]
    return out


def variants(entry, layout):
    """the cases of (entry, layout): one argument varied at a time - [(layouts by argument, arguments on their equal values)]"""
    if layout == "everything":
        lay, eq = {}, []
        for i, a in enumerate(entry.args):
            ns = arg_layouts(a)
            ns = ns[(3 * i) % len(ns):] + ns[:(3 * i) % len(ns)]
            lay[a] = ([n for n in ns if n not in lay.values()] or ns)[0]       # (different ones as far as they go)
            if lay[a] == "expanded":
                eq.append(a)
        return [(lay, tuple(eq))]
    return [({a: layout}, (a,) if layout == "expanded" else ()) for a in entry.args if layout in arg_layouts(a)]


# ---- running a case -----------------------------------------------------------------------------------------------------------------
REPORTS = ("totals", "totals_all", "bad_count", "xent_objf", "xent_objf_per_seq", "l2_term", "out_of_range_term", "weighted_frames",
           "objf_per_seq", "per_seq", "closing")          # (the last two: of the sMBR entries only - test_layouts.py asserts it)


@contextlib.contextmanager
def _route(mode):
    was = ChainLossFunction.overlap
    ChainLossFunction.overlap = mode != "no_overlap"
    try:
        yield
    finally:
        ChainLossFunction.overlap = was


def _host(v):
    if isinstance(v, (tuple, list)):
        return torch.cat([t.detach().reshape(-1).cpu() for t in v])
    return v.detach().cpu()


class Result(object):
    """values: name -> host tensor (the loss, what it reports, an entry's outputs); grads: leaf -> dict(inside = the gradient
    in the buffer where the view lies, outside_zero, dtype_ok, again = the second backward's)"""


def run(entry, dev, D, dname, mode=None, lay=None, eq=()):
    inp = inputs(D, dname)
    c = Case(inp, torch.device(dev), mode, lay or {}, eq, entry.values)
    res = Result()
    res.values, res.grads = {}, {}
    with _route(mode):
        out = entry.fn(c, **entry.kw)
        for a in CLASS_MAPS:
            if a in c.views:
                # the map was uploaded for THIS view - the cache of native.smbr_classes holds its source tensor -, not taken from
                # what the control, or the case before, left there
                assert native._smbr_classes_cache[str(c.t("x").device)][1] is c.views[a], (entry.name, a, "a cached class map was used")
        if isinstance(out, dict):
            res.values = {k: _host(v) for k, v in out.items()}
            return res
        res.values["loss"] = _host(out)
        for name in REPORTS:
            v = getattr(out, name, None)
            if v is not None:
                res.values[name] = _host(v)[:5] if name == "totals_all" else _host(v)
        g = None if entry.gradient is None else c.t(entry.gradient)
        taken = []
        for _ in range(2):                                  # the second backward runs over the retained graph
            out.backward(gradient=g, retain_graph=True)
            taken.append({n: ly.base_of(v).grad.detach().clone() for n, v in c.leaves.items()})
            for v in c.leaves.values():
                ly.base_of(v).grad = None
    for n, v in c.leaves.items():
        base, g1, g2 = ly.base_of(v), taken[0][n], taken[1][n]
        at = lambda t: t.as_strided(v.shape, v.stride(), v.storage_offset()) if base is not v else t
        mask = ly.inside_mask(v)
        res.grads[n] = dict(inside=_host(at(g1)), again=_host(at(g2)), dtype_ok=g1.dtype == base.dtype and g1.shape == base.shape,
                            outside_zero=bool((g1.reshape(-1)[~mask] == 0).all()) and bool((g2.reshape(-1)[~mask] == 0).all()))
    return res


def control(entry, dev, D, dname, mode=None, eq=()):
    """the same call on contiguous clones: run once per (entry, device, D, dtype, route, equal-valued arguments)"""
    key = ("control", entry.name, str(dev), D, dname, mode, tuple(sorted(eq)))
    if key not in _CACHE:
        _CACHE[key] = run(entry, dev, D, dname, mode, {}, eq)
    return _CACHE[key]


def bits(t):
    if t.dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        return t.contiguous().view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])
    return t


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_same(res, ctl, what=""):
    """assertion 1 (to the bit against the control), 3 (finite, the control's bad count), 4 (the gradient in the buffer) and 5 (a
    second backward)"""
    assert sorted(res.values) == sorted(ctl.values), (what, sorted(res.values), sorted(ctl.values))
    for k, v in res.values.items():
        assert same_bits(v, ctl.values[k]), (what, k, v, ctl.values[k])
    assert sorted(res.grads) == sorted(ctl.grads), (what, sorted(res.grads), sorted(ctl.grads))
    for n, g in res.grads.items():
        assert g["dtype_ok"], (what, n, "the gradient at the buffer has another dtype or shape")
        assert bool(torch.isfinite(g["inside"].float()).all()), (what, n, "the poison got into the gradient")
        assert same_bits(g["inside"], ctl.grads[n]["inside"]), (what, n, "gradient differs from the control's")
        assert g["outside_zero"], (what, n, "the gradient outside the view is not zero")
        assert same_bits(g["again"], g["inside"]), (what, n, "a second backward gives another gradient")
    if "loss" in res.values:
        assert bool(torch.isfinite(res.values["loss"].float()).all()), (what, "the poison got into the loss")


def fresh_is_stable(entry, dev, D, dname, mode=None):
    """two controls against each other, once: what bit identity with the control rests on"""
    assert_same(run(entry, dev, D, dname, mode), control(entry, dev, D, dname, mode), "fresh against fresh")


# ---- the float64 references the controls are held to ------------------------------------------------------------------------------
def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _empty_targets():
    return PosteriorTargets(torch.full((B, T, 1), -1, dtype=torch.int32), torch.zeros(B, T, 1))


def _den_ref(inp):
    """(sum_b den_b, gamma_den) in float64: boost_reference.reference without a numerator, un-averaged"""
    return _cached(("den_ref", inp.D, inp.dname), lambda: br.reference(inp.den, inp.xf, inp.lengths, _empty_targets(), None, 0.0, avg=False))


def _num_ref(inp, windows=None):
    return _cached(("num_ref", inp.D, inp.dname, windows is not None), lambda: nr.np_num_fb(inp.num, inp.xf, inp.lengths, windows))


def _want_loss(inp, ref, eq):
    """(loss, d loss / dx [, d loss / dz]) of a ChainLoss entry"""
    u, f = inp.value("u", eq), inp.value("f", eq)
    tg, bt = inp.targets(), inp.targets("bt_pdfs")
    if ref == "loss_plain":
        return br.reference(inp.den, inp.xf, inp.lengths, inp.num, None, 0.0)
    if ref == "post_plain":
        return br.reference(inp.den, inp.xf, inp.lengths, tg, None, 0.0)
    if ref == "post_xent":
        return br.reference(inp.den, inp.xf, inp.lengths, tg, None, 0.0, z=inp.zf, xent_targets=tg, c=XENT_C)
    if ref == "boost_post":
        return br.reference(inp.den, inp.xf, inp.lengths, tg, tg, BOOST)
    if ref == "boost_graph":
        return br.reference(inp.den, inp.xf, inp.lengths, inp.num, bt, BOOST)
    if ref == "windows":
        n = float(inp.lengths.sum())
        den, gden = _den_ref(inp)
        logp, gamma, feas = _num_ref(inp, inp.v["windows"])
        assert feas.all()
        return (den - float(logp.sum())) / n, (gden - gamma) / n
    if ref == "loss_all":
        loss, gx = br.reference(inp.den, inp.xf, inp.lengths, inp.num, None, 0.0, True, u, f, (L2, OOR))
        objf, dz = xr.np_xent(inp.num, inp.xf, inp.zf, inp.lengths, fb=_num_ref(inp))
        ud = u.double().numpy()
        n = float((ud * inp.lengths.numpy()).sum())
        w = ud[:, None] * f.double().numpy()
        return loss - XENT_C * float((ud * objf).sum()) / n, gx, -XENT_C * dz * w[..., None] / n
    raise KeyError(ref)


def smbr_bound(d32):
    """smbr_reference.bound's rule on the fp32 reference's own distance `d32`; beyond 1e-4 the inputs are at fault (SEED_X)"""
    bound = 2.0 * d32 if d32 > sr.F32_SLACK else sr.BAR
    assert bound <= 1e-4, ("the fp32 reference itself is %g from fp64 on these inputs: choose another SEED_X" % d32)
    return bound


def _smbr_ref(inp, ref):
    """((E [B], dE/dx [B,T,D], closing [B]) by the float64 recursions on the up-cast input, the bound, the fp32 recursions' own
    distance, what gradient distances are relative to) of the sMBR entries: pdf-level, by class, by class with class-id targets"""
    def make():
        probs = inp.v["probs"].numpy()
        if ref in ("smbr_pdf", "smbr_loss"):
            args = (inp.den, inp.xf, LENGTHS, inp.v["pdfs"].numpy(), probs, COEF)
            want, w32 = sr.batch(sr.recursions, *args), sr.batch(sr.recursions, *args, dtype=np.float32)
        else:
            tac = ref == "smbr_class_targets"
            args = (inp.den, inp.xf, LENGTHS, inp.v["cls_pdfs" if tac else "pdfs"].numpy(), probs, inp.v["classes64"].numpy(), COEF)
            want = scr.batch(sr.recursions, *args, targets_are_classes=tac)
            w32 = scr.batch(sr.recursions, *args, targets_are_classes=tac, dtype=np.float32)
        scale = float(np.abs(want[1]).max())
        assert scale > 0 and int((want[0] > 0).sum()) >= 3, "the reference has nothing to compare"
        d32 = max(scr.grad_dist(w32[1], want[1], scale), sr.value_dist(w32[0], want[0]))
        return want, smbr_bound(d32), d32, scale
    return _cached(("smbr_ref", ref if ref != "smbr_loss" else "smbr_pdf", inp.D, inp.dname), make)


def _tw_ref(inp, ref):
    """(np_viterbi_tw of `z` inside the windows around the alignment of `x`, the free alignment of `z`)"""
    def make():
        w = inp.v["windows64" if ref == "viterbi_windows64" else "windows"]
        want, free = atr.np_viterbi_tw(inp.num, inp.zf, LENGTHS, w), nr.np_viterbi(inp.num, inp.zf, LENGTHS)
        assert bool(np.isfinite(want[0]).all()) and all(atr.admits(inp.v["windows"], want, LENGTHS)), "a sequence is infeasible"
        assert sum(atr.frames_differing(want, free, LENGTHS)) >= 1, "the windows do not bind: the free path lies inside them"
        return want, free
    return _cached(("tw_ref", ref, inp.D, inp.dname), make)


def _dist(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def check_reference(entry, ctl, dev, D, dname, mode=None, eq=(), record=None):
    """the control of an entry against float64 (the module's docstring says which reference and which bar); returns the
    distances it measured"""
    inp = inputs(D, dname)
    f32 = dname == "float32"
    ref = entry.ref
    v = {k: t.float().numpy() if t.is_floating_point() and t.dtype != torch.float64 else t.numpy() for k, t in ctl.values.items()}
    gx = ctl.grads["x"]["inside"].float().numpy() if "x" in ctl.grads else None
    gz = ctl.grads["z"]["inside"].float().numpy() if "z" in ctl.grads else None
    up = UPSTREAM if entry.gradient == "g0" else 1.0
    d = {}
    if ref in ("loss_plain", "loss_all", "post_plain", "post_xent", "boost_post", "boost_graph", "windows"):
        want = _cached(("want", ref, D, dname, tuple(sorted(eq))), lambda: _want_loss(inp, ref, eq))
        d["loss"] = abs(float(v["loss"]) - want[0]) / abs(want[0])
        if f32:
            d["grad"] = _dist(gx, up * want[1])
            if gz is not None:
                d["zgrad"] = _dist(gz, up * want[2])
        assert max(d.values()) <= br.BAR, (entry.name, mode, d)
    elif ref in ("chain_den", "chain_num", "occupancies"):
        den, gden = _den_ref(inp)
        if ref != "chain_num":
            got = v["loss"] if ref == "chain_den" else None
            if got is not None:
                d["den"] = abs(float(got) - den) / abs(den)
            if f32:
                d["den_grad"] = _dist(gx if ref == "chain_den" else v["den"], gden)
        if ref != "chain_den":
            want = _num_ref(inp)
            if ref == "chain_num":
                d["num"] = abs(float(v["loss"]) - float(want[0].sum())) / abs(float(want[0].sum()))
            if f32:
                d["num_grad"] = _dist(gx if ref == "chain_num" else v["num"], want[1])
        assert max(d.values(), default=0.0) <= br.BAR, (entry.name, d)
    elif ref == "numerator_xent":
        fb = _num_ref(inp)
        want = xr.np_xent(inp.num, inp.xf, inp.zf, inp.lengths, fb=fb)
        own = xr.fp32_distance(inp.num, inp.xf, inp.zf, inp.lengths, fb=fb, ref=want)
        bound = (own[0] + xr.GAMMA_BOUND, own[1] + xr.GAMMA_BOUND + pr.U[dname])
        d["objf"], d["grad"] = xr.check_xent(v["xent_objf_per_seq"], gz, want, LENGTHS, fb[2], bound)
    elif ref == "posterior_xent":
        want = xtr.np_xent_targets(inp.zf.numpy(), LENGTHS, inp.v["pdfs"].numpy(), inp.v["probs"].numpy())
        bound = xtr.bound(xtr.fp32_distance(inp.zf, LENGTHS, inp.v["pdfs"], inp.v["probs"], want), dname)
        d["objf"], d["grad"] = xtr.distances(v["xent_objf_per_seq"], gz, want)
        assert d["objf"] <= bound[0] and d["grad"] <= bound[1], (d, bound)
    elif ref == "posterior_numerator":
        want = pr.np_post_targets(inp.xf.numpy(), LENGTHS, inp.v["pdfs"].numpy(), inp.v["probs"].numpy(), grad=np.zeros((B, T, D)), s=1.0)
        d["objf"] = float((np.abs(v["objf_per_seq"] - want["num"]) / np.maximum(pr.objf_bound(want), 1e-300)).max())
        d["grad"] = orf.worst_ratio(gx, want["want"], pr.grad_bound(want["want"], dname))
        assert max(d.values()) <= 1.0, d
    elif ref == "output_regularizer":
        want = orf.np_outreg(inp.xf.numpy(), LENGTHS, L2, OOR)
        d["loss"] = abs(float(v["loss"]) - want[3]) / (orf.SUM_REL * want[3])
        d["grad"] = orf.worst_ratio(gx, want[2], orf.grad_bound(want[2], orf.term_magnitude(inp.xf.numpy(), LENGTHS, L2, OOR), 1.0, dname))
        assert max(d.values()) <= 1.0, d
    elif ref == "boost_rows":
        E = _host(boost_rows(inp.v["x"].to(dev), inp.lengths, inp.targets(), 0.0)).numpy()       # exp(clamp(x)) as the library forms it
        want, touched, bound, bad = br.np_boost_rows(E, LENGTHS, inp.v["pdfs"].numpy(), inp.v["probs"].numpy(), BOOST)
        live = np.arange(T)[None, :] < np.asarray(LENGTHS)[:, None]
        assert bad == 0 and np.array_equal(v["e"][live][~touched[live]].view(np.int32), E[live][~touched[live]].view(np.int32))
        assert not v["e"][~live].any()
        d["rows"] = orf.worst_ratio(v["e"][live], want[live], np.where(touched[live], bound[live], 0.0))
        assert d["rows"] <= 1.0, d
    elif ref == "weight_rows":
        want = wr.np_weight_rows(inp.v["gy"], LENGTHS, inp.value("u", eq).numpy(), inp.value("f", eq).numpy())
        assert wr.same_bits(ctl.grads["x"]["inside"], want)
    elif ref in ("from_dense", "posterior_targets"):
        rows = inp.v["post"].float().numpy() if ref == "from_dense" else v["occ"]
        pdfs, probs = pr.np_topk(rows, LENGTHS, TOPK)
        assert np.array_equal(v["pdfs"], pdfs) and pr.topk_values_ok(v["probs"], probs, True)
        if ref == "posterior_targets" and f32:
            d["occupancies"] = _dist(v["occ"], _den_ref(inp)[1])
            assert d["occupancies"] <= br.BAR, d
    elif ref == "viterbi_align":
        want = nr.np_viterbi(inp.num, inp.xf, LENGTHS)
        nr.check_alignment(ctl.values["score"], ctl.values["states"], ctl.values["pdfs"], ctl.values["ok"], 0, want, LENGTHS)
    elif ref in ("viterbi_windows", "viterbi_windows64"):
        want, _ = _tw_ref(inp, ref)
        if ref == "viterbi_windows64":                                   # (saturated, the int64 windows admit what the int32 ones do)
            same = _tw_ref(inp, "viterbi_windows")[0]
            assert all(np.array_equal(a, b) for a, b in zip(want[:3], same[:3]))
        nr.check_alignment(ctl.values["score"], ctl.values["states"], ctl.values["pdfs"], ctl.values["ok"], 0, want, LENGTHS)
    elif ref in SMBR_REFS:
        (E, G, _), bound, d32, scale = _smbr_ref(inp, ref)
        s = -1.0 / float(sum(LENGTHS)) if ref == "smbr_loss" else 1.0   # SMBRLoss, avg: -sum_b E_b / sum_b L_b
        d["value"] = sr.value_dist(v["per_seq"], E)
        d["loss"] = abs(float(v["loss"]) - s * E.sum()) / abs(s * E.sum())
        d["closing"] = float(np.abs(v["closing"]).max())
        if f32:
            d["grad"] = scr.grad_dist(gx, up * s * G, abs(up * s) * scale)
            d["rows"] = float(np.abs(gx.astype(np.float64).sum(-1)).max() / (abs(up * s) * scale))
        assert ctl.values["per_seq"].dtype == torch.float64 and ctl.values["bad_count"].tolist() == [0, 0]
        assert max(d.values()) <= bound, (entry.name, d, bound)
        d.update(f32_reference=d32, bound=bound)                         # (recorded beside every measured distance)
        if ref == "smbr_class_targets":                                  # class ids in place of pdfs: the bits of the pdf targets' call
            other = control(BY_NAME["smbr_classes"], dev, D, dname, mode)
            assert all(same_bits(ctl.values[k], other.values[k]) for k in ("per_seq", "closing", "bad_count"))
            assert same_bits(ctl.grads["x"]["inside"], other.grads["x"]["inside"])
    else:
        raise KeyError(ref)
    if record is not None and d:
        record("layouts_%s_%s_D%d_%s" % (entry.name, mode, D, dname), **d)
    return d


def two_heads(dev, D, dname, mode):
    """x = wide[..., :D] and z = wide[..., D + 1:] of ONE leaf, the output of one linear layer with two heads, through the call
    with everything on: wide.grad holds both gradients and a zero column between them.  Returns (wide.grad, the control)."""
    inp = inputs(D, dname)
    e = BY_NAME["loss_all"]
    ctl = control(e, dev, D, dname, mode)
    wide = torch.full((B, T, 2 * D + 1), float("nan"), dtype=inp.dtype, device=dev)
    wide[..., :D], wide[..., D + 1:] = inp.v["x"].to(dev), inp.v["z"].to(dev)
    wide.requires_grad_(True)
    c = Case(inp, torch.device(dev), mode, {}, ())
    c.views["x"], c.views["z"] = wide[..., :D], wide[..., D + 1:]
    with _route(mode):
        loss = _loss_all(c)
        loss.backward()
    return _host(loss), _host(wide.grad), ctl
