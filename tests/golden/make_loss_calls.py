"""Which library calls one training step of ChainLoss makes, and with what arguments, over every combination of its options:

    python tests/golden/make_loss_calls.py [--section cpu|gpu|all] [--out FILE]     # writes tests/golden/loss_calls.json
    python tests/golden/make_loss_calls.py --dump CONFIG                             # prints the full trace of one configuration
    python tests/golden/make_loss_calls.py --bits FILE                               # the results' bits, for comparing two commits
    python tests/golden/make_loss_calls.py --list

A step is `loss = crit(...)`, `loss.backward(retain_graph=True)`, `loss.backward()` (the second one re-evaluates).  For its
duration a proxy stands in place of the loaded library (pychain_amd._lib._lib) and writes down every call of a pychain_hip_*
entry point:
  * the FAMILY name - a trailing _tw / _xent stripped, and the arguments those forms add (time windows, the pychain_hip_xent)
    written down as absent where the narrower form was called: which of the pass-through symbols a wrapper picks is no difference;
  * every int / int64 / size_t argument as it is (sizes of workspaces among them), every float as the hex of its float32 value,
    every pointer as None (null) or "ptr" - addresses are not recorded, and neither is the stream;
  * of a pychain_hip_xent: z_dtype, grad_scale, loss_coef, its workspace's size, and whether xent_grad and xent_totals are given.
The plan's own entry points (compile, info, the time-segment state a plan attaches and detaches when it is collected) are not
written down: when they run is decided by caches and the garbage collector, not by the step.

tests/test_loss_calls.py replays every configuration with the package under test and compares.  The file holds, per
configuration, the family names in order and a SHA-256 of the canonical JSON of the full trace.  The forward section is kept
in order; so are the two backward sections of the fused routes; on the unfused route and on CPU tensors autograd chooses the
order among independent Functions, and the backward sections are sorted.  The file is regenerated only when the sequence of
calls changes ON PURPOSE - from the commit BEFORE a refactor, never from the refactored code; the gpu section on an MI355X.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "loss_calls.json")
if REPO not in sys.path:
    sys.path.insert(0, REPO)
os.environ.setdefault("PYCHAIN_PLAN_CACHE_DIR", "off")

import torch  # noqa: E402

from pychain_amd import ChainLoss, ChainLossFunction, _lib, alignment_windows, native, viterbi_align, synthetic as syn  # noqa: E402

LENGTHS = [7, 4, 1]
B, T, D = 3, 7, 8
XENT_C, L2, OOR = 0.1, 2e-3, 5e-2
DEV = "cuda:0"

_INTS = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_long)
_PLAN_LIFECYCLE = ("pychain_hip_den_plan_build", "pychain_hip_den_plan_info", "pychain_hip_den_tseg_state",
                   "pychain_hip_den_tseg_state_bytes")
# (device entry points whose plain form ends with the stream)
_STREAM_LAST = ("den_forward_backward", "num_forward_backward", "chain_loss_forward", "chain_loss_forward_backward",
                "chain_loss_backward", "output_reg", "weight_rows", "rescale", "loss_total", "align")


def _family(name):
    for suffix in ("_tw", "_xent"):
        if name.endswith(suffix) and name[:-len(suffix)] in _lib._SIGNATURES:
            return name[:-len(suffix)]
    return name


def _value(ctype, a):
    a = getattr(a, "value", a)
    if ctype in _INTS:
        return int(a)
    if ctype is ctypes.c_float:
        return ctypes.c_float(a).value.hex()
    if ctype is ctypes.c_char_p:
        return a.decode() if isinstance(a, bytes) else (None if a is None else "buffer")
    return "ptr" if a else None


def _describe(name, args):
    family = _family(name)
    short = family[len("pychain_hip_"):]
    types = _lib._SIGNATURES[family][1]
    skip = len(types) - 1 if short in _STREAM_LAST else -1
    entry = {"fn": short, "args": [_value(t, a) for i, (t, a) in enumerate(zip(types, args)) if i != skip]}
    if family + "_xent" in _lib._SIGNATURES:
        extra = [getattr(a, "value", a) for a in args[len(types):]] + [None, None]
        entry["windows"] = "ptr" if extra[0] else None
        entry["xent"] = None
        if extra[1]:
            xe = _lib.Xent.from_address(extra[1])
            entry["xent"] = {"z_dtype": xe.z_dtype, "grad_scale": ctypes.c_float(xe.grad_scale).value.hex(),
                             "loss_coef": ctypes.c_float(xe.loss_coef).value.hex(), "xent_grad": "ptr" if xe.xent_grad else None,
                             "xent_totals": "ptr" if xe.xent_totals else None, "workspace_bytes": int(xe.workspace_bytes)}
    return entry


class Recorder(object):
    """Stands where pychain_amd._lib keeps the loaded library; every pychain_hip_* call lands in `calls` first."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("pychain_hip_") or name in _PLAN_LIFECYCLE or getattr(fn, "argtypes", None) is None:
            return fn

        def call(*args):
            self.calls.append(_describe(name, args))
            return fn(*args)
        return call


# ---------------------------------------------------------------------------
# the configurations
# ---------------------------------------------------------------------------
def _name(route, xent, reg, weights, avg, lengths="host", variant=""):
    return "%s/xent%d/reg%d/w-%s/avg%d/len-%s%s" % (route, xent, reg, weights, avg, lengths, "/" + variant if variant else "")


def configs(section):
    """The names of a section's configurations, in file order."""
    out = []
    grid = [(xe, rg, w, avg) for xe in (0, 1) for rg in (0, 1) for w in ("none", "u", "f", "both") for avg in (0, 1)]
    if section == "cpu":
        return [_name("cpu", *g) for g in grid]
    for route in ("fused", "late", "unfused"):           # late: ChainLossFunction.overlap = False; unfused: crit.fused = False
        out += [_name(route, *g, lengths=ln) for g in grid for ln in ("host", "dev")]
    for variant in ("bf16", "windows", "nograd", "zgrad"):
        for route in ("fused", "late"):
            out += [_name(route, xe, rg, w, 1, "host", variant) for xe in ((1,) if variant == "zgrad" else (0, 1))
                    for rg in (0, 1) for w in ("none", "both")]
    return out


def _parse(name):
    parts = name.split("/")
    return dict(route=parts[0], xent=int(parts[1][4:]), reg=int(parts[2][3:]), weights=parts[3][2:], avg=int(parts[4][3:]),
                lengths=parts[5][4:], variant=parts[6] if len(parts) > 6 else "")


_inputs = {}


def _fixture():
    """The step's inputs, made once: (den graph, numerator graphs, the same with time windows set, x, z, u, f)."""
    if not _inputs:
        lengths = torch.tensor(LENGTHS)
        graphs = syn.make_num_graphs(LENGTHS, D, seed=100, max_states=8)
        windowed = syn.make_num_graphs(LENGTHS, D, seed=100, max_states=8)
        x = syn.make_input(B, T, D, seed=5)
        x[0, 0, 0], x[1, 2, 3] = 33.0, -31.5                        # (the out-of-range penalty has something to do)
        ali = viterbi_align(x, lengths, windowed)
        assert bool(ali.ok.all())
        windowed.set_time_windows(alignment_windows(ali, windowed.num_states, 1))
        u = torch.tensor([0.5, 0.0, 2.0])
        f = ((torch.arange(B * T, dtype=torch.float32) % 4) * 0.5).reshape(B, T)       # weights 0, 0.5, 1, 1.5
        _inputs.update(den=syn.make_den_graph(20, 60, D, seed=0), graphs=graphs, windowed=windowed, x=x,
                       z=syn.make_input(B, T, D, seed=6), u=u, f=f, lengths=lengths)
    return _inputs


def _bytes_hash(t):
    if t is None:
        return None
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def step(name, bits=None):
    """One step of the configuration `name` under the recorder: {"forward": [...], "backward": [[...], [...]]}.  `bits`: a dict
    that receives the loss and the hashes of the gradients after each backward."""
    c, fx = _parse(name), _fixture()
    dev = "cpu" if c["route"] == "cpu" else DEV
    crit = ChainLoss(fx["den"], 1e-5, avg=bool(c["avg"]), xent_regularize=XENT_C if c["xent"] else 0.0,
                     output_l2_regularize=L2 if c["reg"] else 0.0, out_of_range_regularize=OOR if c["reg"] else 0.0)
    crit.fused = c["route"] != "unfused"
    dtype = torch.bfloat16 if c["variant"] == "bf16" else torch.float32
    x = fx["x"].clone().to(device=dev, dtype=dtype).requires_grad_(c["variant"] not in ("nograd", "zgrad"))
    z = fx["z"].clone().to(device=dev, dtype=dtype).requires_grad_(c["variant"] != "nograd") if c["xent"] else None
    lengths = fx["lengths"].to(dev) if c["lengths"] == "dev" else fx["lengths"]
    graphs = fx["windowed"] if c["variant"] == "windows" else fx["graphs"]
    kw = {}
    if c["weights"] in ("u", "both"):
        kw["utt_weights"] = fx["u"]
    if c["weights"] in ("f", "both"):
        kw["deriv_weights"] = fx["f"]
    if dev != "cpu":
        graphs.device_tensors(torch.device(dev))               # (uploads are no library calls; made ahead all the same)
        torch.cuda.synchronize()
    native.release_workspaces()                                # (a cached workspace's size would depend on earlier calls)
    real, overlap = _lib.lib(), ChainLossFunction.overlap
    rec = Recorder(real)
    _lib._lib, ChainLossFunction.overlap = rec, c["route"] != "late"
    try:
        loss = crit(x, lengths, graphs, xent_output=z, **kw)
        marks = [len(rec.calls)]
        got = []
        if loss.requires_grad:
            for retain in (True, False):
                loss.backward(retain_graph=retain)
                marks.append(len(rec.calls))
                got.append((_bytes_hash(x.grad), _bytes_hash(None if z is None else z.grad)))
        if dev != "cpu":
            torch.cuda.synchronize()
    finally:
        _lib._lib, ChainLossFunction.overlap = real, overlap
    if bits is not None:
        bits[name] = {"loss": float(loss.detach()).hex(), "x_grad": [g[0] for g in got], "z_grad": [g[1] for g in got]}
    marks += [marks[-1]] * (3 - len(marks))
    backward = [rec.calls[marks[0]:marks[1]], rec.calls[marks[1]:marks[2]]]
    if c["route"] in ("cpu", "unfused"):
        backward = [sorted(s, key=_canonical) for s in backward]
    return {"forward": rec.calls[:marks[0]], "backward": backward}


def _canonical(obj):
    return json.dumps(obj, sort_keys=True, separators=(",", ":"))


def summary(trace):
    """(the family names as one string, "|" between the sections; SHA-256 of the canonical JSON of the full trace)"""
    names = " | ".join(" ".join(e["fn"] for e in s) for s in [trace["forward"]] + trace["backward"])
    return names, hashlib.sha256(_canonical(trace).encode()).hexdigest()


def record(section):
    """{"sequences": [distinct name strings], "configs": {name: [index into sequences, sha256]}} of a section."""
    seqs, out = [], {}
    for name in configs(section):
        names, digest = summary(step(name))
        if names not in seqs:
            seqs.append(names)
        out[name] = [seqs.index(names), digest]
    return {"sequences": seqs, "configs": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--section", default="all", choices=["cpu", "gpu", "all"])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--dump", metavar="CONFIG")
    ap.add_argument("--bits", metavar="FILE")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    sections = ["cpu", "gpu"] if a.section == "all" else [a.section]
    if a.list:
        print("\n".join(n for s in sections for n in configs(s)))
    elif a.dump:
        print(json.dumps(step(a.dump), indent=1, sort_keys=True))
    elif a.bits:
        bits = {}
        with _lib.option("den_tseg", "0"):                     # (include/pychain_hip.h: the switch for bit-for-bit reproducibility)
            for s in sections:
                for name in configs(s):
                    step(name, bits)
        with open(a.bits, "w") as f:
            json.dump(bits, f, indent=0, sort_keys=True)
        print("%d configurations -> %s" % (len(bits), a.bits))
    else:
        golden = {}
        if os.path.exists(OUT):                                # (a section that is not recorded now stays as it is)
            with open(OUT) as f:
                golden = json.load(f)
        for s in sections:
            golden[s] = record(s)
        with open(a.out, "w") as f:
            f.write("{\n" + ",\n".join(
                '"%s": {"sequences": [\n%s\n],\n "configs": {\n%s\n}}' % (
                    s, ",\n".join(json.dumps(q) for q in golden[s]["sequences"]),
                    ",\n".join('%s: %s' % (json.dumps(k), json.dumps(v)) for k, v in golden[s]["configs"].items()))
                for s in sorted(golden)) + "\n}\n")
        print("%s -> %s (%d bytes)" % (", ".join("%s: %d" % (s, len(golden[s]["configs"])) for s in sections), a.out,
                                       os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
