"""What the entry points of the C ABI answer to calls they must refuse: the return code and pychain_hip_last_error().

    python tests/golden/make_api_refusals.py        # writes tests/golden/api_refusals.json

Every case starts from a call that would be accepted and makes one thing wrong (a few make two, to pin which refusal
comes first; a few go through a narrow entry point, to pin the forwarding).  Every call is refused before the library
touches the device or reads through a pointer, so the pointers are made-up 256-aligned addresses and no GPU is needed;
only the sequence lengths of the host twins (which are read) and the pychain_hip_xent struct are real memory.
tests/test_api.py::test_refusals_match_the_recorded_ones repeats every case with the library under test and compares;
the file is only regenerated when a refusal changes ON PURPOSE - a refactor does not regenerate it.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "api_refusals.json")

TILE_HINT = 32 | (32 << 10) | (32 << 20) | (1 << 30)      # a plan in the tile format (make_den_decisions.py: hint)

G8 = ["ft", "fi", "fp", "bt", "bi", "bp", "initial", "final_"]
NUM = G8 + ["stride", "x", "dtype", "lengths", "B", "T", "D", "H", "K", "grad_mode", "grad_scale", "objf", "grad", "bad_count",
            "num_ws", "num_ws_bytes", "stream"]
ALIGN = G8 + ["stride", "x", "dtype", "lengths", "B", "T", "D", "H", "K", "score", "states", "pdfs", "bad_count",
              "align_ws", "align_ws_bytes", "stream"]
_FUSED_HEAD = ["plans", "plan_stride", "hint", "den_H", "leaky"] + G8 + ["stride", "H", "K", "x", "dtype", "lengths", "B", "T", "D"]
_FUSED_TAIL = ["loss_scale", "norm", "totals", "den_ws", "den_ws_bytes", "num_ws", "num_ws_bytes", "stream"]
FWD = _FUSED_HEAD + ["den_objf", "objf", "grad", "grad_scale", "bad_count"] + _FUSED_TAIL
FB = _FUSED_HEAD + ["grad_scale", "den_objf", "objf", "grad", "bad_count"] + _FUSED_TAIL
BWD = ["plans", "plan_stride", "hint", "den_H", "ft", "fi", "fp", "stride", "H", "K", "x", "dtype", "lengths", "B", "T", "D",
       "grad_scale", "scale_dev", "grad", "bad_count", "den_ws", "den_ws_bytes", "num_ws", "num_ws_bytes", "stream"]
DEN = ["plans", "plan_stride", "hint", "den_H", "D", "x", "dtype", "is_exp", "lengths", "B", "T", "leaky", "grad_scale", "den_objf",
       "grad", "bad_count", "totals", "den_ws", "den_ws_bytes", "stream"]
CPU_DEN = ["ft", "fi", "fp", "bt", "bi", "bp", "leaky_probs", "initial", "final_", "stride", "x", "is_exp", "host_lengths",
           "B", "T", "D", "H", "K", "leaky", "grad_scale", "objf", "grad", "bad_count", "threads"]
CPU_NUM = G8 + ["stride", "x", "host_lengths", "B", "T", "D", "H", "K", "grad_mode", "grad_scale", "objf", "grad", "bad_count", "threads"]
CPU_ALIGN = G8 + ["stride", "x", "host_lengths", "B", "T", "D", "H", "K", "score", "states", "pdfs", "bad_count", "threads"]
ENTRIES = {
    "num_forward_backward": NUM, "num_forward_backward_tw": NUM + ["windows"], "num_forward_backward_xent": NUM + ["windows", "xent"],
    "align": ALIGN, "align_tw": ALIGN + ["windows"],
    "chain_loss_forward": FWD, "chain_loss_forward_tw": FWD + ["windows"], "chain_loss_forward_xent": FWD + ["windows", "xent"],
    "chain_loss_forward_backward": FB, "chain_loss_forward_backward_tw": FB + ["windows"],
    "chain_loss_forward_backward_xent": FB + ["windows", "xent"],
    "chain_loss_backward": BWD, "den_forward_backward": DEN,
    "cpu_den_forward_backward": CPU_DEN,
    "cpu_num_forward_backward": CPU_NUM, "cpu_num_forward_backward_tw": CPU_NUM + ["windows"],
    "cpu_num_forward_backward_xent": CPU_NUM + ["windows", "xent"],
    "cpu_align": CPU_ALIGN, "cpu_align_tw": CPU_ALIGN + ["windows"],
}

POINTERS = ["plans"] + G8 + ["x", "lengths", "objf", "den_objf", "grad", "bad_count", "totals", "norm", "scale_dev", "den_ws", "num_ws",
                             "align_ws", "score", "states", "pdfs", "leaky_probs", "windows_at", "z", "xent_grad", "xent_objf", "xent_ws"]
ADDR = {p: 0x10000000 + 0x10000 * i for i, p in enumerate(POINTERS)}
SIZES = {"B": 4, "T": 10, "D": 8, "H": 5, "K": 9, "den_H": 64}
GOOD = dict(ADDR, **SIZES)
GOOD.update(stride=1, dtype=0, grad_mode=2, grad_scale=1.0, stream=None, plan_stride=0, hint=TILE_HINT, leaky=1e-5, loss_scale=1.0,
            norm=None, totals=None, scale_dev=None, is_exp=0, threads=1, windows=None, xent=None)
XENT_GOOD = dict(z=ADDR["z"], z_dtype=0, xent_grad=ADDR["xent_grad"], grad_scale=1.0, grad_scale_dev=None, loss_coef=0.1,
                 xent_objf_per_seq=ADDR["xent_objf"], xent_totals=None, workspace=ADDR["xent_ws"], workspace_bytes="full")
HOST_LENGTHS = {"ok": np.array([10, 7, 1, 3], dtype=np.int64), "long": np.array([10, 11, 1, 3], dtype=np.int64),
                "zero": np.array([10, 7, 0, 3], dtype=np.int64)}


def null(*ps):
    return {p: None for p in ps}


def off4(*ps):
    return {p: ADDR[p] + 4 for p in ps}


def case(entry, set=None, options=None, xent=None):
    return {"entry": entry, "set": dict(set or {}), "options": dict(options or {}), "xent": xent}


def _value_name(k, v):
    if v is None:
        return k + "=null"
    if k in ADDR and v == ADDR[k] + 4:
        return k + "+4"
    if k in ADDR and v == ADDR[k]:
        return k
    return "%s=%s" % (k, v)


def case_name(c):
    parts = [_value_name(k, v) for k, v in c["set"].items()]
    if c["xent"] is not None:
        parts.append("xent{%s}" % ",".join(_value_name(k, v) for k, v in c["xent"].items()))
    parts += ["option %s=%s" % kv for kv in c["options"].items()]
    return "%s: %s" % (c["entry"], ", ".join(parts))


COMPAT = {"num_compat": 1}
WINDOWS = {"windows": ADDR["windows_at"]}


def cases():
    out = []
    dev = {"num_forward_backward_xent": dict(
               ptrs=G8 + ["x", "lengths", "objf", "grad", "bad_count", "num_ws"], sizes=["B", "T", "D", "H", "K"],
               aligned=["x", "grad", "fi", "bi"], ws=["num_ws_bytes"]),
           "align_tw": dict(
               ptrs=["bt", "bi", "bp", "initial", "final_", "x", "lengths", "score", "states", "pdfs", "bad_count", "align_ws"],
               sizes=["B", "T", "D", "H", "K"], aligned=["x", "bi"], ws=["align_ws_bytes"]),
           "chain_loss_forward_xent": dict(
               ptrs=["bad_count", "plans", "x", "lengths", "den_objf", "den_ws"] + G8 + ["objf", "num_ws"],
               sizes=["B", "T", "D", "den_H", "H", "K"], aligned=["plans", "x", "grad", "den_ws", "fi", "bi"],
               ws=["den_ws_bytes", "num_ws_bytes"]),
           "chain_loss_backward": dict(
               ptrs=["bad_count", "ft", "fi", "fp", "plans", "x", "lengths", "grad", "den_ws", "num_ws"],
               sizes=["B", "T", "D", "den_H", "H", "K"], aligned=["plans", "x", "grad", "den_ws", "fi"],
               ws=["den_ws_bytes", "num_ws_bytes"]),
           "den_forward_backward": dict(
               ptrs=["plans", "x", "lengths", "den_objf", "grad", "bad_count", "den_ws"], sizes=["B", "T", "den_H", "D"],
               aligned=["plans", "x", "grad", "den_ws"], ws=["den_ws_bytes"])}
    for entry, d in dev.items():
        out.append(case(entry, {"dtype": 7}))
        out += [case(entry, null(p)) for p in d["ptrs"]]
        out += [case(entry, {s: 0}) for s in d["sizes"]]
        out.append(case(entry, {d["sizes"][0]: -3}))
        if "stride" in ENTRIES[entry]:
            out.append(case(entry, {"stride": 2}))
        out += [case(entry, off4(p)) for p in d["aligned"]]
        out += [case(entry, {w: "small"}) for w in d["ws"]]
        if "plans" in ENTRIES[entry]:
            out.append(case(entry, {"plan_stride": 8}))
            out.append(case(entry, {"plan_stride": -16}))
            out.append(case(entry, {"den_H": 70000}))
        if "leaky" in ENTRIES[entry]:
            out += [case(entry, {"leaky": 0.0}), case(entry, {"leaky": 2.0})]
    out.append(case("num_forward_backward_xent", {"grad_mode": 9}))
    out.append(case("num_forward_backward_xent", {"grad_mode": -1}))
    # 2-byte rows where the shape or the entry point does not take them
    out.append(case("align_tw", {"dtype": 1, "D": 6}))
    out.append(case("num_forward_backward_xent", {"dtype": 2, "D": 6}))
    out.append(case("chain_loss_backward", {"dtype": 1}))
    # the xent struct
    for entry in ("num_forward_backward_xent", "chain_loss_forward_xent"):
        out += [case(entry, xent={"z": None}), case(entry, xent={"xent_objf_per_seq": None}), case(entry, xent={"workspace": None}),
                case(entry, xent={"z_dtype": 5}), case(entry, xent={"z": ADDR["z"] + 4}), case(entry, xent={"xent_grad": ADDR["xent_grad"] + 4}),
                case(entry, xent={"workspace": ADDR["xent_ws"] + 4}), case(entry, xent={"workspace_bytes": "small"}),
                case(entry, {"K": 0}, xent={}), case(entry, xent={}, options=COMPAT), case(entry, WINDOWS, options=COMPAT)]
    out.append(case("chain_loss_forward_backward_xent", null("grad")))
    out.append(case("chain_loss_forward_backward_xent", xent={"z": None}))
    out.append(case("chain_loss_forward_backward_xent", {"leaky": 0.0}))
    # the host twins
    host = {"cpu_num_forward_backward_xent": G8 + ["x", "host_lengths", "objf", "grad", "bad_count"],
            "cpu_align_tw": G8 + ["x", "host_lengths", "score", "states", "pdfs", "bad_count"],
            "cpu_den_forward_backward": G8 + ["leaky_probs", "x", "host_lengths", "objf", "grad", "bad_count"]}
    for entry, ptrs in host.items():
        out += [case(entry, null(p)) for p in ptrs]
        out += [case(entry, {s: 0}) for s in ("B", "T", "D", "H", "K")]
        out.append(case(entry, {"stride": 2}))
        out += [case(entry, {"host_lengths": "long"}), case(entry, {"host_lengths": "zero"})]
    out += [case("cpu_den_forward_backward", {"leaky": 0.0}), case("cpu_den_forward_backward", {"leaky": 2.0}),
            case("cpu_num_forward_backward_xent", {"grad_mode": 9}), case("cpu_num_forward_backward_xent", {"grad_mode": 0x100 | 9}),
            case("cpu_num_forward_backward_xent", xent={"z": None}), case("cpu_num_forward_backward_xent", xent={"xent_objf_per_seq": None}),
            case("cpu_num_forward_backward_xent", xent={"z_dtype": 1})]
    # two things wrong: which refusal comes first
    out += [case("num_forward_backward_xent", dict({"dtype": 7}, **null("ft"))),
            case("num_forward_backward_xent", dict({"B": 0}, **off4("x"))),
            case("num_forward_backward_xent", null("ft"), xent={"z": None}),
            case("num_forward_backward_xent", {"stride": 2, "grad_mode": 9}),
            case("num_forward_backward_xent", dict(WINDOWS, num_ws_bytes="small"), options=COMPAT),
            case("num_forward_backward_xent", {"dtype": 1, "D": 6, "num_ws_bytes": "small"}),
            case("chain_loss_forward_xent", dict(null("bad_count"), den_ws_bytes="small")),
            case("chain_loss_forward_xent", {"den_ws_bytes": "small", "num_ws_bytes": "small"}),
            case("chain_loss_forward_xent", {"leaky": 0.0, "stride": 2}),
            case("chain_loss_forward_xent", dict(null("plans"), dtype=7)),
            case("chain_loss_forward_xent", null("ft"), xent={"workspace_bytes": "small"}),
            case("chain_loss_forward_xent", xent={"z": ADDR["z"] + 4}, options=COMPAT),
            case("chain_loss_forward_backward_xent", null("grad", "bad_count")),
            case("align_tw", {"stride": 2, "align_ws_bytes": "small"}),
            case("align_tw", {"dtype": 1, "D": 6, "align_ws_bytes": "small"}),
            case("den_forward_backward", dict(off4("plans"), plan_stride=8)),
            case("den_forward_backward", {"den_H": 70000, "leaky": 2.0}),
            case("chain_loss_backward", dict(null("plans"), dtype=1)),
            case("chain_loss_backward", dict(null("ft"), dtype=1)),
            case("cpu_num_forward_backward_xent", null("ft"), xent={"z": None}),
            case("cpu_num_forward_backward_xent", {"host_lengths": "long", "stride": 2}),
            case("cpu_den_forward_backward", dict(null("leaky_probs"), stride=2)),
            case("cpu_den_forward_backward", {"stride": 2, "leaky": 2.0}),
            case("cpu_align_tw", dict(null("pdfs"), stride=2))]
    # the narrow entry points forward to the widest one
    out += [case("num_forward_backward", {"dtype": 7}), case("num_forward_backward", null("grad")), case("num_forward_backward_tw", {"stride": 2}),
            case("num_forward_backward_tw", WINDOWS, options=COMPAT),
            case("align", null("bt")), case("align", {"align_ws_bytes": "small"}),
            case("chain_loss_forward", null("bad_count")), case("chain_loss_forward", {"num_ws_bytes": "small"}),
            case("chain_loss_forward_tw", {"leaky": 2.0}), case("chain_loss_forward_tw", WINDOWS, options=COMPAT),
            case("chain_loss_forward_backward", null("grad")), case("chain_loss_forward_backward", {"den_ws_bytes": "small"}),
            case("chain_loss_forward_backward_tw", null("grad")), case("chain_loss_forward_backward_tw", {"B": 0}),
            case("cpu_num_forward_backward", {"grad_mode": 9}), case("cpu_num_forward_backward_tw", {"host_lengths": "long"}),
            case("cpu_align", {"stride": 2}), case("cpu_align", null("pdfs"))]
    return out


def run(L, _lib, c):
    """(return code, last error) of one case with library `L` (pychain_amd._lib.lib())."""
    def go():
        v = dict(GOOD)
        s = SIZES
        full = {"den_ws_bytes": L.pychain_hip_den_workspace_bytes(s["B"], s["T"], s["den_H"], s["D"]),
                "num_ws_bytes": L.pychain_hip_num_workspace_bytes(s["B"], s["T"], s["H"], s["K"], s["D"]),
                "align_ws_bytes": L.pychain_hip_align_workspace_bytes(s["B"], s["T"], s["H"], s["K"], s["D"])}
        v.update(full)
        v["host_lengths"] = "ok"
        v.update(c["set"])
        for k in full:
            if v[k] == "small":
                v[k] = full[k] // 2 // 256 * 256
        if v["host_lengths"] is not None:
            v["host_lengths"] = HOST_LENGTHS[v["host_lengths"]].ctypes.data
        keep = None
        if c["xent"] is not None:
            x = dict(XENT_GOOD, **c["xent"])
            xfull = L.pychain_hip_xent_workspace_bytes(s["B"], s["T"], s["H"], s["K"], s["D"])
            x["workspace_bytes"] = xfull if x["workspace_bytes"] == "full" else xfull - 256
            keep = _lib.Xent(**x)
            v["xent"] = ctypes.addressof(keep)
        rc = getattr(L, "pychain_hip_" + c["entry"])(*[v[p] for p in ENTRIES[c["entry"]]])
        return rc, L.pychain_hip_last_error().decode()
    if not c["options"]:
        return go()
    (name, value), = c["options"].items()
    with _lib.option(name, value):
        return go()


def compute(_lib):
    """[[case name, return code, last error], ...] in the order of cases(); `_lib`: pychain_amd._lib of the tree under test."""
    L = _lib.lib()
    out = []
    for c in cases():
        rc, err = run(L, _lib, c)
        out.append([case_name(c), rc, err])
    return out


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    from pychain_amd import _lib
    got = compute(_lib)
    assert len(set(g[0] for g in got)) == len(got), "case names must be distinct"
    assert all(g[1] < 0 for g in got), [g for g in got if g[1] >= 0]
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(g) for g in got) + "\n]\n")
    print("%d cases -> %s (%d bytes)" % (len(got), OUT, os.path.getsize(OUT)))
