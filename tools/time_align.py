"""Time viterbi_align's device call at C3 (synthetic.make_workload("C3") numerators: B = 64, T <= 1500, H <= 400, D = 3456) next to
the numerator call (num_fb + num_occ, linear gradient: tools/time_num.py) measured in the same process, and the windowed call
(pychain_hip_align_tw: windows at tolerance 2 around the same input's own alignment) next to the unwindowed one, the two legs
alternating call by call: median and [min, max] of each leg, so the spread stands beside the difference.  Prints one JSON line.

    python tools/time_align.py [--reps N]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import Alignment, _lib, alignment_windows, native, synthetic as syn  # noqa: E402


def median_ms(call, reps):
    call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def alternating_ms(calls, reps):
    """[median, min, max] ms of each call, the calls taking turns rep by rep (what drifts, drifts under all of them)."""
    for call in calls:
        call()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls] for _ in range(reps)]
    for row in ev:
        for call, (a, b) in zip(calls, row):
            a.record()
            call()
            b.record()
    torch.cuda.synchronize()
    out = []
    for i in range(len(calls)):
        t = sorted(row[i][0].elapsed_time(row[i][1]) for row in ev)
        out.append([t[len(t) // 2], t[0], t[-1]])
    return out


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
    dev = torch.device("cuda:0")
    w = syn.make_workload("C3", device=dev)
    g = w["num_graphs"]
    gt = g.device_tensors(dev)
    Ld = w["lengths"].to(dev)
    out = {"config": "C3", "B": int(w["x"].shape[0]), "T": int(w["x"].shape[1]), "H": int(g.num_states), "K": int(g.num_transitions),
           "D": int(w["x"].shape[2]), "lib": os.path.basename(_lib.LIB_PATH)}
    out["align_ms"] = median_ms(lambda: native.align(gt, 1, g.num_states, w["x"], Ld), reps)
    out["num_fb_occ_ms"] = median_ms(lambda: native.num_forward_backward(gt, 1, g.num_states, w["x"], Ld, grad_mode=_lib.GRAD_LINEAR), reps)
    xb = w["x"].to(torch.bfloat16)
    out["align_bf16_ms"] = median_ms(lambda: native.align(gt, 1, g.num_states, xb, Ld), reps)
    score, states, pdfs, _ = native.align(gt, 1, g.num_states, w["x"], Ld)
    tw = alignment_windows(Alignment(pdfs, states, score, torch.isfinite(score)), g.num_states, 2)
    out["tau"] = 2
    out["admissible_states_per_frame"] = float(((tw[..., 1] - tw[..., 0] + 1).clamp(min=0).sum(1).double() / (Ld.double() + 1)).mean())
    for tag, x in (("", w["x"]), ("_bf16", xb)):
        free, win = alternating_ms([lambda: native.align(gt, 1, g.num_states, x, Ld),
                                    lambda: native.align(gt, 1, g.num_states, x, Ld, windows=tw)], max(reps, 15))
        out["align_free%s_ms" % tag], out["align_tw%s_ms" % tag] = free, win
    print(json.dumps(out))


if __name__ == "__main__":
    main()
