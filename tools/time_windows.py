"""Cost of alignment time windows at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, H <= 400, D = 3456): the median numerator
call (num_fb + num_occ, linear gradient) and the median fused ChainLoss forward + backward step, each without windows and with
tau = 2 windows around a device viterbi_align of the same input.  The two legs alternate round by round, so drift of the box
falls on both.  Prints one JSON line.

    python tools/time_windows.py [--reps N] [--rounds R]
    python tools/time_windows.py --profile        # a few windowed fused steps only (under rocprofv3 --kernel-trace --stats)
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainLoss, _lib, alignment_windows, native, viterbi_align, synthetic as syn  # noqa: E402


def times_ms(call, reps):
    call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
    dev = torch.device("cuda:0")
    w = syn.make_workload("C3", device=dev)
    g, x, L = w["num_graphs"], w["x"], w["lengths"]
    gt = g.device_tensors(dev)
    Ld = L.to(dev)
    ali = viterbi_align(x, Ld, g)
    tw = alignment_windows(ali, g.num_states, 2)
    crit = ChainLoss(w["den_graph"], 1e-5)

    def num_call(windows):
        return lambda: native.num_forward_backward(gt, 1, g.num_states, x, Ld, grad_mode=_lib.GRAD_LINEAR, windows=windows)

    def step(windows):
        def run():
            g.set_time_windows(windows)
            xx = x.detach().requires_grad_(True)
            crit(xx, L, g).backward()
        return run

    if "--profile" in sys.argv:
        for _ in range(6):
            step(tw)()
        torch.cuda.synchronize()
        return
    acc = {k: [] for k in ("num_ms", "num_tw_ms", "step_ms", "step_tw_ms")}
    for _ in range(rounds):
        acc["num_ms"] += times_ms(num_call(None), reps)
        acc["num_tw_ms"] += times_ms(num_call(tw), reps)
        acc["step_ms"] += times_ms(step(None), reps)
        acc["step_tw_ms"] += times_ms(step(tw), reps)
    g.set_time_windows(None)
    out = {"config": "C3", "B": int(x.shape[0]), "T": int(x.shape[1]), "H": int(g.num_states), "K": int(g.num_transitions),
           "D": int(x.shape[2]), "tau": 2, "reps": reps * rounds}
    out.update({k: round(median(v), 4) for k, v in acc.items()})
    out["num_tw_over_num"] = round(out["num_tw_ms"] / out["num_ms"], 4)
    out["step_tw_over_step"] = round(out["step_tw_ms"] / out["step_ms"], 4)
    # how tight the windows are: admissible (state, time) pairs per frame, averaged over the batch
    Lf = L.to(dev).to(torch.float64)
    span = (tw[..., 1].clamp(max=Ld.view(-1, 1)) - tw[..., 0] + 1).clamp(min=0).to(torch.float64).sum(1)
    out["admissible_states_per_frame"] = round(float((span / (Lf + 1)).mean()), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
