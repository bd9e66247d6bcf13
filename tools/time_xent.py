"""Cost of the xent regularisation at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, H <= 400, D = 3456), one process, the
legs alternating round by round so that drift of the box falls on all of them:

  A       the fused ChainLoss forward + backward step, xent off
  B_f32   the same step with ChainLoss(xent_regularize=c) and an fp32 xent output z (gradient of z written by the step)
  B_bf16  ... with a bf16 z
  C       what the library offered before: the fused step, a second numerator call for dense posteriors
          (native.num_forward_backward, linear gradient) and the torch composition -c / frames * (gamma * log_softmax(z)).sum()
          with its backward

Prints one JSON line: medians, the spread of A (max - min of its per-round medians), B - A, C - B, and the bytes the row
kernel has to move (sum_b L_b D (sizeof z + sizeof dz) + the compact rows).

    python tools/time_xent.py [--reps N] [--rounds R] [--config C3]
    python tools/time_xent.py --profile [bf16]     # a few B steps only (under rocprofv3 --kernel-trace --stats)
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainLoss, _lib, native, synthetic as syn  # noqa: E402

C = 0.1


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
    arg = lambda name, dflt: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else dflt
    reps, rounds, config = int(arg("--reps", 7)), int(arg("--rounds", 4)), arg("--config", "C3")
    dev = torch.device("cuda:0")
    w = syn.make_workload(config, device=dev)
    g, x, L = w["num_graphs"], w["x"], w["lengths"]
    gt = g.device_tensors(dev)
    Ld = L.to(dev)
    frames = float(L.sum())
    z32 = syn.make_input(x.shape[0], x.shape[1], x.shape[2], seed=77, device=dev)
    zs = {"f32": z32, "bf16": z32.to(torch.bfloat16)}
    off = ChainLoss(w["den_graph"], 1e-5)
    on = ChainLoss(w["den_graph"], 1e-5, xent_regularize=C)

    def leg_a():
        xx = x.detach().requires_grad_(True)
        off(xx, L, g).backward()

    def leg_b(z):
        def run():
            xx = x.detach().requires_grad_(True)
            zz = z.detach().requires_grad_(True)
            on(xx, L, g, xent_output=zz).backward()
        return run

    def leg_c():
        xx = x.detach().requires_grad_(True)
        off(xx, L, g).backward()
        _, gamma, _ = native.num_forward_backward(gt, 1, g.num_states, x, Ld, grad_mode=_lib.GRAD_LINEAR)
        zz = z32.detach().requires_grad_(True)
        ((-C / frames) * (gamma * torch.log_softmax(zz, -1)).sum()).backward()

    if "--profile" in sys.argv:
        run = leg_b(zs["bf16" if "bf16" in sys.argv else "f32"])
        for _ in range(6):
            run()
        torch.cuda.synchronize()
        return
    legs = {"A_ms": leg_a, "B_f32_ms": leg_b(zs["f32"]), "B_bf16_ms": leg_b(zs["bf16"]), "C_ms": leg_c}
    acc = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc[k] += t
            per_round[k].append(median(t))
    B, T, D = x.shape
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "K": int(g.num_transitions), "c": C, "reps": reps * rounds}
    out.update({k: round(median(v), 4) for k, v in acc.items()})
    out["A_spread_ms"] = round(max(per_round["A_ms"]) - min(per_round["A_ms"]), 4)
    out["A_round_medians_ms"] = [round(v, 4) for v in per_round["A_ms"]]
    for k in ("B_f32_ms", "B_bf16_ms"):
        out[k.replace("_ms", "_minus_A_ms")] = round(out[k] - out["A_ms"], 4)
        out["C_minus_" + k] = round(out["C_ms"] - out[k], 4)
    live = int(L.sum())
    rows = live * int(g.num_transitions) * 4
    out["row_kernel_bytes_f32"] = live * D * 8 + rows
    out["row_kernel_bytes_bf16"] = live * D * 4 + rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
