"""Cost of the output regularisers at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, D = 3456), one process, the legs
alternating round by round so that drift of the box falls on all of them:

  A, A_bf16    the fused ChainLoss forward + backward step as it is (both coefficients zero), fp32 / bf16 network output
  B_l2_<t>     the same step with ChainLoss(output_l2_regularize=l2)                              <t>: fp32 / bf16 network output
  B_both_<t>   ... with output_l2_regularize=l2 and out_of_range_regularize=r
  C_l2, C_both what the library offered before: step A plus the torch composition of the same terms over the live frames with its
               backward (fp32), autograd adding the second dense gradient
  copy         a streaming copy (torch's copy_ of a buffer as large as the network output): the measured copy rate of the run

Prints one JSON line: medians, the spread of A (max - min of its per-round medians), B - A, C - A, C - B, the bytes the pass has
to move (3 * sizeof(x) * sum_b L_b * D), their time at the measured copy rate and 1.5 x that.

    python tools/time_outreg.py [--reps N] [--rounds R] [--config C3]
    python tools/time_outreg.py --profile [bf16]     # a few B steps only (under rocprofv3 --kernel-trace --stats)
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainLoss, synthetic as syn  # noqa: E402

L2, OOR = 5e-4, 0.01


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
    g, x32, L = w["num_graphs"], w["x"], w["lengths"]
    B, T, D = x32.shape
    frames = float(L.sum())
    xs = {"fp32": x32, "bf16": x32.to(torch.bfloat16)}
    live = (torch.arange(T, device=dev)[None, :] < L.to(dev)[:, None]).to(torch.float32)[..., None]     # [B,T,1]
    off = ChainLoss(w["den_graph"], 1e-5)
    on = {"l2": ChainLoss(w["den_graph"], 1e-5, output_l2_regularize=L2),
          "both": ChainLoss(w["den_graph"], 1e-5, output_l2_regularize=L2, out_of_range_regularize=OOR)}

    def leg_a(x):
        def run():
            xx = x.detach().requires_grad_(True)
            off(xx, L, g).backward()
        return run

    def leg_b(crit, x):
        def run():
            xx = x.detach().requires_grad_(True)
            crit(xx, L, g).backward()
        return run

    def leg_c(both):
        def run():
            xx = x32.detach().requires_grad_(True)
            loss = off(xx, L, g)
            term = 0.5 * L2 * ((xx ** 2) * live).sum()
            if both:
                term = term + OOR * (((xx.abs() - 30.0).clamp_min(0.0) ** 2) * live).sum()
            (loss + term / frames).backward()
        return run

    src, dst = torch.empty_like(x32), torch.empty_like(x32)

    def leg_copy():
        dst.copy_(src)

    if "--profile" in sys.argv:
        run = leg_b(on["both"], xs["bf16" if "bf16" in sys.argv else "fp32"])
        for _ in range(6):
            run()
        torch.cuda.synchronize()
        return
    legs = {"A_ms": leg_a(xs["fp32"]), "A_bf16_ms": leg_a(xs["bf16"]), "copy_ms": leg_copy}
    for t, x in xs.items():
        for k, crit in on.items():
            legs["B_%s_%s_ms" % (k, t)] = leg_b(crit, x)
    legs["C_l2_ms"], legs["C_both_ms"] = leg_c(False), leg_c(True)
    acc = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc[k] += t
            per_round[k].append(median(t))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "live_frames": int(L.sum()), "l2": L2, "oor": OOR, "reps": reps * rounds}
    out.update({k: round(median(v), 4) for k, v in acc.items()})
    out["A_spread_ms"] = round(max(per_round["A_ms"]) - min(per_round["A_ms"]), 4)
    out["A_round_medians_ms"] = [round(v, 4) for v in per_round["A_ms"]]
    # (a copy reads and writes the buffer once: 2 * bytes of it per copy)
    rate = 2.0 * x32.numel() * 4 / (out["copy_ms"] * 1e-3)
    out["copy_rate_TBps"] = round(rate / 1e12, 3)
    for t, size in (("fp32", 4), ("bf16", 2)):
        nbytes = 3 * size * int(L.sum()) * D
        out["pass_bytes_" + t] = nbytes
        out["pass_ms_at_copy_rate_" + t] = round(nbytes / rate * 1e3, 4)
        out["bound_1p5x_ms_" + t] = round(1.5 * nbytes / rate * 1e3, 4)
        for k in on:
            b = out["B_%s_%s_ms" % (k, t)]
            out["B_%s_%s_minus_A_ms" % (k, t)] = round(b - out["A_ms" if t == "fp32" else "A_bf16_ms"], 4)
            out["C_%s_minus_B_%s_%s_ms" % (k, k, t)] = round(out["C_%s_ms" % k] - b, 4)
    for k in on:
        out["C_%s_minus_A_ms" % k] = round(out["C_%s_ms" % k] - out["A_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
