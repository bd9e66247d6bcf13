"""Cost of utterance weights and derivative weights at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, D = 3456), one
process, the legs alternating round by round so that drift of the box falls on all of them; each leg with an fp32 and a bf16
network output (<t>):

  A_<t>       the fused ChainLoss forward + backward step with no weights
  F_<t>       the same step with deriv_weights that are 1 except the first and last 10 frames of each utterance (0 there)
  U_<t>       the same step with utt_weights that are all != 1 (every live row is read, multiplied and written)
  R_<t>       the same step with ChainLoss(output_l2_regularize=l2) and no weights: the regularisers' ACCUM pass, which reads one
              [B,T,D] more than the utterance-weight pass - what U - A is set against
  H_<t>       what the library offered before: step A with a torch hook on x that multiplies the gradient by w[:, :, None]
  copy_<t>    a streaming copy (torch's copy_ of a buffer as large as the network output)

Prints one JSON line: medians, the per-round medians' spread (max - min) of every leg, F - A, U - A, R - A, H - A, the rows the
derivative-weight leg touches and their bytes, the bytes of the utterance-weight pass (2 * sizeof(x) * sum_b L_b * D) and
their time at the measured copy rate.

    python tools/time_weights.py [--reps N] [--rounds R] [--config C3]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainLoss, synthetic as syn  # noqa: E402

L2 = 5e-4
EDGE = 10


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
    xs = {"fp32": x32, "bf16": x32.to(torch.bfloat16)}
    Lc = L.cpu()
    f = torch.ones(B, T)
    for b, n in enumerate(Lc.tolist()):
        f[b, :EDGE] = 0.0
        f[b, max(n - EDGE, 0):n] = 0.0
    edge_rows = int(sum(min(n, 2 * EDGE) for n in Lc.tolist()))
    u = 0.5 + 0.01 * torch.arange(B, dtype=torch.float32)                    # all != 1
    f_dev, u_dev = f.to(dev), u.to(dev)
    w_dev = (u_dev[:, None] * torch.ones(B, T, device=dev))[:, :, None]     # the hook's multiplier
    crit = ChainLoss(w["den_graph"], 1e-5)
    crit_l2 = ChainLoss(w["den_graph"], 1e-5, output_l2_regularize=L2)

    def step(x, c=crit, **kw):
        def run():
            xx = x.detach().requires_grad_(True)
            c(xx, L, g, **kw).backward()
        return run

    def hook(x):
        wx = w_dev.to(x.dtype)

        def run():
            xx = x.detach().requires_grad_(True)
            xx.register_hook(lambda grad: grad * wx)
            crit(xx, L, g).backward()
        return run

    def copy(x):
        src, dst = torch.empty_like(x), torch.empty_like(x)
        return lambda: dst.copy_(src)

    legs = {}
    for t, x in xs.items():
        legs["A_" + t] = step(x)
        legs["F_" + t] = step(x, deriv_weights=f_dev)
        legs["U_" + t] = step(x, utt_weights=u_dev)
        legs["R_" + t] = step(x, crit_l2)
        legs["H_" + t] = hook(x)
        legs["copy_" + t] = copy(x)
    acc = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            v = times_ms(call, reps)
            acc[k] += v
            per_round[k].append(median(v))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "live_frames": int(Lc.sum()), "edge_rows": edge_rows,
           "reps": reps * rounds}
    out.update({k + "_ms": round(median(v), 4) for k, v in acc.items()})
    out.update({k + "_spread_ms": round(max(v) - min(v), 4) for k, v in per_round.items()})
    for t, size in (("fp32", 4), ("bf16", 2)):
        a = out["A_%s_ms" % t]
        for k in "FURH":
            out["%s_minus_A_%s_ms" % (k, t)] = round(out["%s_%s_ms" % (k, t)] - a, 4)
        out["U_minus_R_%s_ms" % t] = round(out["U_%s_ms" % t] - out["R_%s_ms" % t], 4)
        # (a copy reads and writes the buffer once: 2 * bytes of it per copy)
        rate = 2.0 * x32.numel() * size / (out["copy_%s_ms" % t] * 1e-3)
        out["copy_rate_TBps_" + t] = round(rate / 1e12, 3)
        out["U_pass_bytes_" + t] = 2 * size * int(Lc.sum()) * D
        out["U_pass_ms_at_copy_rate_" + t] = round(out["U_pass_bytes_" + t] / rate * 1e3, 4)
        out["F_pass_bytes_" + t] = size * edge_rows * D                       # zero rows: written, not read
        out["F_pass_ms_at_copy_rate_" + t] = round(out["F_pass_bytes_" + t] / rate * 1e3, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
