"""Cost of posterior-target supervision at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, D = 3456), one process, the legs
alternating round by round so that drift of the box falls on all of them:

  A            the fused ChainLoss forward + backward step with graph numerators, for context (fp32)
  P_fp32/bf16  the posterior-target step, ChainLoss(x, lengths, targets) with K = 8 entries per frame, fp32 / bf16 network output
  C            the torch composition that step replaces (fp32): ChainFunction on the denominator, torch.gather of the targets'
               elements, multiply, mask, sum, autograd adding the second dense gradient
  den          the denominator call alone (native.den_forward_backward): what P cannot go below
  topk_hip     PosteriorTargets.from_dense on dense posteriors [64,1500,3456] (fp32), k = 8
  topk_torch   torch.topk(k = 8) on the same rows, then the division by the sum (no lengths, no floor, no tie rule)

Prints one JSON line of medians.

    python tools/time_post.py [--reps N] [--rounds R] [--config C3] [--k K]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainFunction, ChainGraphBatch, ChainLoss, PosteriorTargets, _plan, native, synthetic as syn  # noqa: E402


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
    reps, rounds, config, K = int(arg("--reps", 7)), int(arg("--rounds", 4)), arg("--config", "C3"), int(arg("--k", 8))
    dev = torch.device("cuda:0")
    w = syn.make_workload(config, device=dev)
    g, x32, L, den = w["num_graphs"], w["x"], w["lengths"], w["den_graph"]
    B, T, D = x32.shape
    frames = float(L.sum())
    xs = {"fp32": x32, "bf16": x32.to(torch.bfloat16)}
    # the teacher's posteriors: a softmax of another output stands in for them (the cost does not depend on the values)
    post = torch.softmax(syn.make_input(B, T, D, seed=91).to(dev) * 1.5, dim=2)
    targets = PosteriorTargets.from_dense(post, L, K)
    crit = ChainLoss(den, 1e-5)
    den_batch = ChainGraphBatch(den, B)
    live = (torch.arange(T, device=dev)[None, :] < L.to(dev)[:, None])[..., None]
    ok = (targets.pdfs >= 0) & live
    idx = targets.pdfs.clamp_min(0).to(torch.int64)
    q = torch.where(ok, targets.probs, torch.zeros((), device=dev))
    plan = _plan.graph_plan(den, D, dev)

    def leg_a():
        xx = x32.detach().requires_grad_(True)
        crit(xx, L, g).backward()

    def leg_p(x):
        def run():
            xx = x.detach().requires_grad_(True)
            crit(xx, L, targets).backward()
        return run

    def leg_c():
        xx = x32.detach().requires_grad_(True)
        d = ChainFunction.apply(xx, L, den_batch, 1e-5)
        num = (torch.gather(xx.clamp(-30.0, 30.0), 2, idx) * q).sum()
        ((d - num) / frames).backward()

    def leg_den():
        native.den_forward_backward(plan, x32, L, 1e-5, grad_scale=1.0 / frames, totals=True)

    def leg_topk_hip():
        PosteriorTargets.from_dense(post, L, K)

    def leg_topk_torch():
        v, _ = torch.topk(post, K, dim=2)
        v / v.sum(dim=2, keepdim=True)

    legs = {"A_ms": leg_a, "P_fp32_ms": leg_p(xs["fp32"]), "P_bf16_ms": leg_p(xs["bf16"]), "C_ms": leg_c, "den_ms": leg_den,
            "topk_hip_ms": leg_topk_hip, "topk_torch_ms": leg_topk_torch}
    acc = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc[k] += t
            per_round[k].append(median(t))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "K": K, "live_frames": int(L.sum()), "reps": reps * rounds}
    out.update({k: round(median(v), 4) for k, v in acc.items()})
    out["P_fp32_spread_ms"] = round(max(per_round["P_fp32_ms"]) - min(per_round["P_fp32_ms"]), 4)
    out["P_fp32_minus_den_ms"] = round(out["P_fp32_ms"] - out["den_ms"], 4)
    out["C_minus_P_fp32_ms"] = round(out["C_ms"] - out["P_fp32_ms"], 4)
    out["topk_row_bytes"] = int(post.numel() * 4)
    out["topk_hip_TBps"] = round(post.numel() * 4 / (out["topk_hip_ms"] * 1e-3) / 1e12, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
