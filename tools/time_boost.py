"""Cost of the boosted objective at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, D = 3456), one process, the legs
alternating round by round so that drift of the box falls on all of them:

  P            the posterior-target step without boost, ChainLoss(x, lengths, targets) with K = 8 entries per frame (fp32)
  Bo_fp32/bf16 the boosted step, ChainLoss(boost=1)(x, lengths, targets), fp32 / bf16 network output
  C            the torch composition the boosted step replaces (fp32): x.scatter_add(2, pdfs, -boost * probs) on a dense copy,
               ChainFunction on the denominator, posterior_numerator, autograd adding the second dense gradient (this one boosts
               BEFORE the clamp)
  pass_fp32/bf16  native.boost_rows alone
  den_exp      the denominator call on rows that are already exp'd (input_is_exp), what the boosted step runs behind the pass
  den          the denominator call on x itself

Prints one JSON line of medians.

    python tools/time_boost.py [--reps N] [--rounds R] [--config C3] [--k K] [--boost b]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainFunction, ChainGraphBatch, ChainLoss, PosteriorTargets, _plan, native, posterior_numerator, synthetic as syn  # noqa: E402


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
    boost = float(arg("--boost", 1.0))
    dev = torch.device("cuda:0")
    w = syn.make_workload(config, device=dev)
    x32, L, den = w["x"], w["lengths"], w["den_graph"]
    B, T, D = x32.shape
    frames = float(L.sum())
    xs = {"fp32": x32, "bf16": x32.to(torch.bfloat16)}
    # the reference posteriors: a softmax of another output stands in for them (the cost does not depend on the values)
    post = torch.softmax(syn.make_input(B, T, D, seed=91).to(dev) * 1.5, dim=2)
    targets = PosteriorTargets.from_dense(post, L, K)
    del post
    plain, boosted = ChainLoss(den, 1e-5), ChainLoss(den, 1e-5, boost=boost)
    den_batch = ChainGraphBatch(den, B)
    live = (torch.arange(T, device=dev)[None, :] < L.to(dev)[:, None])[..., None]
    idx = targets.pdfs.clamp_min(0).to(torch.int64)
    minus = torch.where((targets.pdfs >= 0) & live, -boost * targets.probs, torch.zeros((), device=dev))
    plan = _plan.graph_plan(den, D, dev)
    e_rows = native.boost_rows(x32, L, targets.pdfs, targets.probs, boost, out=torch.ones(B, T, D, device=dev))[0]

    def leg_step(crit, x):
        def run():
            xx = x.detach().requires_grad_(True)
            crit(xx, L, targets).backward()
        return run

    def leg_c():
        xx = x32.detach().requires_grad_(True)
        d = ChainFunction.apply(xx.scatter_add(2, idx, minus), L, den_batch, 1e-5)
        ((d - posterior_numerator(xx, L, targets)) / frames).backward()

    def leg_pass(x):
        return lambda: native.boost_rows(x, L, targets.pdfs, targets.probs, boost)

    def leg_den_exp():
        native.den_forward_backward(plan, e_rows, L, 1e-5, input_is_exp=True, grad_scale=1.0 / frames, totals=True)

    def leg_den():
        native.den_forward_backward(plan, x32, L, 1e-5, grad_scale=1.0 / frames, totals=True)

    legs = {"P_ms": leg_step(plain, xs["fp32"]), "Bo_fp32_ms": leg_step(boosted, xs["fp32"]), "Bo_bf16_ms": leg_step(boosted, xs["bf16"]),
            "C_ms": leg_c, "pass_fp32_ms": leg_pass(xs["fp32"]), "pass_bf16_ms": leg_pass(xs["bf16"]), "den_exp_ms": leg_den_exp,
            "den_ms": leg_den}
    acc = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc[k] += t
            per_round[k].append(median(t))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "K": K, "boost": boost, "live_frames": int(L.sum()),
           "reps": reps * rounds}
    out.update({k: round(median(v), 4) for k, v in acc.items()})
    for k in ("Bo_fp32_ms", "C_ms"):
        out[k[:-3] + "_spread_ms"] = round(max(per_round[k]) - min(per_round[k]), 4)
    out["Bo_fp32_minus_P_ms"] = round(out["Bo_fp32_ms"] - out["P_ms"], 4)
    out["C_minus_Bo_fp32_ms"] = round(out["C_ms"] - out["Bo_fp32_ms"], 4)
    # the bytes the pass has to move: the live rows read in x's type and written in fp32
    for name, size in (("fp32", 4), ("bf16", 2)):
        nbytes = int(L.sum()) * D * (size + 4)
        out["pass_%s_bytes" % name] = nbytes
        out["pass_%s_TBps" % name] = round(nbytes / (out["pass_%s_ms" % name] * 1e-3) / 1e12, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
