"""Cost of the xent term against posterior targets at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, D = 3456, K = 8), one
process, the legs alternating round by round so that drift of the box falls on all of them:

  A          the posterior-target step without the term: ChainLoss(x, lengths, targets), forward + backward (fp32 x)
  B_<z>      with the term, the pass on the caller's stream behind post_targets; z in fp32 / bf16
  D_<z>      A plus the torch composition the term replaces: log_softmax of z, gather of the entries, product, sum, backward
  pass_<z>   native.xent_targets alone, with the store

Prints one JSON line of medians, the bytes the pass has to move - sum_b L_b D (sizeof z + sizeof dz) - and the rate reached.

    python tools/time_xent_targets.py [--reps N] [--rounds R] [--config C3] [--k K]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainLoss, PosteriorTargets, native, synthetic as syn  # noqa: E402


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
    x, L, den = w["x"], w["lengths"], w["den_graph"]
    B, T, D = x.shape
    frames = float(L.sum())
    post = torch.softmax(syn.make_input(B, T, D, seed=91).to(dev) * 1.5, dim=2)
    targets = PosteriorTargets.from_dense(post, L, K)
    del post
    z32 = syn.make_input(B, T, D, seed=93).to(dev) * 1.5
    zs = {"fp32": z32, "bf16": z32.to(torch.bfloat16)}
    plain, crit = ChainLoss(den, 1e-5), ChainLoss(den, 1e-5, xent_regularize=0.1)
    live = (torch.arange(T, device=dev)[None, :] < L.to(dev)[:, None])[..., None]
    ok = (targets.pdfs >= 0) & live
    idx = targets.pdfs.clamp_min(0).to(torch.int64)
    q = torch.where(ok, targets.probs, torch.zeros((), device=dev))

    def leg_a():
        xx = x.detach().requires_grad_(True)
        plain(xx, L, targets).backward()

    def leg_term(z):
        def run():
            xx, zz = x.detach().requires_grad_(True), z.detach().requires_grad_(True)
            crit(xx, L, targets, xent_output=zz, xent_targets=targets).backward()
        return run

    def leg_d(z):
        def run():
            xx, zz = x.detach().requires_grad_(True), z.detach().requires_grad_(True)
            xent = (torch.gather(torch.log_softmax(zz, dim=2), 2, idx) * q.to(zz.dtype)).sum()
            (plain(xx, L, targets) - 0.1 * xent / frames).backward()
        return run

    def leg_pass(z):
        return lambda: native.xent_targets(z, L, targets.pdfs, targets.probs, grad_scale=-0.1 / frames)

    legs = {"A_ms": leg_a}
    for name, z in zs.items():
        legs["B_%s_ms" % name] = leg_term(z)
        legs["D_%s_ms" % name] = leg_d(z)
        legs["pass_%s_ms" % name] = leg_pass(z)
    acc = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc[k] += t
            per_round[k].append(median(t))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "K": K, "live_frames": int(L.sum()), "reps": reps * rounds}
    out.update({k: round(median(v), 4) for k, v in acc.items()})
    out["A_spread_ms"] = round(max(per_round["A_ms"]) - min(per_round["A_ms"]), 4)
    for name, esz in (("fp32", 4), ("bf16", 2)):
        out["B_minus_A_%s_ms" % name] = round(out["B_%s_ms" % name] - out["A_ms"], 4)
        out["D_minus_A_%s_ms" % name] = round(out["D_%s_ms" % name] - out["A_ms"], 4)
        nbytes = int(L.sum()) * D * 2 * esz
        out["pass_%s_bytes" % name] = nbytes
        out["pass_%s_TBps" % name] = round(nbytes / (out["pass_%s_ms" % name] * 1e-3) / 1e12, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
