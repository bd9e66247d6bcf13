"""Cost of the numerator's expected arc counts at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, D = 3456, one left-to-right
numerator graph per utterance), beside the numerator calls of the same build, one process, the legs alternating
round by round so that drift of the box falls on all of them:

  chain_num      ChainFunction on the numerator batch: what a training step pays for the numerator alone
  num            the numerator call alone (native.num_forward_backward, LINEAR gradient)
  counts         pychain_hip_num_arc_counts with grad = NULL: the recursions, the count launch, the reduction
  counts_grad    ... with the gradient: the occupancy launch too
  counts_w       ... with the gradient and weights w = 0.1 N(0,1): the weight launch in front
  counts_gather  counts under option num_arcs_gather: the gathered form of the count kernel

The count launch alone is counts_ms - (num_ms - the occupancy launch); a kernel trace of `--only counts` (rocprofv3 --kernel-trace
--stats, a run of its own) tells the kernels apart.  Prints one JSON line of medians, the spread of the per-round medians beside
each, and the workspace bytes of the call and of the plain numerator.

    python tools/time_num_arcs.py [--reps N] [--rounds R] [--config C3] [--only LEG]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainFunction, _lib, native, synthetic as syn  # noqa: E402


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
    reps, rounds, config, only = int(arg("--reps", 5)), int(arg("--rounds", 3)), arg("--config", "C3"), arg("--only", None)
    dev = torch.device("cuda:0")
    wl = syn.make_workload(config, device=dev)
    x, L, num = wl["x"], wl["lengths"], wl["num_graphs"]
    B, T, D = x.shape
    gt = num.device_tensors(dev)
    stride = 0 if num.shared_graph is not None else 1
    H, K = int(num.num_states), int(gt["forward_transitions"].shape[1])
    lib = _lib.lib()
    w = (0.1 * torch.randn(B, K, generator=torch.Generator().manual_seed(1))).to(dev)

    def gathered():
        with _lib.option("num_arcs_gather", 1):
            return native.num_arc_counts(gt, stride, H, x, L)
    legs = {
        "chain_num_ms": lambda: ChainFunction.apply(x, L, num, 1e-5),
        "num_ms": lambda: native.num_forward_backward(gt, stride, H, x, L),
        "counts_ms": lambda: native.num_arc_counts(gt, stride, H, x, L),
        "counts_grad_ms": lambda: native.num_arc_counts(gt, stride, H, x, L, with_grad=True),
        "counts_w_ms": lambda: native.num_arc_counts(gt, stride, H, x, L, w, with_grad=True),
        "counts_gather_ms": gathered,
    }
    if only:
        legs = {only + "_ms": legs[only + "_ms"]}
    acc_t = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc_t[k] += t
            per_round[k].append(median(t))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "H": H, "arcs": K, "live_frames": int(L.sum()), "reps": reps * rounds,
           "workspace_bytes": int(lib.pychain_hip_num_arc_counts_workspace_bytes(B, T, H, K, D)),
           "num_workspace_bytes": int(lib.pychain_hip_num_workspace_bytes(B, T, H, K, D))}
    out.update({k: round(median(v), 4) for k, v in acc_t.items()})
    out.update({k[:-3] + "_spread_ms": round(max(v) - min(v), 4) for k, v in per_round.items()})
    if "counts_grad_ms" in out and "num_ms" in out:
        out["counts_grad_over_num"] = round(out["counts_grad_ms"] / out["num_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
