"""Cost of the expected arc counts at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, H = 3000, K = 30000, D = 3456; DESIGN.md
§3.29), beside the two calls of the same build it shares its shape with, one process, the legs alternating round by round so
that drift of the box falls on all of them:

  counts       pychain_hip_den_arc_counts without a gradient (grad NULL), w = 0.1 N(0,1)
  counts_grad  ... with the gradient of the network output
  counts_bf16  ... with the gradient, on a bf16 network output
  counts_grad_rows    counts_grad on the general kernels, form "rows": the frame's rows in workspace scratch
  counts_grad_global  ... form "global": the state vectors too read back from the trajectories
  beyond_auto  counts_grad under form "auto" on a shape beyond the LDS form: the same graph size on a tree of 17 500 pdfs
               (B = 16, T = 500, every sequence whole), which runs the rows form
  den          the ordinary denominator call (the plan kernels): objective and occupancies
  smbr_rec     stage 2 of sMBR with its accuracy pass (pychain_hip_smbr_frame_accuracy, then pychain_hip_smbr_forward_backward):
               the recursion these kernels were cut from, with its weighted pair

`counts_grad` is form "lds"; the ratios rows_over_lds and global_over_lds are what each tier costs on a shape all three take.
The five kernels of a call are told apart by a kernel trace of `--only counts_grad` (rocprofv3 --kernel-trace --stats, a run of
its own), those of a general form by one of `--only counts_grad_rows`.  Prints one JSON line of medians, the spread of the
per-round medians beside each, the workspace bytes of the LDS form and of the general forms, and the form "auto" resolves to.

    python tools/time_arcs.py [--reps N] [--rounds R] [--config C3] [--only LEG]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import _lib, _plan, native, synthetic as syn  # noqa: E402
from pychain_amd.loss import posterior_targets  # noqa: E402


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
    x32, L, den = wl["x"], wl["lengths"], wl["den_graph"]
    B, T, D = x32.shape
    xbf = x32.to(torch.bfloat16)
    H, K = int(den.num_states), int(den.num_transitions)
    lib = _lib.lib()
    gt = native.smbr_graph(den, D, dev)
    plan = _plan.graph_plan(den, D, dev)
    w = (0.1 * torch.randn(K, generator=torch.Generator().manual_seed(1))).to(dev)
    gamma = native.den_forward_backward(plan, x32, L, 1e-5)[1]
    ref = posterior_targets(x32, L, den, 1, 1e-5)
    legs = {
        "counts_ms": lambda: native.den_arc_counts(gt, H, x32, L, 1e-5, w, with_grad=False),
        "counts_grad_ms": lambda: native.den_arc_counts(gt, H, x32, L, 1e-5, w),
        "counts_bf16_ms": lambda: native.den_arc_counts(gt, H, xbf, L, 1e-5, w),
        "counts_grad_rows_ms": lambda: native.den_arc_counts(gt, H, x32, L, 1e-5, w, form="rows"),
        "counts_grad_global_ms": lambda: native.den_arc_counts(gt, H, x32, L, 1e-5, w, form="global"),
        "den_ms": lambda: native.den_forward_backward(plan, x32, L, 1e-5),
        "smbr_rec_ms": lambda: native.smbr(gt, H, x32, L, gamma, ref.pdfs, ref.probs, 1e-5),
    }
    # a tree beyond the LDS form on a graph of the same size
    Bw, Tw, Dw = 16, 500, 17500
    if not only or only == "beyond_auto":
        wide = syn.make_den_graph(H, K, Dw, seed=3)
        gtw = native.smbr_graph(wide, Dw, dev)
        xw, Lw = syn.make_input(Bw, Tw, Dw, seed=5, device=dev), torch.full((Bw,), Tw, dtype=torch.int64)
        legs["beyond_auto_ms"] = lambda: native.den_arc_counts(gtw, H, xw, Lw, 1e-5, w, form="auto")
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
           "workspace_bytes": int(lib.pychain_hip_den_arc_counts_workspace_bytes(B, T, H, K)),
           "lds_bytes": int(lib.pychain_hip_den_arc_counts_lds_bytes(H, D)),
           "general_workspace_bytes": int(lib.pychain_hip_den_arc_counts_general_workspace_bytes(B, T, H, K, D)),
           "general_lds_bytes": int(lib.pychain_hip_den_arc_counts_general_lds_bytes(H)),
           "beyond": {"B": Bw, "T": Tw, "D": Dw, "lds_bytes": int(lib.pychain_hip_den_arc_counts_lds_bytes(H, Dw)),
                      "auto_form": {v: k for k, v in native.SMBR_FORMS.items()}[lib.pychain_hip_den_arc_counts_form(H, Dw, _lib.SMBR_AUTO)]}}
    out.update({k: round(median(v), 4) for k, v in acc_t.items()})
    out.update({k[:-3] + "_spread_ms": round(max(v) - min(v), 4) for k, v in per_round.items()})
    if "counts_grad_ms" in out and "den_ms" in out:
        out["counts_grad_over_den"] = round(out["counts_grad_ms"] / out["den_ms"], 3)
    for k in ("rows", "global"):
        if "counts_grad_%s_ms" % k in out and "counts_grad_ms" in out:
            out["%s_over_lds" % k] = round(out["counts_grad_%s_ms" % k] / out["counts_grad_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
