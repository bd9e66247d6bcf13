"""Cost of lattice-free sMBR at C3 (synthetic.make_workload("C3"): B = 64, T <= 1500, D = 3456; the reference is the Viterbi
alignment of the numerator graphs), beside the fused LF-MMI step, one process, the legs alternating round by round so that drift
of the box falls on all of them:

  mmi          the fused LF-MMI step, ChainLoss(x, lengths, num_graphs) forward and backward (fp32)
  smbr         the sMBR step, SMBRLoss(x, lengths, ref) forward and backward (fp32): everything below and the autograd glue
  den          stage 1: the ordinary denominator call that yields the occupancies
  frame_acc    pychain_hip_smbr_frame_accuracy (smbr_frame_acc_kernel)
  rec_grad     pychain_hip_smbr_forward_backward: smbr_recursion_kernel, then smbr_grad_kernel
  smbr_bf16    the sMBR step on a bf16 network output
  smbr_classes the sMBR step with the accuracy by class: a synthetic map of 40 classes, cls[n] = 40 n // D -
               beside `smbr` it costs the dense accuracy pass over gamma and the class tables of the two stage-2 kernels
  class_acc    pychain_hip_smbr_frame_accuracy_classes alone (smbr_class_frame_acc_kernel, smbr_class_seq_acc_kernel)
  smbr_rows    the sMBR step on the general kernels, kernels="rows": the frame's rows in workspace scratch
  smbr_global  ... kernels="global": the state vectors too read back from the trajectories
  smbr_auto    the sMBR step under kernels="auto" - what a tree beyond the LDS of a CU runs (C4: the rows form)
  rec_grad_auto   pychain_hip_smbr_forward_backward_general under PYCHAIN_HIP_SMBR_AUTO, the accuracy pass in front of it

`smbr` is kernels="lds"; the ratios rows_over_lds and global_over_lds are what each tier costs on a shape all three take.  A
configuration without numerator graphs (C4) has no alignment: its reference is the best pdf of the denominator's occupancies per
frame, its legs are smbr_auto, den, frame_acc and rec_grad_auto (the LDS kernels refuse C4).  The line also carries the workspace
bytes of the LDS form and of the general forms, and the form `auto` resolves to.

The two kernels of rec_grad are told apart by a kernel trace of `--only rec_grad` (rocprofv3 --kernel-trace --stats, a run of
its own); those of the general forms by one of `--only rec_grad_auto`.  Prints one JSON line of medians.

    python tools/time_smbr.py [--reps N] [--rounds R] [--config C3] [--only LEG] [--legs LEG,LEG,...]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainLoss, PosteriorTargets, SMBRLoss, _lib, _plan, native, synthetic as syn, viterbi_align  # noqa: E402
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
    chosen = arg("--legs", None)
    dev = torch.device("cuda:0")
    w = syn.make_workload(config, device=dev)
    x32, L, den, num = w["x"], w["lengths"], w["den_graph"], w["num_graphs"]
    B, T, D = x32.shape
    xbf = x32.to(torch.bfloat16) if num is not None else None
    lib = _lib.lib()
    H = int(den.num_states)
    fits_lds = lib.pychain_hip_smbr_form(H, D, 0, _lib.SMBR_AUTO) == _lib.SMBR_LDS
    if num is not None:
        ref = PosteriorTargets.from_alignment(viterbi_align(x32, L, num))
    else:
        ref = posterior_targets(x32, L, den, 1, 1e-5)
    mmi, smbr = ChainLoss(den, 1e-5), SMBRLoss(den, 1e-5)
    classes = (40 * torch.arange(D, dtype=torch.int64) // D).to(torch.int32)
    smbr_cls = SMBRLoss(den, 1e-5, classes=classes)
    cls_dev, C = native.smbr_classes(classes, D, dev)
    plan = _plan.graph_plan(den, D, dev)
    gt = native.smbr_graph(den, D, dev)
    gamma = native.den_forward_backward(plan, x32, L, 1e-5)[1]
    ld = L.to(dev)
    facc = torch.empty(B, T, device=dev)
    acc = torch.empty(B, dtype=torch.float64, device=dev)
    bad = torch.empty(2, dtype=torch.int32, device=dev)

    def leg_mmi():
        xx = x32.detach().requires_grad_(True)
        mmi(xx, L, num).backward()

    def leg_smbr(x, loss=smbr):
        def run():
            xx = x.detach().requires_grad_(True)
            loss(xx, L, ref).backward()
        return run

    def leg_den():
        native.den_forward_backward(plan, x32, L, 1e-5)

    def leg_frame_acc():
        _lib.check(lib.pychain_hip_smbr_frame_accuracy(gamma.data_ptr(), ld.data_ptr(), B, T, D, ref.pdfs.data_ptr(), ref.probs.data_ptr(),
                                                       1, facc.data_ptr(), acc.data_ptr(), bad.data_ptr(),
                                                       torch.cuda.current_stream(dev).cuda_stream), "smbr_frame_accuracy")

    ws = torch.empty(lib.pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(B, T), dtype=torch.uint8, device=dev)

    def leg_class_acc():
        _lib.check(lib.pychain_hip_smbr_frame_accuracy_classes(gamma.data_ptr(), ld.data_ptr(), B, T, D, ref.pdfs.data_ptr(), ref.probs.data_ptr(),
                                                               1, facc.data_ptr(), acc.data_ptr(), bad.data_ptr(),
                                                               torch.cuda.current_stream(dev).cuda_stream, cls_dev.data_ptr(), C, 0,
                                                               ws.data_ptr(), ws.numel()), "smbr_frame_accuracy_classes")

    def leg_rec_grad():
        native.smbr(gt, den.num_states, x32, L, gamma, ref.pdfs, ref.probs, 1e-5)      # (the accuracy pass is in it: subtracted below)

    def leg_rec_grad_auto():
        native.smbr(gt, den.num_states, x32, L, gamma, ref.pdfs, ref.probs, 1e-5, form="auto")

    general = {"smbr_rows_ms": leg_smbr(x32, SMBRLoss(den, 1e-5, kernels="rows")),
               "smbr_global_ms": leg_smbr(x32, SMBRLoss(den, 1e-5, kernels="global")),
               "smbr_auto_ms": leg_smbr(x32, SMBRLoss(den, 1e-5, kernels="auto")), "acc_rec_grad_auto_ms": leg_rec_grad_auto}
    if num is not None and fits_lds:
        legs = {"mmi_ms": leg_mmi, "smbr_ms": leg_smbr(x32), "den_ms": leg_den, "frame_acc_ms": leg_frame_acc,
                "acc_rec_grad_ms": leg_rec_grad, "smbr_bf16_ms": leg_smbr(xbf), "smbr_classes_ms": leg_smbr(x32, smbr_cls),
                "class_acc_ms": leg_class_acc}
        legs.update(general)
    else:
        legs = {"smbr_auto_ms": general["smbr_auto_ms"], "den_ms": leg_den, "frame_acc_ms": leg_frame_acc,
                "acc_rec_grad_auto_ms": general["acc_rec_grad_auto_ms"]}
    long_name = lambda k: "acc_" + k + "_ms" if k in ("rec_grad", "rec_grad_auto") else k + "_ms"
    if only:
        legs = {only + "_ms": legs[long_name(only)]}
    elif chosen:
        legs = {long_name(k): legs[long_name(k)] for k in chosen.split(",")}
    acc_t = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc_t[k] += t
            per_round[k].append(median(t))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "H": int(den.num_states), "arcs": int(den.num_transitions),
           "live_frames": int(L.sum()), "reps": reps * rounds,
           "auto_form": {v: k for k, v in native.SMBR_FORMS.items()}[lib.pychain_hip_smbr_form(H, D, 0, _lib.SMBR_AUTO)],
           "workspace_lds_bytes": int(lib.pychain_hip_smbr_workspace_bytes(B, T, H)),
           "workspace_general_bytes": int(lib.pychain_hip_smbr_general_workspace_bytes(B, T, H, D, 0))}
    out.update({k: round(median(v), 4) for k, v in acc_t.items()})
    out.update({k[:-3] + "_spread_ms": round(max(v) - min(v), 4) for k, v in per_round.items()})
    has = lambda *ks: all(k in out for k in ks)
    if has("acc_rec_grad_ms", "frame_acc_ms"):
        out["rec_grad_ms"] = round(out["acc_rec_grad_ms"] - out["frame_acc_ms"], 4)
    if has("acc_rec_grad_auto_ms", "frame_acc_ms"):
        out["rec_grad_auto_ms"] = round(out["acc_rec_grad_auto_ms"] - out["frame_acc_ms"], 4)
    if has("smbr_ms", "mmi_ms"):
        out["smbr_over_mmi"] = round(out["smbr_ms"] / out["mmi_ms"], 3)
    if has("smbr_classes_ms", "smbr_ms"):
        out["classes_over_smbr_ms"] = round(out["smbr_classes_ms"] - out["smbr_ms"], 4)
    for k in ("rows", "global", "auto"):
        if has("smbr_%s_ms" % k, "smbr_ms"):
            out["%s_over_lds" % k] = round(out["smbr_%s_ms" % k] / out["smbr_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
