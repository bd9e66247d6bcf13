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

The two kernels of rec_grad are told apart by a kernel trace of `--only rec_grad` (rocprofv3 --kernel-trace --stats, a run of
its own).  Prints one JSON line of medians.

    python tools/time_smbr.py [--reps N] [--rounds R] [--config C3] [--only LEG]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch  # noqa: E402
from pychain_amd import ChainLoss, PosteriorTargets, SMBRLoss, _lib, _plan, native, synthetic as syn, viterbi_align  # noqa: E402


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
    w = syn.make_workload(config, device=dev)
    x32, L, den, num = w["x"], w["lengths"], w["den_graph"], w["num_graphs"]
    B, T, D = x32.shape
    xbf = x32.to(torch.bfloat16)
    ref = PosteriorTargets.from_alignment(viterbi_align(x32, L, num))
    mmi, smbr = ChainLoss(den, 1e-5), SMBRLoss(den, 1e-5)
    classes = (40 * torch.arange(D, dtype=torch.int64) // D).to(torch.int32)
    smbr_cls = SMBRLoss(den, 1e-5, classes=classes)
    cls_dev, C = native.smbr_classes(classes, D, dev)
    plan = _plan.graph_plan(den, D, dev)
    gt = native.smbr_graph(den, D, dev)
    gamma = native.den_forward_backward(plan, x32, L, 1e-5)[1]
    lib = _lib.lib()
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

    legs = {"mmi_ms": leg_mmi, "smbr_ms": leg_smbr(x32), "den_ms": leg_den, "frame_acc_ms": leg_frame_acc,
            "acc_rec_grad_ms": leg_rec_grad, "smbr_bf16_ms": leg_smbr(xbf), "smbr_classes_ms": leg_smbr(x32, smbr_cls),
            "class_acc_ms": leg_class_acc}
    if only:
        legs = {only + "_ms": legs["acc_rec_grad_ms" if only == "rec_grad" else only + "_ms"]}
    acc_t = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            t = times_ms(call, reps)
            acc_t[k] += t
            per_round[k].append(median(t))
    out = {"config": config, "B": int(B), "T": int(T), "D": int(D), "H": int(den.num_states), "arcs": int(den.num_transitions),
           "live_frames": int(L.sum()), "reps": reps * rounds}
    out.update({k: round(median(v), 4) for k, v in acc_t.items()})
    out.update({k[:-3] + "_spread_ms": round(max(v) - min(v), 4) for k, v in per_round.items()})
    if not only:
        out["rec_grad_ms"] = round(out["acc_rec_grad_ms"] - out["frame_acc_ms"], 4)
        out["smbr_over_mmi"] = round(out["smbr_ms"] / out["mmi_ms"], 3)
        out["classes_over_smbr_ms"] = round(out["smbr_classes_ms"] - out["smbr_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
