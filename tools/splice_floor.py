"""The fp32 floor of the splice check's metric (den_kernels.hip: den_splice_check_kernel): totals[7] - the worst
per-state mismatch of a speculated row - on the shapes of tests/test_gpu_tseg.py::test_segmented_recursions_agree_with_the_chain,
cut in 2 and 4 at pinned burn-ins.  The check's bound has to sit above what two fp32 recursions from different starts attain.
usage (on the MI355X): python tools/splice_floor.py    # prints one JSON line per call"""
import os, sys, json
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import torch
from helpers import rel_err
from pychain_amd import _lib, _plan, native, synthetic as syn
DEV = "cuda:0"
for name, B, T, lens in [("C3", 3, 1300, [1300, 1111, 400]), ("C3", 5, 1024, [1024, 1023, 777, 515, 512]), ("C4", 2, 1100, [1100, 901])]:
    cfg = syn.CONFIGS[name]
    den = syn.make_den_graph(cfg["H"], cfg["K"], cfg["D"], seed=0)
    plan = _plan.graph_plan(den, cfg["D"], torch.device(DEV))
    L = torch.tensor(lens)
    x = syn.make_input(B, T, cfg["D"], seed=21, device=DEV)
    with _lib.option("den_tseg", 0):
        o0, g0, b0, t0 = native.den_forward_backward(plan, x, L, 1e-5, totals=True)
    torch.cuda.synchronize()
    for S in (2, 4):
        for burn in (128, 192, 256, 384):
            if T < 2 * burn:
                continue
            with _lib.option("den_tseg", S), _lib.option("den_tburn", burn):
                o, g, b, t = native.den_forward_backward(plan, x, L, 1e-5, totals=True)
            torch.cuda.synchronize()
            row = dict(shape=name, B=B, T=T, S=S, burn=burn, missed=int(t[5]), segs=int(t[6]), worst=float(t[7]), bad=int(b),
                       grad_vs_uncut=rel_err(g.cpu().numpy(), g0.cpu().numpy()), objf_vs_uncut=float((o - o0).abs().max()) / float(o0.abs().max()))
            print(json.dumps(row), flush=True)
