"""Calls of the denominator alone that are cut into time segments (few sequences): ms per call by device
events (median / min / p90 of 40), automatic settings, the plan's burn-in controller attached as in production, and what the
call reports (segments, rows missed, worst splice mismatch, the burn-in in effect).  To compare two builds, point PYCHAIN_HIP_LIB
at each library in alternating legs of one session (profiles/peaky_splice.md).
usage (on the MI355X): [PYCHAIN_HIP_LIB=other.so] python tools/time_cut_calls.py <tag>    # prints one JSON line per shape"""
import os, sys, json
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch
from pychain_amd import _lib, _plan, native, synthetic as syn
dev = torch.device("cuda:0")
tag = sys.argv[1] if len(sys.argv) > 1 else "this"
for name, B, T, mode in (("C3", 4, 1500, "ragged"), ("C3", 16, 1500, "ragged"), ("C3", 32, 1500, "ragged"), ("C4", 32, 2000, "equal"), ("C3", 64, 1500, "ragged")):
    cfg = syn.CONFIGS[name]
    den = syn.make_den_graph(cfg["H"], cfg["K"], cfg["D"], seed=0)
    plan = _plan.graph_plan(den, cfg["D"], dev)
    L = syn.make_lengths(B, T, mode, seed=3).to(dev)
    x = syn.make_input(B, T, cfg["D"], seed=9, device=dev)
    call = lambda: native.den_forward_backward(plan, x, L, 1e-5, totals=True)
    for _ in range(4):
        out = call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(40)]
    for a, b in ev:
        a.record(); out = call(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    t = out[3]
    st = plan.tseg_state
    row = dict(lib=tag, shape=name, B=B, T=T, median_ms=round(ts[20], 4), min_ms=round(ts[0], 4), p90_ms=round(ts[36], 4), segments=int(t[6]), missed=int(t[5]),
               worst=float(t[7]), burn_in=int(st[1]) if st is not None else None, calls_missed=int(st[4]) if st is not None else None)
    print(json.dumps(row), flush=True)
    native.release_workspaces(); torch.cuda.empty_cache()
