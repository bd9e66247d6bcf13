"""What the library's policy queries answer over a fixed grid of shapes, launch hints and options:

    python tests/golden/make_den_decisions.py        # writes tests/golden/den_decisions.json

The query entry points are host arithmetic and need no device (256 CUs are assumed without one, which is what an MI355X
reports), so the file holds on both machines.  tests/test_api.py::test_den_decisions_match_the_recorded_grid recomputes
every row with the library under test and compares; the file is only regenerated when a policy changes ON PURPOSE.

The file holds "answers", the distinct answer strings - one base-36 digit per column of COLUMNS, kernel names as indices into
NAMES -, "rows", for every configuration of grid() in order the index of its answer string, and "workspace",
{"B,T,H,D": [min bytes, bytes]} for every size of the grid.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "den_decisions.json")

HINT_GENERAL = -(1 << 31)
NAMES = ["den_general_recursion_kernel", "den_general_gamma_kernel", "den_recursion_kernel", "den_recursion_pair_kernel",
         "den_recursion_lazy_kernel", "den_recursion_lazy_kernel<dma>", "den_recursion_lazy_kernel<small>",
         "den_recursion_lazy_kernel<dma; one gather per arc>", "den_recursion_lazy_kernel<dma; one gather per arc; crossing>",
         "den_recursion_lazy_kernel<dma; one-word states>", "den_gamma_kernel", "den_gamma2_kernel"]
CONFIG = ["hint", "H", "D", "B", "T", "option", "value"]
COLUMNS = ["rec_shared", "occ_shared", "rec_strided", "occ_strided",
           "rec_shared_fused", "occ_shared_fused", "rec_strided_fused", "occ_strided_fused",
           "tseg", "tseg_fused", "row_buffer", "row_buffer_exp_input", "den_half_native", "chain_loss_half_native",
           "chain_loss_slices"]
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"
NUM_H, NUM_K = 40, 120     # a numerator graph the tile kernels take (chain_loss_half_native asks about both sides)


def hint(rows, occ=32, occ2=32, bits=(30,)):
    h = rows | (occ << 10) | (occ2 << 20)
    for b in bits:
        h |= 1 << b
    return h


BASE = hint(32)
SG = hint(32, bits=(30, 27))
SMALL = hint(24, bits=(30, 29))
ONE_WORD = hint(32, bits=(30, 19))

HINTS = [hint(r) for r in (16, 24, 32, 40, 64, 200)] + [
    hint(32, bits=()), hint(32, bits=(30, 19)), hint(32, bits=(30, 27)), hint(32, bits=(30, 28)), hint(32, bits=(30, 29)),
    hint(32, bits=(29,)), hint(16, bits=(30, 27)), hint(40, bits=(30, 27)), hint(32, bits=(30, 27, 28)), hint(32, bits=(30, 19, 27)),
    hint(32, bits=(30, 19, 28)), hint(16, bits=(30, 19)), hint(24, bits=(30, 29)), hint(40, bits=(29,)),
    hint(32, occ=0), hint(32, occ=16), hint(32, occ=64), hint(32, occ=300), hint(32, occ=511),
    hint(32, occ2=0), hint(32, occ2=16), hint(32, occ2=64), hint(32, occ2=100), hint(32, occ=64, occ2=0),
    HINT_GENERAL]

# (H, D) on both sides of the limits in the shape predicates
SHAPES = [(H, 3456) for H in (200, 3000, 3072, 3073, 4032, 4033, 4096, 4097)] + \
         [(3000, D) for D in (3452, 3454, 4096, 4100, 9216, 9220, 10240, 10244)] + \
         [(200, 64), (200, 62), (500, 2000), (4096, 4096), (3072, 9216), (4033, 9216)]
BATCHES = [1, 2, 5, 16, 24, 32, 56, 64, 80, 100, 104, 128, 129, 224, 256]
LENGTHS = [40, 64, 150, 300, 383, 1500, 2000]
OPTIONS = [("den_lazy", 0), ("den_pair", 0), ("den_pair", 1), ("den_dma", 0), ("den_dma", 2), ("den_dma", 3),
           ("den_tseg", 0), ("den_tseg", 2), ("den_tseg", 4), ("den_tburn", 0), ("den_tburn", 64), ("den_sg", 0),
           ("den_q", 1), ("den_cross", 1), ("gamma16", 1), ("verbose", 1), ("chain_slices", 0), ("chain_slices", 3)]


def grid():
    """The configurations [hint, H, D, B, T, option, value] ("" / 0: no option set), in file order."""
    out = []
    for h in HINTS:                                   # every hint on every shape
        for (H, D) in SHAPES:
            for B in (2, 128):
                out.append([h, H, D, B, 300, "", 0])
    for h in (BASE, SG, SMALL):                       # every batch size and length
        for (H, D) in ((3000, 3456), (3000, 9216), (200, 64)):
            for B in BATCHES:
                for T in LENGTHS:
                    out.append([h, H, D, B, T, "", 0])
    for (name, value) in OPTIONS:                     # every option that feeds a decision, one at a time
        for h in (BASE, SG, SMALL, ONE_WORD):
            for (H, D) in ((3000, 3456), (3000, 9216), (200, 64)):
                for B in (16, 64, 256):
                    for T in (64, 1500):
                        out.append([h, H, D, B, T, name, value])
    return out


def answers(L, cfg):
    """What library `L` (pychain_amd._lib.lib()) answers for one configuration, as a string of digits; the caller has set the option."""
    h, H, D, B, T = cfg[:5]
    buf = ctypes.create_string_buffer(128)
    row = []
    for shared_fused in (1, 0, 3, 2):                # bit 0: one plan for all sequences; bit 1: part of a fused loss
        rc = L.pychain_hip_den_kernel_names(h, H, D, B, shared_fused, buf, 128)
        assert rc == 0, rc
        rec, occ = buf.value.decode().split(",")
        row += [NAMES.index(rec), NAMES.index(occ)]
    row += [L.pychain_hip_den_time_segments(0, h, H, D, B, T, 0), L.pychain_hip_den_time_segments(0, h, H, D, B, T, 1),
            L.pychain_hip_den_uses_row_buffer(0, h, H, D, B, T, 0), L.pychain_hip_den_uses_row_buffer(0, h, H, D, B, T, 1),
            L.pychain_hip_den_half_native(0, h, H, D, B, T),
            L.pychain_hip_chain_loss_half_native(0, h, H, D, B, T, NUM_H, NUM_K),
            L.pychain_hip_chain_loss_slices(0, h, B)]
    return "".join(DIGITS[v] for v in row)


def compute(_lib):
    """{"rows": [answer string per configuration of grid()], "workspace": {...}}; `_lib`: pychain_amd._lib of the tree under test."""
    L = _lib.lib()
    rows, ws = [], {}
    for cfg in grid():
        if cfg[5]:
            with _lib.option(cfg[5], cfg[6]):
                rows.append(answers(L, cfg))
        else:
            rows.append(answers(L, cfg))
        h, H, D, B, T = cfg[:5]
        ws["%d,%d,%d,%d" % (B, T, H, D)] = [L.pychain_hip_den_workspace_min_bytes(B, T, H, D), L.pychain_hip_den_workspace_bytes(B, T, H, D)]
    return {"rows": rows, "workspace": ws}


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    from pychain_amd import _lib
    got = compute(_lib)
    distinct = sorted(set(got["rows"]))
    a, w = [distinct.index(r) for r in got["rows"]], sorted(got["workspace"].items())
    with open(OUT, "w") as f:
        f.write('{"columns": %s,\n "names": %s,\n "answers": %s,\n "rows": [\n' % (json.dumps(COLUMNS), json.dumps(NAMES), json.dumps(distinct)))
        f.write(",\n".join(",".join(str(r) for r in a[i:i + 100]) for i in range(0, len(a), 100)))
        f.write('\n],\n "workspace": {\n')
        f.write(",\n".join(",".join('"%s":[%d,%d]' % (k, v[0], v[1]) for k, v in w[i:i + 20]) for i in range(0, len(w), 20)))
        f.write("\n}}\n")
    print("%d rows, %d sizes -> %s (%d bytes)" % (len(a), len(w), OUT, os.path.getsize(OUT)))
