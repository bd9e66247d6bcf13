"""Is the device code of two trees the same?  Compiles translation units of both to gfx950 assembly (build_ext.FLAGS plus
--cuda-device-only -S; cross-compiles, no GPU) and compares the listings:

    python tools/device_asm_diff.py PARENT_TREE THIS_TREE [file.hip ...]      (default: the row-pass files and api.hip)

Per file `identical` or `differs` (lines with the per-compilation `__hip_cuid_` symbol dropped).  For a file that differs,
per kernel: whether its descriptor (.amdhsa_*: registers, scratch, LDS) and its metadata entry (segment sizes, spill counts)
are equal, and the per-mnemonic instruction count delta.  It only compares two listings; the output is markdown."""
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pychain_amd.build_ext import FLAGS, _hipcc  # noqa: E402

DEFAULT = ["outreg.hip", "weights.hip", "post.hip", "xent.hip", "boost.hip", "api.hip"]
FIGURES = [".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_accum_offset", ".amdhsa_private_segment_fixed_size",
           ".amdhsa_group_segment_fixed_size", ".amdhsa_enable_private_segment", ".private_segment_fixed_size",
           ".group_segment_fixed_size", ".sgpr_count", ".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
           ".uses_dynamic_stack"]


def listing(tree, name, out):
    src = os.path.join(tree, "pychain_amd", "csrc", name)
    cmd = [_hipcc()] + FLAGS + ["-I", os.path.join(tree, "include"), "--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd, cwd=os.path.join(tree, "pychain_amd", "csrc"))
    with open(out) as f:
        return [l.rstrip("\n") for l in f if "__hip_cuid_" not in l]


def kernels(lines):
    """{symbol: {"code": Counter of mnemonics, "seq": [instructions], "desc": [...], "meta": [...]}}"""
    out = collections.OrderedDict()
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", l)] if m]
    for n in names:
        out[n] = {"code": collections.Counter(), "seq": [], "desc": [], "meta": []}
    cur = None
    for l in lines:                                   # function bodies: `sym:` .. `.Lfunc_end`
        s = l.split(";")[0].strip()
        if s.endswith(":") and s[:-1] in out:
            cur = out[s[:-1]]
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and s and not s.startswith(".") and not s.endswith(":"):
            cur["code"][s.split()[0]] += 1
            cur["seq"].append(s)
    cur = None
    for l in lines:                                   # descriptors: `.amdhsa_kernel sym` .. `.end_amdhsa_kernel`
        s = l.strip()
        m = re.match(r"\.amdhsa_kernel (\S+)", s)
        if m:
            cur = out[m.group(1)]
        elif s == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None:
            cur["desc"].append(s)
    entry = []

    def close():
        for e in entry:
            m = re.match(r"\.name:\s+(\S+)", e)
            if m and m.group(1) in out:
                out[m.group(1)]["meta"] = [x for x in entry if not x.startswith(".symbol")]
    inside = False
    for l in lines:                                   # metadata: one `- .agpr_count` .. entry per kernel
        s = l.strip()
        if s == "amdhsa.kernels:":
            inside = True
        elif inside and (s.startswith("amdhsa.") or s == ".end_amdgpu_metadata"):
            close()
            inside, entry = False, []
        elif inside and l.startswith("  - "):
            close()
            entry = [s[2:].strip()]
        elif inside:
            entry.append(s.lstrip("- ").strip())
    return out


def figures(k):
    got = {}
    for l in k["desc"] + k["meta"]:
        p = l.replace(":", " ").split()
        if p and p[0] in FIGURES:
            got[p[0]] = p[-1]
    return got


def report(name, a, b):
    if a == b:
        print("| `%s` | identical | %d lines |" % (name, len(b)))
        return []
    print("| `%s` | **differs** | %d against %d lines |" % (name, len(a), len(b)))
    ka, kb = kernels(a), kernels(b)
    detail = ["", "### `%s`, per kernel" % name, ""]
    if list(ka) != list(kb):
        detail += ["kernel symbols differ: only in the first tree %s, only in the second %s" %
                   (sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))), ""]
    detail += ["| kernel | descriptor | metadata | figures | instructions | mnemonic counts (second - first) | same multiset of instructions |",
               "|---|---|---|---|---|---|---|"]
    same = 0
    for n in ka:
        if n not in kb:
            continue
        x, y = ka[n], kb[n]
        if x["seq"] == y["seq"] and x["desc"] == y["desc"] and x["meta"] == y["meta"]:
            same += 1
            continue
        delta = {m: y["code"][m] - x["code"][m] for m in set(x["code"]) | set(y["code"]) if y["code"][m] != x["code"][m]}
        fx, fy = figures(x), figures(y)
        fig = "equal" if fx == fy else ", ".join("%s %s -> %s" % (f, fx.get(f), fy.get(f)) for f in FIGURES if fx.get(f) != fy.get(f))
        dem = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"pychain_hip::\(anonymous namespace\)::|pychain_hip::|^void |\(.*\)$", "", dem)
        detail.append("| `%s` | %s | %s | %s | %d / %d | %s | %s |" % (
            dem, "equal" if x["desc"] == y["desc"] else "differs", "equal" if x["meta"] == y["meta"] else "differs", fig,
            len(x["seq"]), len(y["seq"]), ", ".join("%s %+d" % kv for kv in sorted(delta.items())) or "equal",
            "yes" if sorted(x["seq"]) == sorted(y["seq"]) else "no"))
    detail += ["", "%d of %d kernels have the same instruction sequence, descriptor and metadata." % (same, len(ka))]
    return detail


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    first, second = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    files = sys.argv[3:] or DEFAULT
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(t, f, os.path.join(tmp, "%d_%s.s" % (i, f))) for f in files for i, t in enumerate((first, second))]
        with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as ex:
            got = list(ex.map(lambda j: listing(*j), jobs))
    print("flags: `%s --cuda-device-only -S`\n" % " ".join(FLAGS))
    print("| file | device code | |\n|---|---|---|")
    detail, differs = [], 0
    for i, f in enumerate(files):
        d = report(f, got[2 * i], got[2 * i + 1])
        differs += bool(d) or got[2 * i] != got[2 * i + 1]
        detail += d
    print("\n".join(detail))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
