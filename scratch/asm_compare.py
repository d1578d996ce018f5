"""Device assembly of one tree against another, kernel by kernel (DESIGN.md section 4.0's rule of acceptance).

  python scratch/asm_compare.py emit OUT [TREE]   every HIP source of TREE (default: this tree) with build.py's flags + -S --cuda-device-only -> OUT/<file>.s
  python scratch/asm_compare.py compare A B [-v]  A = the parent's listings, B = this tree's

Per kernel symbol: `identical` (same text once comments and the per-function numbering of local labels are dropped), `rule-equal` (equal metadata -- VGPR, AGPR,
SGPR, LDS, private segment, kernarg -- and equal instruction-mnemonic counts), else `DIFFERS` with what moved.  It only diffs and counts.
"""
import collections
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")


def emit(out, tree):
    spec = importlib.util.spec_from_file_location("kf_build", os.path.join(tree, "koifish_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(out, exist_ok=True)
    cmds = [[b.HIPCC] + b.HIP_FLAGS + b.HIP_FILE_FLAGS.get(s, []) + ["-S", "--cuda-device-only", os.path.join(b.CSRC, s), "-o", os.path.join(out, s[:-4] + ".s")]
            for s in b.HIP_SOURCES]
    with ThreadPoolExecutor(max_workers=int(os.environ.get("KF_BUILD_JOBS", "6"))) as ex:
        list(ex.map(subprocess.check_call, cmds))


def kernels(path):
    """{symbol: (normalised text lines, mnemonic counts, metadata)} of one listing"""
    lines = open(path).read().split("\n")
    meta, cur = {}, None
    for ln in lines:   # the .amdgpu_metadata map: kernel-level keys sit at column 4 (a kernel's arguments are nested deeper)
        m = re.match(r"^  (- |  )\.(\w+):\s+(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3)
        if m.group(2) == "symbol":
            meta[m.group(3).strip("'\"")[:-3]] = cur
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(\w+):", lines[i])
        if m and m.group(1) in meta:
            sym, body = m.group(1), []
            i += 1
            while i < len(lines) and not re.match(r"^\.Lfunc_end\d+:", lines[i]):
                ln = re.sub(r"\.LBB\d+_", ".LBB_", lines[i].split(";")[0].rstrip())
                if ln.strip():
                    body.append(ln)
                i += 1
            mn = collections.Counter(ln.split()[0] for ln in body if ln.startswith("\t") and not ln.lstrip().startswith("."))
            out[sym] = (body, mn, tuple(meta[sym].get(k) for k in META))
        i += 1
    return out


def compare(a, b, verbose):
    tally = collections.Counter()
    bad = 0
    for f in sorted(set(os.listdir(a)) | set(os.listdir(b))):
        if not f.endswith(".s"):
            continue
        ka = kernels(os.path.join(a, f)) if os.path.exists(os.path.join(a, f)) else {}
        kb = kernels(os.path.join(b, f)) if os.path.exists(os.path.join(b, f)) else {}
        per = collections.Counter()
        for sym in sorted(set(ka) | set(kb)):
            if sym not in ka or sym not in kb:
                verdict, why = "MISSING", "only in " + ("A" if sym in ka else "B")
            elif ka[sym][0] == kb[sym][0] and ka[sym][2] == kb[sym][2]:
                verdict, why = "identical", ""
            elif ka[sym][1] == kb[sym][1] and ka[sym][2] == kb[sym][2]:
                verdict, why = "rule-equal", ""
            else:
                d = {k: (ka[sym][1][k], kb[sym][1][k]) for k in set(ka[sym][1]) | set(kb[sym][1]) if ka[sym][1][k] != kb[sym][1][k]}
                md = {k: (x, y) for k, x, y in zip(META, ka[sym][2], kb[sym][2]) if x != y}
                verdict, why = "DIFFERS", "meta %s mnemonics %s" % (md, d)
            per[verdict] += 1
            if verdict in ("MISSING", "DIFFERS"):
                bad += 1
            if verbose or verdict != "identical":
                print("%-12s %s %s %s" % (verdict, f, sym, why))
        tally.update(per)
        print("== %-28s %s" % (f, dict(per)))
    print("total", dict(tally))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], "-v" in sys.argv))
    else:
        sys.exit(__doc__)
