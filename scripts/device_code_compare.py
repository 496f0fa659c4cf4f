#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two trees (profiles/r08, r09, r20: device_code_compare.txt).

    python scripts/device_code_compare.py PARENT_TREE BRANCH_TREE OUT_DIR

Compiles every unit that carries kernels in both trees with build.py's flags and `--offload-device-only -S` into
OUT_DIR/{parent,branch}/<unit>.s, then compares per kernel the function body (label to .Lfunc_end) and the .amdhsa_kernel
block as text after local labels are normalised, and prints VGPR / AGPR / scratch / static LDS from the kernels' metadata; for
a kernel that differs also whether the instruction counts per opcode agree. A kernel whose parameter type was renamed is paired
through RENAMES, applied to the demangled name; its own symbol is blanked in the compared text."""
import collections
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mir_optim_amd import build as hipbuild  # noqa: E402

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--offload-device-only", "-S"]
# every unit of the two libraries that can carry kernels, and every example of tests/user_model/
RENAMES = {}        # demangled-name substitutions that pair a kernel whose parameter type was renamed: none
# units and examples of the branch only, whose kernels are listed and not compared (r25: the fitted-curve kernel)
NEW_UNITS = ["batched_predict", "batched_predict_d"]
NEW_USER = ["user_model_predict"]
UNITS = [u[:-4] for u in hipbuild.SOLVER_UNITS + hipbuild.WORKLOAD_UNITS if u.endswith(".hip") and u[:-4] not in NEW_UNITS]
USER = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(os.path.dirname(hipbuild.HERE), "tests", "user_model", "*.hip"))
              if os.path.basename(f)[:-4] not in NEW_USER)


def compile_tree(tree, out):
    os.makedirs(out, exist_ok=True)
    cmds = [["hipcc"] + FLAGS + (["-fopenmp"] if u + ".hip" in hipbuild.WORKLOAD_UNITS else []) + ["mir_optim_amd/csrc/%s.hip" % u, "-o", "%s/%s.s" % (out, u)]
            for u in UNITS]
    cmds += [["hipcc"] + FLAGS + ["-I", "include", "tests/user_model/%s.hip" % u, "-o", "%s/%s.s" % (out, u)] for u in USER]
    cmds += [["hipcc"] + FLAGS + ["mir_optim_amd/csrc/%s.hip" % u, "-o", "%s/%s.s" % (out, u)]
             for u in NEW_UNITS if os.path.exists(os.path.join(tree, "mir_optim_amd/csrc/%s.hip" % u))]
    cmds += [["hipcc"] + FLAGS + ["-I", "include", "tests/user_model/%s.hip" % u, "-o", "%s/%s.s" % (out, u)]
             for u in NEW_USER if os.path.exists(os.path.join(tree, "tests/user_model/%s.hip" % u))]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda c: subprocess.check_call(c, cwd=tree, stderr=subprocess.DEVNULL), cmds))


def norm(t):
    t = re.sub(r"BB[0-9]+_", "BB_", t)
    t = re.sub(r"Lfunc_(end|begin)[0-9]+", r"Lfunc_\1", t)
    return re.sub(r"[ \t]+", " ", t)


def kernels(path):
    if not os.path.exists(path):
        return {}, {}
    s = open(path).read()
    code = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", s, re.M | re.S):
        body = re.search(r"^" + re.escape(m.group(1)) + r":.*?^\.Lfunc_end[0-9]+:", s, re.M | re.S).group(0)
        code[m.group(1)] = tuple(norm(t.replace(m.group(1), "KERNEL")) for t in (body, m.group(2)))
    res = {}
    for m in re.finditer(r"- \.agpr_count:\s+(\d+).*?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?"
                         r"\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", s, re.S):
        res[m.group(3)] = (int(m.group(5)), int(m.group(1)), int(m.group(4)), int(m.group(2)))
    return code, res


def opcounts(body):
    c = collections.Counter()
    for line in body.splitlines():
        line = line.strip()
        if line and not line.startswith((".", ";")) and not line.endswith(":"):
            c[line.split()[0]] += 1
    return c


def by_demangled_name(*dicts):
    """the dicts re-keyed by the demangled kernel name after RENAMES"""
    names = sorted(set().union(*dicts))
    dm = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    for old, new in RENAMES.items():
        dm = [d.replace(old, new) for d in dm]
    dm = dict(zip(names, dm))
    return [{dm[k]: v for k, v in d.items()} for d in dicts]


def main(parent, branch, out):
    pd, bd = os.path.join(out, "parent"), os.path.join(out, "branch")
    compile_tree(parent, pd)
    compile_tree(branch, bd)
    tot = same = alone = 0
    for u in UNITS + USER + NEW_UNITS + NEW_USER:
        pk, pr, bk, br = by_demangled_name(*kernels("%s/%s.s" % (pd, u)), *kernels("%s/%s.s" % (bd, u)))
        print("== %s: %d kernels in the parent, %d in the branch" % (u, len(pk), len(bk)))
        for k in pk:
            print("  " + k)
            if k not in bk:
                print("      only in the parent")
                alone += 1
                continue
            tot += 1
            ident = pk[k] == bk[k]
            same += ident
            extra = ""
            if not ident:
                extra = "   [instruction counts per opcode: %s; .amdhsa_kernel block: %s]" % (
                    "equal" if opcounts(pk[k][0]) == opcounts(bk[k][0]) else "differ", "equal" if pk[k][1] == bk[k][1] else "differs")
            print("      body + .amdhsa_kernel block identical: %s   VGPR %d/%d  AGPR %d/%d  scratch %d/%d  static LDS %d/%d  (parent/branch)%s"
                  % (("yes" if ident else "NO",) + tuple(v for pair in zip(pr[k], br[k]) for v in pair) + (extra,)))
        for k in bk:
            if k not in pk:
                alone += 1
                print("  " + k + "\n      only in the branch   VGPR %d  AGPR %d  scratch %d  static LDS %d" % br[k])
    print("== total: %d kernels present in both trees, %d text-identical, %d in one tree only" % (tot, same, alone))
    return 0 if tot == same and not alone else 1


if __name__ == "__main__":
    sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])))
