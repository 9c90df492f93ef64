#!/usr/bin/env python3
"""Compare the device code of two source trees, function by function.

    python tools/kernel_isa_diff.py LEFT RIGHT [--rename REGEX=REPL ...] [--jobs N] [--list]
                                    [--keep DIR]

Each tree's kernel units (the .hip entries of its hddm_amd.build.SOURCES) are
compiled with its build.CFLAGS plus --cuda-device-only -S. The assembly is cut
per function (its label up to .Lfunc_end, plus a kernel's descriptor block),
labels that carry the function's index in its unit and the compilation-unit id
are normalised, and the whole texts are compared by demangled name: identical /
differing / only left / only right. --rename rewrites mangled names of the
LEFT tree first (a Python regex over the assembly; for a kernel that was
renamed or lost template parameters). Differing functions get their registers,
scratch, occupancy and instruction count on both sides. A function emitted by
several units of a tree counts once per distinct text. Each tree's build.py is
loaded from its own path and must derive CSRC from its own location.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter, defaultdict
from concurrent.futures import ThreadPoolExecutor

INFO = (("VGPRs", r"; NumVgprs: (\d+)"), ("SGPRs", r"; TotalNumSgprs: (\d+)"),
        ("scratch", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"))
NORMALISE = ((r"\.(LBB|LJTI|LCPI)\d+_", r".\1_"), (r"\bBB\d+_", "BB_"),
             (r"\.L(func_begin|func_end|tmp|post_getpc)\d+", r".L\1"),
             (r"__hip_cuid_[0-9a-f]+", "__hip_cuid_"),
             (r"[ \t]+;", " ;"))  # a comment's column follows the label's width


def load_build(tree):
    path = os.path.join(tree, "hddm_amd", "build.py")
    spec = importlib.util.spec_from_file_location("tree_build", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(tree, jobs, tmp, reuse=False):
    os.makedirs(tmp, exist_ok=True)
    b = load_build(tree)
    units = [s for s in b.SOURCES if s.endswith(".hip")]

    def one(src):
        out = os.path.join(tmp, src + ".s")
        if not (reuse and os.path.exists(out)):
            r = subprocess.run([b.HIPCC, *b.CFLAGS, "--cuda-device-only", "-S", "-o", out,
                                os.path.join(b.CSRC, src)], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"{src} of {tree} does not compile:\n{r.stderr[-4000:]}")
        with open(out) as fh:
            return src, fh.read()

    with ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(one, units))


def functions(asm, renames):
    """{mangled name: [(unit, normalised text, info dict)]}"""
    funcs = defaultdict(list)
    for unit, text in asm:
        for pat, repl in renames:
            text = re.sub(pat, repl, text)
        # one piece per function: its label up to .Lfunc_end (a kernel's
        # descriptor block lies in between), then the resource comments
        for piece in re.split(r"^.*; -- Begin function .*\n", text, flags=re.M)[1:]:
            m = re.search(r"^(_Z\w+):.*?^\.Lfunc_end\d+:\n", piece, re.M | re.S)
            if not m:
                continue
            name, body, tail = m.group(1), m.group(0), piece[m.end():]
            for pat, repl in NORMALISE:
                body = re.sub(pat, repl, body)
            info = {k: (re.search(p, tail).group(1) if re.search(p, tail) else "-") for k, p in INFO}
            info["instructions"] = str(len(re.findall(r"^\t[a-z]\w+", body, re.M)))
            funcs[name].append((unit, body, info))
    return funcs


def demangle(names):
    names = list(names)
    if not names:
        return {}
    filt = shutil.which("llvm-cxxfilt") or "c++filt"
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, out.stdout.split("\n")))


def short(name):
    """wfpt::lean_kernel<3, false, 0>(args) -> lean_kernel<3, false, 0>"""
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    depth = 0
    for k, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            name = name[:k]
            break
    return name.replace("wfpt::", "")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("left")
    ap.add_argument("right")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--list", action="store_true", help="also list the identical functions")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly in DIR/left, DIR/right and "
                    "reuse what is already there (the trees must not have changed since)")
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    with tempfile.TemporaryDirectory() as tmp:
        d, reuse = (a.keep, True) if a.keep else (tmp, False)
        L = functions(assembly(os.path.abspath(a.left), a.jobs, os.path.join(d, "left"), reuse),
                      renames)
        R = functions(assembly(os.path.abspath(a.right), a.jobs, os.path.join(d, "right"), reuse), [])
    dm = demangle(set(L) | set(R))
    same, differ = [], []
    for n in sorted(set(L) & set(R), key=lambda n: dm[n]):
        (same if {t for _, t, _ in L[n]} == {t for _, t, _ in R[n]} else differ).append(n)
    only_l, only_r = sorted(set(L) - set(R), key=dm.get), sorted(set(R) - set(L), key=dm.get)
    print(f"identical {len(same)}  differing {len(differ)}  only left {len(only_l)}  "
          f"only right {len(only_r)}")
    for title, names in (("only left", only_l), ("only right", only_r)):
        print(f"\n== {title}: {len(names)}")
        per = Counter(re.sub(r"<.*", "", short(dm[n])) for n in names)
        for k, c in sorted(per.items()):
            print(f"  {c:3d} x {k}")
        for n in names:
            print("     ", short(dm[n]))
    print(f"\n== differing: {len(differ)}")
    for n in differ:
        print("  ", short(dm[n]))
        for side, F in (("left ", L), ("right", R)):
            for unit, _, info in F[n]:
                print(f"      {side} {unit:22s} " + "  ".join(f"{k} {v}" for k, v in info.items()))
    if a.list:
        print(f"\n== identical: {len(same)}")
        for n in same:
            print("  ", short(dm[n]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
