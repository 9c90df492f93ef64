"""Register / scratch / LDS / occupancy of the gfx950 kernels, from the
compiler's own resource-usage remarks (the numbers the code object carries).

    python tools/resource_usage.py [name-filter ...] [-D NAME=VAL ...] [--src sim_kernels.hip]
Without --src: every .hip unit of hddm_amd.build.SOURCES.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hddm_amd.build import CSRC, SOURCES  # noqa: E402

UNITS = [os.path.join(CSRC, s) for s in SOURCES if s.endswith(".hip")]
FIELDS = ("VGPRs", "AGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "LDS Size [bytes/block]")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names),
                         capture_output=True, text=True).stdout.splitlines()
    return out if len(out) == len(names) else names


def usage(defines=(), src=UNITS[0]):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
               "-fPIC", "--offload-arch=gfx950", *[f"-D{d}" for d in defines], "-c", src, "-o",
               os.path.join(td, "k.o"), "-Rpass-analysis=kernel-resource-usage"]
        txt = subprocess.run(cmd, capture_output=True, text=True, cwd=td).stderr
    rows, cur = [], None
    for line in txt.splitlines():
        m = re.search(r"remark: (Function Name|[A-Za-z ]+(?:\[[^\]]*\])?): (.*?) \[-Rpass", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            cur = {"name": val}
            rows.append(cur)
        elif cur is not None and key in FIELDS:
            cur[key] = val
    names = demangle([r["name"] for r in rows])
    for r, n in zip(rows, names):
        r["name"] = n
    return rows


def main():
    args = sys.argv[1:]
    defines, filt, srcs = [], [], UNITS
    while args:
        a = args.pop(0)
        if a == "-D":
            defines.append(args.pop(0))
        elif a == "--src":  # another unit of hddm_amd/csrc
            srcs = [os.path.join(CSRC, args.pop(0))]
        else:
            filt.append(a)
    for r in (r for src in srcs for r in usage(defines, src)):
        if filt and not any(f in r["name"] for f in filt):
            continue
        print(f"{r['name'][:70]:70s} " + " ".join(f"{k.split()[0]}={r.get(k, '-')}" for k in FIELDS))


if __name__ == "__main__":
    main()
