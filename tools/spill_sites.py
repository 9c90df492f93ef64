"""Scratch spill / reload sites of one kernel, attributed to source lines.

    python tools/spill_sites.py [kernel-substring] [-D...]
Searches every .hip unit of hddm_amd.build.SOURCES for the kernel.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hddm_amd.build import CSRC, SOURCES  # noqa: E402


def main():
    pat = sys.argv[1] if len(sys.argv) > 1 else "lean_kernelILi3ELb0ELi0E"
    defs = [a for a in sys.argv[2:] if a.startswith("-D")]
    out = "/tmp/wfpt_spill.s"
    for src in (u for u in SOURCES if u.endswith(".hip")):  # the first unit that has the kernel
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-fno-fast-math", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-gline-tables-only", *defs, "-o", out, os.path.join(CSRC, src)],
                       check=True, stderr=subprocess.DEVNULL)
        s = open(out).read()
        m = re.search(r"^(_Z\w*" + re.escape(pat) + r"\w*):", s, re.M)
        if m:
            break
    else:
        sys.exit(f"no kernel matches {pat}")
    files = {m.group(1): m.group(3).split("/")[-1]
             for m in re.finditer(r'\.file\s+(\d+)\s+("[^"]*"\s+)?"([^"]+)"', s)}
    end = s.index(".Lfunc_end", m.end())
    cur = None
    for i, l in enumerate(s[m.end():end].splitlines()):
        mm = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
        if mm:
            cur = f"{files.get(mm.group(1), mm.group(1))}:{mm.group(2)}"
        elif "scratch_" in l:
            print(i, cur, l.strip()[:90])


if __name__ == "__main__":
    main()
