"""Static ISA statistics of one kernel (device assembly via hipcc -S).

    python tools/isa_stats.py [kernel-substring] [-D...]
Compiles the .hip units of hddm_amd.build.SOURCES in turn, with its CFLAGS,
and stops at the first one that holds the kernel. Prints VGPR/SGPR counts, occupancy and the instruction histogram.
"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hddm_amd.build import CFLAGS, CSRC, HIPCC, SOURCES  # noqa: E402


def main():
    pat = sys.argv[1] if len(sys.argv) > 1 else "lean_kernelILi3ELb0ELi0E"
    defs = [a for a in sys.argv[2:] if a.startswith("-D")]
    out = "/tmp/wfpt_isa.s"
    for src in (u for u in SOURCES if u.endswith(".hip")):
        subprocess.run([HIPCC, *CFLAGS, "--cuda-device-only", "-S", *defs, "-o", out,
                        os.path.join(CSRC, src)], check=True, stderr=subprocess.DEVNULL)
        s = open(out).read()
        if re.search(r"^_Z\w*" + re.escape(pat) + r"\w*:", s, re.M):
            break
    else:
        sys.exit(f"no kernel matches {pat}")
    for m in re.finditer(r"^(_Z\w*" + re.escape(pat) + r"\w*):", s, re.M):
        name = m.group(1)
        end = s.index(".Lfunc_end", m.end())
        body = s[m.end():end].splitlines()
        ins = [l.strip().split()[0] for l in body
               if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        info = s[end:end + 4000]
        g = lambda k: (re.search(k + r":\s*(\d+)", info) or [None, "?"])[1]
        print(f"{name}: {len(ins)} instrs, VGPR {g('NumVgprs')}, SGPR {g('TotalNumSgprs')}, "
              f"scratch {g('ScratchSize')}, occupancy {g('Occupancy')}")
        for k, v in collections.Counter(ins).most_common(int(os.environ.get("TOP", "25"))):
            print(f"   {k:28s}{v}")


if __name__ == "__main__":
    main()
