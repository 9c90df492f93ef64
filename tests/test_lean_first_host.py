"""The lean pass's dispatch index and breakpoint search (lean_index,
lean_chunk_of, lean_first_search, wfpt_lean_tables.hpp) on the host (no GPU):
tests/c/lean_first_host.cpp is a stand-alone program (its own main) built
under AddressSanitizer + UndefinedBehaviorSanitizer and run directly.

For err in {1e-4, 1e-3, 1e-6}, five (a, t, st) and sorted samples of 64 * 48
and 3,001 trials (|rt| over 0.36-6 s; both boundaries, one boundary, NaN RTs,
a boundary switch inside a chunk):
  (a) for every (boundary, t node, finite upper edge of a piece) the chunk the
      binary search names equals a brute-force scan of every chunk's own
      [min, max]: the last chunk of that boundary whose min is <= r, none for
      an r outside the boundary's data; a chunk whose [min, max] holds r is
      that chunk;
  (b) the list is the sorted set of those chunks without duplicates, the
      unused entries cleared;
  (c) empty lists: no index, a table that never answers, data inside one
      piece, breakpoints outside the data, NaN RTs only;
  (d) a synthetic table of 32 pieces over 20,000 trials gives more than 64
      candidates: the 64 latest in stored order are kept.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tests", "c", "lean_first_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    exe = str(tmp_path_factory.mktemp("lean_first") / "lean_first_host")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                    "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    return exe


def test_lean_first_search(program):
    env = dict(os.environ,
               ASAN_OPTIONS="halt_on_error=1:detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([program], capture_output=True, text=True, env=env, timeout=300)
    report = out.stdout + out.stderr
    print(out.stdout)
    assert "ERROR: AddressSanitizer" not in report, report[-4000:]
    assert "runtime error" not in report, report[-4000:]
    assert out.returncode == 0, report[-4000:]
    assert "all checks passed" in out.stdout, report[-4000:]
