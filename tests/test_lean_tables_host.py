"""The lean pass's uniform-wave host table and its per-trial range test, on the
host (no GPU): tests/c/lean_tables_host.cpp is a stand-alone program (its own
main) built from hddm_amd/csrc/wfpt_lean_tables.hpp and wfpt_zgrid.hpp under
AddressSanitizer + UndefinedBehaviorSanitizer.

  * uniform_tab: for 1,000 random (z, sz, boundary, v, sv, a) grids every
    multiplier u[k][i] and every per-K constant is bit-equal to the expression
    a lane of small_grid2d evaluates (the k2 chain included).
  * uniform_guard: over 1e6 random (v, sv, a, x, t, st, grid, K per node)
    draws inside and outside HDDM's generator ranges, whenever the per-trial
    bound passes, small_grid2d's per-node `safe` holds at each small-time node
    and every drift exponent is below 600 in magnitude.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tests", "c", "lean_tables_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    exe = str(tmp_path_factory.mktemp("lean_tables") / "lean_tables_host")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                    "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    return exe


def test_uniform_table_and_guard(program):
    env = dict(os.environ,
               ASAN_OPTIONS="halt_on_error=1:detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([program], capture_output=True, text=True, env=env, timeout=300)
    report = out.stdout + out.stderr
    assert "ERROR: AddressSanitizer" not in report, report[-4000:]
    assert "runtime error" not in report, report[-4000:]
    assert out.returncode == 0, report[-4000:]
    assert "all checks passed" in out.stdout, report[-4000:]
