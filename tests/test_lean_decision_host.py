"""The lean pass's series-decision table (decision_tab, wfpt_lean_tables.hpp)
on the host (no GPU): tests/c/lean_decision_host.cpp is a stand-alone
program (its own main) built under AddressSanitizer +
UndefinedBehaviorSanitizer and run directly.

For each err in {1e-2, 1e-3, 1e-4, 1e-6, 1e-10, 1e-80}:
  (a) the pieces and their codes match a dense scan (400,000 log-spaced tt) of
      the reference's formula: 6, 6, 6, 8, 8 pieces for the first five; at
      1e-80 the pieces with K > 8 have no entry; ks is nondecreasing and kl
      nonincreasing over the domain;
  (b) over 2e6 log-spaced tt, every edge and its neighbouring doubles, and tt
      formed as (x - tc) * ia2 for random (x, t, st, a) (half of them aimed at
      an edge): whenever the table answers, the reference's formula on xx / a2
      gives the same (small, K) and none of decide64's 1e-12 ambiguity tests;
  (c) inside every band, at its ends and outside the domain the table does not
      answer;
  (d) the lookup as a wave does it (edge counts equal and odd at both ends)
      never accepts an interval [tt_min, tt_max] that holds a breakpoint.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tests", "c", "lean_decision_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    exe = str(tmp_path_factory.mktemp("lean_decision") / "lean_decision_host")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                    "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    return exe


def test_decision_table(program):
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
