"""Build libwfpt_amd.so in-tree (hipcc, gfx950 only).

    python -m hddm_amd.build [--force]

The library lands in hddm_amd/lib/ (git-ignored, shipped to the GPU box with
the working tree). No CMake, no JIT cache: the .so that the tests and bench
load is exactly the one built here.
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "libwfpt_amd.so")
# the longest-compiling units first (they start first)
SOURCES = ["wfpt_node.hip", "wfpt_sum.hip", "wfpt_engine.hip", "wfpt_fold.hip",
           "wfpt_level0.hip", "cdfdif_kernels.hip", "rl_kernels.hip", "sim_kernels.hip",
           "rl_sim_kernels.hip", "reg_sim_kernels.hip", "reg_kernels.hip", "stats_kernels.hip",
           "pointwise_kernels.hip", "rl_reg_kernels.hip",
           "capi_core.cpp", "capi_comm.cpp", "capi_rl.cpp", "capi_reg.cpp", "capi_sim.cpp",
           "capi_rl_reg.cpp",
           "wfpt_rendezvous.cpp"]
DEPS = SOURCES + ["wfpt_types.hpp", "wfpt_math.hpp", "wfpt_series.hpp", "wfpt_quad.hpp",
                  "wfpt_zgrid.hpp", "wfpt_grid.hpp", "wfpt_level0.hpp", "wfpt_lean_tables.hpp",
                  "wfpt_lean.hpp", "wfpt_kernel_common.hpp", "wfpt_engine.hpp",
                  "wfpt_internal.h", "rl_internal.h", "sim_internal.h", "reg_internal.h",
                  "stats_internal.h", "sim_philox.hpp", "rl_update.hpp", "reg_predict.hpp",
                  "pointwise_internal.h", "pointwise_update.hpp", "capi_internal.hpp",
                  "capi_layout.hpp", "wfpt_crlibm.hpp", "wfpt_exact.hpp", "rl_reg_internal.h"]
ARCH = os.environ.get("WFPT_OFFLOAD_ARCH", "gfx950")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CFLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
          f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-result"]


def source_digest(defines=()):
    """sha1 over the compiler flags and every source the library is built from:
    identifies a build independently of the binary's bytes (profiles measured
    on one build are matched to the library by it)."""
    import hashlib
    h = hashlib.sha1(" ".join(CFLAGS + list(defines)).encode())
    for f in DEPS:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.join(ROOT, "include", "wfpt_amd.h"), "rb") as fh:
        h.update(fh.read())
    return h.hexdigest()


def built_digest(lib=LIB):
    """The source digest recorded next to a built library (None if absent)."""
    try:
        with open(lib + ".src") as fh:
            return fh.read().strip()
    except OSError:
        return None


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, defines=(), out=None):
    """Compile libwfpt_amd.so. `defines` (e.g. ["WFPT_FAST_WAVES=3"]; entries
    starting with '-' are extra compiler flags) and `out` build experiment
    variants next to the default library."""
    os.makedirs(LIBDIR, exist_ok=True)
    lib = out or LIB
    deps = [os.path.join(CSRC, f) for f in DEPS] + [os.path.join(ROOT, "include", "wfpt_amd.h")]
    if not force and not _stale(lib, deps):
        if built_digest(lib) is None:  # built before digests were recorded
            with open(lib + ".src", "w") as fh:
                fh.write(source_digest(defines) + "\n")
        return lib
    objs, procs = [], []
    tag = os.path.splitext(os.path.basename(lib))[0]
    for src in SOURCES:  # the translation units compile concurrently
        obj = os.path.join(LIBDIR, tag + "_" + os.path.splitext(src)[0] + ".o")
        flags = [f for d in defines if d.startswith("-") for f in d.split()]
        cmd = [HIPCC, *CFLAGS, *flags, *[f"-D{d}" for d in defines if not d.startswith("-")],
               "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((subprocess.Popen(cmd), cmd))
        objs.append(obj)
    for p, cmd in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    tmp = lib + ".tmp"
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp, *objs,
           "-L/opt/rocm/lib", "-lrccl", "-lrocprofiler-sdk-roctx", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(tmp, lib)
    with open(lib + ".src", "w") as fh:
        fh.write(source_digest(defines) + "\n")
    for o in objs:
        os.remove(o)
    return lib


# Diagnostic builds that tests load in a child process (WFPT_AMD_LIB); never
# the product. pubdiag: segment_publish_diag_kernel publishes the node sums;
# its non-last blocks store theirs after the completion word
# (tests/test_parity_trials.py: test_stale_check_detects_late_publication).
VARIANTS = {"pubdiag": ["WFPT_PUB_DIAG=1"]}


def variant_path(name):
    return os.path.join(LIBDIR, f"libwfpt_amd_{name}.so")


# The exact path's two headers as device kernels of their own, one element per
# lane (tests/c/exact_device.hip, loaded by tests/test_exact_device.py): test
# infrastructure built with the library's flags, not part of the library or of
# its source digest.
PROBE = os.path.join(LIBDIR, "libwfpt_exact_probe.so")
PROBE_SRC = os.path.join(ROOT, "tests", "c", "exact_device.hip")


def build_probe(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    deps = [PROBE_SRC] + [os.path.join(CSRC, f) for f in ("wfpt_crlibm.hpp", "wfpt_exact.hpp")]
    if not force and not _stale(PROBE, deps):
        return PROBE
    tmp = PROBE + ".tmp"
    cmd = [HIPCC, *CFLAGS, "-shared", "-o", tmp, PROBE_SRC, "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(tmp, PROBE)
    return PROBE


def build_variants(force=False, verbose=False):
    """The diagnostic libraries and the exact-path probe: everything the GPU
    tests load besides the product."""
    libs = [build(force=force, verbose=verbose, defines=d, out=variant_path(k))
            for k, d in VARIANTS.items()]
    return libs + [build_probe(force=force, verbose=verbose)]


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    if "--variants" in sys.argv:
        print(build_variants(force="--force" in sys.argv, verbose=True))
