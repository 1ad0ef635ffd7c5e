"""Builds libmcmc_hip.so (hipcc, gfx950 only) in-tree under cobaya_amd/csrc/.

One object per compiled dimension (walker_kernels.hip with -DMCMC_D=<d>) and per entry of
translation_units(), compiled in parallel; linked into cobaya_amd/csrc/libmcmc_hip.so.  An object
is rebuilt when a file the compiler read for it last time (its -MD dependency list), the flags or
its defines change.  hipcc cross-compiles without a GPU, so this runs in the CPU-only build
container.

    python -m cobaya_amd.build            # all dimensions 1..32
    MCMC_HIP_DIMS=2,3,30 python -m cobaya_amd.build   # quick developer build
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(CSRC, "libmcmc_hip.so")
ARCH = "gfx950"
ALL_DIMS = list(range(1, 33))
BIG_DPS = [48, 56, 64, 72, 80, 88, 96, 100, 112, 120, 128]  # padded sizes of the d > 32 kernels
INC_DQ_RANGES = [(1, 8), (9, 16), (17, 24), (25, 32)]  # incremental_kernels.hip: ceil(d / 4)
DUO_DQ_RANGES = [(1, 8), (9, 12)]  # incremental_duo.hip: mixtures, two lanes per walker (two modes: d <= 48)
PAIR_DIMS = list(range(33, 57))  # 32 < d <= 48: walker_kernels.hip's two-wave step kernel alone

# -ffp-contract=off: the kernels' arithmetic order is part of the specification (fused
# operations are written as fma()); see DESIGN.md "Ensemble specification".
# -pragma-unroll-threshold: the operand-stream loops must be unrolled completely (their
# register arrays are only addressable with compile-time indices).
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-ffp-contract=off",
         "-fno-fast-math", "-fvisibility=hidden", "-mllvm", "-pragma-unroll-threshold=1000000", "-Wall", "-Wno-unused-function", "-Wno-unused-const-variable",
         "-Wno-unused-result"]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the mcmc_hip engine can only be built with ROCm")
    return exe


_file_digests = {}


def _file_digest(path):
    """sha256 of a file's contents (None if it is gone), read once per build."""
    if path not in _file_digests:
        try:
            with open(path, "rb") as f:
                _file_digests[path] = hashlib.sha256(f.read()).hexdigest()
        except OSError:
            _file_digests[path] = None
    return _file_digests[path]


def _digest(paths, extra=""):
    h = hashlib.sha256(extra.encode())
    for p in paths:
        h.update(str(_file_digest(p)).encode())
    return h.hexdigest()[:16]


def _dependencies(depfile):
    """The files the compiler read for an object: the prerequisites its -MD file lists."""
    with open(depfile) as f:
        text = f.read().replace("\\\n", " ")
    return [w for w in text.split(":", 1)[1].split() if w]


def _compile(src, obj, defines):
    """Compiles src -> obj unless the last successful compile saw the same inputs: the source
    and every header the compiler itself listed then (obj.d), the flags and the defines.  No
    dependency list (never built, or cleaned): compile."""
    stamp_file, depfile = obj + ".stamp", obj + ".d"
    extra = " ".join([*FLAGS, *defines])
    if os.path.exists(obj) and os.path.exists(stamp_file) and os.path.exists(depfile):
        with open(stamp_file) as f:
            if f.read() == _digest(_dependencies(depfile), extra):
                return False
    for stale in (stamp_file, depfile):
        if os.path.exists(stale):
            os.remove(stale)
    cmd = [hipcc(), *FLAGS, *defines, "-MD", "-MF", depfile, "-c", src, "-o", obj]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed: {' '.join(cmd)}\n{res.stdout}\n{res.stderr}")
    with open(stamp_file, "w") as f:
        f.write(_digest(_dependencies(depfile), extra))
    return True


def translation_units(dims, big=True):
    """(source, object name, defines) of every object of the library, in link order."""
    tus = [("walker_kernels.hip", f"walker_d{d}", [f"-DMCMC_D={d}"]) for d in dims]
    if big:   # 32 < d <= 56: the two-wave step kernel; the padded sizes of the d > 32 kernels
        tus += [("walker_kernels.hip", f"walker_d{d}", [f"-DMCMC_D={d}"]) for d in PAIR_DIMS]
        tus += [("walker_kernels_big.hip", f"walker_big{dp}", [f"-DMCMC_DP={dp}"]) for dp in BIG_DPS]
    tus += [("blocked_kernels.hip", "blocked", []),
            ("general_kernels.hip", "general", []),
            ("pliklite_kernels.hip", "pliklite", []),
            ("checkpoint_kernels.hip", "checkpoint", []),
            ("marginal_kernels.hip", "marginal", []),   # streaming 1-D / 2-D marginal histograms
            ("autocorr_kernels.hip", "autocorr", []),   # lagged cross-products (autocorrelation time)
            ("bestfit_kernels.hip", "bestfit", []),     # best fit, MAP and profile likelihoods
            ("evidence_kernels.hip", "evidence", []),   # the sums of the truncated harmonic mean (evidence)
            ("derived_kernels.hip", "derived", []),     # moments of the derived rows
            ("importance_kernels.hip", "importance", []),   # weighted moments under exp(log-weight)
            ("importance_hist_kernels.hip", "importance_hist", []),   # ... and their marginal histograms
            ("comm.hip", "comm", [])]   # the RCCL communicator (bound at run time)
    tus += [("incremental_kernels.hip", f"incremental_{lo}", [f"-DMCMC_DQ_LO={lo}", f"-DMCMC_DQ_HI={hi}"])
            for lo, hi in INC_DQ_RANGES]
    # the EMIT instantiations of step_inc_kernel (emit: chains)
    tus += [("incremental_kernels.hip", f"incremental_emit_{lo}",
             ["-DMCMC_INC_EMIT_TU", f"-DMCMC_DQ_LO={lo}", f"-DMCMC_DQ_HI={hi}"]) for lo, hi in INC_DQ_RANGES]
    # the general incremental kernel: the LDS kernel + KM = 4 | KM = 8 | KM = 16 register planes
    tus += [("incremental_any.hip", f"incremental_any_{part}", [f"-DANY_PART={part}"]) for part in (0, 1, 2)]
    # two lanes per walker (round 6)
    tus += [("incremental_duo.hip", f"incremental_duo_{lo}", [f"-DMCMC_DUO_DQ_LO={lo}", f"-DMCMC_DUO_DQ_HI={hi}"])
            for lo, hi in DUO_DQ_RANGES]
    tus += [("huge_kernels.hip", "huge", []),        # 128 < d <= 256 (run-time d)
            ("function_kernels.hip", "function", []),   # function targets (the user's batched device function)
            ("stretch_kernels.hip", "stretch", []),     # the stretch move on a function target
            ("ensemble_move_kernels.hip", "ensemble_move", []),   # mixtures of stretch, DE and snooker moves
            ("math_probe_kernels.hip", "math_probe", []),   # test entry: det_math.h function by function
            ("host_linalg.cpp", "host_linalg", []),  # the host side: the C ABI, split by job
            ("capi.hip", "capi", []),
            ("capi_targets.hip", "capi_targets", []),
            ("capi_stretch.hip", "capi_stretch", []),
            ("capi_incremental.hip", "capi_incremental", []),
            ("capi_rows.hip", "capi_rows", []),
            ("capi_checkpoint.hip", "capi_checkpoint", []),
            ("capi_marginals.hip", "capi_marginals", []),
            ("capi_autocorr.hip", "capi_autocorr", []),
            ("capi_bestfit.hip", "capi_bestfit", []),
            ("capi_evidence.hip", "capi_evidence", []),
            ("capi_derived.hip", "capi_derived", []),
            ("capi_importance.hip", "capi_importance", []),
            ("capi_math_probe.hip", "capi_math_probe", [])]
    return tus


def selected_dims():
    env = os.environ.get("MCMC_HIP_DIMS")
    if env:
        return sorted({int(s) for s in env.split(",") if s.strip()})
    return ALL_DIMS


def build(dims=None, jobs=None, verbose=True):
    """Compile every selected dimension and link the shared library. Returns its path."""
    dims = list(dims) if dims is not None else selected_dims()
    extra = os.environ.get("MCMC_HIP_EXTRA_FLAGS", "").split()  # developer experiments
    if extra:
        FLAGS.extend(f for f in extra if f not in FLAGS)
    os.makedirs(OBJ, exist_ok=True)
    _file_digests.clear()
    tasks = [(os.path.join(CSRC, src), os.path.join(OBJ, name + ".o"), defines)
             for src, name, defines in translation_units(dims, big=not os.environ.get("MCMC_HIP_NO_BIG"))]
    jobs = jobs or min(len(tasks), os.cpu_count() or 4)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        rebuilt = list(ex.map(lambda t: _compile(*t), tasks))
    objs = [t[1] for t in tasks]
    link_stamp = _digest(objs)
    stamp_file = LIB + ".stamp"
    need_link = any(rebuilt) or not os.path.exists(LIB)
    if not need_link and os.path.exists(stamp_file):
        with open(stamp_file) as f:
            need_link = f.read() != link_stamp
    if need_link:
        cmd = [hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-ldl", "-o", LIB]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"link failed: {' '.join(cmd)}\n{res.stdout}\n{res.stderr}")
        with open(stamp_file, "w") as f:
            f.write(link_stamp)
    if verbose:
        print(f"[cobaya_amd.build] {LIB}: dims {dims[0]}..{dims[-1]} ({len(dims)}), "
              f"{sum(rebuilt)} objects rebuilt")
    return LIB


if __name__ == "__main__":
    build()
    sys.exit(0)
