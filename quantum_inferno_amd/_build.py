"""Builds libqi_tfr.so in-tree for gfx950 (hipcc cross-compiles without a GPU).

The library is linked against the HIP runtime and hipFFT that PyTorch-ROCm ships
(torch/lib), not the copies under /opt/rocm/lib: device pointers and streams cross the
C ABI from torch, so both sides must share ONE HIP runtime in the process.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libqi_tfr.so")
SOURCES = ["qi_api.hip", "qi_api_ops.hip", "qi_host_util.hip", "qi_plan_build.hip", "qi_run.hip", "qi_kernels.hip", "qi_native.hip", "qi_block.hip", "qi_zoom.hip", "qi_shannon1d.hip", "qi_stft_hipfft.hip", "qi_stft_fused.hip", "qi_zoom64.hip", "qi_pool.hip", "qi_small.hip", "qi_filter.hip", "qi_peaks.hip", "qi_resample.hip", "qi_calculus.hip", "qi_synth.hip", "qi_csd.hip", "qi_beam.hip", "qi_whiten.hip", "qi_eigh.hip", "qi_steer.hip", "qi_lags.hip", "qi_timebeam.hip", "qi_squeeze.hip"]
ARCH = "gfx950"
# the FFT kernels lose ~10 % to the register shuffles of SLP-packed v_pk_* arithmetic (no throughput gain on gfx950)
PER_FILE_FLAGS = {"qi_native.hip": ("-fno-slp-vectorize",), "qi_block.hip": ("-fno-slp-vectorize",), "qi_zoom.hip": ("-fno-slp-vectorize",),
                  "qi_small.hip": ("-fno-slp-vectorize",),
                  # the IIR recurrences round every product and sum on their own, as SciPy's C loops do (bit-exact results)
                  "qi_filter.hip": ("-ffp-contract=off",),
                  # the scaled values are NumPy's quotients bit for bit: IEEE float32 division, no fused multiply-add
                  "qi_peaks.hip": ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"),
                  # the grid is np.arange's and the interpolation np.interp's bit for bit: every product and sum rounded on its own
                  "qi_resample.hip": ("-ffp-contract=off",),
                  # the trapezoid terms are SciPy's and the derivatives NumPy's bit for bit: no fused multiply-add, IEEE float32 division
                  "qi_calculus.hip": ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"),
                  # the argument of every transcendental is NumPy's bit for bit, and so is every formula without one
                  "qi_synth.hip": ("-ffp-contract=off",),
                  # the order and the rounding of every sum are the header's contract: the fused multiply-adds are written out
                  "qi_timebeam.hip": ("-ffp-contract=off",),
                  # a product is rounded before it is added, and the fused call equals the two-call composition bit for bit
                  "qi_squeeze.hip": ("-ffp-contract=off",)}


def torch_lib_dir():
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        raise RuntimeError("PyTorch-ROCm is required (its bundled HIP runtime is the one the library links)")
    return os.path.join(list(spec.submodule_search_locations)[0], "lib")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if not f.endswith(".o")]
    deps += [os.path.join(ROOT, "include", "qi_tfr.h"), os.path.join(ROOT, "include", "qi_array.h"), os.path.join(ROOT, "include", "qi_beam.h"),
             os.path.join(ROOT, "include", "qi_adaptive.h"), os.path.join(ROOT, "include", "qi_subspace.h"), os.path.join(ROOT, "include", "qi_steer.h"),
             os.path.join(ROOT, "include", "qi_windows.h"), os.path.join(ROOT, "include", "qi_lags.h"),
             os.path.join(ROOT, "include", "qi_bands.h"), os.path.join(ROOT, "include", "qi_timebeam.h"),
             os.path.join(ROOT, "include", "qi_squeeze.h"),
             os.path.abspath(__file__)]  # (the flags live in this file)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, extra_flags=(), lib=None):
    lib = lib or LIB
    if not force and not extra_flags and not needs_build():
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tlib = torch_lib_dir()
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".dbg.o" if extra_flags else ".o"))
        cmd = [hipcc, "-c", "-fPIC", "-O3", "-std=c++17", f"--offload-arch={ARCH}", "-I", os.path.join(ROOT, "include"),
               "-I", CSRC, "-Wall", "-Wno-unused-function", *PER_FILE_FLAGS.get(src, ()), *extra_flags,
               os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    link = ["g++", "-shared", "-o", lib, *objs, f"-L{tlib}", "-lamdhip64", "-lhipfft", f"-Wl,-rpath,{tlib}",
            "-Wl,--no-undefined", "-lpthread"]
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.check_call(link)
    return lib


if __name__ == "__main__":
    if "--stamps" in sys.argv:  # diagnostic library with in-kernel phase stamps (never the shipped one)
        print(build(force=True, extra_flags=("-DQI_NATIVE_STAMPS", "-DQI_NATIVE_DEBUG"),
                    lib=os.path.join(HERE, "libqi_tfr_stamps.so")))
    elif "--variant" in sys.argv:  # experiment library: --variant NAME -DFLAG ... -> libqi_tfr_NAME.so
        i = sys.argv.index("--variant")
        print(build(force=True, extra_flags=tuple(sys.argv[i + 2:]),
                    lib=os.path.join(HERE, f"libqi_tfr_{sys.argv[i + 1]}.so")))
    else:
        build(force="--force" in sys.argv)
        print(LIB)
