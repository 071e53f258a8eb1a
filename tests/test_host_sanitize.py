"""Host sanitizer target (CPU only): the library's translation units compiled for the host under AddressSanitizer +
UBSan and linked with a stand-in HIP runtime, driven through the C ABI over every order 1 .. 12 x 2^14 .. 2^22 samples x both
precisions x 1 / 4 / 16 / 64 records, then over the synthetic (not constant-Q) tables of tests/band_tables.py x 1 / 4 / 16
records and a set of degenerate tables the library must refuse (tests/sanitize/walk.cpp has the list of what is checked).
Needs hipcc (the build container has it; the run takes about a minute); a GPU is neither needed nor used."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "sanitize")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="the host sanitizer build needs hipcc")
def test_host_code_under_asan_ubsan_over_every_layout():
    build = os.path.join(SAN, "_build")
    make = subprocess.run(["make", "-C", SAN, f"-j{min(8, os.cpu_count() or 1)}", f"HIPCC={HIPCC}"], capture_output=True, text=True, timeout=1200)
    assert make.returncode == 0, make.stdout[-2000:] + make.stderr[-4000:]
    tables = os.path.join(build, "tables.bin")
    gen = subprocess.run([sys.executable, os.path.join(SAN, "gen_tables.py"), tables], capture_output=True, text=True, timeout=600)
    assert gen.returncode == 0, gen.stderr[-3000:]
    syn = json.loads(gen.stdout.strip().splitlines()[-1])  # the synthetic tables appended behind the 864 dyadic layouts
    assert syn["synthetic_plans"] >= 50
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(build, "walk"), tables], capture_output=True, text=True, timeout=1500, env=env)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr and "LeakSanitizer" not in run.stderr
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    # 12 orders x 9 lengths x 2 precisions x 4 batch sizes, eight transform calls each (+ the atoms bank on a few)
    total = 864 + syn["synthetic_plans"]
    assert rec["ok"] and rec["plans"] == total and rec["calls"] >= 8 * total and rec["scratch_regions_checked"] > 60000
    assert rec["synthetic_plans"] == syn["synthetic_plans"]
    # the plan-less STFT family: seven calls on each of three geometries (two fused, one hipFFT) in both precisions
    assert rec["stft_calls"] == 2 * 3 * 7
    # the plan-less record calls: ten accepted calls in both precisions and three no-ops, then the single-fault refusals of
    # qi_filtfilt, qi_decimate, qi_find_peaks, qi_interp_grid, qi_resample_fft, qi_cumtrapz and qi_derivative
    assert rec["record_calls"] == 2 * 10 + 3 + (8 + 9 + 9 + 15 + 7 + 10 + 13)
    # (every dyadic table of these shapes is one for the native engines, but float64 at 2^14 samples: hipFFT engine by choice;
    # the walker itself checks that each synthetic table comes out native / on the hipFFT engine as it was built to)
    assert rec["plans_on_native_engines"] - rec["synthetic_on_native"] == 864 - 12 * 4
    assert rec["synthetic_on_native"] >= syn["synthetic_on_native_at_least"] > 0
    # degenerate band parameters (sigma / p_re of 0, negative, NaN, inf; NaN p_im / omega / amp; shift index outside [0, n)):
    # seventeen tables per plan, each refused with QI_ERR_ARG while the previous table stays usable
    assert rec["degenerate_tables_refused"] >= 17 and rec["degenerate_tables_refused"] % 17 == 0
