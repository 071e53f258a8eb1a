"""Host sanitizer walk of the STFT segment-range entry points (CPU only): the library's host code under AddressSanitizer +
UBSan with the stand-in HIP runtime of tests/sanitize, driven by a stand-alone program (tests/sanitize_stream/walk_stream.cpp)
over every item of four records, both precisions, panels and no panels, several pooling factors, and every single-fault
refusal.  Needs hipcc; shares the library objects of tests/test_host_sanitize.py's build.  A GPU is neither needed nor used."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "sanitize_stream")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="the host sanitizer build needs hipcc")
def test_range_entry_points_under_asan_ubsan():
    make = subprocess.run(["make", "-C", HERE, f"-j{min(8, os.cpu_count() or 1)}", f"HIPCC={HIPCC}"], capture_output=True, text=True, timeout=1200)
    assert make.returncode == 0, make.stdout[-2000:] + make.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "sanitize", "_build", "walk_stream")], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr and "LeakSanitizer" not in run.stderr
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    assert rec["ok"] and rec["accepted"] >= 100 and rec["refused"] >= 8 * rec["accepted"] // 2
