"""Host thread walk (CPU only): the library's host code under ThreadSanitizer with the stand-in HIP runtime of tests/sanitize,
driven by a stand-alone program (tests/sanitize_threads/walk_threads.cpp) from four threads at once: plans of their own on the
five layouts of stream_cases.ENGINES, and the plan-less calls that share process-wide state (the hipFFT cache and its work
areas, the strip partials per stream, the twiddle and LDS-limit maps), with the error text read back per thread.  Needs hipcc;
its objects are its own (ThreadSanitizer does not mix with AddressSanitizer), under tests/sanitize/_build/tsan/.  A GPU is
neither needed nor used."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "sanitize_threads")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
THREADS, LOOPS = 4, 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="the host sanitizer build needs hipcc")
def test_host_code_under_tsan_from_four_threads():
    make = subprocess.run(["make", "-C", HERE, f"-j{min(8, os.cpu_count() or 1)}", f"HIPCC={HIPCC}"], capture_output=True, text=True, timeout=1200)
    assert make.returncode == 0, make.stdout[-2000:] + make.stderr[-4000:]
    build = os.path.join(ROOT, "tests", "sanitize", "_build", "tsan")
    tables = os.path.join(build, "engines.bin")
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sanitize", "gen_tables.py"), "--engines", tables],
                         capture_output=True, text=True, timeout=600)
    assert gen.returncode == 0, gen.stderr[-3000:]
    made = json.loads(gen.stdout.strip().splitlines()[-1])
    assert made["layouts"] == [[dtype, n] for dtype, n, _ in sc.ENGINES.values()] and made["records"] == list(sc.RECORD_COUNTS)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1")
    run = subprocess.run([os.path.join(build, "walk_threads"), tables], capture_output=True, text=True, timeout=1500, env=env)
    assert "WARNING: ThreadSanitizer" not in run.stderr, run.stderr[:6000]
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-6000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    per_thread = THREADS * LOOPS
    assert rec["ok"] and rec["threads"] == THREADS and rec["loops"] == LOOPS and rec["layouts"] == len(sc.ENGINES) == 5
    # per thread and loop: a plan per layout and record count, six transform calls on each (panels, reductions only)
    assert rec["plans"] == per_thread * len(sc.ENGINES) * len(sc.RECORD_COUNTS) and rec["plan_calls"] == 6 * rec["plans"]
    # walk_stft's seven calls on five geometries (its three, a fused nfft of the thread's own, a hipFFT length of its own) x 2 precisions
    assert rec["stft_calls"] == per_thread * 5 * 2 * 7
    # walk_records' cases (tests/test_host_sanitize.py has the sum)
    assert rec["record_calls"] == per_thread * (2 * 10 + 3 + (8 + 9 + 9 + 15 + 7 + 10 + 13))
    # qi_shannon_fft, qi_csd fused and hipFFT, qi_cross_spectra twice; qi_pool_strip and its statistics on two streams -- x 2 precisions
    assert rec["fft_calls"] == per_thread * 2 * 5 and rec["strip_calls"] == per_thread * 2 * 2 * 2
    assert rec["own_errors"] == per_thread  # every refusal read back as the thread's own text
    assert rec["kernel_launches"] > rec["plan_calls"] and rec["shared_fft_plans"] > 0 and rec["fft_handles_left"] == 0
