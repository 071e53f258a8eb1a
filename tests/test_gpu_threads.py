"""Several host threads inside the library at once (-m gpu).

`_lib.load()` is a ctypes.CDLL, which releases the GIL inside every call, so Python threads really run in libqi_tfr.so at the
same time.  include/qi_tfr.h allows it for the plan-less entry points (each thread on its own stream and buffers) and gives a
plan to one thread and stream at a time; what the threads then share is what the library keeps for the process: the hipFFT
cache of the plan-less entry points with its work area per stream, the strip partials per (device, stream), the twiddle and
LDS-limit maps, and -- per thread by design -- the error text.  tests/test_host_threads_sanitize.py holds that host code under
ThreadSanitizer on the CPU; here the same calls run on the device and every output is compared, bit for bit (same_bits), with
the result of the same call made alone on the default stream.

The common shape (run_threads): every thread calls torch.cuda.set_device(0) and works under its own torch.cuda.Stream on its
own instance of a case of tests/stream_cases.py or tests/array_stream_cases.py (a closure makes its outputs, an instance is
never shared); everything cached -- the cases, their serial results, the delay chain -- is made before the threads start, and
every buffer exists and holds legal records by then.  A barrier releases the threads together, and each thread's stream first
waits for one gate event behind Delay.queue(FLOOR_MS), as tests/stream_order.py's released_together does, so the queued
work is released together on the device as well.  A thread makes CALLS calls, alternating the record sets A and B, keeps a copy
of every call's outputs and then synchronises its own stream only; what a thread raises is raised again in the main thread.
Nothing is sampled: every output of every call is compared.

As in the two-stream tests, whether two calls really meet -- on the host or on the device -- is up to the schedulers: a pass
can be luck, a failure cannot be.  These are loops of a few calls at the shapes of the case table, not repetition until
something breaks.  The thread and call counts and the number of call pairs of different threads whose host intervals overlapped
go to profiles/host_threads.txt when every test here has run: a record, not an assertion."""
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

import array_stream_cases as asc
import stream_cases as sc
import stream_order as so
from stream_order import FLOOR_MS, delay, keep, mismatches, same_bits

from quantum_inferno_amd import _lib, cwt_atoms, engine, styx_cwt, styx_stx

pytestmark = pytest.mark.gpu

ROOT = sc.ROOT
CALLS = 8
THREADS = 4
LOG_PATH = os.environ.get("QI_HOST_THREADS_LOG") or os.path.join(ROOT, "profiles", "host_threads.txt")
_LOG = {}
PLAN_LESS = [(table, cid) for table in (sc.TABLE, asc.TABLE) for cid in table.plan_less_ids()]
ONE_PLAN_KEYS = ("f32_n16384", "f64_n32768", "f32_n2048", "f32_n3000")
OTHER_TESTS = ("mixed_shared_state", "one_plan_each", "wrappers_from_threads", "wrapper_on_two_streams", "fft_work_area")


@pytest.fixture(scope="module", autouse=True)
def _plans_and_log():
    yield
    torch.cuda.synchronize()
    engine.clear_plans()
    sc.close_plans()
    so.clear_cases()
    expected = [f"same_op[{cid}]" for _, cid in PLAN_LESS] + list(OTHER_TESTS)
    if all(name in _LOG for name in expected):  # (a partial run does not overwrite the record of a whole one)
        lines = ["host threads: several Python threads inside libqi_tfr.so at once (tests/test_gpu_threads.py)",
                 f"per thread {CALLS} calls under its own stream, released by a barrier and one gate event behind a {FLOOR_MS:g} ms delay",
                 "overlapping pairs: pairs of calls of DIFFERENT threads whose host intervals (perf_counter around the call) overlapped",
                 "", f"{'test':52s} {'threads':>7s} {'calls':>6s} {'overlapping pairs':>18s}"]
        for name in expected:
            r = _LOG[name]
            lines.append(f"{name:52s} {r['threads']:7d} {r['calls']:6d} {r['overlaps']:18d}")
        lines += [""] + [f"{name}: {_LOG[name]['note']}" for name in expected if _LOG[name].get("note")]
        with open(LOG_PATH, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def overlapping_pairs(spans):
    """Calls of different threads whose host intervals overlapped; spans: per thread a list of (start, end)."""
    count = 0
    for p in range(len(spans)):
        for q in range(p + 1, len(spans)):
            count += sum(1 for a0, a1 in spans[p] for b0, b1 in spans[q] if a0 < b1 and b0 < a1)
    return count


def run_threads(name, jobs, extras=(), calls=CALLS, keeper=keep, compare=mismatches):
    """jobs: per thread (call, expected): call(i) makes the thread's i-th call under the thread's stream and returns its outputs,
    of which `keeper` keeps a copy; expected(i) is the serial result they must equal (`compare`: the outputs that differ).
    extras: functions run meanwhile, each in a thread and under a stream of its own."""
    count = len(jobs) + len(extras)
    streams = [torch.cuda.Stream() for _ in range(count)]
    s0 = torch.cuda.Stream()
    kept, spans, raised = [[] for _ in jobs], [[] for _ in range(count)], [None] * count
    barrier = threading.Barrier(count)
    d = delay()
    torch.cuda.synchronize()
    gate = torch.cuda.Event()
    with torch.cuda.stream(s0):
        d.queue(FLOOR_MS)
        gate.record(s0)

    def body(k):
        try:
            torch.cuda.set_device(0)
            s = streams[k]
            barrier.wait(timeout=120)
            with torch.cuda.stream(s):
                s.wait_event(gate)
                if k >= len(jobs):
                    t0 = time.perf_counter()
                    extras[k - len(jobs)]()
                    spans[k].append((t0, time.perf_counter()))
                else:
                    for i in range(calls):
                        t0 = time.perf_counter()
                        out = jobs[k][0](i)
                        spans[k].append((t0, time.perf_counter()))
                        kept[k].append(keeper(out))
            s.synchronize()  # its own stream only
        except BaseException as e:  # noqa: BLE001 (raised again in the main thread)
            raised[k] = e
            barrier.abort()

    threads = [threading.Thread(target=body, args=(k,)) for k in range(count)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    s0.synchronize()
    for e in raised:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    assert not any(raised), raised
    _LOG[name] = dict(threads=count, calls=sum(len(s) for s in spans), overlaps=overlapping_pairs(spans))
    for k, (_, expected) in enumerate(jobs):
        assert len(kept[k]) == calls
        for i, got in enumerate(kept[k]):
            bad = compare(got, expected(i))
            assert not bad, f"{name}: thread {k}, call {i}: outputs {bad} differ from the result of the same call made alone"


def case_job(op, a_dev, b_dev, on_a, on_b):
    """Call i of a thread: the op on the records A, B, A, ..."""
    return (lambda i: op(b_dev if i % 2 else a_dev)), (lambda i: on_b if i % 2 else on_a)


def reference(table, cid):
    """(result on A, result on B) of the case's shared instance, alone on the default stream."""
    want, stale, _ = so.serial(table, cid)
    return stale, want


def instance(table, cid):
    """A new instance of a case: (op, A on the device, B on the device)."""
    b = table.by_id(cid).build()
    a_dev, b_dev = (torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in (b.a, b.b))
    return b.op, a_dev, b_dev


@pytest.mark.parametrize("table,cid", PLAN_LESS, ids=[cid for _, cid in PLAN_LESS])
def test_threads_same_op(table, cid):
    """Four threads, four instances of one plan-less case at the same shape."""
    assert table.by_id(cid).engine is None
    refs = reference(table, cid)
    jobs = [case_job(*instance(table, cid), *refs) for _ in range(THREADS)]
    run_threads(f"same_op[{cid}]", jobs)


def test_threads_mixed_shared_state():
    """One thread per case of stream_cases.SHARED_STATE, all at once: the hipFFT cache meets four transform shapes and the strip
    partials from six threads (below the 16 CPUs a run may use)."""
    assert len(sc.SHARED_STATE) == 6
    jobs = [case_job(*instance(sc.TABLE, cid), *reference(sc.TABLE, cid)) for cid in sc.SHARED_STATE]
    run_threads("mixed_shared_state", jobs)


def test_threads_one_plan_each():
    """One thread per engine key, each on that key's plan (stream_cases.engine_plan hands out one plan per key, so one thread
    per key keeps to the header's rule), running both transforms with every output; a fifth thread creates, sets up and closes
    a further small plan three times meanwhile (table uploads, hipMalloc and hipFree, the device synchronisation of
    qi_plan_destroy)."""
    jobs = []
    for key in ONE_PLAN_KEYS:
        cid = f"cwt_stx-{key}-all-r1"
        assert sc.TABLE.by_id(cid).engine == key
        b, a_dev, b_dev = so.built(sc.TABLE, cid)
        jobs.append(case_job(b.op, a_dev, b_dev, *reference(sc.TABLE, cid)))
    n = 1 << 10
    nb = len(engine.scales.log_frequency_hz_from_fft_points(sc.FS, n, sc.ORDER))
    ws = engine.TfrPlan.workspace_for(n, nb, torch.float32, 1)

    def churn():
        for _ in range(3):
            plan = engine.TfrPlan(n, torch.float32, None, ws)
            plan.set_styx_bank(sc.ORDER, sc.FS)
            plan.set_stx_bands(sc.ORDER, sc.FS)
            plan.close()

    run_threads("one_plan_each", jobs, extras=(churn,))


# ---- the reference-signature wrappers and their plan cache (engine.borrowed_plan) -------------------------------------------
# (samples, order) per thread: the first two share every key; with three wrappers that is twelve keys against _MAX_PLANS = 3
WRAPPER_SHAPES = ((2048, 3), (2048, 3), (2048, 6), (3000, 3), (16384, 3))


def wrapper_calls(order):
    """The three wrappers as op(x) -> tuple of results, in the order a thread cycles through them."""
    return (lambda x: (styx_cwt.cwt_complex_any_scale_pow2(order, x, sc.FS)[2],),
            lambda x: (styx_stx.stx_complex_any_scale_pow2(order, x, sc.FS)[2],),
            lambda x: cwt_atoms.cwt_chirp_from_sig(x, sc.FS, order)[:2])


def numpy_mismatches(got, want):
    assert len(got) == len(want)
    return [k for k, (g, w) in enumerate(zip(got, want)) if not same_bits(torch.from_numpy(np.ascontiguousarray(g)), torch.from_numpy(np.ascontiguousarray(w)))]


def test_wrappers_from_threads():
    """cwt_complex_any_scale_pow2, stx_complex_any_scale_pow2 and cwt_chirp_from_sig with NumPy records from five threads: two
    on the same keys (2048 samples, order 3, float32: a second concurrent caller of a key gets a plan of its own), one each at
    2048 samples and order 6, at 3000 and at 16384 samples -- twelve keys against _MAX_PLANS = 3, so plans are evicted while
    others run.  A thread cycles through the wrappers and alternates its records A and B; every result equals the one
    computed before on one thread, bit for bit, and the cache ends within its bound."""
    engine.clear_plans()
    jobs = []
    for n, order in WRAPPER_SHAPES:
        records = sc.record_pair((n,), "float32", (50, n, order))
        ops = wrapper_calls(order)
        alone = {(w, r): ops[w](records[r]) for w in range(3) for r in range(2)}
        assert all(numpy_mismatches(alone[(w, 0)], alone[(w, 1)]) for w in range(3)), "the records A and B give the same bits"
        # call i: wrapper i % 3 on the records i % 2 -- all six combinations within the eight calls
        jobs.append(((lambda i, ops=ops, records=records: ops[i % 3](records[i % 2])), (lambda i, alone=alone: alone[(i % 3, i % 2)])))
    engine.clear_plans()
    try:
        run_threads("wrappers_from_threads", jobs, keeper=lambda out: out, compare=numpy_mismatches)  # (NumPy results: the caller's own)
        with engine._PLANS_LOCK:
            idle = len(engine._PLANS)
        assert idle <= engine._MAX_PLANS, idle
        _LOG["wrappers_from_threads"]["note"] = f"{idle} idle plans in the cache at the end (_MAX_PLANS = {engine._MAX_PLANS})"
    finally:
        engine.clear_plans()


def test_wrapper_on_two_streams():
    """One thread, device tensors in, the same key on two streams: the call on s1 sits behind a delay, the call on s2 follows at
    once with no host wait in between -- both streams are released by the same gate, so without the cache's event the second
    call's launches would run in the plan's one scratch beside the first's.  Both results equal their serial results, and the
    second call returned before the gate had passed (`early`): the cache orders the streams on the device, the host never
    waits.  Sixteen records per call, so that a call's kernels last."""
    engine.clear_plans()
    n, order, records = 2048, 3, 16
    x1, x2 = (torch.from_numpy(r).cuda() for r in sc.record_pair((records, n), "float32", (51, n)))
    try:
        for w, op in enumerate(wrapper_calls(order)):
            want1, want2 = keep(op(x1)), keep(op(x2))  # (also: the key's plan is idle in the cache, last used on the default stream)
            assert mismatches(want1, want2)
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            torch.cuda.synchronize()
            gate = torch.cuda.Event()
            with torch.cuda.stream(s1):
                delay().queue(FLOOR_MS)
                gate.record(s1)
                got1 = keep(op(x1))
            with torch.cuda.stream(s2):
                s2.wait_event(gate)
                got2 = keep(op(x2))
                early = not gate.query()
            s1.synchronize()
            s2.synchronize()
            assert not mismatches(got1, want1), f"wrapper {w}: the call on s1 differs in {mismatches(got1, want1)}"
            assert not mismatches(got2, want2), f"wrapper {w}: the call on s2 differs in {mismatches(got2, want2)}"
            assert early, f"wrapper {w}: the second call returned after the gate had passed: it waited on the host"
        _LOG["wrapper_on_two_streams"] = dict(threads=1, calls=2 * 3, overlaps=0)
    finally:
        torch.cuda.synchronize()
        engine.clear_plans()


# ---- the shared hipFFT work areas grow under a queued transform (a child process: the cache starts empty) ---------------------
FFT_LOOP_N = 4999  # prime
FFT_GROW = ((1009, 503), (10007, 5003), (100003, 50021))  # (n, m) of qi_resample_fft, all prime: about tenfold each
FFT_LOOP_CALLS = 12


def _fft_child():
    """Thread 1 loops qi_shannon_fft at a prime length on stream s1 behind a delay; thread 2 makes the FIRST calls of
    qi_resample_fft at growing prime lengths on s2 -- each makes new hipFFT plans whose work size exceeds the areas the cache
    holds, so the areas of both streams are retired while s1's transforms are still queued.  Every result is compared with the
    same call made alone afterwards."""
    torch.cuda.set_device(0)
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    d = delay()
    records, code = 3, _lib.QI_F32
    x1 = torch.from_numpy(sc.noise(60, (records, FFT_LOOP_N), np.float32)).to(dev)
    xs = [torch.from_numpy(sc.noise((61, n), (records, n), np.float32)).to(dev) for n, _ in FFT_GROW]
    nf = FFT_LOOP_N // 2 + 1
    nbytes = int(lib.qi_shannon_scratch_bytes(code, records, FFT_LOOP_N))

    def shannon(x):
        spec = torch.full((records, nf), sc.FILL, dtype=torch.complex64, device=dev)
        angle, marginal = (torch.full((records, nf), sc.FILL, dtype=torch.float32, device=dev) for _ in range(2))
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.call(lib.qi_shannon_fft, dev, code, dev.index, _lib.ptr(x), records, FFT_LOOP_N, _lib.ptr(spec), _lib.ptr(angle),
                  _lib.ptr(marginal), _lib.ptr(scratch), nbytes)
        return spec, angle, marginal

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    looped, grown, raised, spans = [], [], [], [[], []]
    barrier = threading.Barrier(2)
    torch.cuda.synchronize()

    def loop():
        try:
            torch.cuda.set_device(0)
            barrier.wait(timeout=120)
            with torch.cuda.stream(s1):
                d.queue(10 * FLOOR_MS)
                for _ in range(FFT_LOOP_CALLS):
                    t0 = time.perf_counter()
                    out = shannon(x1)
                    spans[0].append((t0, time.perf_counter()))
                    looped.append(keep(out))
            s1.synchronize()
        except BaseException as e:  # noqa: BLE001
            raised.append(e)
            barrier.abort()

    def grow():
        try:
            torch.cuda.set_device(0)
            barrier.wait(timeout=120)
            with torch.cuda.stream(s2):
                for x, (_, m) in zip(xs, FFT_GROW):
                    t0 = time.perf_counter()
                    out = engine.fft_resample(x, m)
                    spans[1].append((t0, time.perf_counter()))
                    grown.append(keep((out,)))
            s2.synchronize()
        except BaseException as e:  # noqa: BLE001
            raised.append(e)
            barrier.abort()

    threads = [threading.Thread(target=loop), threading.Thread(target=grow)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if raised:
        raise raised[0]
    torch.cuda.synchronize()
    alone = keep(shannon(x1))
    bad = [("qi_shannon_fft", i, mismatches(got, alone)) for i, got in enumerate(looped) if mismatches(got, alone)]
    for k, (x, (n, m)) in enumerate(zip(xs, FFT_GROW)):
        want = keep((engine.fft_resample(x, m),))
        if mismatches(grown[k], want):
            bad.append(("qi_resample_fft", n, m))
    torch.cuda.synchronize()
    print(json.dumps({"ok": not bad, "mismatches": bad, "looped": len(looped), "grown": len(grown), "overlaps": overlapping_pairs(spans)}))


def test_fft_work_area_grows_under_a_queued_transform():
    """In one fresh child process (started beside this one, which has no work pending), so the library's hipFFT cache is empty:
    see _fft_child.  A prime length takes hipFFT's work area at any size.  For three float32 records on an MI355X
    hipfftMakePlanMany (the call FftCache::get sizes the areas with) and hipfftGetSize both gave, real-to-complex: 382 120 bytes
    at 4999 points (the looping thread), 56 984 at 1009, 1 059 368 at 10007 and 18 874 368 at 100003; complex-to-real: 28 456 at
    503, 382 216 at 5003 and 7 372 800 at 50021.  So the growing thread's second and third calls always outgrow every area made
    before them (its first does when it comes before the looping thread's plan), and the areas of both streams are retired
    twice at least while s1's transforms are queued.  As above, a pass can be luck (the retired areas stay allocated by design:
    a defect there is a stale or freed work area under a running transform), a failure cannot be."""
    torch.cuda.synchronize()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--fft-child"], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    assert rec["looped"] == FFT_LOOP_CALLS and rec["grown"] == len(FFT_GROW)
    assert rec["ok"], f"results that differ from the same call made alone: {rec['mismatches']}"
    _LOG["fft_work_area"] = dict(threads=2, calls=rec["looped"] + rec["grown"], overlaps=rec["overlaps"])


if __name__ == "__main__" and "--fft-child" in sys.argv:
    _fft_child()
