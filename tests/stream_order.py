"""The harness of the stream-order tests (a plain helper module, not collected; imports without a GPU, touches the device on
first use).  tests/test_gpu_streams.py, tests/test_gpu_header_streams.py and tests/test_gpu_threads.py run the cases of
TABLES with it.

A case runs on a side stream `s` whose input is still being written when the call is made:

    s:  [delay: a chain of in-place passes over a 256 MiB tensor] [op(A) ...] [x <- B] (written) [op(x) ...]

`x` holds record set A until the copy runs; the call on A in front keeps the op's own state busy (see behind_producer).  A
launch that is not ordered behind `s` reads A (or a buffer still holding FILL) and the result differs from the serial result
on B bit for bit; a call that waits on the host returns after `written` has completed, and `early` is false.  The delay is
sized per case: ten times the host time of the warm call on the default stream, at least FLOOR_MS; the chain is timed once
per session with events, never by the code under test.

All of that sees a misordered launch only if the default stream does not wait for `s`.  side_streams hands out streams of
which that has been shown, by a probe that involves no code of the library; no test takes a side stream of its own.  The
probe's verdicts, the measured times, the delays and whether `early` held go to profiles/stream_order.txt when every case of
every table has run (write_log).

A new header with entry points that take a `qi_stream`: a module with a stream_table.Table of its cases, listed in TABLES
here, and the census of that table against the header in the header's CPU test.
"""
import functools
import itertools
import math
import os
import time

import numpy as np
import torch

import adaptive_stream_cases
import array_stream_cases
import beam_stream_cases
import lag_stream_cases
import steer_stream_cases
import stream_cases as sc
import subspace_stream_cases
import window_stream_cases
from stream_table import ROOT

TABLES = (sc.TABLE,) + tuple(m.TABLE for m in (array_stream_cases, beam_stream_cases, adaptive_stream_cases, subspace_stream_cases,
                                               steer_stream_cases, window_stream_cases, lag_stream_cases))
FLOOR_MS = 20.0  # a short op's host time is microseconds: ten times that is timer noise, not a delay
MARGIN = 10      # delay / host time of the call: covers the jitter of the host's enqueue time
POOL = 32        # the streams PyTorch hands out in turn, per device and priority
MOST_STREAMS = 3  # the most side streams one test takes (released_together)
NO_SIDE_STREAM = "the default stream waited for the side stream: the harness cannot see a misordered launch here"
LOG_PATH = os.environ.get("QI_STREAM_ORDER_LOG") or os.path.join(ROOT, "profiles", "stream_order.txt")
LOG = {}  # (table name, case id) -> the case's row; "control", "probe"


class Delay:
    """Ordinary queued device work of a known duration: in-place passes over one large tensor, timed once with events."""

    def __init__(self):
        self.buf = torch.zeros(64 << 20, dtype=torch.int32, device="cuda")  # 256 MiB: a pass is hundreds of microseconds
        for _ in range(5):
            self.buf.add_(1)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.timed = 50
        start.record()
        for _ in range(self.timed):
            self.buf.add_(1)
        stop.record()
        stop.synchronize()
        self.pass_ms = start.elapsed_time(stop) / self.timed
        assert 0.01 < self.pass_ms < 50.0, self.pass_ms

    def passes(self, ms):
        return int(math.ceil(ms / self.pass_ms))

    def queue(self, ms):
        """On the current stream."""
        for _ in range(self.passes(ms)):
            self.buf.add_(1)


@functools.lru_cache(maxsize=None)
def delay():
    return Delay()


def delay_ms_for(host_seconds):
    return max(FLOOR_MS, MARGIN * host_seconds * 1e3)


# ---- side streams the default stream does not wait for -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _independent_streams():
    """The streams of PyTorch's pool, each probed once: a delay and an event are queued on the side stream, then one small
    kernel and an event on the default stream, which is waited for.  The side stream is independent if its own event is still
    pending then: the default stream's kernel ran beside, not behind, the delay.  -> an endless round of the independent ones."""
    d = delay()
    pool = list({s.cuda_stream: s for s in (torch.cuda.Stream() for _ in range(POOL))}.values())  # (each stream once)
    default = torch.cuda.default_stream()
    cell = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    verdicts = []
    for s in pool:
        side, main = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(s):
            d.queue(FLOOR_MS)
            side.record(s)
        with torch.cuda.stream(default):
            cell.add_(1)
            main.record(default)
        main.synchronize()
        verdicts.append(not side.query())
        s.synchronize()
    LOG["probe"] = verdicts
    free = [s for s, independent in zip(pool, verdicts) if independent]
    assert len(free) >= MOST_STREAMS, f"{NO_SIDE_STREAM} ({len(free)} of {len(pool)} pool streams are independent: {verdicts})"
    return itertools.cycle(free)


def side_streams(k):
    """k distinct side streams, each shown independent of the default stream; successive calls go round the independent ones."""
    assert 1 <= k <= MOST_STREAMS, k
    return [next(_independent_streams()) for _ in range(k)]


# ---- results, bit for bit ---------------------------------------------------------------------------------------------------------
def same_bits(x, y):
    """Equal as integers: equal NaN patterns count as equal, +0 and -0 do not."""
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    xr, yr = (torch.view_as_real(t) if t.is_complex() else t for t in (x, y))
    return torch.equal(xr.contiguous().view(torch.uint8), yr.contiguous().view(torch.uint8))


def mismatches(got, want):
    assert len(got) == len(want), (len(got), len(want))
    return [k for k, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]


def keep(outputs):
    """Copies on the current stream: the closures' kept buffers may be written again by the next call."""
    return tuple(t.clone() for t in outputs)


# ---- a table's cases: built once, run serially once ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(table, cid):
    """(Built, A on the device, B on the device) of a case, shared by every test that runs it."""
    b = table.by_id(cid).build()
    assert b.a.shape == b.b.shape and b.a.dtype == b.b.dtype and np.isfinite(b.a).all() and np.isfinite(b.b).all(), cid
    dev = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in (b.a, b.b)]
    if table.complex_input:  # uploaded as interleaved (re, im) values
        dev = [torch.view_as_complex(t) for t in dev]
    torch.cuda.synchronize()
    return b, dev[0], dev[1]


@functools.lru_cache(maxsize=None)
def serial(table, cid):
    """(want = op(B), stale = op(A), host seconds of the second, warm, call) on the default stream, held to what the table
    declares of its outputs."""
    b, a_dev, b_dev = built(table, cid)
    torch.cuda.synchronize()
    want = keep(b.op(b_dev))  # also the warm call: lazy hipFFT plans, per-stream buffers, the caching allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = b.op(a_dev)
    host = time.perf_counter() - t0  # the enqueue alone: nothing is synchronised
    stale = keep(out)
    torch.cuda.synchronize()
    differ = mismatches(stale, want)
    power = {"any": bool(differ), "first": 0 in differ, "every": differ == list(range(len(want)))}[table.power]
    assert power, f"{cid}: of the results on A and on B only outputs {differ} differ ({table.power} must): the case has no power"
    for t in want + stale:
        assert not table.finite or torch.isfinite(t).all(), cid
        assert not table.no_fill or not (t == sc.FILL).any(), cid
    if cid in table.zero_outputs:
        k = table.zero_outputs[cid]
        assert not want[k].any() and not stale[k].any(), f"{cid}: output {k} is not zero on both record sets"
    return want, stale, host


def clear_cases():
    """Forget the built cases and their serial results (a module's teardown, before the plans they run on are closed)."""
    serial.cache_clear()
    built.cache_clear()


def behind_producer(op, s, x, src, ms, before=None):
    """On stream `s`: the delay, x <- src, then op(x) while x is still unwritten -> (copies of the outputs, early, copies
    of the outputs of op(before)).  `before`: a buffer that already holds the other record set; the op runs on it first,
    behind the same delay, so that whatever the op keeps between calls (partial sums a memset clears, scratch, handles) is
    still in use by a queued call when the call under test is made -- a clear or a launch that leaves the stream then meets
    the earlier call's work instead of an idle device."""
    with torch.cuda.stream(s):
        delay().queue(ms)
        first = keep(op(before)) if before is not None else None
        x.copy_(src)
        written = torch.cuda.Event()
        written.record(s)
        got = op(x)
        early = not written.query()
        return keep(got), early, first


def ordered_behind_producer(table, cid):
    """The test of one case: its result behind the delayed producer equals the serial result on B bit for bit, differs from
    the stale one as the table's power rule says, and an asynchronous call returned before its input was written."""
    case = table.by_id(cid)
    b, a_dev, b_dev = built(table, cid)
    want, stale, host = serial(table, cid)
    ms = delay_ms_for(host)
    (s,) = side_streams(1)
    x = a_dev.clone()
    torch.cuda.synchronize()
    got, early, first = behind_producer(b.op, s, x, b_dev, ms, before=a_dev)
    s.synchronize()  # this stream only, never the device
    LOG[(table.name, cid)] = dict(asynchronous=case.asynchronous, host_ms=host * 1e3, delay_ms=ms, passes=delay().passes(ms), early=early, note=b.note)
    assert not mismatches(first, stale), f"{cid}: the call queued in front (on A) differs from its serial result in {mismatches(first, stale)}"
    bad = mismatches(got, want)
    assert not bad, f"{cid}: outputs {bad} differ from the serial result (equal to the stale one: {[k for k in bad if same_bits(got[k], stale[k])]})"
    if table.power == "first":
        assert mismatches(got, stale) == mismatches(want, stale)
    elif table.power == "every":
        assert mismatches(got, stale) == list(range(len(got)))
    if case.asynchronous:
        assert early, f"{cid}: the call returned after its input was written ({host * 1e3:.3f} ms warm, delay {ms:.1f} ms): it waited on the host"


def released_together(ops, inputs, wants, what):
    s0, s1, s2 = side_streams(3)
    torch.cuda.synchronize()
    gate = torch.cuda.Event()
    with torch.cuda.stream(s0):
        delay().queue(FLOOR_MS)
        gate.record(s0)
    results = []
    for s, op, x in zip((s1, s2), ops, inputs):
        with torch.cuda.stream(s):
            s.wait_event(gate)
            results.append(keep(op(x)))
    s1.synchronize()
    s2.synchronize()
    for k, (got, ref) in enumerate(zip(results, wants)):
        assert not mismatches(got, ref), f"{what}: stream {k + 1} differs in outputs {mismatches(got, ref)}"


# ---- the record ---------------------------------------------------------------------------------------------------------------------
def write_log():
    """profiles/stream_order.txt, once the probe, the control and every case of every table have run in this process (a
    partial run does not overwrite the record of a whole one): called by the teardown of each module that runs cases."""
    rows = [(f"{t.name}/{cid}", LOG.get((t.name, cid))) for t in TABLES for cid in t.ids()]
    if "probe" not in LOG or "control" not in LOG or any(r is None for _, r in rows):
        return
    d, probe = delay(), LOG["probe"]
    lines = [f"stream order: {len(rows)} cases of {len(TABLES)} tables ({', '.join(f'{t.header} {len(t.cases)}' for t in TABLES)}) behind a delayed producer",
             "(tests/stream_order.py; run by tests/test_gpu_streams.py and tests/test_gpu_header_streams.py)",
             f"delay chain: {d.timed} in-place passes over 256 MiB timed with events on the default stream: {d.pass_ms:.4f} ms per pass",
             f"delay = max({FLOOR_MS:g} ms, {MARGIN} x host time of the warm call on the default stream)",
             "", f"side streams: the {len(probe)} streams of PyTorch's pool in pool order; independent: the default stream ran a kernel to its end while a",
             f"{FLOOR_MS:g} ms delay was pending on the side stream.  {sum(probe)} of {len(probe)} are independent; the tests take those in turn.",
             *(" ".join(f"{k:2d}:{'independent' if probe[k] else 'WAITED':11s}" for k in range(row, min(row + 8, len(probe)))).rstrip()
               for row in range(0, len(probe), 8)),
             "", f"{'case':52s} {'async':>5s} {'host ms':>9s} {'delay ms':>9s} {'passes':>6s} {'early':>5s}"]
    for name, r in rows:
        lines.append(f"{name:52s} {str(r['asynchronous']):>5s} {r['host_ms']:9.3f} {r['delay_ms']:9.2f} {r['passes']:6d} {str(r['early']):>5s}")
    lines += ["", "notes of the builds (what each plan's own queries said):"] + sorted({r["note"] for _, r in rows if r["note"]})
    lines += ["", f"control: {LOG['control']}"]
    with open(LOG_PATH, "w") as fh:
        fh.write("\n".join(lines) + "\n")
