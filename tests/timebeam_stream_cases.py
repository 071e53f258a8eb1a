"""Case table of the stream-order tests of include/qi_timebeam.h (a plain helper module: imports on the CPU, builds its
closures on the GPU), in the shape of tests/band_stream_cases.py, with the helpers of tests/stream_cases.py.

qi_time_beam_power on float64 records [RECORDS, SAMPLES] (the producer's tensor) with windows summed from per-hop sums -- two
launches with the scratch between them -- giving the mean square of the beam and the peak's value; qi_time_beam_traces on
float32 records, one launch.  The tables and the bank are on the device before the closure is called.
tests/test_timebeam_cpu.py holds the table against the header; tests/test_gpu_timebeam.py runs each case behind the delayed
producer of tests/stream_order.py.  Both are asynchronous: the header promises no host synchronisation.  Every output
differs between the two record sets, is finite and holds no FILL.
"""
import functools

import numpy as np

import stream_cases as sc
import timebeam_cases as tb
from stream_table import Built, Table

TABLE = Table("qi_timebeam.h", power="every", finite=True, no_fill=True)  # (no plans: every case is plan-less)
_case = TABLE.case
RECORDS, SAMPLES, ROWS = 5, 3000, 33  # one ragged chunk, three row blocks
WIN, HOP = 512, 256                   # a hop of one chunk that divides the window
PHASES, TAPS, REACH = 64, 8, 20


def _tables(torch, dev, dtype):
    rng = np.random.default_rng([41, ROWS])
    shift = rng.integers(-REACH, REACH + 1, (ROWS, RECORDS)).astype(np.int32)
    phase = rng.integers(0, PHASES, (ROWS, RECORDS)).astype(np.int32)
    taps = tb.bank(PHASES, TAPS).astype(dtype)
    return [torch.from_numpy(a).to(dev) for a in (shift, phase, taps)]


def _build(traces):
    torch, _lib, lib, dev = sc._gpu()
    name = "float32" if traces else "float64"
    a, b = sc.record_pair((RECORDS, SAMPLES), name, (83, int(traces)))
    tdtype = torch.float32 if traces else torch.float64
    code = _lib.dtype_code(tdtype)
    shift, phase, taps = _tables(torch, dev, name)
    torch.cuda.synchronize()
    nwin = tb.windows(SAMPLES, WIN, HOP)
    nbytes = 0 if traces else int(lib.qi_time_beam_power_scratch_bytes(code, RECORDS, SAMPLES, PHASES, TAPS, ROWS, WIN, HOP, REACH))
    assert nbytes >= 0

    def op(x):
        if traces:
            out = sc._full(torch, (ROWS, SAMPLES), tdtype, dev)
            _lib.call(lib.qi_time_beam_traces, dev, code, dev.index, _lib.ptr(x), RECORDS, SAMPLES, _lib.ptr(taps), PHASES, TAPS,
                      _lib.ptr(shift), _lib.ptr(phase), ROWS, REACH, _lib.ptr(out))
            return (out,)
        power, value = sc._full(torch, (nwin, ROWS), tdtype, dev), sc._full(torch, (nwin,), tdtype, dev)
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_time_beam_power, dev, code, dev.index, _lib.ptr(x), RECORDS, SAMPLES, _lib.ptr(taps), PHASES, TAPS,
                  _lib.ptr(shift), _lib.ptr(phase), ROWS, REACH, WIN, HOP, 0, _lib.ptr(power), None, _lib.ptr(value), _lib.ptr(scratch), nbytes)
        return power, value

    return Built(op, a, b, f"time beam {'traces' if traces else 'power'}: {ROWS} rows, {nwin} windows, {nbytes} bytes of scratch")


_case("time_beam_power-f64-hop-sums", ("qi_time_beam_power",), functools.partial(_build, False))
_case("time_beam_traces-f32", ("qi_time_beam_traces",), functools.partial(_build, True))
