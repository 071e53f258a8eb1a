"""Case table of the stream-order tests of include/qi_steer.h (a plain helper module: imports on the CPU, builds its closures
on the GPU), in the shape of tests/subspace_stream_cases.py, with the helpers of tests/stream_cases.py.

qi_beam_weights: MVDR weights in float32, where the delayed producer's tensor is the whitener stack, and Bartlett weights in
float64, where it is the delay table -- the call's one device input.  qi_beam_steer in both precisions with 17 beams (a
second beam tile): the producer's tensor is the panel, the weights are fixed.  Complex tensors are uploaded as interleaved
(re, im) values.  The matrices are adaptive_stream_cases.definite_pair's; the whitener stacks are capon_cases.whiten of them.
tests/test_steer_cpu.py holds the table against the header; tests/test_gpu_header_streams.py runs each case behind the delayed
producer of tests/stream_order.py.  All are asynchronous: the header promises no host synchronisation, the frequencies
ride in kernel arguments.  Each case has one output: it differs between the two record sets, is finite and holds no FILL.
"""
import functools

import numpy as np

import adaptive_stream_cases as asc
import capon_cases as cpc
import stream_cases as sc
from stream_table import Built, Table

TABLE = Table("qi_steer.h", power="every", finite=True, no_fill=True)  # (no plans: every case is plan-less)
_case = TABLE.case
SENSORS, MATRICES, LOADING = asc.SENSORS, asc.MATRICES, asc.LOADING
BEAMS = 17  # a second beam tile
TIMES = 300  # a third chunk of time
definite_pair, interleaved = asc.definite_pair, asc.interleaved


def _types(torch, dtype):
    return (torch.float64, torch.complex128) if dtype == "float64" else (torch.float32, torch.complex64)


def _build_weights(dtype, capon):
    """Weights of MATRICES bins over BEAMS delay rows: MVDR from whitener stacks (the producer's tensor), or Bartlett's, where the
    producer's tensor is the delay table [BEAMS, SENSORS] of doubles."""
    torch, _lib, lib, dev = sc._gpu()
    rdtype, _ = _types(torch, dtype)
    code = _lib.dtype_code(rdtype)
    rng = np.random.default_rng(59)
    if capon:
        a, b = (interleaved(cpc.whiten(s, LOADING), dtype) for s in definite_pair(dtype, (59, 0)))
        tau = torch.from_numpy(rng.uniform(-0.15, 0.15, (BEAMS, SENSORS))).to(dev)
    else:
        a, b = (np.ascontiguousarray(rng.uniform(-0.15, 0.15, (BEAMS, SENSORS))) for _ in range(2))
    nbytes = int(lib.qi_beam_weights_scratch_bytes(code, SENSORS, MATRICES, BEAMS))
    f_host, f_ptr = _lib.darr(np.linspace(1.0, 200.0, MATRICES))

    def op(x):
        weights = sc._full(torch, (MATRICES, BEAMS, SENSORS, 2), rdtype, dev)
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_beam_weights, dev, code, dev.index, _lib.ptr(x) if capon else None, SENSORS, MATRICES, f_ptr,
                  _lib.ptr(tau) if capon else _lib.ptr(x), BEAMS, _lib.ptr(weights), _lib.ptr(scratch), nbytes)
        return (weights,)

    return Built(op, a, b, f"{len(f_host)} host frequencies")


def _build_steer(dtype):
    """BEAMS beams of a panel [SENSORS, MATRICES, TIMES] (the producer's tensor) with fixed weights."""
    torch, _lib, lib, dev = sc._gpu()
    rdtype, _ = _types(torch, dtype)
    code = _lib.dtype_code(rdtype)
    a, b = sc.record_pair((SENSORS, MATRICES, TIMES, 2), dtype, (59, 3))
    w = torch.from_numpy(sc.noise((59, 4), (MATRICES, BEAMS, SENSORS, 2), dtype)).to(dev)

    def op(x):
        out = sc._full(torch, (BEAMS, MATRICES, TIMES, 2), rdtype, dev)
        _lib.call(lib.qi_beam_steer, dev, code, dev.index, _lib.ptr(x), SENSORS, MATRICES, TIMES, _lib.ptr(w), BEAMS, _lib.ptr(out))
        return (out,)

    return Built(op, a, b, "no host table")


_case("weights-capon", ("qi_beam_weights",), functools.partial(_build_weights, "float32", True))
_case("weights-bartlett", ("qi_beam_weights",), functools.partial(_build_weights, "float64", False))
_case("steer-f32", ("qi_beam_steer",), functools.partial(_build_steer, "float32"))
_case("steer-f64", ("qi_beam_steer",), functools.partial(_build_steer, "float64"))
