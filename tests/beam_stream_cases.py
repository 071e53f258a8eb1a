"""Case table of the stream-order tests of include/qi_beam.h (a plain helper module: imports on the CPU, builds its closures
on the GPU), in the shape of tests/array_stream_cases.py, with the helpers of tests/stream_cases.py.

One case per path of qi_beam_power: every matrix its own band with the power alone, and a host band table with the
semblance and both peak outputs.  The delayed producer's tensor is the matrix stack, viewed as complex.  tests/test_beam_cpu.py
holds the table against the header; tests/test_gpu_header_streams.py runs each case behind the delayed producer of
tests/stream_order.py.  Both are asynchronous: the header promises no host synchronisation, the frequencies and the band
offsets ride in kernel arguments.  Every output differs between the two record sets and is finite.
"""
import functools

import numpy as np

import stream_cases as sc
from stream_table import Built, Table

TABLE = Table("qi_beam.h", complex_input=True, power="every", finite=True)  # (no plans: every case is plan-less)
_case = TABLE.case
SENSORS = 5  # one ragged tile
MATRICES, GRID = 33, 300


def _build_beam(dtype, bands, normalize, peaks):
    """Steered power of MATRICES matrices [SENSORS x SENSORS] (noise, as interleaved (re, im) values with a non-zero mean:
    the traces are positive) over GRID delay sets."""
    torch, _lib, lib, dev = sc._gpu()
    a, b = sc.record_pair((MATRICES, SENSORS, SENSORS, 2), dtype, (43, int(normalize)))
    rdtype = torch.float64 if dtype == "float64" else torch.float32
    code = _lib.dtype_code(rdtype)
    nb = MATRICES if bands is None else len(bands) - 1
    nbytes = int(lib.qi_beam_power_scratch_bytes(code, SENSORS, MATRICES, GRID, nb))
    f_host, f_ptr = _lib.darr(np.linspace(1.0, 200.0, MATRICES))
    b_host, b_ptr = (None, None) if bands is None else _lib.iarr(bands)
    tau = torch.from_numpy(np.random.default_rng(43).uniform(-0.15, 0.15, (GRID, SENSORS))).to(dev)

    def op(x):
        power = sc._full(torch, (nb, GRID), rdtype, dev)
        index = torch.full((nb,), -1, dtype=torch.int64, device=dev) if peaks else None
        value = sc._full(torch, (nb,), rdtype, dev) if peaks else None
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_beam_power, dev, code, dev.index, _lib.ptr(x), SENSORS, MATRICES, f_ptr, _lib.ptr(tau), GRID, b_ptr, nb,
                  int(normalize), _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)
        return (power, index, value) if peaks else (power,)

    return Built(op, a, b, f"{len(f_host)} host frequencies" + ("" if b_host is None else f", {len(b_host)} host offsets"))


_case("beam-bins", ("qi_beam_power",), functools.partial(_build_beam, "float64", None, False, False))
_case("beam-bands-semblance-peaks", ("qi_beam_power",), functools.partial(_build_beam, "float32", (0, 3, 4, 33), True, True))
