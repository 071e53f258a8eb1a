"""Case table of the stream-order tests of include/qi_adaptive.h (a plain helper module: imports on the CPU, builds its
closures on the GPU), in the shape of tests/beam_stream_cases.py, with the helpers of tests/stream_cases.py.

One case for qi_csd_whiten (float32, with info) and one per path of qi_beam_capon: every matrix its own band in float64 with
the power alone, and a host band table with both peak outputs in float32.  The delayed producer's tensor is the matrix stack,
resp. the whitener stack, as interleaved (re, im) values.  The matrices are Z Z^H / K + I of stream_cases.record_pair's noise
(K = 2 SENSORS columns): positive definite, so that both A and B factor; the whitener stacks are capon_cases.whiten of them.
tests/test_capon_cpu.py holds the table against the header; tests/test_gpu_header_streams.py runs each case behind the
delayed producer of tests/stream_order.py.  All are asynchronous: the header promises no host synchronisation, the
frequencies and the band offsets ride in kernel arguments.  The first output, the whitener or the power, always differs
between the two record sets; `info` is 0 on both and a band's peak index may coincide.
"""
import functools

import numpy as np

import capon_cases as cpc
import stream_cases as sc
from stream_table import Built, Table

# (no plans: every case is plan-less; output 1 of whiten-info is `info`: both record sets factor)
TABLE = Table("qi_adaptive.h", complex_input=True, power="first", finite=True, zero_outputs={"whiten-info": 1})
_case = TABLE.case
SENSORS = 5  # one ragged tile
MATRICES, GRID = 33, 300
LOADING = 1e-2


def definite_pair(dtype, salt):
    """Two stacks [MATRICES, SENSORS, SENSORS] complex128 of positive definite matrices."""
    out = []
    for z in sc.record_pair((MATRICES, SENSORS, 2 * SENSORS, 2), "float64", salt):
        z = z[..., 0] + 1j * z[..., 1]
        s = z @ np.conj(np.swapaxes(z, 1, 2)) / (2 * SENSORS) + np.eye(SENSORS)
        out.append(0.5 * (s + np.conj(np.swapaxes(s, 1, 2))))
    return out


def interleaved(stack, dtype):
    """[..., 2] (re, im) values of `dtype`: what the stream tests upload and view as complex."""
    return np.ascontiguousarray(np.stack([stack.real, stack.imag], axis=-1).astype(dtype))


def _build_whiten(dtype):
    """Whitening factors of MATRICES positive definite matrices [SENSORS x SENSORS], with info."""
    torch, _lib, lib, dev = sc._gpu()
    a, b = (interleaved(s, dtype) for s in definite_pair(dtype, (47, 0)))
    rdtype = torch.float64 if dtype == "float64" else torch.float32
    cdtype = torch.complex128 if dtype == "float64" else torch.complex64
    code = _lib.dtype_code(rdtype)

    def op(x):
        whitener = torch.view_as_complex(sc._full(torch, (MATRICES, SENSORS, SENSORS, 2), rdtype, dev))
        info = torch.full((MATRICES,), -1, dtype=torch.int32, device=dev)
        _lib.call(lib.qi_csd_whiten, dev, code, dev.index, _lib.ptr(x), SENSORS, MATRICES, LOADING, _lib.ptr(whitener), _lib.ptr(info))
        assert whitener.dtype == cdtype
        return whitener, info

    return Built(op, a, b, "no host table")


def _build_capon(dtype, bands, peaks):
    """Capon power of MATRICES whiteners [SENSORS x SENSORS] over GRID delay sets."""
    torch, _lib, lib, dev = sc._gpu()
    a, b = (interleaved(cpc.whiten(s, LOADING), dtype) for s in definite_pair(dtype, (47, 1 + int(peaks))))
    rdtype = torch.float64 if dtype == "float64" else torch.float32
    code = _lib.dtype_code(rdtype)
    nb = MATRICES if bands is None else len(bands) - 1
    nbytes = int(lib.qi_beam_capon_scratch_bytes(code, SENSORS, MATRICES, GRID, nb))
    f_host, f_ptr = _lib.darr(np.linspace(1.0, 200.0, MATRICES))
    b_host, b_ptr = (None, None) if bands is None else _lib.iarr(bands)
    tau = torch.from_numpy(np.random.default_rng(47).uniform(-0.15, 0.15, (GRID, SENSORS))).to(dev)

    def op(x):
        power = sc._full(torch, (nb, GRID), rdtype, dev)
        index = torch.full((nb,), -1, dtype=torch.int64, device=dev) if peaks else None
        value = sc._full(torch, (nb,), rdtype, dev) if peaks else None
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_beam_capon, dev, code, dev.index, _lib.ptr(x), SENSORS, MATRICES, f_ptr, _lib.ptr(tau), GRID, b_ptr, nb,
                  _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)
        return (power, index, value) if peaks else (power,)

    return Built(op, a, b, f"{len(f_host)} host frequencies" + ("" if b_host is None else f", {len(b_host)} host offsets"))


_case("whiten-info", ("qi_csd_whiten",), functools.partial(_build_whiten, "float32"))
_case("capon-bins", ("qi_beam_capon",), functools.partial(_build_capon, "float64", None, False))
_case("capon-bands-peaks", ("qi_beam_capon",), functools.partial(_build_capon, "float32", (0, 3, 4, 33), True))
