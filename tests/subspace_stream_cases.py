"""Case table of the stream-order tests of include/qi_subspace.h (a plain helper module: imports on the CPU, builds its
closures on the GPU), in the shape of tests/adaptive_stream_cases.py, with the helpers of tests/stream_cases.py.

One case for qi_csd_eigh (float32, with info) and one per path of qi_beam_music: every matrix its own band in float64 with
the power alone, and a host band table with both peak outputs in float32.  The delayed producer's tensor is the matrix stack,
resp. the eigenvector stack, as interleaved (re, im) values.  The matrices are adaptive_stream_cases.definite_pair's; the
eigenvector stacks are music_cases.eigh64 of them.  tests/test_music_cpu.py holds the table against the header;
tests/test_gpu_header_streams.py runs each case behind the delayed producer of tests/stream_order.py.  All are
asynchronous: the header promises no host synchronisation, the frequencies and the band offsets ride in kernel arguments.
The first output, the eigenvalues or the power, always differs between the two record sets; `info` is 0 on both and a
band's peak index may coincide.
"""
import functools

import numpy as np

import adaptive_stream_cases as asc
import music_cases as mc
import stream_cases as sc
from stream_table import Built, Table

# (no plans: every case is plan-less; output 2 of eigh-info is `info`: both record sets converge)
TABLE = Table("qi_subspace.h", complex_input=True, power="first", finite=True, zero_outputs={"eigh-info": 2})
_case = TABLE.case
SENSORS, MATRICES, GRID = asc.SENSORS, asc.MATRICES, asc.GRID
SOURCES = 2
definite_pair, interleaved = asc.definite_pair, asc.interleaved


def _build_eigh(dtype):
    """Eigenpairs of MATRICES positive definite matrices [SENSORS x SENSORS], with info."""
    torch, _lib, lib, dev = sc._gpu()
    a, b = (interleaved(s, dtype) for s in definite_pair(dtype, (53, 0)))
    rdtype = torch.float64 if dtype == "float64" else torch.float32
    cdtype = torch.complex128 if dtype == "float64" else torch.complex64
    code = _lib.dtype_code(rdtype)

    def op(x):
        values = sc._full(torch, (MATRICES, SENSORS), rdtype, dev)
        vectors = torch.view_as_complex(sc._full(torch, (MATRICES, SENSORS, SENSORS, 2), rdtype, dev))
        info = torch.full((MATRICES,), -1, dtype=torch.int32, device=dev)
        _lib.call(lib.qi_csd_eigh, dev, code, dev.index, _lib.ptr(x), SENSORS, MATRICES, _lib.ptr(values), _lib.ptr(vectors), _lib.ptr(info))
        assert vectors.dtype == cdtype
        return values, vectors, info

    return Built(op, a, b, "no host table")


def _build_music(dtype, bands, peaks):
    """MUSIC power of MATRICES eigenvector stacks [SENSORS x SENSORS] over GRID delay sets."""
    torch, _lib, lib, dev = sc._gpu()
    a, b = (interleaved(mc.eigh64(s)[1], dtype) for s in definite_pair(dtype, (53, 1 + int(peaks))))
    rdtype = torch.float64 if dtype == "float64" else torch.float32
    code = _lib.dtype_code(rdtype)
    nb = MATRICES if bands is None else len(bands) - 1
    nbytes = int(lib.qi_beam_music_scratch_bytes(code, SENSORS, MATRICES, GRID, nb))
    f_host, f_ptr = _lib.darr(np.linspace(1.0, 200.0, MATRICES))
    b_host, b_ptr = (None, None) if bands is None else _lib.iarr(bands)
    tau = torch.from_numpy(np.random.default_rng(53).uniform(-0.15, 0.15, (GRID, SENSORS))).to(dev)

    def op(x):
        power = sc._full(torch, (nb, GRID), rdtype, dev)
        index = torch.full((nb,), -1, dtype=torch.int64, device=dev) if peaks else None
        value = sc._full(torch, (nb,), rdtype, dev) if peaks else None
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_beam_music, dev, code, dev.index, _lib.ptr(x), SENSORS, MATRICES, SOURCES, f_ptr, _lib.ptr(tau), GRID, b_ptr, nb,
                  _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)
        return (power, index, value) if peaks else (power,)

    return Built(op, a, b, f"{len(f_host)} host frequencies" + ("" if b_host is None else f", {len(b_host)} host offsets"))


_case("eigh-info", ("qi_csd_eigh",), functools.partial(_build_eigh, "float32"))
_case("music-bins", ("qi_beam_music",), functools.partial(_build_music, "float64", None, False))
_case("music-bands-peaks", ("qi_beam_music",), functools.partial(_build_music, "float32", (0, 3, 4, 33), True))
