"""Case table of the stream-order tests of include/qi_bands.h (a plain helper module: imports on the CPU, builds its closures
on the GPU), in the shape of tests/window_stream_cases.py, with the helpers of tests/stream_cases.py.

qi_cross_spectra_bands on a float64 panel [RECORDS, 7 bands, 300 columns] (the producer's tensor, as interleaved (re, im)
values), the bands 2 .. 4 with three different (terms, hop, stride): once the matrices alone with no weights, once the
coherence alone with host weights -- the matrices go through scratch.  tests/test_bands_cpu.py holds the table against the
header; tests/test_gpu_bands.py runs each case behind the delayed producer of tests/stream_order.py.  Both are
asynchronous: the header promises no host synchronisation, the host tables and weights ride in kernel arguments.  Each case
has one output: it differs between the two record sets, is finite and holds no FILL.
"""
import functools

import numpy as np

import stream_cases as sc
from stream_table import Built, Table

TABLE = Table("qi_bands.h", power="every", finite=True, no_fill=True)  # (no plans: every case is plan-less)
_case = TABLE.case
RECORDS = 5  # one ragged tile of records
BANDS, COLUMNS, BINS = 7, 300, (2, 3)
TERMS, HOP, STRIDE = (40, 17, 9), (17, 50, 4), (1, 3, 7)  # spans 40, 49, 57: 16, 6 and 61 windows, a gap in the second band


def windows():
    return [(COLUMNS - ((t - 1) * s + 1)) // h + 1 for t, h, s in zip(TERMS, HOP, STRIDE)]


def _build_cross_spectra_bands(coherence):
    torch, _lib, lib, dev = sc._gpu()
    a, b = sc.record_pair((RECORDS, BANDS, COLUMNS, 2), "float64", (71, int(coherence)))
    code = _lib.QI_F64
    first, count = BINS
    tables = [_lib.iarr(t) for t in (TERMS, HOP, STRIDE)]
    (_, t_ptr), (_, h_ptr), (_, s_ptr) = tables
    total = int(lib.qi_cross_spectra_bands_layout(COLUMNS, count, t_ptr, h_ptr, s_ptr, None))
    assert total == sum(windows())
    nbytes = int(lib.qi_cross_spectra_bands_scratch_bytes(code, RECORDS, BANDS, COLUMNS, first, count, t_ptr, h_ptr, s_ptr))
    w_host, w_ptr = _lib.darr(np.linspace(0.5, 2.0, count)) if coherence else (None, None)

    def op(x):
        assert tables  # (the host tables live as long as the closure)
        out = sc._full(torch, (total, RECORDS, RECORDS), torch.float64 if coherence else torch.complex128, dev)
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_cross_spectra_bands, dev, code, dev.index, _lib.ptr(x), RECORDS, BANDS, COLUMNS, first, count, t_ptr, h_ptr, s_ptr,
                  w_ptr, None if coherence else _lib.ptr(out), _lib.ptr(out) if coherence else None, _lib.ptr(scratch), nbytes)
        return (out,)

    return Built(op, a, b, f"{total} matrices" + ("" if w_host is None else f", {len(w_host)} host weights"))


_case("cross_spectra_bands-matrices", ("qi_cross_spectra_bands",), functools.partial(_build_cross_spectra_bands, False))
_case("cross_spectra_bands-coherence", ("qi_cross_spectra_bands",), functools.partial(_build_cross_spectra_bands, True))
