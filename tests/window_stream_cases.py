"""Case table of the stream-order tests of include/qi_windows.h (a plain helper module: imports on the CPU, builds its
closures on the GPU), in the shape of tests/steer_stream_cases.py and tests/array_stream_cases.py, with the helpers of
tests/stream_cases.py.

qi_cross_spectra_windows on a float64 panel [RECORDS, 7 bands, 300 columns] (the producer's tensor, as interleaved (re, im)
values), windows of 40 columns every 17, the bands 2 .. 5: once the matrices alone with no weights, once the coherence alone
with host weights -- the matrices go through scratch.  qi_csd_windows on float32 records at stream_cases' fused and hipFFT
STFT shapes (five Welch segments, windows of three every one), each with the matrices and with the coherence only.
tests/test_windows_cpu.py holds the table against the header; tests/test_gpu_header_streams.py runs each case behind the
delayed producer of tests/stream_order.py.  All are asynchronous: the header promises no host synchronisation, the host
weights ride in kernel arguments.  Each case has one output: it differs between the two record sets, is finite and holds no
FILL.
"""
import functools

import numpy as np

import stream_cases as sc
from stream_table import Built, Table

TABLE = Table("qi_windows.h", power="every", finite=True, no_fill=True)  # (no plans: every case is plan-less)
_case = TABLE.case
RECORDS = 5  # one ragged tile of records
BANDS, COLUMNS, BINS = 7, 300, (2, 4)
WINDOW, HOP = 40, 17  # 16 windows, odd starts, a checked tail in either precision
CSD_WINDOW, CSD_HOP = 3, 1  # of the five Welch segments: three windows


def _build_cross_spectra_windows(coherence):
    torch, _lib, lib, dev = sc._gpu()
    a, b = sc.record_pair((RECORDS, BANDS, COLUMNS, 2), "float64", (61, int(coherence)))
    code = _lib.QI_F64
    first, count = BINS
    n_win = (COLUMNS - WINDOW) // HOP + 1
    nbytes = int(lib.qi_cross_spectra_windows_scratch_bytes(code, RECORDS, BANDS, COLUMNS, first, count, WINDOW, HOP))
    w_host, w_ptr = _lib.darr(np.linspace(0.5, 2.0, count)) if coherence else (None, None)

    def op(x):
        out = sc._full(torch, (n_win, count, RECORDS, RECORDS), torch.float64 if coherence else torch.complex128, dev)
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_cross_spectra_windows, dev, code, dev.index, _lib.ptr(x), RECORDS, BANDS, COLUMNS, first, count, WINDOW, HOP,
                  w_ptr, None if coherence else _lib.ptr(out), _lib.ptr(out) if coherence else None, _lib.ptr(scratch), nbytes)
        return (out,)

    return Built(op, a, b, "" if w_host is None else f"{len(w_host)} host weights")


def _build_csd_windows(shape, coherence):
    torch, _lib, lib, dev = sc._gpu()
    seg, hop, nfft, n = sc.STFT_SHAPES[shape]
    a, b = sc.record_pair((RECORDS, n), "float32", (62, seg, int(coherence)))
    win, scale = sc._stft_window(torch, seg, dev)
    n_f, code = nfft // 2 + 1, _lib.QI_F32
    n_win = ((n - seg) // hop + 1 - CSD_WINDOW) // CSD_HOP + 1
    first, count = 1, n_f - 1  # a range ending at the last bin
    nbytes = int(lib.qi_csd_windows_scratch_bytes(code, RECORDS, n, seg, hop, nfft, first, count, CSD_WINDOW, CSD_HOP))

    def op(x):
        out = sc._full(torch, (n_win, count, RECORDS, RECORDS), torch.float32 if coherence else torch.complex64, dev)
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_csd_windows, dev, code, dev.index, _lib.ptr(x), RECORDS, n, _lib.ptr(win), seg, hop, nfft, scale, first, count,
                  CSD_WINDOW, CSD_HOP, None if coherence else _lib.ptr(out), _lib.ptr(out) if coherence else None, _lib.ptr(scratch),
                  nbytes)
        return (out,)

    return Built(op, a, b, f"{n_win} windows")


_case("cross_spectra_windows-matrices", ("qi_cross_spectra_windows",), functools.partial(_build_cross_spectra_windows, False))
_case("cross_spectra_windows-coherence", ("qi_cross_spectra_windows",), functools.partial(_build_cross_spectra_windows, True))
for _shape in sc.STFT_SHAPES:
    _case(f"csd_windows-{_shape}-matrices", ("qi_csd_windows",), functools.partial(_build_csd_windows, _shape, False))
    _case(f"csd_windows-{_shape}-coherence", ("qi_csd_windows",), functools.partial(_build_csd_windows, _shape, True))
