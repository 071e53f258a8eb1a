"""Case table of the stream-order tests of include/qi_array.h (a plain helper module: imports on the CPU, builds its closures
on the GPU), in the shape of tests/stream_cases.py, whose helpers it uses.

One case per path of every function of qi_array.h that takes a `qi_stream`: qi_csd at a fused and at a hipFFT shape,
qi_cross_spectra with and without the coherence (and with and without host weights).  tests/test_csd_cpu.py holds the table
against the header; tests/test_gpu_header_streams.py runs each case behind the delayed producer of tests/stream_order.py.
All four are asynchronous: the header promises no host synchronisation, the host weights ride in kernel arguments.  Every
output differs between the two record sets and is finite.
"""
import functools

import numpy as np

import stream_cases as sc
from stream_table import Built, Table

TABLE = Table("qi_array.h", power="every", finite=True)  # (no plans: every case is plan-less)
_case = TABLE.case
RECORDS = 5  # one ragged tile of records


def _build_csd(shape):
    """csd and coherence of RECORDS float32 records at stream_cases' fused / hipFFT STFT shape (Welch segments)."""
    torch, _lib, lib, dev = sc._gpu()
    seg, hop, nfft, n = sc.STFT_SHAPES[shape]
    a, b = sc.record_pair((RECORDS, n), "float32", (40, seg))
    win, scale = sc._stft_window(torch, seg, dev)
    n_f, code = nfft // 2 + 1, _lib.QI_F32
    nbytes = int(lib.qi_csd_scratch_bytes(code, RECORDS, n, seg, hop, nfft))

    def op(x):
        csd = sc._full(torch, (n_f, RECORDS, RECORDS), torch.complex64, dev)
        coh = sc._full(torch, (n_f, RECORDS, RECORDS), torch.float32, dev)
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_csd, dev, code, dev.index, _lib.ptr(x), RECORDS, n, _lib.ptr(win), seg, hop, nfft, scale, _lib.ptr(csd),
                  _lib.ptr(coh), _lib.ptr(scratch), nbytes)
        return (csd, coh)

    return Built(op, a, b, "")


def _build_cross_spectra(coherence):
    """A float64 panel [RECORDS, 7 bands, 300 columns] as interleaved (re, im) values.  With the coherence: host weights and no
    csd output -- the matrices go through scratch; without: no weights, the matrices alone."""
    torch, _lib, lib, dev = sc._gpu()
    bands, cols = 7, 300
    a, b = sc.record_pair((RECORDS, bands, cols, 2), "float64", (41, int(coherence)))
    code = _lib.QI_F64
    nbytes = int(lib.qi_cross_spectra_scratch_bytes(code, RECORDS, bands, cols))
    w_host, w_ptr = _lib.darr(np.linspace(0.5, 2.0, bands)) if coherence else (None, None)

    def op(x):
        out = sc._full(torch, (bands, RECORDS, RECORDS), torch.float64 if coherence else torch.complex128, dev)
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_cross_spectra, dev, code, dev.index, _lib.ptr(x), RECORDS, bands, cols, w_ptr,
                  None if coherence else _lib.ptr(out), _lib.ptr(out) if coherence else None, _lib.ptr(scratch), nbytes)
        return (out,)

    return Built(op, a, b, "" if w_host is None else f"{len(w_host)} host weights")


for _shape in sc.STFT_SHAPES:
    _case(f"csd-{_shape}", ("qi_csd",), functools.partial(_build_csd, _shape))
_case("cross_spectra-coherence", ("qi_cross_spectra",), functools.partial(_build_cross_spectra, True))
_case("cross_spectra-matrices", ("qi_cross_spectra",), functools.partial(_build_cross_spectra, False))
