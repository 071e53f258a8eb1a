"""Case table of the stream-order tests of include/qi_squeeze.h (a plain helper module: imports on the CPU, builds its closures
on the GPU), in the shape of tests/timebeam_stream_cases.py, with the helpers of tests/stream_cases.py.

The producer's tensor is the panel [RECORDS, BANDS, COLUMNS] (as interleaved (re, im) values): qi_tfr_ifreq on a float32 panel
with host carriers; qi_tfr_squeeze on a float64 panel with a frequency table that is on the device before the closure is
called, host edges and host weights; qi_tfr_synchrosqueeze on a float32 panel with every host table.  Each call is the tables'
launches and one more.  tests/test_squeeze_cpu.py holds the table against the header; tests/test_gpu_squeeze.py runs
each case behind the delayed producer of tests/stream_order.py.  All are asynchronous: the header promises no host
synchronisation, the host tables ride in kernel arguments.  Every output differs between the two panels, is finite and holds
no FILL.
"""
import functools

import numpy as np

import squeeze_cases as sq
import stream_cases as sc
from stream_table import Built, Table

TABLE = Table("qi_squeeze.h", complex_input=True, power="every", finite=True, no_fill=True)  # (no plans: every case is plan-less)
_case = TABLE.case
RECORDS, BANDS, COLUMNS = 3, 24, 3000  # twelve tiles, the last one ragged
BINS = {"ifreq": 1, "squeeze": 40, "synchrosqueeze": 63}


def _build(which):
    torch, _lib, lib, dev = sc._gpu()
    name = "float64" if which == "squeeze" else "float32"
    a, b = sc.record_pair((RECORDS, BANDS, COLUMNS, 2), name, (89, len(which)))
    rdtype, cdtype = (torch.float64, torch.complex128) if name == "float64" else (torch.float32, torch.complex64)
    code = _lib.dtype_code(rdtype)
    nbin = BINS[which]
    tables = dict(carrier=_lib.darr(sq.carrier_of(BANDS)), weight=_lib.darr(sq.weight_of(BANDS)), edges=_lib.darr(sq.case_edges(nbin)))
    (_, c_ptr), (_, w_ptr), (_, e_ptr) = tables["carrier"], tables["weight"], tables["edges"]
    rng = np.random.default_rng([97, nbin])
    given = torch.from_numpy(rng.uniform(-0.5 * sq.FS, 0.5 * sq.FS, (RECORDS, BANDS, COLUMNS)).astype(name)).to(dev)
    torch.cuda.synchronize()
    nbytes = int(lib.qi_tfr_squeeze_scratch_bytes(code, RECORDS, BANDS, COLUMNS, nbin))
    assert nbytes > 0

    def op(z):
        assert tables  # (the host tables live as long as the closure)
        scratch = sc._scratch(torch, nbytes, dev)
        if which == "ifreq":
            out = sc._full(torch, (RECORDS, BANDS, COLUMNS), rdtype, dev)
            _lib.call(lib.qi_tfr_ifreq, dev, code, dev.index, _lib.ptr(z), RECORDS, BANDS, COLUMNS, c_ptr, sq.FS, 0.0, _lib.ptr(out),
                      _lib.ptr(scratch), nbytes)
            return (out,)
        out = sc._full(torch, (RECORDS, nbin, COLUMNS), cdtype, dev)
        if which == "squeeze":
            _lib.call(lib.qi_tfr_squeeze, dev, code, dev.index, _lib.ptr(z), _lib.ptr(given), RECORDS, BANDS, COLUMNS, e_ptr, nbin, w_ptr,
                      _lib.ptr(out), _lib.ptr(scratch), nbytes)
        else:
            _lib.call(lib.qi_tfr_synchrosqueeze, dev, code, dev.index, _lib.ptr(z), RECORDS, BANDS, COLUMNS, c_ptr, sq.FS, 0.0, e_ptr, nbin,
                      w_ptr, _lib.ptr(out), _lib.ptr(scratch), nbytes)
        return (out,)

    return Built(op, a, b, f"tfr {which}: {nbin} bins, {nbytes} bytes of tables")


_case("tfr_ifreq-f32-carriers", ("qi_tfr_ifreq",), functools.partial(_build, "ifreq"))
_case("tfr_squeeze-f64-given", ("qi_tfr_squeeze",), functools.partial(_build, "squeeze"))
_case("tfr_synchrosqueeze-f32-tables", ("qi_tfr_synchrosqueeze",), functools.partial(_build, "synchrosqueeze"))
