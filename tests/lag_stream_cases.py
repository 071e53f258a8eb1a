"""Case table of the stream-order tests of include/qi_lags.h (a plain helper module: imports on the CPU, builds its
closures on the GPU), in the shape of tests/window_stream_cases.py, with the helpers of tests/stream_cases.py.

qi_pair_lags on a stack [STACKS, 65 bins, RECORDS, RECORDS] of matrices (the producer's tensor, as interleaved (re, im)
values; only the entries i <= j are read, so noise with a positive mean serves), nfft 128 zero-padded fourfold, the bins
3 .. 60, in both precisions: unweighted as the correlation coefficient (the auto-powers are read too) with every output, PHAT
weights with the peaks alone, PHAT weights with the window alone, and unweighted, not normalised, with the window alone.
tests/test_lags_cpu.py holds the table against the header; tests/test_gpu_header_streams.py runs each case behind the delayed
producer of tests/stream_order.py.  All are asynchronous: the header promises no host synchronisation.  Every output differs
between the two record sets, is finite and holds no FILL.
"""
import functools

import stream_cases as sc
from stream_table import Built, Table

TABLE = Table("qi_lags.h", power="every", finite=True, no_fill=True)  # (no plans: every case is plan-less)
_case = TABLE.case
STACKS, RECORDS, NFFT, UPSAMPLE, MAX_LAG, BINS = 3, 5, 128, 4, 40, (3, 60)


def _build_pair_lags(dtype, weighting, normalize, outputs):
    torch, _lib, lib, dev = sc._gpu()
    n_f, n_pair = NFFT // 2 + 1, RECORDS * (RECORDS - 1) // 2
    a, b = sc.record_pair((STACKS, n_f, RECORDS, RECORDS, 2), dtype, (71, weighting, normalize))
    code = _lib.QI_F64 if dtype == "float64" else _lib.QI_F32
    real = torch.float64 if dtype == "float64" else torch.float32
    nbytes = int(lib.qi_pair_lags_scratch_bytes(code, STACKS, RECORDS, NFFT, UPSAMPLE))
    want_cc, want_peaks = outputs in ("all", "cc"), outputs in ("all", "peaks")

    def op(x):
        cc = sc._full(torch, (STACKS, n_pair, 2 * MAX_LAG + 1), real, dev) if want_cc else None
        lag, value = (sc._full(torch, (STACKS, n_pair), real, dev) if want_peaks else None for _ in range(2))
        scratch = sc._scratch(torch, nbytes, dev)
        _lib.call(lib.qi_pair_lags, dev, code, dev.index, _lib.ptr(x), STACKS, RECORDS, NFFT, BINS[0], BINS[1], weighting, 1, normalize,
                  UPSAMPLE, MAX_LAG, _lib.ptr(cc), _lib.ptr(lag), _lib.ptr(value), _lib.ptr(scratch), nbytes)
        return tuple(t for t in (lag, value, cc) if t is not None)

    return Built(op, a, b, f"{STACKS * n_pair} workgroups")


_case("pair_lags-f64-plain-all", ("qi_pair_lags",), functools.partial(_build_pair_lags, "float64", 0, 1, "all"))
_case("pair_lags-f32-phat-peaks", ("qi_pair_lags",), functools.partial(_build_pair_lags, "float32", 1, 1, "peaks"))
_case("pair_lags-f64-phat-cc", ("qi_pair_lags",), functools.partial(_build_pair_lags, "float64", 1, 1, "cc"))
_case("pair_lags-f32-plain-cc", ("qi_pair_lags",), functools.partial(_build_pair_lags, "float32", 0, 0, "cc"))
