"""Resampling on the GPU.  qi_interp_grid through ctypes, bit for bit against np.interp itself and against the reference's
recorded results (tests/golden/resample.npz): every record length, rate, epoch and dtype of the matrix, timestamps on the
grid, a gap that holds whole workgroups, bursts of knots on both sides of the LDS limit, 65 records with shared and with
per-record timestamps, m = 0 and the argument checks.  qi_resample_fft against the recorded results within the project's
hipFFT bounds, for 1, 3 and 65 records.  The reference-signature wrappers end to end.  Every buffer is pre-filled with a
sentinel and carries a guard column.  No test feeds unsorted timestamps to the GPU."""
import numpy as np
import pytest
import torch

import resample_cases as rc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import sampling

pytestmark = pytest.mark.gpu

GUARD = 1  # elements behind each buffer that the call must leave alone
FILL = -3.0e300


@pytest.fixture(scope="module")
def g(golden):
    return golden("resample.npz")


def interp(values, knots, start, delta, m, expect=0, override=None):
    """qi_interp_grid on device tensors values [C, n], knots [n] or [C, n] -> out [C, m] on the host, after checking that
    every output was written and the guard was not.  `expect`: the status the call must return (then -> None);
    `override`: arguments of the C call to replace (the buffers stay those of the shapes given here)."""
    lib = _lib.require_gpu()
    dev = values.device
    n_ch, n = values.shape
    out = torch.full((n_ch * max(m, 0) + GUARD,), FILL, dtype=torch.float64, device=dev)
    a = dict(dtype=_lib.QI_F64 if values.dtype == torch.float64 else _lib.QI_F32, values=_lib.ptr(values), knots=_lib.ptr(knots),
             stride=n if knots.dim() == 2 else 0, c=n_ch, n=n, start=float(start), delta=float(delta), m=m, out=_lib.ptr(out))
    a.update(override or {})
    with torch.cuda.device(dev):
        rc_ = lib.qi_interp_grid(a["dtype"], dev.index, a["values"], a["knots"], a["stride"], a["c"], a["n"], a["start"], a["delta"],
                                 a["m"], a["out"], _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc_ == expect, (rc_, lib.qi_last_error())
    assert out[-1].item() == FILL, "the guard was written"
    if expect != 0:
        assert (out == FILL).all(), "a refused call wrote"
        return None
    got = out[:-GUARD].view(n_ch, max(m, 0)).cpu().numpy()
    assert not (got == FILL).any(), "an output was not written"
    return got


def check(got, x, ts, y, where):
    """got [m] against np.interp itself, bit for bit (the figure first)."""
    with np.errstate(all="ignore"):
        want = np.interp(x, ts, y)
        fin = np.isfinite(want) & np.isfinite(got)
        diff = np.max(np.abs(got[fin] - want[fin]), initial=0.0)
    if not rc.same_bits(got, want):
        print(f"{where}: max |difference| {diff:.3e} over {len(want)} outputs, "
              f"{int(np.sum(got.view(np.uint64) != want.view(np.uint64)))} differ (bit for bit asked)")
    assert rc.same_bits(got, want), where


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_matrix_equals_numpy_and_the_reference(g, dtype):
    from_fixture = 0
    for t0 in (0.0, rc.EPOCH):
        for n in rc.LENGTHS:
            ts, y = rc.uneven_record(n, dtype, t0)
            d_ts, d_y = torch.from_numpy(ts).cuda(), torch.from_numpy(y[None, :]).cuda()
            for rk, rate in rc.RATES.items():
                if (n, rk) not in rc.interp_cases():
                    continue
                rate = 1 / np.mean(np.diff(ts)) if rate is None else rate
                start, delta, m = rc.grid_ref(ts[0], ts[-1], rate)
                x = np.arange(ts[0], ts[-1], 1 / rate)
                assert m == len(x)
                got = interp(d_y, d_ts, start, delta, m)[0]
                where = f"{dtype} t0 {t0} n {n} rate {rk}"
                check(got, x, ts, y, where)
                if rc.fixture_combo(n, rk) == (dtype, t0):
                    assert rc.same_bits(got, g[rc.interp_key(n, rk)]), where
                    from_fixture += 1
    assert from_fixture >= 12


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_timestamps_on_the_grid_a_gap_and_bursts(g, dtype):
    ts, y = rc.on_grid_record(dtype)
    d_ts, d_y = torch.from_numpy(ts).cuda(), torch.from_numpy(y[None, :]).cuda()
    for rate in rc.ON_GRID_RATES:
        start, delta, m = rc.grid_ref(ts[0], ts[-1], rate)
        got = interp(d_y, d_ts, start, delta, m)[0]
        check(got, np.arange(ts[0], ts[-1], 1 / rate), ts, y, f"{dtype} on the grid at {rate}")
        assert rc.same_bits(got, g[f"interp_ongrid_{dtype}_{int(rate)}"])
        step = int(rate) // 1024
        assert rc.same_bits(got[::step], y[:-1].astype(np.float64))  # on a knot the value itself
    # one interval over more than three workgroups
    ts, y = rc.gap_record(dtype)
    start, delta, m = rc.grid_ref(ts[0], ts[-1], rc.FS)
    x = rc.grid_values(start, delta, m)
    inside = (x > ts[199]) & (x < ts[200])
    assert inside.sum() > 3 * rc.T and ts[200] - ts[199] > 3 * rc.T / rc.FS
    got = interp(torch.from_numpy(y[None, :]).cuda(), torch.from_numpy(ts).cuda(), start, delta, m)[0]
    check(got, x, ts, y, f"{dtype} gap")
    # the first workgroup brackets exactly K, K + 1 and 4 K knots: the LDS path, its boundary and the path in global memory
    for held in (rc.K, rc.K + 1, 4 * rc.K):
        ts, y, start, delta, m = rc.burst_record(held, dtype)
        x = rc.grid_values(start, delta, m)
        j_lo = np.searchsorted(ts, x[0], side="right") - 1
        j_hi = np.searchsorted(ts, x[rc.T - 1], side="right") - 1
        assert j_lo == 0 and min(j_hi + 1, len(ts) - 1) - j_lo + 1 == held
        got = interp(torch.from_numpy(y[None, :]).cuda(), torch.from_numpy(ts).cuda(), start, delta, m)[0]
        check(got, x, ts, y, f"{dtype} burst of {held}")


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_65_records_shared_and_per_record_timestamps(dtype):
    records = 65
    ts, _ = rc.uneven_record(3 * rc.T + 17, dtype, rc.EPOCH)
    y = np.random.default_rng(11).standard_normal((records, len(ts))).astype(dtype)
    start, delta, m = rc.grid_ref(ts[0], ts[-1], rc.FS * 2.37)
    x = rc.grid_values(start, delta, m)
    d_y = torch.from_numpy(y).cuda()
    got = interp(d_y, torch.from_numpy(ts).cuda(), start, delta, m)
    for r in range(records):
        check(got[r], x, ts, y[r], f"{dtype} shared timestamps, record {r}")
    assert rc.same_bits(got, interp(d_y, torch.from_numpy(ts).cuda(), start, delta, m))  # the same call, the same bits
    # many clocks, one grid: each row shifted and stretched differently, the grid wider than some rows
    ts2, y2, start, delta, m = rc.many_clocks(records, dtype)
    x = rc.grid_values(start, delta, m)
    assert (x[0] < ts2[:, 0]).any() and (x[-1] > ts2[:, -1]).any() and m > 3 * rc.T
    got = interp(torch.from_numpy(y2).cuda(), torch.from_numpy(ts2).cuda(), start, delta, m)
    for r in range(records):
        check(got[r], x, ts2[r], y2[r], f"{dtype} per-record timestamps, record {r}")
    # the same through the engine, NumPy and device tensors, and one record of it
    via = engine.interp_to_grid(y2, ts2, start, delta, m)
    assert isinstance(via, np.ndarray) and rc.same_bits(via, got)
    via = engine.interp_to_grid(torch.from_numpy(y2).cuda(), torch.from_numpy(ts2).cuda(), start, delta, m)
    assert via.is_cuda and via.dtype == torch.float64 and rc.same_bits(via.cpu().numpy(), got)
    one = engine.interp_to_grid(torch.from_numpy(y2[3]).cuda(), torch.from_numpy(ts2[3]).cuda(), start, delta, m)
    assert one.shape == (m,) and rc.same_bits(one.cpu().numpy(), got[3])


def test_grid_wider_than_the_record_through_the_engine():
    for dtype in rc.DTYPES:
        ts, y = rc.uneven_record(rc.T + 1, dtype, 0.0)
        start, delta, m = ts[0] - 0.05, 1 / (rc.FS * 1.5), int((ts[-1] - ts[0] + 0.1) * rc.FS * 1.5)
        x = rc.grid_values(start, delta, m)
        assert x[0] < ts[0] and x[-1] > ts[-1]
        got = engine.interp_to_grid(torch.from_numpy(y).cuda(), torch.from_numpy(ts).cuda(), start, delta, m).cpu().numpy()
        check(got, x, ts, y, f"{dtype} wider grid")
        assert rc.same_bits(got[x < ts[0]], np.full((x < ts[0]).sum(), np.float64(y[0])))
        assert rc.same_bits(got[x > ts[-1]], np.full((x > ts[-1]).sum(), np.float64(y[-1])))
        assert engine.interp_to_grid(torch.from_numpy(y).cuda(), torch.from_numpy(ts).cuda(), start, delta, 0).shape == (0,)


def test_no_outputs_and_refused_arguments():
    lib = _lib.require_gpu()
    ts, y = rc.uneven_record(rc.T, "float64", 0.0)
    d_ts, d_y = torch.from_numpy(ts).cuda(), torch.from_numpy(y[None, :]).cuda()
    assert interp(d_y, d_ts, 0.0, 0.01, 0).shape == (1, 0)  # m = 0: success, nothing written (the guard is checked)
    for bad, word in ((dict(dtype=2), b"dtype"), (dict(n=0), b"record length"), (dict(m=-1), b"output length"),
                      (dict(c=0), b"record count"), (dict(delta=0.0), b"delta"), (dict(delta=-0.01), b"delta"),
                      (dict(delta=float("nan")), b"delta"), (dict(delta=float("inf")), b"delta"),
                      (dict(start=float("nan")), b"start"), (dict(start=float("inf")), b"start"), (dict(stride=rc.T - 1), b"knot_stride"),
                      (dict(values=None), b"null"), (dict(knots=None), b"null"), (dict(out=None), b"null")):
        # (the helper allocates for m = 4 and checks that a refused call wrote nothing)
        assert interp(d_y, d_ts, 0.0, 0.01, 4, expect=-1, override=bad) is None
        assert word in lib.qi_last_error(), bad


def test_uneven_wrapper_numpy_cuda_and_integers():
    ts, y = rc.uneven_record(3 * rc.T + 17, "float64", rc.EPOCH)
    y2 = np.stack([y, -y, y * 0.5])
    for rate in (rc.FS * 2.37, None):
        np_rate = 1 / np.mean(np.diff(ts)) if rate is None else rate
        x = np.arange(ts[0], ts[-1], 1 / np_rate)
        got, got_rate = sampling.resample_uneven_timeseries(y, ts, rate)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got_rate == np_rate
        check(got, x, ts, y, f"wrapper NumPy 1-D rate {rate}")
        got, _ = sampling.resample_uneven_timeseries(y2, ts, rate)
        assert got.shape == (3, len(x))
        for r in range(3):
            check(got[r], x, ts, y2[r], f"wrapper NumPy 2-D rate {rate}")
        # CUDA in, CUDA out; with None the rate is the device's: within 1e-12 of NumPy's, and the result np.interp on ITS grid
        for series in (y, y2, y.astype(np.float32)):
            got, got_rate = sampling.resample_uneven_timeseries(torch.from_numpy(series).cuda(), torch.from_numpy(ts).cuda(), rate)
            assert got.is_cuda and got.dtype == torch.float64
            assert abs(got_rate - np_rate) <= 1e-12 * np_rate, (got_rate, np_rate)
            xg = np.arange(ts[0], ts[-1], 1 / got_rate)
            got = got.cpu().numpy().reshape(-1, len(xg))
            for r, row in enumerate(np.atleast_2d(series)):
                check(got[r], xg, ts, row, f"wrapper CUDA {series.dtype} {series.ndim}-D rate {rate}")
    # integers are read as float64
    yi = (y * 1000).astype(np.int16)
    got, _ = sampling.resample_uneven_timeseries(yi, ts, rc.FS)
    check(got, np.arange(ts[0], ts[-1], 1 / rc.FS), ts, yi, "wrapper int16")
    got, _ = sampling.resample_uneven_timeseries(torch.from_numpy(yi).cuda(), ts, rc.FS)
    check(got.cpu().numpy(), np.arange(ts[0], ts[-1], 1 / rc.FS), ts, yi, "wrapper int16 CUDA")


def fft_resample(x, m):
    """qi_resample_fft on a device tensor x [C, n] -> out [C, m] on the host, after checking the guards."""
    lib = _lib.require_gpu()
    dev = x.device
    n_ch, n = x.shape
    code = _lib.QI_F64 if x.dtype == torch.float64 else _lib.QI_F32
    need = int(lib.qi_resample_fft_scratch_bytes(code, n_ch, n, m))
    assert need > 0
    scratch = torch.full((need // 8 + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    scratch[-1] = FILL
    out = torch.full((n_ch * m + GUARD,), 2.0 ** 100, dtype=x.dtype, device=dev)
    keep = x.clone()
    with torch.cuda.device(dev):
        rc_ = lib.qi_resample_fft(code, dev.index, _lib.ptr(x), n_ch, n, m, _lib.ptr(out), _lib.ptr(scratch), need, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc_ == 0, (rc_, lib.qi_last_error())
    assert out[-1].item() == 2.0 ** 100 and scratch[-1].item() == FILL, "a guard was written"
    assert torch.equal(x, keep), "the records were overwritten"
    return out[:-GUARD].view(n_ch, m).cpu().numpy()


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_fft_resampler_equals_the_reference(g, dtype):
    worst = 0.0
    for n, m in rc.FFT_SHAPES:
        want1 = g[rc.fft_key(n, m, dtype)].astype(np.float64)
        for records in (1, 3, 65):
            x, factors = rc.fft_batch(n, m, dtype, records)
            got = fft_resample(torch.from_numpy(x).cuda(), m)
            assert got.dtype == np.dtype(dtype)
            want = factors[:, None] * want1[None, :]
            err = np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)
            worst = max(worst, err.max())
            print(f"{dtype} n {n} m {m} records {records}: max error {err.max():.3e} of the record's maximum (bound {rc.FFT_TOL[dtype]:.0e})")
            assert np.all(err <= rc.FFT_TOL[dtype]), (n, m, records, err.max())
    print(f"{dtype}: worst {worst:.3e}")
    # records that differ, against the float64 restatement (SciPy's bits in float64, within 3.6e-7 of its float32 results)
    for n, m in ((1000, 441), (1009, 1013), (6, 9)):
        x = (np.random.default_rng(n + m).standard_normal((65, n)) + 0.5).astype(dtype)
        got = fft_resample(torch.from_numpy(x).cuda(), m)
        want = rc.fft_resample_ref(x, m)
        err = np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)
        print(f"{dtype} n {n} m {m} 65 different records: max error {err.max():.3e}")
        assert np.all(err <= rc.FFT_TOL[dtype]), (n, m, err.max())


def test_fft_wrappers_end_to_end(g):
    for dtype in rc.DTYPES:
        n, m = 1000, 441
        x = rc.fft_record(n, m, dtype)
        want = g[rc.fft_key(n, m, dtype)].astype(np.float64)
        bound = rc.FFT_TOL[dtype] * np.max(np.abs(want))
        got, rate = sampling.resample_with_sample_rate(x, 1000.0, 441.0)
        assert isinstance(got, np.ndarray) and got.dtype == np.dtype(dtype) and got.shape == (m,) and rate == 441.0
        assert np.max(np.abs(got - want)) <= bound
        got, _ = sampling.resample_with_sample_rate(torch.from_numpy(np.stack([x, -x])).cuda(), 1000.0, 441.0)
        assert got.is_cuda and got.shape == (2, m) and got.dtype == torch.from_numpy(x).dtype
        assert np.max(np.abs(got.cpu().numpy() - np.stack([want, -want]))) <= bound
        got = engine.fft_resample(torch.from_numpy(x).cuda(), m)
        assert got.shape == (m,) and np.max(np.abs(got.cpu().numpy() - want)) <= bound
    # the reference's rule for the new length: int(n * new / old), truncated
    x = rc.fft_record(1000, 441, "float64")
    for new, old in ((441.9, 1000.0), (48000.0, 44100.0), (1.0, 3.0)):
        got, rate = sampling.resample_with_sample_rate(x, old, new)
        assert got.shape == (int(1000 * new / old),) and rate == new
    xi = (x * 100).astype(np.int16)  # integers are read as float64
    got, _ = sampling.resample_with_sample_rate(xi, 1000.0, 441.0)
    want = rc.fft_resample_ref(xi, 441)
    assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want))
