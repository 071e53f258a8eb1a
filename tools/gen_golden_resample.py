"""Generator of tests/golden/resample.npz -- TEST INFRASTRUCTURE, run where the reference package is installed or checked out
(QI_REFERENCE names its directory) and SciPy is.  Feeds the reference's utilities.sampling.resample_uneven_timeseries and
resample_with_sample_rate the records tests/resample_cases.py builds from fixed seeds and stores what they return; the
inputs are not stored (the cases rebuild them) and nothing of the reference itself is copied.

    python tools/gen_golden_resample.py

Interpolation: every record length of the matrix (1, 2, 3, T - 1, T, T + 1, 3 T + 17 with T = the tile of qi_interp_grid)
at the four rates (x 2.37, x 1, x 1 / 3.1, None), each case for one of the four (dtype, first timestamp) pairs in turn, and
the records whose timestamps lie on the grid.  Fourier resampler: one record per shape and dtype, the reference called with
the rates (n, m) so that its new length is m.  The generator asserts what the tests rely on: the restatements of
resample_cases reproduce every recorded result (bit for bit, float32 Fourier results within 2e-5), and the grid equals
np.arange."""
import os
import sys

import numpy as np
import scipy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("QI_REFERENCE", "/root/reference"))

from quantum_inferno.utilities import sampling  # noqa: E402

import resample_cases as rc  # noqa: E402


def interp_case(out, key, ts, y, rate):
    with np.errstate(all="ignore"):
        got, got_rate = sampling.resample_uneven_timeseries(y.copy(), ts.copy(), rate)
    assert got.dtype == np.float64
    start, delta, m = rc.grid_ref(ts[0], ts[-1], got_rate)
    assert np.array_equal(rc.grid_values(start, delta, m), np.arange(ts[0], ts[-1], 1 / got_rate)), key
    assert rc.same_bits(rc.interp_ref(rc.grid_values(start, delta, m), ts, y), got), key
    out[key] = got
    out[key + "_rate"] = np.float64(got_rate)


def main():
    out = {}
    for n, rk in rc.interp_cases():
        dtype, t0 = rc.fixture_combo(n, rk)
        ts, y = rc.uneven_record(n, dtype, t0)
        interp_case(out, rc.interp_key(n, rk), ts, y, rc.RATES[rk])
    for dtype in rc.DTYPES:
        ts, y = rc.on_grid_record(dtype)
        for rate in rc.ON_GRID_RATES:
            interp_case(out, f"interp_ongrid_{dtype}_{int(rate)}", ts, y, rate)
    for n, m in rc.FFT_SHAPES:
        for dtype in rc.DTYPES:
            x = rc.fft_record(n, m, dtype)
            got, rate = sampling.resample_with_sample_rate(x.copy(), float(n), float(m))
            assert got.shape == (m,) and got.dtype == np.dtype(dtype) and rate == float(m), (n, m, dtype)
            want = rc.fft_resample_ref(x, m)
            if dtype == "float64":
                assert rc.same_bits(want, got), (n, m)
            else:
                assert np.max(np.abs(want - got)) <= rc.FFT_TOL[dtype] * np.max(np.abs(want)), (n, m)
            out[rc.fft_key(n, m, dtype)] = got
    path = os.path.join(ROOT, "tests", "golden", "resample.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, scipy.__version__, "quantum-inferno 1.1.3"]), **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays")


if __name__ == "__main__":
    main()
