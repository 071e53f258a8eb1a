"""Generator of tests/golden/calculus.npz -- TEST INFRASTRUCTURE, run where the reference package is installed or checked out
(QI_REFERENCE names its directory) and SciPy is.  Feeds the reference's utilities.calculations and utilities.window functions
the records tests/calculus_cases.py builds from fixed seeds and stores what they return; the inputs are not stored (the
cases rebuild them) and nothing of the reference itself is copied.

    python tools/gen_golden_calculus.py

Integration: the exactly summable records at every length of the matrix, both dtypes, with a sample rate and with
timestamps; random records at two lengths; where the records with NaN and infinities give NaN, +inf and -inf (classes, not
values).  Derivatives: np.gradient and the padded differences of one record per dtype, every fill type and location, with a
rate and with timestamps, and with a NaN in the record.  Tapers: every case of calculus_cases.  The generator asserts what
the tests rely on: the restated terms, gradient and difference are the reference's bits."""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import scipy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if os.environ.get("QI_REFERENCE"):
    sys.path.insert(0, os.environ["QI_REFERENCE"])

from quantum_inferno.utilities import calculations as ref  # noqa: E402
from quantum_inferno.utilities import window as ref_window  # noqa: E402

import calculus_cases as cc  # noqa: E402


def left_to_right(terms):
    return np.concatenate([np.zeros(1, terms.dtype), np.cumsum(terms)])


def main():
    out = {}
    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    for dtype in cc.DTYPES:
        for n in cc.LENGTHS:
            y = cc.exact_record(n, dtype)
            got = ref.integrate_with_cumtrapz_sample_rate_hz(cc.EXACT_RATE, y.copy())
            assert got.dtype == np.dtype(dtype) and cc.same_bits(got, left_to_right(cc.terms_ref(y, None, 1 / cc.EXACT_RATE)))
            assert np.array_equal(got, cc.exact_sums(cc.terms_ref(y, None, 1 / cc.EXACT_RATE))), (n, dtype)  # exactly summable
            out[cc.exact_key(n, dtype, "rate")] = got
            ts = cc.exact_timestamps(n, epoch=True)
            got = ref.integrate_with_cumtrapz_timestamps_s(ts, y.copy())
            assert got.dtype == np.float64 and cc.same_bits(got, left_to_right(cc.terms_ref(y, ts)))
            out[cc.exact_key(n, dtype, "ts")] = got
        for n in cc.WRAP_LENGTHS:
            y = cc.random_records(n, dtype)[0]
            out[f"rand_{dtype}_rate_n{n}"] = ref.integrate_with_cumtrapz_sample_rate_hz(cc.FS, y.copy())
            ts = cc.timestamps(n, "sharedE")
            out[f"rand_{dtype}_ts_n{n}"] = ref.integrate_with_cumtrapz_timestamps_s(ts, y.copy())
            for form, t in (("rate", None), ("ts", ts)):
                if n != cc.GRAD_N:
                    continue
                if t is None:
                    got = ref.derivative_with_gradient_sample_rate_hz(cc.FS, y.copy())
                    assert cc.same_bits(got, cc.gradient_ref(y, None, 1 / cc.FS))
                else:
                    got = ref.derivative_with_gradient_timestamps_s(t, y.copy())
                    assert cc.same_bits(got, cc.gradient_ref(y, t))
                assert got.dtype == np.dtype(dtype)
                out[f"grad_{dtype}_{form}_n{n}"] = got
        rows = cc.special_records(dtype)
        ts = cc.timestamps(cc.SPECIAL_N, "shared0")
        out[f"special_{dtype}_rate"] = np.stack([cc.classes(ref.integrate_with_cumtrapz_sample_rate_hz(cc.FS, r.copy())) for r in rows])
        out[f"special_{dtype}_ts"] = np.stack([cc.classes(ref.integrate_with_cumtrapz_timestamps_s(ts, r.copy())) for r in rows])
        for with_nan in (False, True):
            y = cc.fill_record(dtype, with_nan)
            ts = cc.fill_timestamps()
            for fill_type in cc.FILL_TYPES:
                for fill_loc in cc.FILL_LOCATIONS:
                    got = ref.derivative_with_difference_sample_rate_hz(cc.FS, y.copy(), fill_type, fill_loc)
                    d = got[1:] if fill_loc == "start" else got[:-1]
                    assert np.array_equal(d, cc.difference_ref(y, None, cc.FS).astype(got.dtype), equal_nan=True)
                    out[cc.fill_key(dtype, "rate", fill_type, fill_loc, with_nan)] = got
                    got = ref.derivative_with_difference_timestamps_s(ts, y.copy(), fill_type, fill_loc)
                    d = got[1:] if fill_loc == "start" else got[:-1]
                    assert got.dtype == np.float64 and cc.same_bits(d, cc.difference_ref(y, ts))
                    out[cc.fill_key(dtype, "ts", fill_type, fill_loc, with_nan)] = got
    # one sample: what the reference answers where there is no difference to take (the raising fill types are pinned in the test)
    for fill_type in ("zero", "nan", "mean", "median"):
        for fill_loc in cc.FILL_LOCATIONS:
            out[f"one_{fill_type}_{fill_loc}"] = ref.derivative_with_difference_sample_rate_hz(cc.FS, np.array([1.5]), fill_type, fill_loc)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        for points, alpha in cc.WINDOW_CASES:
            out[f"tukey_{points}_{alpha}"] = ref_window.get_tukey(np.zeros(points), alpha)
        for points, taper_num, alpha in cc.BUFFER_CASES:
            out[f"buffer_{points}_{taper_num}_{alpha}"] = ref_window.get_tukey_by_buffer_num(np.zeros(points), taper_num, alpha)
        for points, taper_s, rate, alpha in cc.BUFFER_S_CASES:
            out[f"buffer_s_{points}_{taper_s}_{rate}_{alpha}"] = ref_window.get_tukey_by_buffer_s(np.zeros(points), taper_s, rate, alpha)
    out["window_warnings"] = np.array(sink.getvalue().splitlines())
    path = os.path.join(ROOT, "tests", "golden", "calculus.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, scipy.__version__, "quantum-inferno 1.1.3"]), **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays")


if __name__ == "__main__":
    main()
