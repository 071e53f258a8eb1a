"""Generator of tests/golden/csd.npz -- TEST INFRASTRUCTURE, run where SciPy is.  Feeds scipy.signal.csd (both scalings) and
scipy.signal.coherence the seeded records of tests/csd_cases.py, every pair at once (x[:, None, :] against x[None, :, :],
the frequency axis moved to the front), and stores the records and SciPy's float64 results.

    python tools/gen_golden_csd.py

The generator asserts what the tests rely on (tests/test_csd_cpu.py asserts the second again): SciPy's [j][i] is the
conjugate of its [i][j] to four float64 epsilons of the largest entry (the fixture keeps the pairs i <= j), and in every case
with more than one segment every auto-power is at least csd_cases.FLOOR of its record's maximum over the bins, bin 0
included -- so no bin is masked out of any comparison.
(The one-segment case cannot hold a floor: its bin 0 is what the mean removal leaves.)  A seed that fails is changed in
csd_cases.py; the floor is not."""
import os
import sys

import numpy as np
import scipy
import scipy.signal as signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import csd_cases as cc  # noqa: E402


def scipy_matrices(x, case, scaling):
    kw = dict(fs=cc.FS, window=("tukey", cc.ALPHA), nperseg=case.seg, noverlap=case.overlap, nfft=case.nfft, detrend="constant")
    f, p = signal.csd(x[:, None, :], x[None, :, :], scaling=scaling, return_onesided=True, average="mean", **kw)
    return f, np.moveaxis(p, -1, 0)


def main():
    out = {}
    for case in cc.CASES:
        x32 = cc.records(case)
        x = x32.astype(np.float64)
        out[cc.key(case, "records")] = x32
        for scaling in cc.SCALINGS:
            f, p = scipy_matrices(x, case, scaling)
            assert np.array_equal(f, np.fft.rfftfreq(case.nfft, 1 / cc.FS))
            skew = np.abs(p - np.conj(np.swapaxes(p, 1, 2))).max() / np.abs(p).max()
            assert skew <= 4 * np.finfo(np.float64).eps, (case.id, skew)
            if cc.segments(case) > 1:
                floor = cc.auto_power_floor(p)
                assert floor >= cc.FLOOR, (case.id, floor)
                print(f"{case.id} {scaling}: smallest auto-power / its record's maximum = {floor:.3g}")
            out[cc.key(case, f"csd_{scaling}")] = cc.pack(p, case)
        kw = dict(fs=cc.FS, window=("tukey", cc.ALPHA), nperseg=case.seg, noverlap=case.overlap, nfft=case.nfft, detrend="constant")
        _, coh = signal.coherence(x[:, None, :], x[None, :, :], **kw)
        coh = np.moveaxis(coh, -1, 0)
        with np.errstate(invalid="ignore"):
            assert not np.nanmax(np.abs(coh - np.swapaxes(coh, 1, 2))) > 8 * np.finfo(np.float64).eps, case.id
        out[cc.key(case, "coherence")] = cc.pack(coh, case)
    np.savez_compressed(cc.GOLDEN, versions=np.array([np.__version__, scipy.__version__]), **out)
    print(f"{cc.GOLDEN}: {os.path.getsize(cc.GOLDEN) / 1e6:.3f} MB, {len(out)} arrays")


if __name__ == "__main__":
    main()
