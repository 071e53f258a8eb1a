"""Generator of tests/golden/peaks.npz -- TEST INFRASTRUCTURE, run where the reference package is installed or checked out
(QI_REFERENCE names its directory) and SciPy is.  Feeds the reference's utilities.picker functions (scale_signal_by_
extraction_type, find_peaks_by_extraction_type, find_peaks_with_bits, find_peaks_by_extraction_type_with_bandpass, the
three index helpers) seeded records, row by row, and stores the inputs and the reference's results; nothing of the
reference itself is copied.

    python tools/gen_golden_peaks.py

The records are seeded noise plus records built to break a tiled picker (T = the tile of qi_find_peaks): peaks at samples
1 and n - 2, plateaus across tile boundaries, over whole tiles, from sample 0 and up to the last sample, even-length
plateaus, constant, rising, all-negative records, a maximum of 0, NaN, +-inf, and float32 records in which the division
by the maximum itself makes a plateau.  The generator asserts what the tests rely on (tests/peak_cases.py restates the
checks): no log2* case with unequal neighbours within 1e-6 bits, no log2* candidate within 1e-6 of its height, no distance
case with two equal candidates within the distance, and 1e-6 between every band-passed pick and its height.  A seed that
fails one of these is changed here; the margin is not."""
import io
import os
import sys
import warnings
from contextlib import redirect_stdout

import numpy as np
import scipy
import scipy.signal as signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("QI_REFERENCE", "/root/reference"))

from quantum_inferno.utilities import picker  # noqa: E402

import peak_cases as pc  # noqa: E402

T = pc.TILE
SEED = 5100000


def quiet(fn, *args, **kwargs):
    with redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def noise(rng, n, dtype):
    return (rng.standard_normal(n) + 0.25).astype(dtype)


def plateau(x, a, b, value):
    x[a:b] = value


def records(dtype, n, seed):
    """[RECORDS, n] of `dtype`: what each record is built to break is said where it is built."""
    rng = np.random.default_rng(seed)
    x = np.stack([noise(rng, n, dtype) for _ in range(pc.RECORDS)])
    top = x.dtype.type(5.0)
    if n == 1:
        x[1, 0] = np.nan
        x[2, 0] = 0.0
    elif n == 2:
        x[1] = [1.0, np.nan]
        x[2] = [2.0, 2.0]
    elif n == 3:
        x[1] = [0.5, 1.0, 0.25]  # the only sample that can be a peak is one
        x[2] = [0.5, 1.0, 1.0]   # ... and here its run reaches the last sample
    elif n == 4:
        x[1] = [0.0, 1.0, 1.0, 0.5]   # an even plateau: the midpoint 1.5 rounds down to 1
        x[2] = [1.0, 1.0, 0.5, 0.75]  # a plateau from sample 0, and a last sample that rises
    elif n == T - 1:
        x[0] = np.nan  # a record of NaNs
        plateau(x[2], 0, 6, top)  # a plateau from sample 0: no peak
        plateau(x[2], 100, 104, 4.0)  # an even plateau: 100 .. 103 -> 101
        x[2, 99], x[2, 104] = 1.0, 1.0
    elif n == T:
        x[0] = 1.5  # a constant record
        x[1] = np.cumsum(np.abs(x[1]) + x.dtype.type(0.01))  # strictly rising
        assert np.all(np.diff(x[1]) > 0)
        x[2, 0], x[2, 1], x[2, 2] = 0.0, top, 0.0  # peaks at samples 1 and n - 2
        x[2, n - 3], x[2, n - 2], x[2, n - 1] = 0.0, 4.5, 0.0
    elif n == T + 1:
        plateau(x[0], 40, 45, 3.5)  # one NaN inside a plateau that would be a peak
        x[0, 39], x[0, 45], x[0, 42] = 0.0, 0.0, np.nan
        x[0, 120], x[0, 200] = np.inf, -np.inf
        x[1] = -np.abs(x[1]) - x.dtype.type(0.5)  # all negative: sigmax divides by a negative maximum
        plateau(x[2], T - 1, T + 1, top)  # a plateau over the tile boundary that reaches the last sample: no peak
        x[2] = x[2] - np.max(x[2])  # ... and the maximum of the record is 0
        assert np.max(x[2]) == 0.0
    else:
        assert n == 3 * T + 17
        x[0, 0], x[0, 1], x[0, 2] = 0.0, top, 0.0  # peaks at samples 1 and n - 2
        x[0, n - 3], x[0, n - 2], x[0, n - 1] = 0.0, 4.5, 0.0
        plateau(x[0], T - 1, T + 1, 4.0)  # one sample on either side of the first tile boundary (even: -> T - 1)
        x[0, T - 2], x[0, T + 1] = 0.0, 0.0
        plateau(x[0], 2 * T - 1, 2 * T + 2, 3.75)  # one before, two behind the second (-> 2 T)
        x[0, 2 * T - 2], x[0, 2 * T + 2] = 0.0, 0.0
        plateau(x[1], T - 6, 3 * T + 5, 4.25)  # tiles 1 and 2 entirely, ending inside tile 3: a peak
        x[1, T - 7], x[1, 3 * T + 5] = 0.0, 0.0
        plateau(x[2], T - 6, n, 4.25)  # the same up to the last sample: no peak
        x[2, T - 7] = 0.0
    x = x + x.dtype.type(0.0)  # (no -0.0: NumPy leaves the sign of a maximum of zeros open)
    assert x.dtype == np.dtype(dtype) and x.shape == (pc.RECORDS, n)
    return np.ascontiguousarray(x)


def division_plateau(seed):
    """float32 records [RECORDS, T - 1] with samples i, i + 1 that are unequal, neighbours as float32 values, and divide by
    the record's maximum to the SAME float32, between lower samples: the scaled record has a plateau there and the peak is
    at i, where the unscaled record has it at i + 1."""
    n = T - 1
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < pc.RECORDS:
        x = noise(rng, n, "float32")
        i = int(rng.integers(8, n - 8))
        x[i] = np.float32(1.0) + np.float32(rng.random())
        x[i + 1] = np.nextafter(x[i], np.float32(np.inf))
        x[i - 1], x[i + 2] = 0.0, 0.0
        m = np.nanmax(x)
        if m > x[i + 1] and x[i] / m == x[i + 1] / m:
            assert x[i] != x[i + 1] and (x / m).dtype == np.float32
            got = signal.find_peaks(x / m)[0]
            assert i in got and i + 1 not in got and i + 1 in signal.find_peaks(x)[0]
            rows.append(x)
    return np.ascontiguousarray(np.stack(rows))


def extraction_cases(out, dtype, tag, x):
    """-> {case id: rows}; the scaled records go to `out`."""
    cases = {}
    for kind in pc.types_of(tag):
        scaled = np.stack([quiet(picker.scale_signal_by_extraction_type, row.copy(), kind) for row in x])
        assert scaled.dtype == pc.scaled_type(dtype, kind), (dtype, kind, scaled.dtype)
        out[pc.scaled_key(dtype, tag, kind)] = scaled
        for h in pc.HEIGHTS:
            cases[("ext", kind, h)] = [quiet(picker.find_peaks_by_extraction_type, row.copy(), kind, h) for row in x]
            if kind in ("log2", "log2max") and h is not None:
                for s in scaled:
                    cand = s[signal.find_peaks(s)[0]]
                    assert not np.any(np.abs(cand - h) <= pc.MARGIN), (dtype, tag, kind, h)
    return cases


def bits_cases(dtype, tag, x):
    cases = {}
    assert pc.log2_neighbours_clear(x), (dtype, tag)
    for scaling in pc.BITS_SCALINGS:
        for t in pc.BITS_THRESHOLDS:
            for row in x:  # the candidates keep the margin to the height, and equal ones are further apart than any distance
                bits = quiet(picker.to_log2_with_epsilon, row)
                with np.errstate(all="ignore"):
                    h = np.max(bits) - t if scaling == "log2" else np.max(row) - 2 ** t
                pos = signal.find_peaks(bits)[0]
                assert not np.any(np.abs(bits[pos] - h) <= pc.MARGIN), (dtype, tag, scaling, t)
                if np.isfinite(h):
                    pos = pos[bits[pos] >= h]
                    assert not pc.equal_values_within(pos, bits[pos], max(pc.BITS_DISTANCES)), (dtype, tag, scaling, t)
            for d in pc.BITS_DISTANCES:
                cases[("bits", scaling, t, d)] = [
                    quiet(picker.find_peaks_with_bits, row.copy(), pc.SAMPLE_RATE_HZ, scaling, t, float(d)) for row in x]
    return cases


def bandpass_cases(out, dtype):
    x = np.stack([noise(np.random.default_rng(SEED + 900 + 10 * pc.DTYPES.index(dtype) + r), pc.BP_N, dtype)
                  for r in range(pc.RECORDS)])
    out[pc.x_key(dtype, "bp")] = x
    kept, results = [], []
    for name, (band, order) in pc.BP_DESIGNS.items():
        y = np.stack([picker.apply_bandpass(row.copy(), band, pc.FS_BP, order) for row in x])
        for kind in pc.TYPES:
            s = np.stack([quiet(picker.scale_signal_by_extraction_type, row, kind) for row in y])
            # the device's filtered record is the reference's to a few ulp: every comparison the picks rest on keeps a margin
            clear = np.all(np.abs(np.diff(s, axis=1)) > 1e-9)
            for h in pc.BP_HEIGHTS:
                cand = np.concatenate([row[signal.find_peaks(row)[0]] for row in s])
                if not clear or np.any(np.abs(cand - h) <= pc.MARGIN):
                    print("dropped", dtype, name, kind, h)
                    continue
                results.append([quiet(picker.find_peaks_by_extraction_type_with_bandpass, row.copy(), band, pc.FS_BP, order,
                                      kind, h) for row in x])
                kept.append(f"{name}|{kind}|{h}")
    out[f"{dtype}_bp_cases"] = np.array(kept)
    out[pc.peaks_key(dtype, "bp")] = pc.pack(results)


def helper_cases(out):
    """The three pure helpers: (sample rate, peak, intro, outro) rows, the indices and the cut lengths the reference gives
    for a record of 100 samples, and a comb."""
    rows = np.array([[10.0, 50, 1.0, 2.0], [10.0, 5, 1.0, 2.0], [10.0, 95, 0.35, 2.0], [8.0, 40, 0.0, 0.0], [3.0, 10, 2.5, 40.0]])
    x = np.arange(100.0)
    idx, cut = [], []
    for fs, peak, a, b in rows:
        idx.append(picker.extract_signal_index_with_buffer(fs, int(peak), a, b))
        piece = quiet(picker.extract_signal_with_buffer_seconds, x, fs, int(peak), a, b)
        cut.append([piece[0] if len(piece) else -1, len(piece)])
    out["helpers_rows"] = rows
    out["helpers_index"] = np.asarray(idx, dtype=np.int64)
    out["helpers_cut"] = np.asarray(cut, dtype=np.float64)
    out["helpers_comb_peaks"] = np.array([3, 17, 99], dtype=np.int64)
    out["helpers_comb"] = picker.find_peaks_to_comb_function(x, out["helpers_comb_peaks"])


def main():
    out = {}
    for di, dtype in enumerate(pc.DTYPES):
        for tag in pc.tags(dtype):
            if tag == "div":
                x = division_plateau(SEED + 700)
            else:
                x = records(dtype, int(tag[1:]), SEED + 1000 * di + int(tag[1:]))
            out[pc.x_key(dtype, tag)] = x
            cases = extraction_cases(out, dtype, tag, x)
            if pc.has_bits(tag):
                cases.update(bits_cases(dtype, tag, x))
            ids = pc.case_ids(tag)
            assert set(ids) == set(cases)
            out[pc.peaks_key(dtype, tag)] = pc.pack([cases[cid] for cid in ids])
        bandpass_cases(out, dtype)
    helper_cases(out)
    path = os.path.join(ROOT, "tests", "golden", "peaks.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, scipy.__version__, "quantum-inferno 1.1.3"]), **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays")


if __name__ == "__main__":
    main()
