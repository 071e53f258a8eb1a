"""Generator of tests/golden/decimate.npz -- TEST INFRASTRUCTURE, run where the reference package is installed or checked
out (QI_REFERENCE names its directory) and SciPy is.  Feeds the reference's utilities.sampling.decimate_timeseries (row by
row) and decimate_timeseries_collection (the block; the two must agree) seeded records and stores the inputs, the
reference's results, the tables SciPy designs for them (sos, zi in the record's type, the extension length) and the
sensitivity of the results to the last bit of those tables; nothing of the reference itself is copied.

    python tools/gen_golden_decimate.py

sens: as tools/gen_golden_filter.py defines it -- per record, the largest change of the decimated result, relative to the
record's largest result, over 8 seeded draws in which every section coefficient and zi entry moves by one ulp OF THE
TABLE'S TYPE up or down (SciPy's sosfilt on the same odd extension, with the moved tables)."""
import os
import sys

import numpy as np
import scipy
import scipy.signal as signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("QI_REFERENCE", "/root/reference"))

from quantum_inferno.utilities import sampling  # noqa: E402

import decimate_cases as dc  # noqa: E402
import filter_cases as fc  # noqa: E402


def design(q, dtype):
    """The tables scipy.signal.decimate(x, q, zero_phase=True) filters a record of `dtype` with."""
    sos = np.asarray(signal.cheby1(8, 0.05, 0.8 / q, output="sos"), dtype=dtype)
    ntaps = 2 * sos.shape[0] + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
    zi = signal.sosfilt_zi(sos)
    assert zi.dtype == sos.dtype == np.dtype(dtype)
    return {"sos": sos, "zi": zi, "edge": np.int64(3 * ntaps)}


def reference(x, q):
    rows = np.stack([sampling.decimate_timeseries(row.copy(), q) for row in x])
    block = sampling.decimate_timeseries_collection(x.copy(), q)
    assert rows.dtype == block.dtype == x.dtype and rows.shape == block.shape == (x.shape[0], dc.columns(x.shape[1], q))
    assert np.array_equal(rows, block)
    return np.ascontiguousarray(block)


def zero_phase(ext, d):
    """SciPy's two passes over the extended records with the given tables, in the tables' type."""
    y, _ = signal.sosfilt(d["sos"], ext, axis=-1, zi=d["zi"][:, None, :] * ext[:, :1][None, :, :])
    y, _ = signal.sosfilt(d["sos"], y[:, ::-1], axis=-1, zi=d["zi"][:, None, :] * y[:, -1:][None, :, :])
    assert y.dtype == ext.dtype
    return y[:, ::-1]


def moved(d, rng):
    out = dict(d)
    for k in ("sos", "zi"):
        v = d[k].copy()
        up = np.where(rng.integers(0, 2, v.shape) == 1, np.inf, -np.inf).astype(v.dtype)
        v = np.nextafter(v, up)
        assert v.dtype == d[k].dtype
        if k == "sos":
            v[:, 3] = 1.0
            v[d[k] == 0] = 0.0
        out[k] = v
    return out


def sensitivity(x, q, d, y_ref):
    edge = int(d["edge"])
    two = x.dtype.type(2)
    ext = np.concatenate((two * x[:, :1] - x[:, edge:0:-1], x, two * x[:, -1:] - x[:, -2:-(edge + 2):-1]), axis=1)
    keep = slice(edge, edge + x.shape[1], q)
    assert np.array_equal(zero_phase(ext, d)[:, keep], y_ref), q  # the same passes reproduce the reference
    rng = np.random.default_rng(20240607)
    worst = np.zeros(x.shape[0])
    for _ in range(8):
        y = zero_phase(ext, moved(d, rng))[:, keep].astype(np.float64)
        ref = y_ref.astype(np.float64)
        worst = np.maximum(worst, np.max(np.abs(y - ref), axis=1) / np.max(np.abs(ref), axis=1))
    return worst


def main():
    out = {}
    for q in dc.FACTORS:
        for dtype in dc.DTYPES:
            d = design(q, dtype)
            assert int(d["edge"]) == dc.EDGE and d["sos"].shape == (dc.SECTIONS, 6)
            for k, v in d.items():
                out[dc.table_key(q, dtype, k)] = v
            for n in dc.LENGTHS:
                x = fc.noise(dc.seed(q, dtype, n), dc.RECORDS, n, dtype)
                y = reference(x, q)
                out[dc.key(q, dtype, n, "x")] = x
                out[dc.key(q, dtype, n, "y")] = y
                out[dc.key(q, dtype, n, "sens")] = sensitivity(x, q, d, y)
    path = os.path.join(ROOT, "tests", "golden", "decimate.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, scipy.__version__, "quantum-inferno 1.1.3"]), **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays")
    for q in dc.FACTORS:
        for dtype in dc.DTYPES:
            print(q, dtype, "sens", max(float(out[dc.key(q, dtype, n, "sens")].max()) for n in dc.LENGTHS))


if __name__ == "__main__":
    main()
