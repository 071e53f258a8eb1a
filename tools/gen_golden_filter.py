"""Generator of tests/golden/filter.npz -- TEST INFRASTRUCTURE, run where the reference package is installed or checked
out (QI_REFERENCE names its directory) and SciPy is.  Feeds the reference's styx_fft.butter_lowpass / butter_highpass /
butter_bandpass and utilities.picker.apply_bandpass seeded records, row by row, and stores the inputs, the reference's
results, the tables SciPy designs for them (b, a or sos, zi, the extension length) and the sensitivity of the results to
the last bit of those tables; nothing of the reference itself is copied.

    python tools/gen_golden_filter.py

sens: per record, the largest change of the zero-phase result, relative to the record's largest result, over 8 seeded
draws in which every coefficient and zi entry moves by one ulp up or down (SciPy's lfilter / sosfilt on the same odd
extension, with the moved tables).  The (b, a) form at low cut-offs is ill-conditioned: that is the reference's property."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import scipy
import scipy.signal as signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("QI_REFERENCE", "/root/reference"))

from quantum_inferno import styx_fft  # noqa: E402
from quantum_inferno.utilities import picker  # noqa: E402

import filter_cases as fc  # noqa: E402


def design(name):
    kind, order, band = fc.DESIGNS[name]
    if kind == "sos":
        sos = signal.butter(order, band, fs=fc.FS_SOS, btype="band", output="sos")
        ntaps = 2 * sos.shape[0] + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
        return {"sos": sos, "zi": signal.sosfilt_zi(sos), "edge": np.int64(3 * ntaps)}
    b, a = signal.butter(N=order, Wn=list(band), btype=kind)
    return {"b": b, "a": a, "zi": signal.lfilter_zi(b, a), "edge": np.int64(3 * max(len(a), len(b)))}


def reference_rows(name, x):
    kind, order, band = fc.DESIGNS[name]
    rows = []
    for row in x:
        with redirect_stdout(io.StringIO()):
            if kind == "sos":
                y = picker.apply_bandpass(row.copy(), band, fc.FS_SOS, order)
            elif kind == "bandpass":
                y = styx_fft.butter_bandpass(row.copy(), fc.FS_BA, band[0], band[1], order, fc.TUKEY_ALPHA)
            elif kind == "highpass":
                y = styx_fft.butter_highpass(row.copy(), fc.FS_BA, band[0], order, fc.TUKEY_ALPHA)
            else:
                y = styx_fft.butter_lowpass(row.copy(), fc.FS_BA, band[0], order, fc.TUKEY_ALPHA)
        assert y.dtype == np.float64 and y.shape == row.shape
        rows.append(y)
    return np.ascontiguousarray(np.stack(rows))


def zero_phase(ext, d, sos):
    """SciPy's two passes over the extended records with the given tables."""
    if sos:
        y, _ = signal.sosfilt(d["sos"], ext, axis=-1, zi=d["zi"][:, None, :] * ext[:, :1][None, :, :])
        y, _ = signal.sosfilt(d["sos"], y[:, ::-1], axis=-1, zi=d["zi"][:, None, :] * y[:, -1:][None, :, :])
    else:
        y, _ = signal.lfilter(d["b"], d["a"], ext, axis=-1, zi=d["zi"][None, :] * ext[:, :1])
        y, _ = signal.lfilter(d["b"], d["a"], y[:, ::-1], axis=-1, zi=d["zi"][None, :] * y[:, -1:])
    return y[:, ::-1]


def moved(d, rng, sos):
    out = dict(d)
    for k in (("sos", "zi") if sos else ("b", "a", "zi")):
        v = d[k].copy()
        v = np.nextafter(v, np.where(rng.integers(0, 2, v.shape) == 1, np.inf, -np.inf))
        if k == "a":
            v[0] = 1.0
        if k == "sos":
            v[:, 3] = 1.0
            v[d[k] == 0] = 0.0
        out[k] = v
    return out


def sensitivity(name, x, d, y_ref):
    sos = fc.form_of(name) == fc.QI_IIR_SOS
    edge = int(d["edge"])
    x = x.copy()
    if not sos:
        x *= signal.windows.tukey(M=x.shape[1], alpha=fc.TUKEY_ALPHA)
    two = x.dtype.type(2)
    ext = np.concatenate((two * x[:, :1] - x[:, edge:0:-1], x, two * x[:, -1:] - x[:, -2:-(edge + 2):-1]), axis=1).astype(np.float64)
    keep = slice(edge, edge + x.shape[1])
    assert np.array_equal(zero_phase(ext, d, sos)[:, keep], y_ref), name  # the same passes reproduce the reference
    rng = np.random.default_rng(20240607)
    worst = np.zeros(x.shape[0])
    for _ in range(8):
        y = zero_phase(ext, moved(d, rng, sos), sos)[:, keep]
        worst = np.maximum(worst, np.max(np.abs(y - y_ref), axis=1) / np.max(np.abs(y_ref), axis=1))
    return worst


def main():
    out = {}
    for di, name in enumerate(fc.DESIGNS):
        d = design(name)
        for k, v in d.items():
            out[f"{name}_{k}"] = v
        for ti, dtype in enumerate(("float64", "float32")):
            if dtype == "float32" and name not in fc.F32_DESIGNS:
                continue
            for n in fc.lengths(int(d["edge"])):
                x = fc.noise(100000 * ti + 1000 * di + n, fc.RECORDS, n, dtype)
                y = reference_rows(name, x)
                out[fc.key(name, dtype, n, "x")] = x
                out[fc.key(name, dtype, n, "y")] = y
                out[fc.key(name, dtype, n, "sens")] = sensitivity(name, x, d, y)
    path = os.path.join(ROOT, "tests", "golden", "filter.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, scipy.__version__, "quantum-inferno 1.1.3"]), **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays")
    for name in fc.DESIGNS:
        print(name, "edge", int(out[f"{name}_edge"]), "sens", max(float(out[k].max()) for k in out if k.startswith(name + "_") and k.endswith("_sens")))


if __name__ == "__main__":
    main()
