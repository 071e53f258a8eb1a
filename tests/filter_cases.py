"""Cases of the zero-phase filter tests and a NumPy restatement of qi_filtfilt's semantics (include/qi_tfr.h), shared by
the CPU and GPU tests and by tools/gen_golden_filter.py.  The restatement is a plain loop over time (vectorised over the
records only), every product and sum rounded on its own, in the order SciPy's lfilter / sosfilt evaluate them."""
import numpy as np

QI_IIR_BA, QI_IIR_SOS = 0, 1
RECORDS = 3
GRID = 1024.0
# name -> (wrapper, filter order, band in units of Nyquist (butter_*) or in Hz at FS_SOS (apply_bandpass))
FS_BA = 2.0  # sample rate the butter_* wrappers are called with: the cut-offs in Hz are then the fractions of Nyquist
FS_SOS = 1000.0
DESIGNS = {
    "lp2": ("lowpass", 2, (0.3,)),
    "lp4": ("lowpass", 4, (0.1,)),
    "hp4": ("highpass", 4, (0.01,)),
    "bp4": ("bandpass", 4, (0.05, 0.2)),
    "bp4low": ("bandpass", 4, (0.005, 0.05)),
    "bp8": ("bandpass", 8, (0.1, 0.3)),  # (b, a) of order 16, the cap of the C ABI
    "sos7": ("sos", 7, (100.0, 200.0)),  # 7 sections
    "sos3": ("sos", 3, (10.0, 400.0)),
}
F32_DESIGNS = ("lp4", "bp4", "sos7")
TUKEY_ALPHA = 0.5


def form_of(name):
    return QI_IIR_SOS if DESIGNS[name][0] == "sos" else QI_IIR_BA


def lengths(edge):
    """The shortest legal record (both extensions reach across the whole record), a short one, and a prime length (every
    time tile ragged, no row after the first aligned)."""
    return (edge + 1, 300, 1031)


def cases(g):
    """(name, dtype, n) of every case of fixture g."""
    out = []
    for name in DESIGNS:
        for dtype in ("float64", "float32"):
            if dtype == "float32" and name not in F32_DESIGNS:
                continue
            for n in lengths(int(g[f"{name}_edge"])):
                out.append((name, dtype, n))
    return out


def key(name, dtype, n, what):
    return f"{name}_{dtype}_n{n}_{what}"


def tables(g, name):
    """(form, coef, zi, edge) of design `name` as the C ABI takes them."""
    edge = int(g[f"{name}_edge"])
    if form_of(name) == QI_IIR_SOS:
        return QI_IIR_SOS, np.ascontiguousarray(g[f"{name}_sos"]), np.ascontiguousarray(g[f"{name}_zi"]), edge
    return QI_IIR_BA, np.ascontiguousarray(np.stack([g[f"{name}_b"], g[f"{name}_a"]])), np.ascontiguousarray(g[f"{name}_zi"]), edge


def noise(seed, records, n, dtype):
    """Seeded noise with a non-zero mean on a grid of 2^-10."""
    rng = np.random.default_rng(seed)
    x = np.round((rng.standard_normal((records, n)) + 0.75) * GRID) / GRID
    return x.astype(dtype)


def tukey_symmetric(n, alpha):
    """scipy.signal.windows.tukey(n, alpha) (sym=True), restated for the tests."""
    if n == 1 or alpha <= 0:
        return np.ones(n)
    if alpha >= 1.0:
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))  # (not used by the cases)
    k = np.arange(0, n)
    width = int(np.floor(alpha * (n - 1) / 2.0))
    n1, n2, n3 = k[0:width + 1], k[width + 1:n - width - 1], k[n - width - 1:]
    w1 = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * n1 / alpha / (n - 1))))
    w3 = 0.5 * (1 + np.cos(np.pi * (-2.0 / alpha + 1 + 2.0 * n3 / alpha / (n - 1))))
    return np.concatenate((w1, np.ones(n2.shape), w3))


def _pass_ba(x, b, a, z):
    """One lfilter pass over the columns of x [R, m] from the state z [R, N]; returns y [R, m]."""
    order = len(b) - 1
    y = np.empty_like(x)
    z = z.copy()
    for k in range(x.shape[1]):
        xk = x[:, k]
        yk = b[0] * xk + z[:, 0]
        for i in range(order - 1):
            z[:, i] = (b[i + 1] * xk + z[:, i + 1]) - a[i + 1] * yk
        z[:, order - 1] = b[order] * xk - a[order] * yk
        y[:, k] = yk
    return y


def _pass_sos(x, sos, z):
    """One sosfilt pass; z [R, S, 2]."""
    y = np.empty_like(x)
    z = z.copy()
    for k in range(x.shape[1]):
        xc = x[:, k]
        for s in range(sos.shape[0]):
            xn = sos[s, 0] * xc + z[:, s, 0]
            z[:, s, 0] = (sos[s, 1] * xc - sos[s, 4] * xn) + z[:, s, 1]
            z[:, s, 1] = sos[s, 2] * xc - sos[s, 5] * xn
            xc = xn
        y[:, k] = xc
    return y


def filtfilt_ref(x, form, coef, zi, edge, taper=None):
    """qi_filtfilt's semantics on records x [R, n] (float32 or float64): -> [R, n] float64."""
    x = np.array(x, copy=True)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64) and x.shape[1] > edge
    if taper is not None:
        x[...] = (x.astype(np.float64) * taper).astype(x.dtype)  # the product in float64, rounded to the record's type
    two = x.dtype.type(2)
    ext = np.concatenate((two * x[:, :1] - x[:, edge:0:-1], x, two * x[:, -1:] - x[:, -2:-(edge + 2):-1]), axis=1)
    assert ext.dtype == x.dtype and ext.shape[1] == x.shape[1] + 2 * edge
    ext = ext.astype(np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    zi = np.asarray(zi, dtype=np.float64)
    if form == QI_IIR_BA:
        run = lambda v, s: _pass_ba(v, coef[0], coef[1], zi[None, :] * s[:, None])  # noqa: E731
    else:
        run = lambda v, s: _pass_sos(v, coef, zi[None, :, :] * s[:, None, None])  # noqa: E731
    y = run(ext, ext[:, 0])
    y = run(y[:, ::-1], y[:, -1])[:, ::-1]
    return np.ascontiguousarray(y[:, edge:edge + x.shape[1]])
