"""Cases of the resampling tests and NumPy restatements of qi_interp_grid's and qi_resample_fft's semantics
(include/qi_tfr.h) without SciPy, shared by the CPU and GPU tests and by tools/gen_golden_resample.py.  The inputs are
built here from fixed seeds; tests/golden/resample.npz holds only what the reference returned for them."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))


T = _header_constant("QI_INTERP_TILE")   # outputs of one workgroup
K = _header_constant("QI_INTERP_KNOTS")  # knots a workgroup stages in LDS
DTYPES = ("float64", "float32")
FS = 800.0  # mean rate of the uneven records, Hz
EPOCH = 1.7e9 + 0.123
LENGTHS = (1, 2, 3, T - 1, T, T + 1, 3 * T + 17)
RATES = {"x2.37": FS * 2.37, "x1": FS, "x0.32": FS / 3.1, "none": None}
COMBOS = [(d, t0) for d in DTYPES for t0 in (0.0, EPOCH)]
SEED = 5200000
# (n, m) of the Fourier resampler
FFT_SHAPES = ((1024, 512), (1024, 1536), (1000, 441), (1001, 2000), (1009, 1013), (1013, 1009), (4096, 4096), (64, 1), (6, 9),
              (9, 6), (2, 2), (1, 5), (8190, 4099))
FFT_TOL = {"float64": 1e-11, "float32": 2e-5}  # of the record's maximum: the project's bounds for its hipFFT engine (README)


# ---- restatements ---------------------------------------------------------------------------------------------------------
def grid_ref(first, last, rate):
    """np.arange(first, last, 1 / rate) as (start, delta, m): the values are start + i * delta, i < m."""
    first, last = float(first), float(last)
    step = 1.0 / float(rate)
    m = max(int(np.ceil((last - first) / step)), 0)
    return first, (first + step) - first, m


def grid_values(start, delta, m):
    return start + np.arange(m, dtype=np.float64) * delta


def interp_ref(x, xp, fp):
    """np.interp(x, xp, fp) restated (include/qi_tfr.h, qi_interp_grid): every operation a NumPy float64 operation of its own."""
    x = np.asarray(x, dtype=np.float64)
    xp = np.asarray(xp, dtype=np.float64)
    fp = np.asarray(fp).astype(np.float64)
    n = len(xp)
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 1)  # the last index with xp[j] <= x
    j1 = np.minimum(j + 1, n - 1)
    with np.errstate(all="ignore"):
        s = (fp[j1] - fp[j]) / (xp[j1] - xp[j])
        r = s * (x - xp[j]) + fp[j]
        r2 = s * (x - xp[j1]) + fp[j1]
    again = np.isnan(r)
    r = np.where(again, r2, r)
    r = np.where(again & np.isnan(r2) & (fp[j] == fp[j1]), fp[j], r)
    r = np.where((j == n - 1) | (xp[j] == x), fp[j], r)
    r = np.where(x > xp[-1], fp[-1], r)
    return np.where(x < xp[0], fp[0], r)


def fft_resample_ref(x, m):
    """scipy.signal.resample(x, m, axis=-1) of real records, no window, in float64 (SciPy's bits for float64 records)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    X = np.fft.rfft(x, axis=-1)
    Y = np.zeros(x.shape[:-1] + (m // 2 + 1,), dtype=complex)
    N = min(n, m)
    Y[..., :N // 2 + 1] = X[..., :N // 2 + 1]
    if N % 2 == 0:
        if m < n:
            Y[..., N // 2] *= 2.0
        elif n < m:
            Y[..., N // 2] *= 0.5
    return np.fft.irfft(Y, m, axis=-1) * (float(m) / float(n))


def same_bits(a, b):
    """Equal shapes, dtypes and bits; any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(bits)[~nan], b.view(bits)[~nan])


# ---- uneven records ---------------------------------------------------------------------------------------------------------
def jittered(rng, n, t0, fs=FS):
    """n timestamps from t0 whose steps are 1 / fs +- 30 %."""
    steps = (1.0 + 0.3 * rng.uniform(-1.0, 1.0, max(n - 1, 0))) / fs
    return t0 + np.concatenate([[0.0], np.cumsum(steps)])


def uneven_record(n, dtype, t0):
    """(timestamps [n] float64, values [n] of dtype): 30 % jitter; from T - 1 samples on, runs of duplicate timestamps, one of
    them over the samples a workgroup boundary falls on at unit rate; at T + 1 samples NaN, +-inf and adjacent equal infinities."""
    rng = np.random.default_rng(SEED + 10 * n + DTYPES.index(dtype) + (2 if t0 else 0))
    steps = (1.0 + 0.3 * rng.uniform(-1.0, 1.0, max(n - 1, 0))) / FS
    if n >= T - 1:
        steps[40:43] = 0.0
        steps[T - 6:T - 2] = 0.0
        steps[200] = 0.0
    ts = t0 + np.concatenate([[0.0], np.cumsum(steps)])
    y = rng.standard_normal(n).astype(dtype)
    if n == T + 1:
        y[17] = np.nan
        y[90], y[91] = np.inf, np.inf  # adjacent equal infinities: the slope is NaN and the result inf
        y[150] = -np.inf
        y[300] = np.inf
        y[41] = np.nan  # a NaN on a run of duplicate timestamps
    return ts, y


def interp_cases():
    """(n, rate name) of every case of the matrix: a record of one sample has no average rate."""
    return [(n, rk) for n in LENGTHS for rk in RATES if not (n == 1 and rk == "none")]


def fixture_combo(n, rk):
    """The (dtype, t0) whose reference result the fixture holds for case (n, rate name): the four of them in turn, so every
    length and every rate meets every dtype and both epochs."""
    return COMBOS[(LENGTHS.index(n) + list(RATES).index(rk)) % len(COMBOS)]


def interp_key(n, rk):
    return f"interp_n{n}_{rk}"


def on_grid_record(dtype):
    """Timestamps k / 1024 exactly: at 1024 and 2048 Hz every (every second) output lies on a knot."""
    n = 300
    rng = np.random.default_rng(SEED + 7000 + DTYPES.index(dtype))
    return np.arange(n, dtype=np.float64) / 1024.0, rng.standard_normal(n).astype(dtype)


ON_GRID_RATES = (1024.0, 2048.0)


def gap_record(dtype):
    """Unit-rate record with one interval that spans 3 T + 100 outputs: whole workgroups sit inside it."""
    rng = np.random.default_rng(SEED + 7100 + DTYPES.index(dtype))
    a = jittered(rng, 200, 5.0)
    b = jittered(rng, 300, a[-1] + (3 * T + 100) / FS)
    ts = np.concatenate([a, b])
    return ts, rng.standard_normal(len(ts)).astype(dtype)


def burst_record(held, dtype):
    """(timestamps, values, start, delta, m): on the grid i * 1.0 the first workgroup's outputs 0 .. T - 1 bracket exactly
    `held` knots -- knot 0 on output 0, held - 2 knots between outputs 100 and 400, the next knot behind output T - 1 --
    and the following workgroups run over ordinary knots."""
    rng = np.random.default_rng(SEED + 7200 + held + DTYPES.index(dtype))
    inner = held - 2
    burst = 100.0 + 300.0 * (np.arange(inner, dtype=np.float64) + 1.0) / inner
    tail = T + 88.0 + np.cumsum(0.7 * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, 2 * T)))
    ts = np.concatenate([[0.0], burst, tail])
    assert np.all(np.diff(ts) >= 0) and ts[inner] <= T - 1 < ts[inner + 1]
    return ts, rng.standard_normal(len(ts)).astype(dtype), 0.0, 1.0, 2 * T + 37


def many_clocks(records, dtype):
    """(timestamps [records, n], values [records, n], start, delta, m): every row the same jittered clock shifted and
    stretched differently; the common grid starts before some rows' first knot and ends behind some rows' last."""
    n = 3 * T + 17
    rng = np.random.default_rng(SEED + 7300 + DTYPES.index(dtype))
    base = jittered(rng, n, 0.0)
    shift = rng.uniform(-0.2, 0.2, records)
    stretch = 1.0 + rng.uniform(-0.1, 0.1, records)
    ts = EPOCH + shift[:, None] + stretch[:, None] * base[None, :]
    y = rng.standard_normal((records, n)).astype(dtype)
    start, delta, m = grid_ref(EPOCH - 0.1, EPOCH + base[-1] + 0.1, FS * 1.3)
    return np.ascontiguousarray(ts), y, start, delta, m


# ---- Fourier resampler -------------------------------------------------------------------------------------------------------
def fft_record(n, m, dtype):
    rng = np.random.default_rng(SEED + 9000 + 17 * n + m + DTYPES.index(dtype))
    return (rng.standard_normal(n) + 0.5).astype(dtype)


def fft_key(n, m, dtype):
    return f"fft_{dtype}_n{n}_m{m}"


def fft_batch(n, m, dtype, records):
    """(records [R, n], factors [R]): the fixture's record times a power of two of either sign per row -- exact in binary
    floating point, in the transform as well, so the reference's result for row r is its recorded result times factors[r]."""
    factors = np.array([(1.0, -2.0, 0.5, -1.0, 4.0)[r % 5] for r in range(records)])
    x = fft_record(n, m, dtype)
    return (factors[:, None] * x[None, :].astype(np.float64)).astype(dtype), factors
