"""Cases of the integration / differentiation tests and NumPy restatements of qi_cumtrapz's and qi_derivative's semantics
(include/qi_tfr.h), shared by the CPU and GPU tests and by tools/gen_golden_calculus.py.  The inputs are built here from
fixed seeds; tests/golden/calculus.npz holds only what the reference returned for them."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))


T = _header_constant("QI_SCAN_TILE")  # terms of one tile of the summation tree
LANES, RUN, WAVE = 256, 16, 64        # lanes of a tile, consecutive terms of a lane, lanes of a wave
DTYPES = ("float64", "float32")
FS = 800.0                            # mean rate of the jittered timestamps, Hz
EPOCH = 1.7e9 + 0.123
LENGTHS = (1, 2, 3, 17, 1025, T, T + 1, T + 2, 2 * T + 1, 3 * T + 17)
LONG = (1 << 20) + T + 2              # more than 256 tiles: past any width a carry pass could have
RECORDS = (1, 3, 65)
LAYOUTS = ("dx", "shared0", "sharedE", "rows0", "rowsE")  # constant spacing; shared / per-record timestamps near 0 / at the epoch
SEED = 6100000
EXACT_RATE = 1024.0
TOL = {"float64": 1e-11, "float32": 2e-5}  # of the result's maximum: the project's bounds
UNIT = {"float64": 2.0 ** -53, "float32": 2.0 ** -24}
FILL_TYPES = ("zero", "nan", "mean", "median", "min", "max", "tail", "head")
FILL_LOCATIONS = ("start", "end")
FILL_N = 257
WRAP_LENGTHS = (1025, T + 17)  # records whose results the fixture holds for the wrappers
GRAD_N = 1025


# ---- restatements ---------------------------------------------------------------------------------------------------------
def terms_ref(y, x=None, dx=1.0):
    """The terms of scipy.integrate.cumulative_trapezoid along the last axis, by SciPy's own expression: dx a Python float
    (a float32 record then stays float32), x float64 [n] or [C, n] (the result is float64)."""
    y = np.asarray(y)
    d = dx if x is None else np.diff(np.asarray(x, dtype=np.float64), axis=-1)
    with np.errstate(all="ignore"):
        return d * (y[..., 1:] + y[..., :-1]) / 2.0


def scan_ref(terms):
    """qi_cumtrapz's summation tree (include/qi_tfr.h) on terms [C, N] -> [C, N + 1], every addition in the terms' type:
    lanes sum 16 consecutive terms left to right, a Hillis-Steele scan over the 64 lanes of a wave, the four waves of a
    tile and the tiles of a record left to right, out = (carry + (wave offset + lane's exclusive value)) + running sum."""
    t = np.asarray(terms)
    C, N = t.shape
    tiles = max(-(-N // T), 1)
    p = np.zeros((C, tiles * T), t.dtype)
    p[:, :N] = t
    p = p.reshape(C, tiles, LANES // WAVE, WAVE, RUN)
    with np.errstate(all="ignore"):
        r = np.cumsum(p, axis=-1)  # r_0 = t_0, r_k = r_(k-1) + t_k
        v = r[..., -1].copy()
        for s in (1, 2, 4, 8, 16, 32):
            nv = v.copy()
            nv[..., s:] = v[..., :-s] + v[..., s:]
            v = nv
        e = np.zeros_like(v)
        e[..., 1:] = v[..., :-1]
        W = v[..., -1]
        o = np.zeros_like(W)
        o[..., 1] = W[..., 0]
        o[..., 2] = W[..., 0] + W[..., 1]
        o[..., 3] = o[..., 2] + W[..., 2]
        total = o[..., 3] + W[..., 3]
        c = np.zeros_like(total)
        c[:, 1:] = np.cumsum(total[:, :-1], axis=1)  # c_1 = T_0, c_t = c_(t-1) + T_(t-1)
        tiles_out = (c[:, :, None, None, None] + (o[..., None, None] + e[..., None])) + r
    assert tiles_out.dtype == t.dtype and r.dtype == t.dtype
    out = np.zeros((C, N + 1), t.dtype)
    out[:, 1:] = tiles_out.reshape(C, -1)[:, :N]
    return out


def cumtrapz_ref(y, x=None, dx=1.0):
    """What qi_cumtrapz returns for records [C, n]."""
    return scan_ref(terms_ref(y, x, dx))


def exact_sums(terms):
    """The float64 running sum of the terms as they are (the float32 ones widened), with the leading 0."""
    t = np.asarray(terms, dtype=np.float64)
    return np.concatenate([np.zeros(t.shape[:-1] + (1,)), np.cumsum(t, axis=-1)], axis=-1)


def gradient_ref(y, x=None, h=1.0):
    """np.gradient(y, h | x, axis=-1, edge_order=1) restated (include/qi_tfr.h, QI_DERIV_GRADIENT); always the uneven
    formula when x is given."""
    f = np.asarray(y)
    out = np.empty_like(f)
    with np.errstate(all="ignore"):
        if x is None:
            out[..., 1:-1] = (f[..., 2:] - f[..., :-2]) / (2.0 * h)
            out[..., 0] = (f[..., 1] - f[..., 0]) / h
            out[..., -1] = (f[..., -1] - f[..., -2]) / h
        else:
            d = np.diff(np.asarray(x, dtype=np.float64), axis=-1)
            dx1, dx2 = d[..., :-1], d[..., 1:]
            a = -(dx2) / (dx1 * (dx1 + dx2))
            b = (dx2 - dx1) / (dx1 * dx2)
            c = dx1 / (dx2 * (dx1 + dx2))
            out[..., 1:-1] = a * f[..., :-2] + b * f[..., 1:-1] + c * f[..., 2:]
            out[..., 0] = (f[..., 1] - f[..., 0]) / d[..., 0]
            out[..., -1] = (f[..., -1] - f[..., -2]) / d[..., -1]
    return out


def difference_ref(y, x=None, rate=1.0):
    """np.diff(y) * rate (rate a Python float) or np.diff(y) / np.diff(x) along the last axis (QI_DERIV_DIFFERENCE)."""
    with np.errstate(all="ignore"):
        if x is None:
            return np.diff(np.asarray(y), axis=-1) * rate
        return np.diff(np.asarray(y), axis=-1) / np.diff(np.asarray(x, dtype=np.float64), axis=-1)


def same_bits(a, b):
    """Equal shapes, dtypes and bits; any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(bits)[~nan], b.view(bits)[~nan])


def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.asarray(a)
    return (np.isnan(a) * 1 + (a == np.inf) * 2 + (a == -np.inf) * 3).astype(np.int8)


# ---- records --------------------------------------------------------------------------------------------------------------
def timestamps(n, layout, records=1):
    """None for "dx"; jittered timestamps (steps of 1 / FS +- 30 %), [n] for "shared*", [records, n] for "rows*" (every
    row its own clock), from 0 or from the epoch."""
    if layout == "dx":
        return None
    rng = np.random.default_rng(SEED + 31 * n + LAYOUTS.index(layout))
    rows = records if layout.startswith("rows") else 1
    steps = (1.0 + 0.3 * rng.uniform(-1.0, 1.0, (rows, max(n - 1, 0)))) / FS
    ts = (EPOCH if layout.endswith("E") else 0.0) + np.concatenate([np.zeros((rows, 1)), np.cumsum(steps, axis=1)], axis=1)
    return np.ascontiguousarray(ts if layout.startswith("rows") else ts[0])


def random_records(n, dtype, records=1, salt=0):
    """Zero-mean records [records, n]."""
    rng = np.random.default_rng(SEED + 1000 + 17 * n + DTYPES.index(dtype) + 7 * salt)
    y = rng.standard_normal((records, n))
    return (y - y.mean(axis=1, keepdims=True)).astype(dtype)


def exact_record(n, dtype):
    """Integer samples in [-8, 8]: at EXACT_RATE = 1024 Hz every term and every partial sum is a multiple of 2^-11 below
    2^13 -- exact in float32, whatever the order of summation."""
    rng = np.random.default_rng(SEED + 2000 + n)
    return rng.integers(-8, 9, n).astype(dtype)


def exact_timestamps(n, epoch):
    return (1700000000.0 if epoch else 0.0) + np.arange(n, dtype=np.float64) / EXACT_RATE


def exact_key(n, dtype, form):
    return f"exact_{dtype}_{form}_n{n}"


SPECIAL_N = 2 * T + 17
SPECIAL_AT = (0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, SPECIAL_N - 1)
SPECIAL_VALUES = (np.nan, np.inf, -np.inf)


def special_records(dtype):
    """Rows of SPECIAL_N samples: one NaN, +inf or -inf each, at the first and last sample of a tile and on both sides of a
    tile boundary (samples and terms: term i reads samples i and i + 1); then rows with +inf and -inf on either side of
    a boundary, and two equal infinities next to each other."""
    base = random_records(SPECIAL_N, dtype, 1, salt=3)[0]
    rows = []
    for at in SPECIAL_AT:
        for value in SPECIAL_VALUES:
            y = base.copy()
            y[at] = value
            rows.append(y)
    for first, second in ((T - 2, T + 2), (T, 2 * T + 3), (5, 6)):
        y = base.copy()
        y[first], y[second] = np.inf, -np.inf
        rows.append(y)
    y = base.copy()
    y[T - 1], y[T] = np.inf, np.inf
    rows.append(y)
    return np.ascontiguousarray(np.stack(rows))


def batch_of(record, records):
    """(rows [records, n], factors [records]): the record times a power of two of either sign per row -- exact in binary
    floating point through every sum, product and quotient here, so row r of a result is the record's result times
    factors[r]."""
    factors = np.array([(1.0, -2.0, 0.5, -1.0, 4.0)[r % 5] for r in range(records)])
    return (factors[:, None] * record[None, :].astype(np.float64)).astype(record.dtype), factors


def fill_record(dtype, with_nan=False):
    y = random_records(FILL_N, dtype, 1, salt=5)[0]
    if with_nan:
        y[100] = np.nan
    return y


def fill_timestamps():
    return timestamps(FILL_N, "sharedE")


def fill_key(dtype, form, fill_type, fill_loc, with_nan=False):
    return f"diff_{dtype}_{form}_{fill_type}_{fill_loc}" + ("_nan" if with_nan else "")


WINDOW_CASES = ((0, 0.5), (1, 0.5), (2, 0.5), (17, 0.5), (256, 0.25), (1001, 0.1), (64, 0.0), (64, 1.0), (33, 1.5))  # (points, alpha)
BUFFER_CASES = ((100, 10, 0.5), (101, 25, 0.25), (64, 32, 0.5), (20, 11, 0.5), (10, 0, 0.5), (7, 4, 1.0))  # (points, taper_num, alpha)
BUFFER_S_CASES = ((800, 0.1, 800.0, 0.5), (800, 0.26, 48.0, 0.3), (30, 1.0, 16.0, 0.5))  # (points, taper_s, rate, alpha)
