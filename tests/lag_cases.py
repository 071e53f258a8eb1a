"""Cases and the float64 NumPy restatement of qi_pair_lags (include/qi_lags.h): a plain helper module, importable on the CPU.

restate() is the header's definition word for word: the per-bin weights, numpy.fft.irfft of the zero-padded spectrum,
numpy.argmax over the lag window, the three-point parabola with circular neighbours.  tests/test_lags_cpu.py holds it against
a time-domain numpy.correlate and holds the fixtures' conditions; tests/test_gpu_lags.py compares the device with it on the
same matrices, upcast.

Parity fixtures: a few averaged "segments" of band-shaped noise from one source, delayed per sensor on the finer grid by an
integer plus 0 .. 4 tenths (so a pair's delay is an integer or a fraction that is never within a tenth of the half-way point
between two samples), plus independent noise, with qi_csd's one-sided doubling.  The delays are kept inside the lag window.
"""
import collections
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float32", "float64")
# the array tests' reduction contract: |d r| <= TOL max |r| of the case
TOL = {"float32": 1e-4, "float64": 1e-10}
MARGIN = 1e-2  # the restatement's maximum exceeds every non-adjacent sample of the window by this much of the peak
WEIGHTINGS = ("plain", "phat", "scot")
BIN_KINDS = ("all", "no_dc", "low", "mid", "high")

Case = collections.namedtuple("Case", "id L upsample C nstack max_lag weighting halve normalize bins")


def _case(L, up, C, nstack, max_lag, weighting, halve, normalize, bins):
    lag = L // 2 - 1 if max_lag == "full" else max_lag
    cid = f"L{L}_u{up}_c{C}_s{nstack}_m{max_lag}_{WEIGHTINGS[weighting]}_h{int(halve)}n{int(normalize)}_{bins}"
    return Case(cid, L, up, C, nstack, lag, weighting, bool(halve), bool(normalize), bins)


# every L x upsample the call has a pass structure for (log2 M = 5, 6, 10, 12: first passes of radix 2 and 4, and none), and
# every value of the other arguments at least once beside each
CASES = (
    _case(64, 1, 2, 1, 0, 0, 1, 1, "all"), _case(64, 1, 17, 3, 17, 1, 0, 0, "mid"), _case(64, 1, 5, 1, "full", 2, 1, 0, "no_dc"),
    _case(64, 1, 3, 3, 1, 0, 0, 0, "high"),
    _case(128, 1, 3, 1, 1, 1, 1, 1, "low"), _case(128, 1, 5, 3, "full", 0, 1, 1, "all"), _case(128, 1, 17, 1, 0, 2, 0, 1, "high"),
    _case(128, 1, 2, 3, 17, 2, 1, 1, "mid"),
    _case(2048, 1, 5, 1, 17, 0, 1, 1, "mid"), _case(2048, 1, 2, 3, "full", 1, 1, 1, "no_dc"), _case(2048, 1, 3, 1, 0, 2, 0, 0, "low"),
    _case(2048, 4, 17, 3, 17, 1, 0, 1, "all"), _case(2048, 4, 3, 1, "full", 0, 1, 0, "high"), _case(2048, 4, 5, 3, 1, 2, 1, 1, "no_dc"),
    _case(2048, 4, 2, 1, 0, 1, 1, 0, "mid"),
    _case(8192, 1, 3, 3, 17, 2, 1, 0, "all"), _case(8192, 1, 5, 1, "full", 1, 0, 1, "low"), _case(8192, 1, 2, 1, 1, 0, 0, 1, "high"),
    _case(8192, 4, 5, 3, "full", 0, 1, 1, "no_dc"), _case(8192, 4, 2, 3, 17, 1, 1, 1, "low"), _case(8192, 4, 3, 1, 1, 2, 0, 1, "mid"),
    _case(8192, 4, 17, 1, 0, 0, 0, 0, "all"),
)


def ids():
    return [c.id for c in CASES]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def complex_of(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def pair_table(C):
    """(i [npair], j [npair]) of the pairs in the header's order."""
    return np.triu_indices(C, 1)


def pair_index(C, i, j):
    return i * C - i * (i + 1) // 2 + (j - i - 1)


def bin_range(kind, nf):
    lo, hi = nf // 8, nf // 8 + nf // 2
    return {"all": (0, nf), "no_dc": (1, nf), "low": (0, hi), "mid": (lo, hi), "high": (lo, nf)}[kind]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
Restated = collections.namedtuple("Restated", "r cc peak_lag peak_value index delta bound")


def restate(csd, bins=None, weighting=0, halve=True, normalize=True, upsample=1, max_lag=None):
    """csd [nstack, nf, C, C] -> Restated, all float64: r [nstack, npair, L] the whole correlation, cc its window, peak_lag in
    samples of the records, peak_value, index (the integer lag of the first maximum), delta (the parabola's offset) and bound:
    |d delta / d a| + |d delta / d b| + |d delta / d c|, the first-order propagation of an error of a, b, c into delta."""
    s = np.asarray(csd).astype(np.complex128)
    nstack, nf, C, _ = s.shape
    nfft = 2 * (nf - 1)
    L = nfft * upsample
    M = L // 2
    lo, hi = (0, nf) if bins is None else bins
    max_lag = M - 1 if max_lag is None else max_lag
    rows, cols = pair_table(C)
    f = np.arange(nf)
    band = (f >= lo) & (f < hi)
    h = np.where(bool(halve) & (f > 0) & (f < nfft // 2), 0.5, 1.0)
    mult = np.where((f == 0) | (f == M), 1.0, 2.0)
    sij = np.moveaxis(s[:, :, rows, cols], 1, 2)  # [nstack, npair, nf]
    aii = np.moveaxis(s[:, :, rows, rows].real, 1, 2)
    ajj = np.moveaxis(s[:, :, cols, cols].real, 1, 2)
    autos = weighting == 2 or (normalize and weighting == 0)
    with np.errstate(all="ignore"):
        if weighting == 0:
            w = np.ones(sij.shape)
        elif weighting == 1:
            mag = np.abs(sij)
            w = np.where(mag == 0, 0.0, 1.0 / np.where(mag == 0, 1.0, mag))
        else:
            prod = np.sqrt(aii) * np.sqrt(ajj)
            zero = (aii == 0) | (ajj == 0)
            w = np.where(zero, 0.0, 1.0 / np.where(zero, 1.0, prod))
        x = np.where(band, sij * w * h, 0.0)
        bad = (~np.isfinite(np.where(band, sij, 0.0))).any(axis=-1) | (~np.isfinite(x)).any(axis=-1)
        if autos:
            bad |= (~np.isfinite(np.where(band, aii, 0.0))).any(axis=-1) | (~np.isfinite(np.where(band, ajj, 0.0))).any(axis=-1)
        x = np.where(bad[..., None], 0.0, x)
        spectrum = np.zeros(sij.shape[:2] + (M + 1,), dtype=np.complex128)
        spectrum[..., :nf] = x
        R = np.fft.irfft(spectrum, n=L, axis=-1) * L
        if not normalize:
            r = R / nfft
        elif weighting == 0:
            si = np.where(band, mult * (np.where(bad[..., None], 0.0, aii) * h), 0.0).sum(axis=-1)
            sj = np.where(band, mult * (np.where(bad[..., None], 0.0, ajj) * h), 0.0).sum(axis=-1)
            r = R / (np.sqrt(si) * np.sqrt(sj))[..., None]
        else:
            r = R / np.where(band & (w != 0), mult, 0.0).sum(axis=-1)[..., None]
        r = np.where(bad[..., None], np.nan, r)
        lags = np.arange(-max_lag, max_lag + 1)
        cc = r[..., lags % L]
        q = np.argmax(np.where(bad[..., None], 0.0, cc), axis=-1)
        index = q - max_lag
        a = np.take_along_axis(r, ((index - 1) % L)[..., None], axis=-1)[..., 0]
        b = np.take_along_axis(r, (index % L)[..., None], axis=-1)[..., 0]
        c = np.take_along_axis(r, ((index + 1) % L)[..., None], axis=-1)[..., 0]
        den = a - 2.0 * b + c
        safe = np.where(den == 0, 1.0, den)
        delta = np.where(den == 0, 0.0, 0.5 * (a - c) / safe)
        peak_lag = (index + delta) / upsample
        peak_value = b - 0.25 * (a - c) * delta
        g = 0.5 * (a - c) / (safe * safe)
        bound = np.where(den == 0, np.inf, np.abs(0.5 / safe - g) + np.abs(2.0 * g) + np.abs(-0.5 / safe - g))
    return Restated(r, cc, peak_lag, peak_value, index, delta, bound)


# ---- the parity fixtures ----------------------------------------------------------------------------------------------------------------
SEGMENTS, OWN = 4, 0.2


def sensor_delays(case, stack):
    """[C] delays on the finer grid: integer + tenths / 10, tenths in 0 .. 4, every pair's difference inside the lag window."""
    rng = np.random.default_rng([20260301, case.L, case.upsample, case.C, stack])
    span = min(max(case.max_lag - 1, 0), 12)
    whole = rng.integers(0, span + 1, case.C) if span else np.zeros(case.C, dtype=np.int64)
    tenths = rng.integers(0, 5, case.C)
    if case.max_lag == 0:
        tenths[:] = 0
    elif case.max_lag == 1:
        whole[:] = 0
        tenths = np.where(rng.integers(0, 3, case.C) == 0, 10, tenths)  # some pairs sit on the window's edge, +-1
    d = whole + tenths / 10.0
    d[0] = 0.0
    return d


@functools.lru_cache(maxsize=None)
def matrices(cid):
    """(csd [nstack, nf, C, C] complex128 with qi_csd's one-sided doubling, delays [nstack, C] on the finer grid)."""
    case = by_id(cid)
    nfft = case.L // case.upsample
    nf = nfft // 2 + 1
    f = np.arange(nf)
    shape = 0.25 + np.exp(-0.5 * ((f - 0.4 * nf) / (0.3 * nf)) ** 2)
    out, delays = [], []
    for k in range(case.nstack):
        rng = np.random.default_rng([20260302, case.L, case.upsample, case.C, k])
        d = sensor_delays(case, k)
        src = (rng.standard_normal((SEGMENTS, 1, nf)) + 1j * rng.standard_normal((SEGMENTS, 1, nf))) * shape
        own = rng.standard_normal((SEGMENTS, case.C, nf)) + 1j * rng.standard_normal((SEGMENTS, case.C, nf))
        x = src * np.exp(-2j * np.pi * f[None, None, :] * d[None, :, None] / case.L) + OWN * own
        x[:, :, 0] = x[:, :, 0].real  # a real record's bins 0 and nfft / 2
        x[:, :, -1] = x[:, :, -1].real
        s = np.einsum("mif,mjf->fij", np.conj(x), x) / SEGMENTS
        s[1:-1] *= 2.0
        out.append(s)
        delays.append(d)
    s = np.stack(out)
    s.setflags(write=False)
    return s, np.stack(delays)


@functools.lru_cache(maxsize=None)
def restated(cid):
    case = by_id(cid)
    nf = case.L // case.upsample // 2 + 1
    return restate(matrices(cid)[0], bin_range(case.bins, nf), case.weighting, case.halve, case.normalize, case.upsample, case.max_lag)


def call_args(case):
    """The keyword arguments of engine.pair_lags for a case."""
    nf = case.L // case.upsample // 2 + 1
    return dict(bins=bin_range(case.bins, nf), weighting=WEIGHTINGS[case.weighting], halve_interior=case.halve, normalize=case.normalize,
                upsample=case.upsample, max_lag=case.max_lag)


def margins(res):
    """(the smallest of (peak - sample) / peak over the window's samples that are not adjacent to the maximum -- inf where there
    is none --, the same over the two adjacent samples a and c of the full correlation) of a restatement."""
    n = res.cc.shape[-1]
    max_lag = (n - 1) // 2
    q = (res.index + max_lag)[..., None]
    pos = np.arange(n)
    peak = np.take_along_axis(res.cc, q, axis=-1)
    far = np.where(np.abs(pos - q) > 1, (peak - res.cc) / peak, np.inf)
    L = res.r.shape[-1]
    near = [(peak[..., 0] - np.take_along_axis(res.r, ((res.index + k) % L)[..., None], axis=-1)[..., 0]) / peak[..., 0] for k in (-1, 1)]
    return float(far.min()), float(np.min(near))


# ---- planted single delays (the edge cases) and exact spectra ---------------------------------------------------------------------------
def delayed_pair(nfft, delay, seed=5):
    """csd [1, nf, 2, 2] complex128 of two records, the second the first delayed by `delay` samples (circularly), broadband."""
    rng = np.random.default_rng([20260303, nfft, seed])
    nf = nfft // 2 + 1
    f = np.arange(nf)
    a = rng.standard_normal(nf) + 1j * rng.standard_normal(nf)
    a[0], a[-1] = a[0].real, a[-1].real
    x = np.stack([a, a * np.exp(-2j * np.pi * f * delay / nfft)])
    if float(delay).is_integer():
        x[1, -1] = x[1, -1].real
    s = np.einsum("if,jf->fij", np.conj(x), x)
    return s[None]


def exact_matrices(nfft, upsample, C=3, nstack=2):
    """Gaussian-integer matrices that are non-zero only at the bins whose twiddles are exact in the transform of length
    L = nfft upsample -- 0, L / 4 and L / 2 where nfft / 2 reaches them -- and differ for every (stack, i, j)."""
    nf = nfft // 2 + 1
    L = nfft * upsample
    s = np.zeros((nstack, nf, C, C), dtype=np.complex128)
    for b, f in enumerate((0, L // 4, L // 2)):
        if f >= nf:
            continue
        for k in range(nstack):
            for i in range(C):
                s[k, f, i, i] = 4 + 2 * i + k + b
                for j in range(i + 1, C):
                    s[k, f, i, j] = (3 + i - 2 * j + 5 * k + b) + 1j * (2 * i + j - 3 * k - 2 * b + 1)
                    s[k, f, j, i] = np.conj(s[k, f, i, j])
    return s


def exact_correlation(csd, upsample, halve):
    """r [nstack, npair, L] of exact_matrices with weighting 0 and no normalisation, from the integers: exact in float64."""
    nstack, nf, C, _ = csd.shape
    nfft = 2 * (nf - 1)
    L = nfft * upsample
    rows, cols = pair_table(C)
    lag = np.arange(L)
    total = np.zeros((nstack, rows.size, L))
    for f in (0, L // 4, L // 2):
        if f >= nf:
            continue
        x = csd[:, f, rows, cols]  # [nstack, npair]
        h = 0.5 if halve and 0 < f < nfft // 2 else 1.0
        if f == 0:
            total += x.real[..., None]
        elif f == L // 2:
            total += x.real[..., None] * np.where(lag % 2 == 0, 1.0, -1.0)
        else:  # 2 Re(x i^l)
            quarter = np.array([1, 1j, -1, -1j])[lag % 4]
            total += 2.0 * h * (x[..., None] * quarter).real
    return total / nfft
