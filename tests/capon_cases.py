"""Cases of the Capon tests and NumPy restatements of qi_csd_whiten and qi_beam_capon (include/qi_adaptive.h), shared by the CPU
and GPU tests and tools/capon_bench.py.  The shapes, grids, frequencies and band tables are those of tests/beam_cases.py.

`whiten` is the float64 statement: the Hermitian matrix of the lower triangle, loaded, np.linalg.cholesky and a triangular
inverse.  `whiten_steps` is the kernel's algorithm with every operation rounded to `dtype` (`whiten32`: float32): the
right-looking Cholesky column by column, the inverse by substitution with its sums in ascending order, on separate real and
imaginary parts -- also where the pivots fail, so it gives `info` and the NaN outputs.  `capon` is the float64 form: the phase
reduced as in beam_cases.reduced_turns, an einsum, the reciprocal and the band sum (ascending) in double.  `capon32` rounds the
factors, the products and the sum of squares to float32 and keeps the reciprocal and the band sum in double.

The matrices of a shape case are seeded Hermitian positive definite, Q diag(lambda) Q^H with Q unitary and the eigenvalues
log-uniform in [1, 100], both ends present; with LOADING = 1e-2 the loaded condition number is below 100.
"""
import functools

import numpy as np

import beam_cases as bc

ROOT = bc.ROOT
DTYPES = bc.DTYPES
TOL = bc.TOL
LOADING = 1e-2
# The largest deviations of the float32 restatements from the float64 ones over all shape cases, as NumPy gave them on the CPU:
# the power (capon32 of whiten32 against capon of whiten) as a fraction of the case's largest power, and max |V^H R V - I| of
# whiten32's V.  tests/test_capon_cpu.py computes both again, holds the constants to them and holds them to TOL["float32"] / 16.
CAPON32_RESTATEMENT = 7.08e-7  # (7.074e-07: c5_g300_f33)
WHITEN32_RESIDUAL = 1.75e-6  # (1.743e-06: c64_g300_f33_b3)
PW_RATIO = 4.0  # the plane wave's peak is at least this many times the runner-up in every band (measured worst: 4.56, band 3)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _definite_matrices(C, nf):
    rng = np.random.default_rng([31, C, nf])
    out = np.empty((nf, C, C), dtype=np.complex128)
    for f in range(nf):
        q, _ = np.linalg.qr(rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
        lam = 10.0 ** rng.uniform(0.0, 2.0, C)
        lam[0] = 1.0
        lam[-1] = 100.0  # (C = 1: the one eigenvalue is 100)
        s = (q * lam[None, :]) @ np.conj(q.T)
        out[f] = 0.5 * (s + np.conj(s.T))
    out.setflags(write=False)
    return out


def inputs(shape, dtype):
    """(csd [nf, C, C] complex of dtype, Hermitian positive definite; frequency_hz [nf]; delays_s [G, C] float64) of a shape
    case: the frequencies and delays are beam_cases.inputs'."""
    _, freq, tau = bc.inputs(shape, dtype)
    return _definite_matrices(shape.C, shape.nf).astype(bc.complex_of(dtype)), freq, tau


def hermitian_of_lower(csd):
    """What qi_csd_whiten reads: the lower triangle and the real part of the diagonal -> the Hermitian matrix, complex128."""
    s = np.asarray(csd).astype(np.complex128)
    low = np.tril(s, -1)
    d = np.real(np.einsum("fii->fi", s))
    out = low + np.conj(np.swapaxes(low, 1, 2))
    idx = np.arange(s.shape[1])
    out[:, idx, idx] = d
    return out


def loaded(csd, loading, dtype=None):
    """R = S + loading * mean(diag S) I in float64; with `dtype` the loaded diagonal is rounded once to it, as the kernel does
    (loading 0: left alone)."""
    r = hermitian_of_lower(csd)
    if loading != 0.0:
        idx = np.arange(r.shape[1])
        d = np.real(r[:, idx, idx])
        mean = np.zeros(r.shape[0])
        for i in idx:
            mean = mean + d[:, i]  # ascending
        mean = mean / float(r.shape[1])
        d = d + (loading * mean)[:, None]
        r[:, idx, idx] = d if dtype is None else d.astype(dtype).astype(np.float64)
    return r


# ---- the factorisation ----------------------------------------------------------------------------------------------------------
def whiten(csd, loading, dtype=None):
    """V [nf, C, C] complex128, upper triangular: R = L L^H by np.linalg.cholesky, V = L^-H by a triangular solve."""
    r = loaded(csd, loading, dtype)
    low = np.linalg.cholesky(r)
    eye = np.broadcast_to(np.eye(r.shape[1], dtype=np.complex128), r.shape)
    winv = np.linalg.solve(low, eye)  # L^-1, lower triangular
    return np.triu(np.conj(np.swapaxes(winv, 1, 2)))


def whiten_steps(csd, loading, dtype):
    """The kernel's algorithm, every operation rounded to `dtype` -> (V [nf, C, C] complex of dtype, info [nf] int32)."""
    rt = np.dtype(dtype).type
    s = np.asarray(csd).astype(bc.complex_of(dtype))
    nf, C, _ = s.shape
    idx = np.arange(C)
    ar, ai = np.tril(s.real).astype(rt), np.tril(s.imag, -1).astype(rt)  # A[f, i, j], i >= j; the diagonal's real part alone
    if loading != 0.0:
        d64 = ar[:, idx, idx].astype(np.float64)
        mean = np.zeros(nf)
        for i in idx:
            mean = mean + d64[:, i]
        mean = mean / float(C)
        ar[:, idx, idx] = (d64 + (loading * mean)[:, None]).astype(rt)
    lr, li = np.zeros((nf, C, C), rt), np.zeros((nf, C, C), rt)  # L below the diagonal
    rd, piv = np.zeros((nf, C), rt), np.zeros((nf, C), rt)
    with np.errstate(all="ignore"):
        for k in range(C):
            d = ar[:, k, k].copy()
            piv[:, k] = d
            root = np.sqrt(d)
            rd[:, k] = rt(1) / root
            xr, xi = ar[:, k + 1:, k] / root[:, None], ai[:, k + 1:, k] / root[:, None]  # l_i, i > k
            lr[:, k + 1:, k], li[:, k + 1:, k] = xr, xi
            # A[i][j] -= l_i conj(l_j), i >= j > k
            ar[:, k + 1:, k + 1:] -= xr[:, :, None] * xr[:, None, :] + xi[:, :, None] * xi[:, None, :]
            ai[:, k + 1:, k + 1:] -= xi[:, :, None] * xr[:, None, :] - xr[:, :, None] * xi[:, None, :]
            ai[:, idx, idx] = 0
        # X U = I, U = L^T: Y[r][j] += x_r[m] U[m][j] for r <= m < j in ascending m, x_r[j] = -Y[r][j] / U[j][j]
        xr, xi = np.zeros((nf, C, C), rt), np.zeros((nf, C, C), rt)
        yr, yi = np.zeros((nf, C, C), rt), np.zeros((nf, C, C), rt)
        xr[:, idx, idx] = rd
        for m in range(C - 1):
            ur, ui = lr[:, m + 1:, m][:, None, :], li[:, m + 1:, m][:, None, :]  # U[m][j], j > m
            pr, pi = xr[:, :m, m][:, :, None], xi[:, :m, m][:, :, None]  # x_r[m], r < m
            yr[:, :m, m + 1:], yi[:, :m, m + 1:] = (yr[:, :m, m + 1:] + (pr * ur - pi * ui), yi[:, :m, m + 1:] + (pr * ui + pi * ur))
            yr[:, m, m + 1:], yi[:, m, m + 1:] = rd[:, m, None] * ur[:, 0, :], rd[:, m, None] * ui[:, 0, :]  # r = m: the first term
            xr[:, :m + 1, m + 1] = rt(0) - yr[:, :m + 1, m + 1] * rd[:, m + 1, None]
            xi[:, :m + 1, m + 1] = rt(0) - yi[:, :m + 1, m + 1] * rd[:, m + 1, None]
        bad = ~(piv > 0) | ~(piv < np.inf)
        info = np.where(bad.any(axis=1), np.argmax(bad, axis=1) + 1, 0).astype(np.int32)
        v = np.zeros((nf, C, C), dtype=bc.complex_of(dtype))
        v.real, v.imag = np.triu(xr), np.triu(rt(0) - xi, 1)
    upper = np.triu(np.ones((C, C), dtype=bool))
    v[info != 0] = np.where(upper, complex(np.nan, np.nan), 0)
    return v, info


def whiten32(csd, loading):
    return whiten_steps(csd, loading, np.float32)[0]


def residual(v, r):
    """max |V^H R V - I| per stack, in float64."""
    v = np.asarray(v).astype(np.complex128)
    eye = np.eye(v.shape[1])
    return float(np.abs(np.conj(np.swapaxes(v, 1, 2)) @ r @ v - eye).max())


# ---- the form ---------------------------------------------------------------------------------------------------------------------
def _band_sums(inv, first):
    """Each band's sum of the [nf, G] doubles in ascending f -> [nb, G]."""
    out = np.zeros((len(first) - 1, inv.shape[1]))
    for b, (lo, hi) in enumerate(zip(first[:-1], first[1:])):
        for f in range(lo, hi):
            out[b] = out[b] + inv[f]
    return out


def capon(v, freq, tau, bands=None, e=None):
    """power [nb, G] float64: D = sum_j |sum_i conj(V[i][j]) e_i|^2 per matrix, 1 / D summed over each band in ascending f.
    e: the factors [nf, G, C] where they are not exp(2 pi i reduced turns) (the exact case's units)."""
    v = np.asarray(v).astype(np.complex128)
    if e is None:
        e = np.exp(2j * np.pi * bc.reduced_turns(freq, tau))
    w = np.einsum("fij,fgi->fgj", np.conj(v), e, optimize=True)
    d = (w.real ** 2 + w.imag ** 2).sum(axis=-1)
    with np.errstate(all="ignore"):
        return _band_sums(1.0 / d, bc.band_table(bands, v.shape[0]))


def capon32(v, freq, tau, bands=None):
    """The same in float32: the phase in double, the factors rounded to float32, products and sums in complex64 / float32, the
    reciprocal and the band sum in double, rounded once."""
    v = np.asarray(v).astype(np.complex64)
    t = bc.reduced_turns(freq, tau).astype(np.float32).astype(np.float64)
    e = (np.cos(2 * np.pi * t).astype(np.float32) + 1j * np.sin(2 * np.pi * t).astype(np.float32)).astype(np.complex64)
    w = np.einsum("fij,fgi->fgj", np.conj(v), e)
    assert w.dtype == np.complex64
    d = (w.real * w.real + w.imag * w.imag).sum(axis=-1, dtype=np.float32)
    with np.errstate(all="ignore"):
        return _band_sums(1.0 / d.astype(np.float64), bc.band_table(bands, v.shape[0])).astype(np.float32)


def bartlett_of_loaded(csd, loading, freq, tau, bands=None):
    """beam_cases.restate on the loaded matrices: what Capon never exceeds."""
    return bc.restate(loaded(csd, loading), freq, tau, bands)


# ---- the exact case: every pivot 1, every entry of V a unit of the Gaussian integers ---------------------------------------------------
def exact_inputs(C, nf, G):
    """R = L L^H with L unit lower bidiagonal, its sub-diagonal drawn from {1, i, -1, -i}: R has Gaussian-integer entries of
    modulus <= 2; frequencies, delays and quarter turns of beam_cases.exact_inputs -> (csd complex128, L, freq, tau, turns4)."""
    _, freq, tau, turns4 = bc.exact_inputs(C, nf, G)
    units = np.array([1, 1j, -1, -1j])
    i, f = np.arange(C - 1)[None, :], np.arange(nf)[:, None]
    low = np.zeros((nf, C, C), dtype=np.complex128)
    low[:, np.arange(C), np.arange(C)] = 1
    low[:, np.arange(1, C), np.arange(C - 1)] = units[(3 * i + 5 * f + i * f) % 4]
    return low @ np.conj(np.swapaxes(low, 1, 2)), low, freq, tau, turns4


def exact_factors(turns4):
    return np.array([1, 1j, -1, -1j])[turns4]


# ---- info ---------------------------------------------------------------------------------------------------------------------------
def info_cases(C):
    """(name, matrix [C, C] complex128, loading, the info LAPACK's convention gives)."""
    ones = np.ones((C, C), dtype=np.complex128)
    nan = np.eye(C, dtype=np.complex128) * 4
    nan[0, 0] = np.nan
    return (("rank one, no loading", ones, 0.0, 2), ("rank one, loaded", ones, 0.5, 0), ("zero", np.zeros((C, C), dtype=np.complex128), 0.0, 1),
            ("NaN diagonal", nan, 0.0, 1))


# ---- the plane wave ---------------------------------------------------------------------------------------------------------------
def peak_ratio(row):
    order = np.argsort(row)
    return int(order[-1]), float(row[order[-1]] / row[order[-2]])
