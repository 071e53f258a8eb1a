"""Cases of the MUSIC tests and NumPy restatements of qi_csd_eigh and qi_beam_music (include/qi_subspace.h), shared by the CPU
and GPU tests and tools/music_bench.py.  The shapes, grids, frequencies and band tables are those of tests/beam_cases.py.

`eigh64` is the float64 statement: np.linalg.eigh of the Hermitian matrix of the lower triangle.  `eigh_steps` is the kernel's
algorithm with every operation rounded to `dtype`: the round-robin schedule of disjoint pairs, each pair's rotation from
(A[p][p], A[q][q], A[p][q]) with the phase taken out of A[p][q], the column rotations of A and V, then the row rotations of A,
the skipped rotations, the norms in double, the sweep test and cap, the stable sort -- also where the matrix is not finite, so
it gives `info` and the NaN outputs (and the sweeps each matrix took).  `music` is the float64 form: the phase reduced as in
beam_cases.reduced_turns, an einsum over the noise columns, the band sum (ascending) and the quotient in double.  `music32`
rounds the factors, the products and the sum of squares to float32 and keeps the band sum and the quotient in double.

The matrices of a shape case are seeded Hermitian, Q diag(lambda) Q^H with Q unitary: C - k noise eigenvalues uniform in
[1, 2] and k = min(2, C - 1) signal eigenvalues uniform in [50, 100]; n_sources = k.  The gap keeps the noise subspace well
conditioned: projectors are compared, where single eigenvectors of the near-degenerate noise cluster cannot be.
"""
import functools

import numpy as np

import beam_cases as bc

ROOT = bc.ROOT
DTYPES = bc.DTYPES
TOL = bc.TOL
SWEEP_CAP = 40
# The largest deviations of the float32 restatements from the float64 ones over all shape cases, as NumPy gave them on the CPU
# (tests/test_music_cpu.py computes them again and holds the constants to them): the eigenvalues as a fraction of the largest,
# the noise projector and 1 / power absolute.
EIGH32_VALUES = 1.27e-6  # (1.265e-06: c64_g300_f33_b3)
EIGH32_PROJECTOR = 9.9e-6  # (9.868e-06: c64_g300_f33_b3)
MUSIC32_RECIPROCAL = 9.2e-6  # (9.176e-06: c64_g16_f1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def sources_of(C):
    return min(2, C - 1)


@functools.lru_cache(maxsize=None)
def _subspace_matrices(C, nf):
    rng = np.random.default_rng([41, C, nf])
    k = sources_of(C)
    out = np.empty((nf, C, C), dtype=np.complex128)
    for f in range(nf):
        q, _ = np.linalg.qr(rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
        lam = np.concatenate([rng.uniform(1.0, 2.0, C - k), rng.uniform(50.0, 100.0, k)])
        s = (q * lam[None, :]) @ np.conj(q.T)
        out[f] = 0.5 * (s + np.conj(s.T))
    out.setflags(write=False)
    return out


def inputs(shape, dtype):
    """(csd [nf, C, C] complex of dtype, Hermitian; frequency_hz [nf]; delays_s [G, C] float64; n_sources) of a shape case: the
    frequencies and delays are beam_cases.inputs'."""
    _, freq, tau = bc.inputs(shape, dtype)
    return _subspace_matrices(shape.C, shape.nf).astype(bc.complex_of(dtype)), freq, tau, sources_of(shape.C)


def hermitian_of_lower(csd):
    """What qi_csd_eigh reads: the lower triangle and the real part of the diagonal -> the Hermitian matrix, complex128."""
    s = np.asarray(csd).astype(np.complex128)
    low = np.tril(s, -1)
    out = low + np.conj(np.swapaxes(low, 1, 2))
    idx = np.arange(s.shape[1])
    out[:, idx, idx] = np.real(s[:, idx, idx])
    return out


# ---- the eigenpairs ---------------------------------------------------------------------------------------------------------------
def eigh64(csd):
    """(eigenvalues [nf, C] ascending, eigenvectors [nf, C, C] complex128, column j the unit vector of value j)."""
    return np.linalg.eigh(hermitian_of_lower(csd))


def schedule(C):
    """The round-robin steps of C (rounded up to even) players: per step the disjoint pairs (p < q), the pair of the bye left out."""
    n = C + (C & 1)
    steps = []
    for s in range(n - 1):
        pairs = []
        for k in range(n // 2):
            a, b = (n - 1, s) if k == 0 else ((s + k) % (n - 1), (s - k) % (n - 1))
            if max(a, b) < C:
                pairs.append((min(a, b), max(a, b)))
        steps.append(pairs)
    return steps


def _norms(ar, ai):
    """(off-diagonal, whole) sums of squares in double."""
    sq = ar.astype(np.float64) ** 2 + ai.astype(np.float64) ** 2
    idx = np.arange(ar.shape[1])
    diag = sq[:, idx, idx].sum(axis=1)
    sq[:, idx, idx] = 0  # (summed apart: the difference of two sums would cancel)
    off = sq.sum(axis=(1, 2))
    return off, off + diag


def eigh_steps(csd, dtype):
    """The kernel's algorithm, every operation rounded to `dtype` -> (eigenvalues [nf, C] of dtype, eigenvectors [nf, C, C]
    complex of dtype, info [nf] int32, sweeps [nf])."""
    rt = np.dtype(dtype).type
    eps = float(np.finfo(rt).eps)
    s = np.asarray(csd).astype(bc.complex_of(dtype))
    nf, C, _ = s.shape
    idx = np.arange(C)
    low_r, low_i = np.tril(s.real).astype(rt), np.tril(s.imag, -1).astype(rt)
    ar = low_r + np.swapaxes(np.tril(low_r, -1), 1, 2)
    ai = low_i - np.swapaxes(low_i, 1, 2)
    vr, vi = np.broadcast_to(np.eye(C, dtype=rt), (nf, C, C)).copy(), np.zeros((nf, C, C), rt)
    info, sweeps = np.zeros(nf, np.int32), np.zeros(nf, np.int64)
    live = np.ones(nf, dtype=bool)
    steps = schedule(C)
    with np.errstate(all="ignore"):
        while live.any():
            off2, fro2 = _norms(ar, ai)
            bad = live & ~(fro2 < np.inf)
            done = live & ~bad & (off2 <= (C * eps) ** 2 * fro2)
            capped = live & ~bad & ~done & (sweeps == SWEEP_CAP)
            info[bad | capped] = 1
            live &= ~(bad | done | capped)
            m = np.flatnonzero(live)
            if not m.size:
                break
            thr = (eps * eps * fro2[m])[:, None]
            a_r, a_i, v_r, v_i = ar[m], ai[m], vr[m], vi[m]
            for pairs in steps:
                if not pairs:
                    continue
                P, Q = np.array([p for p, _ in pairs]), np.array([q for _, q in pairs])
                app, aqq, xr, xi = a_r[:, P, P], a_r[:, Q, Q], a_r[:, P, Q], a_i[:, P, Q]
                rot = xr.astype(np.float64) ** 2 + xi.astype(np.float64) ** 2 > thr
                big = np.maximum(np.abs(xr), np.abs(xi))
                im = rt(1) / big
                ur, ui = xr * im, xi * im
                h2 = ur * ur + ui * ui
                rh = rt(1) / np.sqrt(h2)
                phr, phi = ur * rh, ui * rh
                g = big * (h2 * rh)
                tau = (aqq - app) * (rt(0.5) * (im * rh))
                t = np.where(tau >= 0, rt(1), rt(-1)) / (np.abs(tau) + np.sqrt(rt(1) + tau * tau))
                c = rt(1) / np.sqrt(rt(1) + t * t)
                sn = t * c
                c = np.where(rot, c, rt(1)).astype(rt)
                sr, si = np.where(rot, sn * phr, rt(0)).astype(rt), np.where(rot, sn * phi, rt(0)).astype(rt)
                dp, dq = np.where(rot, app - t * g, app).astype(rt), np.where(rot, aqq + t * g, aqq).astype(rt)
                cc, srr, sii = c[:, None, :], sr[:, None, :], si[:, None, :]
                # columns p and q of A and of V: p' = c p - conj(s ph) q,  q' = s ph p + c q
                for mr, mi in ((a_r, a_i), (v_r, v_i)):
                    x_r, x_i, y_r, y_i = mr[:, :, P], mi[:, :, P], mr[:, :, Q], mi[:, :, Q]
                    mr[:, :, P], mi[:, :, P] = cc * x_r - (srr * y_r + sii * y_i), cc * x_i - (srr * y_i - sii * y_r)
                    mr[:, :, Q], mi[:, :, Q] = (srr * x_r - sii * x_i) + cc * y_r, (srr * x_i + sii * x_r) + cc * y_i
                # rows p and q of A: p' = c p - s ph q,  q' = conj(s ph) p + c q
                cc, srr, sii = c[:, :, None], sr[:, :, None], si[:, :, None]
                x_r, x_i, y_r, y_i = a_r[:, P, :], a_i[:, P, :], a_r[:, Q, :], a_i[:, Q, :]
                a_r[:, P, :], a_i[:, P, :] = cc * x_r - (srr * y_r - sii * y_i), cc * x_i - (srr * y_i + sii * y_r)
                a_r[:, Q, :], a_i[:, Q, :] = (srr * x_r + sii * x_i) + cc * y_r, (srr * x_i - sii * x_r) + cc * y_i
                # the rotated pair itself: the two new diagonal entries, zeros between them
                a_r[:, P, P], a_r[:, Q, Q] = dp, dq
                a_i[:, P, P], a_i[:, Q, Q] = 0, 0
                for u, v in ((P, Q), (Q, P)):
                    a_r[:, u, v] = np.where(rot, rt(0), a_r[:, u, v])
                    a_i[:, u, v] = np.where(rot, rt(0), a_i[:, u, v])
            ar[m], ai[m], vr[m], vi[m] = a_r, a_i, v_r, v_i
            sweeps[m] += 1
    d = ar[:, idx, idx]
    order = np.argsort(d, axis=1, kind="stable")
    w = np.take_along_axis(d, order, axis=1)
    u = np.empty((nf, C, C), dtype=bc.complex_of(dtype))
    u.real, u.imag = np.take_along_axis(vr, order[:, None, :], axis=2), np.take_along_axis(vi, order[:, None, :], axis=2)
    w[info != 0] = np.nan
    u[info != 0] = complex(np.nan, np.nan)
    return w, u, info, sweeps


def noise_projector(u, n_sources):
    """U_n U_n^H of the C - n_sources first columns, complex128."""
    un = np.asarray(u).astype(np.complex128)[:, :, :u.shape[1] - n_sources]
    return un @ np.conj(np.swapaxes(un, 1, 2))


def residuals(w, u, csd):
    """(max |U^H U - I|, max |S U - U diag(w)| / max |w|) in float64."""
    u, w = np.asarray(u).astype(np.complex128), np.asarray(w).astype(np.float64)
    s = hermitian_of_lower(csd)
    ortho = np.abs(np.conj(np.swapaxes(u, 1, 2)) @ u - np.eye(u.shape[1])).max()
    pairs = np.abs(s @ u - u * w[:, None, :]).max() / np.abs(w).max()
    return float(ortho), float(pairs)


# ---- the form ---------------------------------------------------------------------------------------------------------------------
def _band_quotient(d, first, C):
    """C n_b over each band's sum of the [nf, G] doubles in ascending f -> [nb, G]."""
    out = np.zeros((len(first) - 1, d.shape[1]))
    for b, (lo, hi) in enumerate(zip(first[:-1], first[1:])):
        total = np.zeros(d.shape[1])
        for f in range(lo, hi):
            total = total + d[f]
        with np.errstate(all="ignore"):
            out[b] = (float(C) * float(hi - lo)) / total
    return out


def null_spectrum(u, n_sources, freq, tau, e=None):
    """D [nf, G] float64 = sum_{j < C - n_sources} |sum_i conj(U[i][j]) e_i|^2."""
    u = np.asarray(u).astype(np.complex128)
    if e is None:
        e = np.exp(2j * np.pi * bc.reduced_turns(freq, tau))
    w = np.einsum("fij,fgi->fgj", np.conj(u[:, :, :u.shape[1] - n_sources]), e, optimize=True)
    return (w.real ** 2 + w.imag ** 2).sum(axis=-1)


def music(u, n_sources, freq, tau, bands=None, e=None):
    """power [nb, G] float64.  e: the factors [nf, G, C] where they are not exp(2 pi i reduced turns) (the exact case's units)."""
    d = null_spectrum(u, n_sources, freq, tau, e)
    return _band_quotient(d, bc.band_table(bands, d.shape[0]), np.shape(u)[1])


def music32(u, n_sources, freq, tau, bands=None):
    """The same in float32: the phase in double, the factors rounded to float32, products and sums in complex64 / float32, the
    band sum and the quotient in double, rounded once."""
    u = np.asarray(u).astype(np.complex64)
    t = bc.reduced_turns(freq, tau).astype(np.float32).astype(np.float64)
    e = (np.cos(2 * np.pi * t).astype(np.float32) + 1j * np.sin(2 * np.pi * t).astype(np.float32)).astype(np.complex64)
    w = np.einsum("fij,fgi->fgj", np.conj(u[:, :, :u.shape[1] - n_sources]), e)
    assert w.dtype == np.complex64
    d = (w.real * w.real + w.imag * w.imag).sum(axis=-1, dtype=np.float32)
    return _band_quotient(d.astype(np.float64), bc.band_table(bands, u.shape[0]), u.shape[1]).astype(np.float32)


# ---- the exact cases: diagonal matrices --------------------------------------------------------------------------------------------
def exact_inputs(C, nf, G):
    """Diagonal matrices with distinct scrambled integer diagonals -- the last matrix repeats a value -- and NaN above the
    diagonal (never read); frequencies, delays and quarter turns of beam_cases.exact_inputs -> (csd complex128, sorted
    diagonals [nf, C], permutation matrices [nf, C, C], freq, tau, turns4)."""
    _, freq, tau, turns4 = bc.exact_inputs(C, nf, G)
    step = next(k for k in (7, 5, 3, 1) if np.gcd(k, C) == 1)
    d = np.stack([(step * np.arange(C) + 3 * f) % C + 1 + f for f in range(nf)]).astype(np.float64)
    if C > 2:
        d[-1, C - 1] = d[-1, 0]  # equal values: the lower position first
    s = np.zeros((nf, C, C), dtype=np.complex128)
    s[:, np.triu(np.ones((C, C), dtype=bool), 1)] = complex(np.nan, np.nan)
    s[:, np.arange(C), np.arange(C)] = d + 3j  # (the diagonal's imaginary part is not read either)
    order = np.argsort(d, axis=1, kind="stable")
    u = np.zeros((nf, C, C), dtype=np.complex128)
    f_i, j_i = np.meshgrid(np.arange(nf), np.arange(C), indexing="ij")
    u[f_i, order, j_i] = 1
    return s, np.take_along_axis(d, order, axis=1), u, freq, tau, turns4


def exact_factors(turns4):
    return np.array([1, 1j, -1, -1j])[turns4]


# ---- info ---------------------------------------------------------------------------------------------------------------------------
def info_base(C):
    """The finite matrix [C, C] complex128 the info cases are made of."""
    return np.array(_subspace_matrices(C, 1)[0])


def info_cases(C):
    """(name, matrix [C, C] complex128, the info the contract gives): a NaN or an inf in the triangle that is read ends at 1,
    the same value above the diagonal is ignored."""
    base = info_base(C)
    out = []
    for name, value in (("NaN", np.nan), ("inf", np.inf)):
        low, up = base.copy(), base.copy()
        low[C - 1, 0] = value
        up[0, C - 1] = value
        out += [(f"{name} below the diagonal", low, 1), (f"{name} above the diagonal", up, 0)]
    return tuple(out)


# ---- plane waves --------------------------------------------------------------------------------------------------------------------
TWO_WAVES = ((7, 2), (5, 3))  # (ix, iy) of the two sources in beam_cases' slowness grid: (2.25, -1.5) and (0.75, -0.75) ms/m
TWO_WAVES_GAIN = (1.0, 0.8)


def two_wave_indices():
    return sorted(iy * bc.PW_GRID_POINTS + ix for ix, iy in TWO_WAVES)


@functools.lru_cache(maxsize=None)
def two_wave_records():
    """[5, n] float64: two independent noise sources on beam_cases' array, each later at sensor i by its own tau_i (circular
    delays), plus independent noise at PW_OWN."""
    rng = np.random.default_rng([43, bc.PW_N])
    f = np.fft.rfftfreq(bc.PW_N, 1 / bc.PW_FS)
    x = bc.PW_OWN * rng.standard_normal((len(bc.PW_POSITIONS_M), bc.PW_N))
    for (ix, iy), gain in zip(TWO_WAVES, TWO_WAVES_GAIN):
        tau = bc.pw_delays()[iy * bc.PW_GRID_POINTS + ix]
        src = gain * rng.standard_normal(bc.PW_N)
        x = x + np.fft.irfft(np.fft.rfft(src)[None, :] * np.exp(-2j * np.pi * f[None, :] * tau[:, None]), bc.PW_N)
    x.setflags(write=False)
    return x


def local_maxima(row, points=None):
    """Indices of the local maxima of a [points x points] map (8 neighbours, the border included), the largest first."""
    points = points or bc.PW_GRID_POINTS
    m = np.asarray(row, dtype=np.float64).reshape(points, points)
    pad = np.full((points + 2, points + 2), -np.inf)
    pad[1:-1, 1:-1] = m
    top = np.ones_like(m, dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                top &= m > pad[1 + dy:1 + dy + points, 1 + dx:1 + dx + points]
    at = np.flatnonzero(top.reshape(-1))
    return [int(k) for k in at[np.argsort(-m.reshape(-1)[at])]]


def peak_ratio(row):
    order = np.argsort(row)
    return int(order[-1]), float(row[order[-1]] / row[order[-2]])
