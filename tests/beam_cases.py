"""Cases of the beamforming tests and NumPy restatements of qi_beam_power's semantics (include/qi_beam.h), shared by the CPU
and GPU tests and tools/beam_bench.py.

`restate` is the float64 statement: the steering tensor e[f, g, i] = exp(2 pi i freq[f] tau[g, i]) and an einsum.
`restate32` is what rounding in the matrices' precision alone costs: the phase formed and reduced in double, the factors
rounded to float32, every product and sum in float32 (complex64), the quotient in double and rounded once.

The matrices of a shape case are csd_cases.restate of csd_cases' noise records (partly coherent pairs, positive auto-powers:
the semblance is finite) at 64-sample segments and a 128-point transform; the case takes the bins 1 .. nf (bin 0 is what the
mean removal leaves) and their frequencies.  The delays are uniform in +-0.15 s: up to 56 turns at the highest bin.
"""
import collections
import functools

import numpy as np

import csd_cases as cc

ROOT = cc.ROOT
DTYPES = ("float32", "float64")
MAX_SENSORS = 64
# SURVEY s8d, the project's reduction contract: |d power| <= TOL max |power| (the semblance: absolute)
TOL = {"float32": 1e-4, "float64": 1e-10}
# The largest deviation of restate32 from restate over all shape cases and both normalisations, as a fraction of the case's
# largest power (the semblance: absolute), as NumPy gave it on the CPU (2.274e-07: c16_g37_f33_b3, the power);
# tests/test_beam_cpu.py computes it again, holds the constant to it and holds it to TOL["float32"] / 16.
BEAM32_RESTATEMENT = 2.28e-7

Shape = collections.namedtuple("Shape", "id C G nf bands")


def _shape(C, G, nf, bands=None):
    cid = f"c{C}_g{G}_f{nf}" + ("" if bands is None else f"_b{len(bands) - 1}")
    return Shape(cid, C, G, nf, None if bands is None else tuple(bands))


B7, B33 = (0, 1, 7), (0, 3, 4, 33)  # a one-bin band, uneven widths
# every C of (1, 5, 16, 17, 33, 64), G of (1, 15, 16, 17, 37, 300), nf of (1, 7, 33) and band table of (None, B7, B33)
SHAPES = (
    _shape(1, 1, 1), _shape(5, 15, 7, B7), _shape(16, 16, 7), _shape(17, 17, 33, B33), _shape(33, 37, 7, B7),
    _shape(64, 300, 33, B33), _shape(64, 16, 1), _shape(5, 300, 33), _shape(17, 1, 7), _shape(33, 15, 33),
    _shape(16, 37, 33, B33), _shape(1, 17, 7, B7),
)
MAX_DELAY_S = 0.15


def ids():
    return [s.id for s in SHAPES]


def by_id(cid):
    return next(s for s in SHAPES if s.id == cid)


def complex_of(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def band_table(bands, nf):
    return np.arange(nf + 1) if bands is None else np.asarray(bands, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _noise_matrices(C):
    case = cc.Case(f"beam_c{C}", C, 1024, 64, 32, 128, "fused", None)
    s = cc.restate(cc.records(case).astype(np.float64), case, "spectrum")
    s.setflags(write=False)
    return s, np.fft.rfftfreq(case.nfft, 1 / cc.FS)


def inputs(shape, dtype):
    """(csd [nf, C, C] complex of dtype, frequency_hz [nf], delays_s [G, C] float64) of a shape case."""
    s, f = _noise_matrices(shape.C)
    rng = np.random.default_rng([23, shape.C, shape.G])
    tau = rng.uniform(-MAX_DELAY_S, MAX_DELAY_S, (shape.G, shape.C))
    return np.ascontiguousarray(s[1:shape.nf + 1]).astype(complex_of(dtype)), f[1:shape.nf + 1].copy(), tau


def reduced_turns(freq, tau):
    """freq[f] tau[g, i] in double, reduced to [-1/2, 1/2] turns -> [nf, G, C]."""
    t = np.asarray(freq, dtype=np.float64)[:, None, None] * np.asarray(tau, dtype=np.float64)[None, :, :]
    return t - np.rint(t)


def _finish(q, trace, first, C, normalize, dtype):
    """Band sums in `dtype`, the quotient in double, rounded once."""
    qb = np.stack([q[a:b].sum(axis=0, dtype=dtype) for a, b in zip(first[:-1], first[1:])])
    if normalize:
        tb = np.array([trace[a:b].sum(dtype=dtype) for a, b in zip(first[:-1], first[1:])])
        den = float(C) * tb.astype(np.float64)[:, None]
    else:
        den = float(C) * float(C)
    with np.errstate(all="ignore"):
        return (qb.astype(np.float64) / den).astype(dtype)


def restate(csd, freq, tau, bands=None, normalize=False):
    """power [nb, G] float64: Re e^H S e summed over each band's matrices, over C^2 or C sum tr S."""
    s = np.asarray(csd).astype(np.complex128)
    e = np.exp(2j * np.pi * reduced_turns(freq, tau))
    q = np.real(np.einsum("fgi,fij,fgj->fg", np.conj(e), s, e, optimize=True))
    trace = np.real(np.einsum("fii->f", s))
    return _finish(q, trace, band_table(bands, s.shape[0]), s.shape[1], normalize, np.float64)


def restate32(csd, freq, tau, bands=None, normalize=False):
    """The same in float32: the phase in double, the factors rounded to float32, products and sums in complex64 / float32."""
    s = np.asarray(csd).astype(np.complex64)
    t = reduced_turns(freq, tau).astype(np.float32).astype(np.float64)
    e = (np.cos(2 * np.pi * t).astype(np.float32) + 1j * np.sin(2 * np.pi * t).astype(np.float32)).astype(np.complex64)
    w = np.einsum("fgi,fij->fgj", np.conj(e), s)
    assert w.dtype == np.complex64
    q = np.real(np.einsum("fgj,fgj->fg", w, e))
    trace = np.real(np.einsum("fii->f", s))
    return _finish(q.astype(np.float32), trace.astype(np.float32), band_table(bands, s.shape[0]), s.shape[1], normalize, np.float32)


def peaks_of(power):
    """np.argmax's rules: the first maximum, the first NaN if there is one -> (index [nb] int64, value [nb])."""
    idx = np.argmax(power, axis=1).astype(np.int64)
    return idx, power[np.arange(power.shape[0]), idx]


# ---- the exact case: every factor a unit of the Gaussian integers, every sum an integer below 2^24 ---------------------------
def exact_inputs(C, nf, G):
    """Hermitian matrices with Gaussian-integer entries (|re|, |im| <= 8) that depend asymmetrically on (i, j), a positive
    integer diagonal; frequencies 1 .. nf Hz; delays that are multiples of 0.25 s -> (csd complex128, freq, tau, quarter
    turns [nf, G, C] as integers mod 4)."""
    i, j, f = np.arange(C)[None, :, None], np.arange(C)[None, None, :], np.arange(nf)[:, None, None]
    re = (3 * i + 5 * j + f) % 17 - 8
    im = (7 * i + 2 * j + 3 * f) % 17 - 8
    upper = np.triu(np.ones((C, C), dtype=bool), 1)[None]
    s = np.where(upper, re + 1j * im, 0)
    s = s + np.conj(np.swapaxes(s, 1, 2))
    d = (np.arange(C)[None, :] + np.arange(nf)[:, None]) % 8 + 1
    s[:, np.arange(C), np.arange(C)] = d
    g, k = np.arange(G)[:, None], np.arange(C)[None, :]
    quarters = (5 * g + 3 * k + g * k) % 8 - 4
    freq = np.arange(1, nf + 1, dtype=np.float64)
    turns4 = (freq.astype(np.int64)[:, None, None] * quarters[None]) % 4
    return s.astype(np.complex128), freq, 0.25 * quarters.astype(np.float64), turns4


def exact_sums(csd, turns4, bands=None):
    """(sum over each band of Q [nb, G], sum over each band of tr S [nb]) as exact integers in float64."""
    e = np.array([1, 1j, -1, -1j])[turns4]
    q = np.real(np.einsum("fgi,fij,fgj->fg", np.conj(e), csd, e))
    trace = np.real(np.einsum("fii->f", csd))
    first = band_table(bands, csd.shape[0])
    qb = np.stack([q[a:b].sum(axis=0) for a, b in zip(first[:-1], first[1:])])
    tb = np.array([trace[a:b].sum() for a, b in zip(first[:-1], first[1:])])
    assert np.array_equal(qb, np.rint(qb)) and np.abs(qb).max() < 2 ** 24 and np.all(tb > 0) and tb.max() < 2 ** 24
    return qb, tb


# ---- the plane-wave case --------------------------------------------------------------------------------------------------------
PW_FS = 800.0
PW_N = 4096
PW_SEG, PW_OVERLAP = 256, 128
PW_BANDS = (8, 24, 40, 72, 73)  # bin offsets: 25 .. 225 Hz, the last band one bin
PW_GRID_POINTS, PW_MAX_SLOWNESS = 9, 3e-3
PW_TRUE = (7, 2)  # (ix, iy) of the source's slowness in the grid: (2.25, -1.5) ms/m
PW_OWN = 0.1
PW_MARGIN = 1e-2  # the best semblance lies at least this far above the runner-up
# five sensors over about 60 m (x east, y north), irregular: no grid point aliases onto the source's in any band
PW_POSITIONS_M = np.array([[0.0, 0.0], [27.0, 4.0], [-13.0, 22.0], [-21.0, -17.0], [9.0, -31.0]])


def pw_slowness():
    """[81, 2] (s_x, s_y), x fastest -- beamform.slowness_grid's order, restated."""
    axis = np.linspace(-PW_MAX_SLOWNESS, PW_MAX_SLOWNESS, PW_GRID_POINTS)
    sy, sx = np.meshgrid(axis, axis, indexing="ij")
    return np.stack([sx.reshape(-1), sy.reshape(-1)], axis=1)


def pw_true_index():
    return PW_TRUE[1] * PW_GRID_POINTS + PW_TRUE[0]


def pw_delays(slowness=None):
    s = pw_slowness() if slowness is None else slowness
    return s @ PW_POSITIONS_M.T  # tau[g, i] = s_g . r_i


@functools.lru_cache(maxsize=None)
def pw_records():
    """[5, n] float64: one noise source, at sensor i later by tau_i (an FFT phase ramp: a circular delay), plus independent
    noise at PW_OWN."""
    rng = np.random.default_rng([29, PW_N])
    src = rng.standard_normal(PW_N)
    own = rng.standard_normal((len(PW_POSITIONS_M), PW_N))
    tau = pw_delays()[pw_true_index()]
    f = np.fft.rfftfreq(PW_N, 1 / PW_FS)
    x = np.fft.irfft(np.fft.rfft(src)[None, :] * np.exp(-2j * np.pi * f[None, :] * tau[:, None]), PW_N)
    x = x + PW_OWN * own
    x.setflags(write=False)
    return x


def pw_case():
    return cc.Case("beam_plane_wave", len(PW_POSITIONS_M), PW_N, PW_SEG, PW_OVERLAP, PW_SEG, "fused", None)


def pw_true_azimuth_velocity():
    """(back azimuth in degrees clockwise from north, trace velocity in m/s) of the source: where -s points, 1 / |s|."""
    sx, sy = pw_slowness()[pw_true_index()]
    return float(np.degrees(np.arctan2(-sx, -sy)) % 360.0), float(1.0 / np.hypot(sx, sy))
