"""Cases of the beam-weights and beam-steering tests and NumPy restatements of qi_beam_weights and qi_beam_steer
(include/qi_steer.h), shared by the CPU and GPU tests and tools/steer_bench.py.

`weights` is the float64 statement: the steering tensor e[f, k, i] = exp(2 pi i freq[f] tau[k, i]) (the phase reduced as in
beam_cases.reduced_turns), Bartlett's e / C, or, with whiteners V, u = V^H e, D = sum |u|^2, a = V u / D.  `steer` is a plain
einsum, out[k, f, t] = sum_i a[f, k, i] Z[i, f, t].  `weights32` and `steer32` are what rounding in float32 alone costs
(beam_cases.restate32's rule): the phase formed and reduced in double, the factors rounded to float32, every product and sum in
complex64 / float32, the quotients in double and rounded once.

The whiteners of a shape case are capon_cases.whiten / whiten32 of capon_cases.inputs' matrices at capon_cases.LOADING; the
frequencies and the delays are beam_cases.inputs' (the first nbeam of 37 delay rows); the panel is seeded complex normal.
"""
import collections
import functools

import numpy as np

import beam_cases as bc
import capon_cases as cpc

ROOT = bc.ROOT
DTYPES = bc.DTYPES
TOL = bc.TOL
LOADING = cpc.LOADING
# The largest deviations of the float32 restatements from the float64 ones over all shape cases, as fractions of the case's
# largest modulus, as NumPy gave them on the CPU: the MVDR weights (weights32 of whiten32 against weights of whiten), the MVDR
# beams (steer32 of them against steer), the Bartlett beams.  tests/test_steer_cpu.py computes them again, holds the constants
# to them and holds them to TOL["float32"] / 16.
MVDR32_WEIGHTS = 1.65e-6  # (1.648e-06: c64_k37_f33_t300)
MVDR32_BEAMS = 1.63e-6  # (1.628e-06: c17_k17_f33_t17)
BARTLETT32_BEAMS = 3.79e-7  # (3.787e-07: c64_k37_f33_t300)

Shape = collections.namedtuple("Shape", "id C nbeam nf nt")
DELAY_ROWS = 37  # rows of a case's delay table: the case takes the first nbeam


def _shape(C, nbeam, nf, nt):
    return Shape(f"c{C}_k{nbeam}_f{nf}_t{nt}", C, nbeam, nf, nt)


# every C of (1, 5, 16, 17, 33, 64), nbeam of (1, 15, 16, 17, 37), nf of (1, 7, 33) and nt of (1, 15, 16, 17, 64, 65, 300): ragged
# and full tiles of sensors, beams and time, a second and third beam tile, a second and third chunk of time (128 columns); the
# last case has 561 workgroups of four waves where all others have one wave each (kSteerFill of csrc/qi_steer.hip)
SHAPES = (
    _shape(1, 1, 1, 1), _shape(5, 15, 7, 15), _shape(16, 16, 7, 16), _shape(17, 17, 33, 17), _shape(33, 37, 7, 64),
    _shape(64, 37, 33, 300), _shape(64, 16, 1, 65), _shape(5, 37, 33, 300), _shape(17, 1, 7, 300), _shape(33, 15, 33, 65),
    _shape(16, 37, 33, 17), _shape(1, 17, 7, 64), _shape(5, 37, 33, 2700),
)


def ids():
    return [s.id for s in SHAPES]


def by_id(cid):
    return next(s for s in SHAPES if s.id == cid)


def _beam_shape(shape):
    return bc.Shape(shape.id, shape.C, DELAY_ROWS, shape.nf, None)


def inputs(shape, dtype):
    """(csd [nf, C, C] complex of dtype, Hermitian positive definite; frequency_hz [nf]; delays_s [nbeam, C] float64; panel
    [C, nf, nt] complex of dtype) of a shape case."""
    s, freq, tau = cpc.inputs(_beam_shape(shape), dtype)
    rng = np.random.default_rng([37, shape.C, shape.nf, shape.nt])
    z = rng.standard_normal((shape.C, shape.nf, shape.nt)) + 1j * rng.standard_normal((shape.C, shape.nf, shape.nt))
    return s, freq, np.ascontiguousarray(tau[:shape.nbeam]), z.astype(bc.complex_of(dtype))


def whiteners(shape, dtype):
    """What the device reads in `dtype`: whiten (float64) or whiten32 of the case's matrices at LOADING."""
    s = inputs(shape, dtype)[0]
    return cpc.whiten(s, LOADING) if np.dtype(dtype) == np.float64 else cpc.whiten32(s, LOADING)


# ---- the restatements -------------------------------------------------------------------------------------------------------------
def factors(freq, tau):
    return np.exp(2j * np.pi * bc.reduced_turns(freq, tau))


def factors32(freq, tau):
    t = bc.reduced_turns(freq, tau).astype(np.float32).astype(np.float64)
    return (np.cos(2 * np.pi * t).astype(np.float32) + 1j * np.sin(2 * np.pi * t).astype(np.float32)).astype(np.complex64)


def weights(freq, tau, v=None, e=None):
    """a [nf, nbeam, C] complex128: e / C, or V u / D with u = V^H e and D = sum |u|^2.  e: the factors [nf, nbeam, C] where
    they are not exp(2 pi i reduced turns) (the exact case's units)."""
    if e is None:
        e = factors(freq, tau)
    if v is None:
        return e / float(e.shape[-1])
    v = np.asarray(v).astype(np.complex128)
    u = np.einsum("fij,fki->fkj", np.conj(v), e, optimize=True)
    d = (u.real ** 2 + u.imag ** 2).sum(axis=-1)
    with np.errstate(all="ignore"):
        return np.einsum("fij,fkj->fki", v, u, optimize=True) / d[..., None]


def weights32(freq, tau, v=None):
    """The same in float32: the phase in double, the factors rounded to float32, products and sums in complex64 / float32, the
    quotients in double per component, rounded once."""
    e = factors32(freq, tau)
    if v is None:
        return (e.astype(np.complex128) / float(e.shape[-1])).astype(np.complex64)
    v = np.asarray(v).astype(np.complex64)
    u = np.einsum("fij,fki->fkj", np.conj(v), e)
    d = (u.real * u.real + u.imag * u.imag).sum(axis=-1, dtype=np.float32)
    vu = np.einsum("fij,fkj->fki", v, u)
    assert u.dtype == np.complex64 and vu.dtype == np.complex64 and d.dtype == np.float32
    with np.errstate(all="ignore"):
        return (vu.astype(np.complex128) / d.astype(np.float64)[..., None]).astype(np.complex64)


def steer(panel, a):
    """out [nbeam, nf, nt] complex128 = sum_i a[f, k, i] Z[i, f, t]: no conjugate."""
    return np.einsum("fki,ift->kft", np.asarray(a).astype(np.complex128), np.asarray(panel).astype(np.complex128), optimize=True)


def steer32(panel, a):
    out = np.einsum("fki,ift->kft", np.asarray(a).astype(np.complex64), np.asarray(panel).astype(np.complex64))
    assert out.dtype == np.complex64
    return out


def cross_spectra(panel):
    """S[f, i, j] = mean_t conj(Z[i, f, t]) Z[j, f, t], complex128: engine.cross_spectra with weight 1 / nt."""
    z = np.asarray(panel).astype(np.complex128)
    return np.einsum("ift,jft->fij", np.conj(z), z, optimize=True) / z.shape[2]


def gain(freq, tau, a):
    """e^H a [nf, nbeam]: 1 for MVDR and Bartlett weights."""
    return np.einsum("fki,fki->fk", np.conj(factors(freq, tau)), np.asarray(a).astype(np.complex128))


def output_power(a, r):
    """a^H R a [nf, nbeam], real."""
    a = np.asarray(a).astype(np.complex128)
    return np.real(np.einsum("fki,fij,fkj->fk", np.conj(a), r, a, optimize=True))


# ---- the exact cases --------------------------------------------------------------------------------------------------------------
def exact_steer_inputs(C, nbeam, nf, nt):
    """Gaussian-integer weights [nf, nbeam, C] that depend asymmetrically on (k, i), a Gaussian-integer panel [C, nf, nt]
    (|re|, |im| <= 8 and <= 4), and their beams: every sum an integer below 2^24."""
    k, i, f, t = np.arange(nbeam), np.arange(C), np.arange(nf), np.arange(nt)
    wr = (3 * k[None, :, None] + 5 * i[None, None, :] + f[:, None, None]) % 17 - 8
    wi = (7 * k[None, :, None] + 2 * i[None, None, :] + 3 * f[:, None, None]) % 17 - 8
    zr = (2 * i[:, None, None] + 3 * t[None, None, :] + f[None, :, None]) % 9 - 4
    zi = (5 * i[:, None, None] + t[None, None, :] + 2 * f[None, :, None]) % 9 - 4
    a, z = (wr + 1j * wi).astype(np.complex128), (zr + 1j * zi).astype(np.complex128)
    out = steer(z, a)
    assert np.array_equal(out.real, np.rint(out.real)) and np.array_equal(out.imag, np.rint(out.imag))
    assert max(np.abs(out.real).max(), np.abs(out.imag).max()) < 2 ** 24
    assert a[0, 1, 0] != a[0, 0, 1] and a[0, 2, 1] != a[0, 1, 2]  # asymmetric in (k, i)
    return a, z, out


def unit_weights(turns4, C):
    """exp(2 pi i quarter turns) / C with every zero a +0: Bartlett's weights at quarter-turn delays."""
    re = np.array([1.0, 0.0, -1.0, 0.0])[turns4 % 4] / float(C)
    im = np.array([0.0, 1.0, 0.0, -1.0])[turns4 % 4] / float(C)
    out = np.empty(turns4.shape, dtype=np.complex128)
    out.real, out.imag = re + 0.0, im + 0.0
    return out


# ---- the plane wave, through the oracle's ShortTimeFFT-convention transform ----------------------------------------------------------
PW_TRACE_SEG, PW_TRACE_OVERLAP = 1024, 768
PW_TRACE_SHORT = (256, 128)
PW_TRACE_ALPHA = 0.25
PW_TRUE_MAX, PW_CENTRE_MIN = 0.065, 0.8  # the Bartlett trace's relative RMS distance from the source: at the true slowness, at the centre
PW_CAPON_LOADING = 0.1


def pw_source():
    """The source of beam_cases.pw_records(): the first draw of its generator."""
    return np.random.default_rng([29, bc.PW_N]).standard_normal(bc.PW_N)


def pw_steer_rows():
    """[2, 2] slowness vectors: the source's and the grid centre (0, 0)."""
    s = bc.pw_slowness()
    return np.stack([s[bc.pw_true_index()], s[(bc.PW_GRID_POINTS ** 2) // 2]])


@functools.lru_cache(maxsize=None)
def oracle_panel(seg, overlap):
    """The oracle's complex panel [C, f_pts, slices] of the plane-wave records and its transform object."""
    from oracle import tfr_oracle as orc

    o = orc.SlidingStft(bc.PW_FS, PW_TRACE_ALPHA, seg, overlap, "magnitude")
    z = np.stack([o.stft(x) for x in bc.pw_records()])
    z.setflags(write=False)
    return o, z


def panel_weights(panel, freq, tau, method, loading):
    """beamform._panel_weights restated in float64 -> (weights [nf, K, C], csd or None)."""
    if method == "bartlett":
        return weights(freq, tau), None
    s = cross_spectra(panel)
    return weights(freq, tau, cpc.whiten(s, loading)), s


@functools.lru_cache(maxsize=None)
def oracle_traces(seg, overlap, method="bartlett", loading=LOADING, zero_delays=False):
    """(beams [K, f_pts, slices], traces [K, samples]) of the plane-wave records steered at pw_steer_rows() (zero_delays: one
    beam with all delays 0) through the oracle's stft and istft: computed once, shared, left unchanged."""
    o, z = oracle_panel(seg, overlap)
    tau = np.zeros((1, z.shape[0])) if zero_delays else bc.pw_delays(pw_steer_rows())
    a, _ = panel_weights(z, o.f, tau, method, loading)
    beams = steer(z, a)
    last = (z.shape[2] - 1) * o.hop
    traces = np.stack([o.istft(b, last) for b in beams])
    beams.setflags(write=False)
    traces.setflags(write=False)
    return beams, traces


def relative_rms(trace, seg):
    """The trace's RMS distance from the source over the interior samples [seg, n - seg), over the source's RMS there."""
    src = pw_source()
    lo, hi = seg, bc.PW_N - seg
    return float(np.sqrt(np.mean((trace[lo:hi] - src[lo:hi]) ** 2) / np.mean(src[lo:hi] ** 2)))
