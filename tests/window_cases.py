"""Cases of the windowed cross-spectrum tests and NumPy restatements of include/qi_windows.h, shared by the CPU and GPU tests
(a plain helper module, as tests/steer_cases.py is).

SHAPES: the smallest panels at which the windowed kernel can go wrong.  Every window length of WINS -- below, at and above
one and two iterations of the kernel in either precision (16 segments in float32, 8 in float64): the two-deep load pipeline,
its single leftover iteration, the checked tail -- against 5, 17 and 64 records (one ragged tile, a second tile with one
record, the cap), and the remaining record counts once each.  The hop, the bin count, the bin range, the number of windows and
the segments left over after the last window cycle through their values along the table; tests/test_windows_cpu.py asserts
that every value occurs.

`restate` is the float64 statement of qi_cross_spectra_windows: an einsum per window.

The timeline case: beam_cases' five sensors, slowness grid and bands, two records of 4096 samples end to end -- a noise
source at grid point 25, then another at grid point 55, each built as beam_cases.pw_records builds its one -- at 256-sample
segments with overlap 128 (63 segments) in windows of 8 segments every 4: 14 windows, the first six wholly in the first half,
the last six wholly in the second.
"""
import collections
import functools

import numpy as np

import beam_cases as bc
import capon_cases as cpc
import csd_cases as cc
import music_cases as mc

ROOT = bc.ROOT
DTYPES = bc.DTYPES
TOL = bc.TOL

Shape = collections.namedtuple("Shape", "id C nf nseg win hop bins nwin rest")

RECORD_COUNTS = (1, 2, 5, 16, 17, 33, 64)
WINS = (1, 3, 7, 8, 9, 16, 17, 31, 32, 33, 40)
HOPS = ("1", "3", "win", "win+3")
BIN_COUNTS = (1, 5, 9)
RANGES = ("all", "interior", "to_end", "single")


def _bins(nf, kind):
    if nf == 1 or kind == "all":
        return (0, nf)
    if kind == "interior":
        return (1, nf - 2)
    if kind == "to_end":
        return (nf // 2, nf - nf // 2)
    return (nf - 2, 1)


def _table():
    out = []
    pairs = [(C, win) for win in WINS for C in (5, 17, 64)] + [(1, 9), (2, 17), (16, 33), (33, 8), (33, 40), (16, 1)]
    for k, (C, win) in enumerate(pairs):
        hop_kind = HOPS[(k + k // 4) % 4]
        hop = {"1": 1, "3": 3, "win": win, "win+3": win + 3}[hop_kind]
        nf = BIN_COUNTS[(k + k // 3) % 3]
        kind = RANGES[(k + k // 5) % 4]
        nwin = 2 + k % 3
        rest = (hop - 1) * (k % 2)  # nothing left over, or as much as fits without another window
        nseg = (nwin - 1) * hop + win + rest
        first, count = _bins(nf, kind)
        cid = f"c{C}_w{win}_h{hop}_s{nseg}_f{nf}_b{first}+{count}"
        out.append(Shape(cid, C, nf, nseg, win, hop, (first, count), nwin, rest))
    return tuple(out)


SHAPES = _table()


def ids():
    return [s.id for s in SHAPES]


def by_id(cid):
    return next(s for s in SHAPES if s.id == cid)


def range_kind(shape):
    first, count = shape.bins
    if (first, count) == (0, shape.nf):
        return "all"
    if count == 1:
        return "single"
    return "to_end" if first + count == shape.nf else "interior"


def windows(nseg, win, hop):
    return (nseg - win) // hop + 1


def panel(shape):
    """[C, nf, nseg] complex128 of float32 values: both precisions read the same numbers.  Random in EVERY segment: what lies
    past a window's end is there to leak."""
    rng = np.random.default_rng([53, shape.C, shape.nseg, shape.win])
    z = rng.standard_normal((shape.C, shape.nf, shape.nseg, 2)).astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(z[..., 0] + 1j * z[..., 1])


def weights(shape):
    """One host weight per FORMED bin, none a power of two."""
    return np.linspace(0.3, 1.9, shape.bins[1]) if shape.bins[1] > 1 else np.array([0.7])


def covered(nseg, win, hop):
    """[nseg] bool: the segments that some window holds."""
    c = np.zeros(nseg, dtype=bool)
    for w in range(windows(nseg, win, hop)):
        c[w * hop:w * hop + win] = True
    return c


def restate(z, first, count, win, hop, weight=None):
    """csd [nwin, count, C, C] complex128: per window w the einsum over the segments w hop .. w hop + win - 1."""
    z = np.asarray(z).astype(np.complex128)
    nwin = windows(z.shape[2], win, hop)
    w = np.ones(count) if weight is None else np.asarray(weight, dtype=np.float64)
    out = np.empty((nwin, count, z.shape[0], z.shape[0]), dtype=np.complex128)
    for k in range(nwin):
        cut = z[:, first:first + count, k * hop:k * hop + win]
        out[k] = np.einsum("ifs,jfs->fij", np.conj(cut), cut) * w[:, None, None]
    return out


def integer_panel(C, nf, nseg):
    """Gaussian-integer panel (|re|, |im| <= 3), asymmetric in the record index, of tests/test_gpu_csd.py's kind: every sum
    of up to 40 products is an integer below 2^24, exact in either precision."""
    i, f, s = np.arange(C)[:, None, None], np.arange(nf)[None, :, None], np.arange(nseg)[None, None, :]
    re = (3 * i + 5 * f + 2 * s + i * s) % 7 - 3
    im = (5 * i + 2 * f + 3 * s + (i * i) % 5) % 7 - 3
    return (re + 1j * im).astype(np.complex128)


# ---- the timeline case ------------------------------------------------------------------------------------------------------
TL_SEG, TL_OVERLAP, TL_HALF = 256, 128, 4096
TL_WIN, TL_HOP = 8, 4
TL_POINTS = (25, 55)  # rows of beam_cases.pw_slowness(): the source of the first and of the second half
TL_FIRST, TL_SECOND = range(0, 6), range(8, 14)  # the windows wholly in one half; 6 and 7 straddle the change
TL_CAPON_LOADING = 0.1
TL_MARGIN = 1.03  # the smallest peak over its runner-up is 1.06 (Bartlett, band 3; tests/test_windows_cpu.py computes it again)


def _half(point, seed):
    """One half, built as beam_cases.pw_records builds its record."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(TL_HALF)
    own = rng.standard_normal((len(bc.PW_POSITIONS_M), TL_HALF))
    tau = bc.pw_delays()[point]
    f = np.fft.rfftfreq(TL_HALF, 1 / bc.PW_FS)
    x = np.fft.irfft(np.fft.rfft(src)[None, :] * np.exp(-2j * np.pi * f[None, :] * tau[:, None]), TL_HALF)
    return x + bc.PW_OWN * own


@functools.lru_cache(maxsize=None)
def timeline_records():
    """[5, 8192] float64."""
    x = np.concatenate([_half(TL_POINTS[0], [31, 0]), _half(TL_POINTS[1], [31, 1])], axis=1)
    x.setflags(write=False)
    return x


def timeline_case():
    return cc.Case("timeline_two_sources", len(bc.PW_POSITIONS_M), 2 * TL_HALF, TL_SEG, TL_OVERLAP, TL_SEG, "fused", None)


def timeline_edges_hz():
    return np.fft.rfftfreq(TL_SEG, 1 / bc.PW_FS)[list(bc.PW_BANDS)]


def timeline_times():
    """The centre of the samples every window spans, in seconds."""
    hop = TL_SEG - TL_OVERLAP
    nwin = windows(cc.segments(timeline_case()), TL_WIN, TL_HOP)
    return (np.arange(nwin) * TL_HOP * hop + ((TL_WIN - 1) * hop + TL_SEG) / 2) / bc.PW_FS


@functools.lru_cache(maxsize=None)
def timeline_matrices():
    """(csd [nwin, bins, 5, 5] complex128 of the bins of the bands with csd_windows_pow2's weights, their frequencies, the
    bands as offsets into them)."""
    case = timeline_case()
    z = cc.panel(timeline_records(), case)
    first, count = bc.PW_BANDS[0], bc.PW_BANDS[-1] - bc.PW_BANDS[0]
    w = cc.bin_weights(case.nfft, TL_WIN, cc.scale2(cc.window_of(case), "spectrum"))[first:first + count]
    s = restate(z, first, count, TL_WIN, TL_HOP, w)
    s.setflags(write=False)
    return s, np.fft.rfftfreq(case.nfft, 1 / bc.PW_FS)[first:first + count], np.asarray(bc.PW_BANDS) - first


@functools.lru_cache(maxsize=None)
def timeline_power(method):
    """power [nwin, nb, G] float64 of the restatements: beam_cases.restate (the semblance), capon_cases.capon at
    TL_CAPON_LOADING, music_cases.music with one source."""
    s, freq, bands = timeline_matrices()
    tau = bc.pw_delays()
    out = []
    for sw in s:
        if method == "bartlett":
            out.append(bc.restate(sw, freq, tau, bands, normalize=True))
        elif method == "capon":
            out.append(cpc.capon(cpc.whiten(sw, TL_CAPON_LOADING), freq, tau, bands))
        else:
            out.append(mc.music(mc.eigh64(sw)[1], 1, freq, tau, bands))
    p = np.stack(out)
    p.setflags(write=False)
    return p


def peak_ratios(power):
    """(peak index [nwin, nb], peak over runner-up [nwin, nb]) of a timeline's power."""
    order = np.argsort(power, axis=2)
    best = np.take_along_axis(power, order[:, :, -1:], axis=2)[..., 0]
    second = np.take_along_axis(power, order[:, :, -2:-1], axis=2)[..., 0]
    return order[:, :, -1], best / second
