"""Cases of the time-domain beam tests and float64 NumPy restatements of include/qi_timebeam.h, shared by the CPU and GPU
tests (a plain helper module: imports without a GPU).

`delayed` is the header's y for one delay row, written from the formula: every tap is multiplied in, zero or not, and a read
outside the record is a zero.  `restate` gives the traces and both normalisations of the power for a whole table; a row
beyond max_shift or with a phase outside the bank is NaN.  `bank` and `quantize` restate engine.delay_bank and
engine.quantize_delays.

The shape cases: records that carry one signal of magnitude 1 .. 2 and random sign, at sensor i later by a whole number of
samples d_i (a circular roll), plus own noise at 0.1 (none where the window is one sample long).  Row TRUE_ROW of the grid
(the last row but one, or the only one) holds shift = d, phase = 0: the semblance there is near 1 in every window, far above
the random rows -- peak_index has to agree in every window.  The other rows draw shifts from -SHIFT .. SHIFT and phases from
the whole bank.
"""
import collections
import functools
import os

import numpy as np

import beam_cases as bc
from beam_cases import PW_FS, PW_MARGIN, PW_N, PW_POSITIONS_M, pw_delays, pw_records, pw_slowness, pw_true_index  # noqa: F401
from steer_cases import pw_source, relative_rms  # noqa: F401

ROOT = bc.ROOT
DTYPES = bc.DTYPES
TOL = bc.TOL  # the project's tolerance of the array calls, as a fraction of the case's largest value
MAX_SENSORS = 64
# the kernel's sizes (csrc/qi_timebeam.hip: kTbChunk samples of a record and kTbRowBlock delay rows per workgroup; the
# header's QI_TIMEBEAM_CHUNK and QI_TIMEBEAM_ROW_BLOCK) and the bound of its LDS halo (QI_TIMEBEAM_LDS_MAX_SHIFT)
CHUNK, ROW_BLOCK, LDS_MAX_SHIFT, MAX_SHIFT = 256, 16, 1024, 1 << 20
SHIFT = 60  # the random rows' largest |shift|
BANKS = ((1, 1), (1, 8), (64, 2), (64, 4), (64, 8), (64, 16), (256, 8))
BETA = 5.0

Case = collections.namedtuple("Case", "id n C G win hop P T reach noise")


def _case(n, C, G, win, hop, bank, reach=SHIFT, noise=0.1):
    P, T = bank
    win = n if win == "n" else win
    return Case(f"n{n}_c{C}_g{G}_w{win}h{hop}_p{P}t{T}_r{reach}", n, C, G, win, hop, P, T, reach, noise)


CASES = (
    # the issue's record lengths, sensor counts, grids, windows and banks
    _case(700, 2, 1, 64, 32, (1, 1)), _case(700, 3, 7, 1, 1, (64, 8), noise=0.0), _case(700, 5, 65, 100, 37, (64, 2)),
    _case(2048, 17, 257, 64, 32, (64, 4)), _case(2048, 64, 7, "n", 1, (64, 16)), _case(3001, 5, 65, 100, 37, (256, 8)),
    _case(3001, 2, 7, 64, 32, (1, 8)), _case(700, 64, 1, 100, 37, (64, 8)),
    # a hop that divides the window and is a chunk or more: windows from per-hop sums; one below, at, above the chunk
    _case(2048, 3, 17, 512, 256, (64, 8)), _case(2048, 5, 16, 256, 256, (64, 4)), _case(3001, 3, 15, 1024, 512, (1, 8)),
    _case(2048, 5, 7, 255, 128, (64, 8)), _case(2048, 3, 7, 257, 100, (64, 2)), _case(2048, 2, 7, 256, 128, (64, 16)),
    _case(255, 3, 15, "n", 1, (64, 8)), _case(256, 5, 16, "n", 1, (64, 8)), _case(257, 3, 17, 256, 1, (64, 8)),
    # the LDS halo at its bound, and the path through L2 above it
    _case(3001, 3, 17, 100, 37, (64, 8), reach=LDS_MAX_SHIFT), _case(700, 5, 17, 100, 37, (64, 8), reach=LDS_MAX_SHIFT + 1),
    _case(2048, 3, 16, 512, 256, (1, 8), reach=LDS_MAX_SHIFT + 1), _case(700, 17, 7, 64, 32, (256, 8), reach=MAX_SHIFT),
)


def ids():
    return [c.id for c in CASES]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def true_row(case):
    return max(case.G - 2, 0)


def windows(n, win, hop):
    return 1 + (n - win) // hop


# ---- the bank and the quantiser, restated -------------------------------------------------------------------------------------------
def bank(P, T, beta=BETA):
    """[P, T] float64: the Kaiser-windowed sinc of the issue, row by row."""
    if T == 1:
        assert P == 1
        return np.ones((1, 1))
    c = (T - 1) // 2
    rows = []
    for p in range(P):
        u = (np.arange(T) - c).astype(np.float64) - p / P
        a = u / (T / 2.0)
        inside = np.abs(a) <= 1.0
        h = np.where(inside, np.sinc(u) * np.i0(beta * np.sqrt(np.where(inside, 1.0 - a * a, 0.0))) / np.i0(beta), 0.0)
        rows.append(h / h.sum())
    rows[0] = np.zeros(T)
    rows[0][c] = 1.0
    return np.stack(rows)


def quantize(tau_s, rate_hz, P):
    """(shift, phase) int64 and the largest |shift|: q = floor(tau rate P + 0.5), shift = q // P, phase = q mod P."""
    q = np.floor(np.asarray(tau_s, dtype=np.float64) * rate_hz * P + 0.5).astype(np.int64)
    shift, phase = q // P, q % P
    return shift, phase, int(np.abs(shift).max())


# ---- the calls, restated ----------------------------------------------------------------------------------------------------------------
def delayed(x, taps, shift_row, phase_row):
    """y [C, n] of one delay row: sum over m of taps[phase_i][m] x_i[t + shift_i + m - c], zeros outside the record."""
    C, n = x.shape
    T = taps.shape[1]
    c = (T - 1) // 2
    t = np.arange(n, dtype=np.int64)
    y = np.zeros((C, n))
    with np.errstate(all="ignore"):
        for i in range(C):
            for m in range(T):
                idx = t + int(shift_row[i]) + m - c
                ok = (idx >= 0) & (idx < n)
                y[i] = y[i] + taps[int(phase_row[i]), m] * np.where(ok, x[i, np.clip(idx, 0, n - 1)], 0.0)
    return y


def row_is_good(shift_row, phase_row, P, max_shift):
    s, p = np.asarray(shift_row, dtype=np.int64), np.asarray(phase_row, dtype=np.int64)
    return bool(np.all(np.abs(s) <= max_shift) and np.all((p >= 0) & (p < P)))


def window_sums(v, win, hop):
    """sum of v[w hop : w hop + win] for every window -> [nwin]."""
    with np.errstate(all="ignore"):
        return np.lib.stride_tricks.sliding_window_view(v, win)[::hop].sum(axis=-1)


Restated = collections.namedtuple("Restated", "traces mean_square semblance")


def restate(x, taps, shift, phase, max_shift, win, hop):
    """traces [rows, n], and the power [nwin, rows] of both normalisations, float64."""
    x, taps = np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    C, n = x.shape
    rows = len(shift)
    nwin = windows(n, win, hop)
    traces, ms, sem = np.full((rows, n), np.nan), np.full((nwin, rows), np.nan), np.full((nwin, rows), np.nan)
    for g in range(rows):
        if not row_is_good(shift[g], phase[g], taps.shape[0], max_shift):
            continue
        y = delayed(x, taps, shift[g], phase[g])
        b = y.sum(axis=0)
        traces[g] = b / C
        with np.errstate(all="ignore"):
            B, E = window_sums(b * b, win, hop), window_sums((y * y).sum(axis=0), win, hop)
            ms[:, g] = B / (C * C * win)
            sem[:, g] = B / (C * E)
    return Restated(traces, ms, sem)


def samples_read(n, T, shift, phase, P, max_shift, t_count=None):
    """[C, n] bool: the samples some tap of some good row reads for an output t in 0 .. t_count - 1."""
    shift = np.asarray(shift, dtype=np.int64)
    c = (T - 1) // 2
    read = np.zeros((shift.shape[1], n), dtype=bool)
    t_count = n if t_count is None else t_count
    for g in range(len(shift)):
        if not row_is_good(shift[g], phase[g], P, max_shift):
            continue
        for i in range(shift.shape[1]):
            lo, hi = int(shift[g, i]) - c, int(shift[g, i]) - c + t_count - 1 + T - 1
            read[i, max(lo, 0):max(min(hi, n - 1) + 1, 0)] = True
    return read


def peaks_of(power):
    """np.argmax's rules -> (index [nwin] int64, value [nwin])."""
    return bc.peaks_of(power)


def margins(power):
    """[nwin]: the best value's distance to the runner-up; inf where the row holds a NaN (the first NaN is the peak, whatever
    the numbers) or a single entry."""
    p = np.asarray(power, dtype=np.float64)
    out = np.full(p.shape[0], np.inf)
    if p.shape[1] < 2:
        return out
    clean = ~np.isnan(p).any(axis=1)
    top = np.sort(p[clean], axis=1)
    out[clean] = top[:, -1] - top[:, -2]
    return out


def largest(a):
    return float(np.nanmax(np.abs(a)))


# ---- the shape cases' inputs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(records [C, n] float64, taps [P, T] float64, shift [G, C] int32, phase [G, C] int32) of a case; read-only."""
    case = by_id(cid)
    rng = np.random.default_rng([31, case.n, case.C, case.G, case.T])
    src = rng.uniform(1.0, 2.0, case.n) * rng.choice([-1.0, 1.0], case.n)
    d = rng.integers(-SHIFT // 2, SHIFT // 2 + 1, case.C)
    x = np.stack([np.roll(src, int(k)) for k in d]) + case.noise * rng.standard_normal((case.C, case.n))
    shift = rng.integers(-SHIFT, SHIFT + 1, (case.G, case.C)).astype(np.int32)
    phase = rng.integers(0, case.P, (case.G, case.C)).astype(np.int32)
    shift[true_row(case)], phase[true_row(case)] = d, 0
    out = (x, bank(case.P, case.T), shift, phase)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(cid):
    case = by_id(cid)
    x, taps, shift, phase = inputs(cid)
    return restate(x, taps, shift, phase, case.reach, case.win, case.hop)


# ---- the exact cases: whole numbers through the impulse bank ----------------------------------------------------------------------------
def exact_inputs(C, n=512, G=9):
    """Records of whole numbers in -8 .. 8, shifts in -40 .. 40 (row 0: none; the last row: wholly off the record), phase 0."""
    rng = np.random.default_rng([37, C, n])
    x = rng.integers(-8, 9, (C, n)).astype(np.float64)
    shift = rng.integers(-40, 41, (G, C)).astype(np.int32)
    shift[0] = 0
    shift[-1] = np.where(np.arange(C) % 2 == 0, n, -n)
    return x, shift, np.zeros((G, C), dtype=np.int32)


def exact_restate(x, shift, win, hop):
    """(traces [G, n], mean square [nwin, G]) in whole-number arithmetic (int64 sums), the quotients exact in float32."""
    C, n = x.shape
    xi = x.astype(np.int64)
    t = np.arange(n)
    traces, power = [], []
    for row in shift:
        idx = t[None, :] + row.astype(np.int64)[:, None]
        y = np.where((idx >= 0) & (idx < n), np.take_along_axis(xi, np.clip(idx, 0, n - 1), axis=1), 0)
        b = y.sum(axis=0)
        assert np.abs(b).max() ** 2 * win < 2 ** 24
        traces.append(b / C)
        power.append(window_sums(b * b, win, hop) / (C * C * win))
    return np.stack(traces), np.stack(power, axis=1)


# ---- the plane wave of tests/beam_cases.py ------------------------------------------------------------------------------------------------
PW_WINDOWS = ((256, 128), (100, 37), (64, 32))  # 31, 109 and 127 windows
PW_BANK = (64, 8)
PW_INTERIOR = 256  # samples left out at either end of a trace


def pw_tables(P):
    """(shift, phase, max_shift) of the grid of beam_cases.pw_slowness() at PW_FS."""
    return quantize(pw_delays(), PW_FS, P)


@functools.lru_cache(maxsize=None)
def pw_restated(win, hop, P=PW_BANK[0], T=PW_BANK[1]):
    shift, phase, reach = pw_tables(P)
    return restate(pw_records(), bank(P, T), shift, phase, reach, win, hop)


def pw_steer_tables(P):
    """The two rows of the trace tests: the source's slowness and the grid centre (0, 0)."""
    s = pw_slowness()
    rows = np.stack([s[pw_true_index()], s[len(s) // 2]])
    return rows, quantize(pw_delays(rows), PW_FS, P)


def low_pass(a):
    """The ideal low-pass at half of Nyquist along the last axis (an FFT mask)."""
    spec = np.fft.rfft(a, axis=-1)
    spec[..., np.fft.rfftfreq(a.shape[-1]) > 0.25] = 0.0
    return np.fft.irfft(spec, a.shape[-1], axis=-1)


@functools.lru_cache(maxsize=None)
def pw_low_passed():
    """(records [5, n], source [n]) of the plane wave, both through low_pass; read-only."""
    out = (low_pass(pw_records()), low_pass(pw_source()))
    for a in out:
        a.setflags(write=False)
    return out


def rms_from(trace, src, margin=PW_INTERIOR):
    """relative_rms's figure against another source: the RMS distance over the interior, over the source's RMS there."""
    lo, hi = margin, len(src) - margin
    return float(np.sqrt(np.mean((trace[lo:hi] - src[lo:hi]) ** 2) / np.mean(src[lo:hi] ** 2)))


def header_text():
    with open(os.path.join(ROOT, "include", "qi_timebeam.h")) as fh:
        return fh.read()
