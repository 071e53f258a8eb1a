"""Cases of the banded cross-spectrum tests and NumPy restatements of include/qi_bands.h, shared by the CPU and GPU tests (a
plain helper module, as tests/window_cases.py is).

SHAPES: the smallest panels at which the banded kernel can go wrong.  Every band has its own (terms, stride, hop).  The term
counts of TERMS lie below, at and above one and two iterations of the kernel in either precision (16 terms in float32, 8 in
float64): the two-deep load pipeline, its single leftover iteration, the checked tail, and 200 terms for a long chain.  The
first band of a shape takes every term count against 5, 17 and 64 records (one ragged tile, a second tile with one record, the
cap) and the remaining record counts once each; the other bands, the strides, the hops (1, 3, the span, the span + 3: gaps),
the number of formed bands (1 .. 6) inside a panel of up to 9 and the samples left over after the longest band's last window
cycle through their values along the table.  Every fourth shape has stride 1 throughout: those are held against
engine.cross_spectra_windows.  tests/test_bands_cpu.py asserts that every value occurs.

`layout` restates qi_cross_spectra_bands_layout, `restate` is the float64 statement of qi_cross_spectra_bands: an einsum per
window on the strided slice.

The plane-wave case: beam_cases' five sensors at a quarter of their distances (the largest delay across the array is then
about 13 samples at 800 Hz: the narrow-band assumption of beamform.fk_timeline_cq holds in the lower bands and fails towards
the highest), its slowness grid and its source, 4096 samples, the order-12 CWT, windows of PW_CYCLES periods.
"""
import collections
import functools

import numpy as np

import beam_cases as bc

ROOT = bc.ROOT
DTYPES = bc.DTYPES
TOL = bc.TOL

Shape = collections.namedtuple("Shape", "id C nb n bins terms hop stride")

RECORD_COUNTS = (1, 2, 5, 16, 17, 33, 64)
TERMS = (1, 3, 16, 17, 31, 33, 40, 200)
STRIDES = (1, 2, 3, 7)
HOPS = ("1", "3", "span", "span+3")
N_MAX = 700


def span_of(terms, stride):
    return (np.asarray(terms, dtype=np.int64) - 1) * np.asarray(stride, dtype=np.int64) + 1


def layout(n, terms, hop, stride):
    """offsets [count + 1] int64: offset[b + 1] - offset[b] = (n - span[b]) // hop[b] + 1."""
    span = span_of(terms, stride)
    assert np.all(span <= n) and np.all(np.asarray(hop) >= 1) and np.all(np.asarray(terms) >= 1) and np.all(np.asarray(stride) >= 1)
    n_win = (n - span) // np.asarray(hop, dtype=np.int64) + 1
    return np.concatenate([[0], np.cumsum(n_win)]).astype(np.int64)


def _table():
    out = []
    pairs = [(C, t) for t in TERMS for C in (5, 17, 64)] + [(1, 17), (2, 33), (16, 40), (33, 16), (33, 3), (16, 1)]
    for k, (C, lead) in enumerate(pairs):
        count = 1 + k % 6
        nb = min(9, count + k % 4)
        first = (k // 2) % (nb - count + 1)
        terms, stride, hop = [], [], []
        for b in range(count):
            t = lead if b == 0 else TERMS[(k + 3 * b) % len(TERMS)]
            s = 1 if k % 4 == 0 else STRIDES[(k + b + k // 4) % 4]
            while (t - 1) * s + 1 > N_MAX - 10:  # (200 terms: stride 1, 2 or 3)
                s = STRIDES[STRIDES.index(s) - 1]
            span = (t - 1) * s + 1
            kind = HOPS[(k + 2 * b + k // 3 + b // 2) % 4]
            terms.append(t)
            stride.append(s)
            hop.append({"1": 1, "3": 3, "span": span, "span+3": span + 3}[kind])
        spans = span_of(terms, stride)
        long = int(np.argmax(spans))
        # the longest band gets one, two or three windows and, every other shape, samples left over after the last one
        n = int(spans[long]) + (k % 3) * hop[long] + (hop[long] - 1) * (k % 2)
        n = min(max(n, int(spans[long])), N_MAX)
        cid = f"c{C}_n{n}_b{first}+{count}of{nb}_t{'.'.join(map(str, terms))}_s{'.'.join(map(str, stride))}_h{'.'.join(map(str, hop))}"
        out.append(Shape(cid, C, nb, n, (first, count), tuple(terms), tuple(hop), tuple(stride)))
    return tuple(out)


SHAPES = _table()


def ids():
    return [s.id for s in SHAPES]


def by_id(cid):
    return next(s for s in SHAPES if s.id == cid)


def offsets_of(shape):
    return layout(shape.n, shape.terms, shape.hop, shape.stride)


def hop_kinds(shape):
    """The names of HOPS that each band's hop goes by (a hop may go by two: span 1 and hop 1)."""
    spans = span_of(shape.terms, shape.stride)
    return [{k for k, h in (("1", 1), ("3", 3), ("span", int(sp)), ("span+3", int(sp) + 3)) if h == hp} for sp, hp in zip(spans, shape.hop)]


def panel(shape):
    """[C, nb, n] complex128 of float32 values: both precisions read the same numbers.  Random in EVERY sample: what lies
    between the strided terms, in the gaps, past the last window and in the other bands is there to leak."""
    rng = np.random.default_rng([59, shape.C, shape.n, shape.terms[0]])
    z = rng.standard_normal((shape.C, shape.nb, shape.n, 2)).astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(z[..., 0] + 1j * z[..., 1])


def weights(shape):
    """One host weight per FORMED band, none a power of two."""
    return np.linspace(0.3, 1.9, shape.bins[1]) if shape.bins[1] > 1 else np.array([0.7])


def read(shape):
    """[count, n] bool: the samples of every formed band that some term of some window reads."""
    off = offsets_of(shape)
    c = np.zeros((shape.bins[1], shape.n), dtype=bool)
    for b, (t, h, s) in enumerate(zip(shape.terms, shape.hop, shape.stride)):
        for w in range(off[b + 1] - off[b]):
            c[b, w * h:w * h + (t - 1) * s + 1:s] = True
    return c


def window_slice(b, w, terms, hop, stride):
    """The samples of window w of band b as a slice of the time axis."""
    return slice(w * hop[b], w * hop[b] + (terms[b] - 1) * stride[b] + 1, stride[b])


def restate(z, first, terms, hop, stride, weight=None):
    """(offsets [count + 1], csd [total, C, C] complex128): per band and window the einsum over the strided slice."""
    z = np.asarray(z).astype(np.complex128)
    count = len(terms)
    off = layout(z.shape[2], terms, hop, stride)
    wt = np.ones(count) if weight is None else np.asarray(weight, dtype=np.float64)
    out = np.empty((off[-1], z.shape[0], z.shape[0]), dtype=np.complex128)
    for b in range(count):
        for w in range(off[b + 1] - off[b]):
            cut = z[:, first + b, window_slice(b, w, terms, hop, stride)]
            out[off[b] + w] = np.einsum("is,js->ij", np.conj(cut), cut) * wt[b]
    return off, out


def coherence_of(csd):
    d = np.real(np.einsum("mii->mi", csd))
    with np.errstate(all="ignore"):
        return np.abs(csd) ** 2 / (d[:, :, None] * d[:, None, :])


def integer_panel(C, nb, n):
    """Gaussian-integer panel (|re|, |im| <= 3), asymmetric in the record index, of tests/window_cases.py's kind: every sum
    of up to 200 products is an integer below 2^24, exact in either precision."""
    i, f, s = np.arange(C)[:, None, None], np.arange(nb)[None, :, None], np.arange(n)[None, None, :]
    re = (3 * i + 5 * f + 2 * s + i * s + (s * s) % 11) % 7 - 3
    im = (5 * i + 2 * f + 3 * s + (i * i) % 5 + (s // 3) % 5) % 7 - 3
    return (re + 1j * im).astype(np.complex128)


# ---- the plane-wave case ------------------------------------------------------------------------------------------------------
PW_SCALE = 0.25  # of beam_cases' positions
PW_N, PW_ORDER, PW_CYCLES, PW_HOP_FRACTION = 4096, 12, 40.0, 0.5
PW_MAX_TERMS = 64  # the four lowest bands that fit are summed at every 63rd sample, the highest at every second
PW_MIN_BANDS = 3


def pw_positions():
    return bc.PW_POSITIONS_M * PW_SCALE


def pw_delays():
    return bc.pw_slowness() @ pw_positions().T  # tau[g, i]


@functools.lru_cache(maxsize=None)
def pw_records():
    """[5, 4096] float64, built as beam_cases.pw_records builds its own, on the smaller array."""
    rng = np.random.default_rng([67, PW_N])
    src = rng.standard_normal(PW_N)
    own = rng.standard_normal((len(bc.PW_POSITIONS_M), PW_N))
    tau = pw_delays()[bc.pw_true_index()]
    f = np.fft.rfftfreq(PW_N, 1 / bc.PW_FS)
    x = np.fft.irfft(np.fft.rfft(src)[None, :] * np.exp(-2j * np.pi * f[None, :] * tau[:, None]), PW_N)
    x = x + bc.PW_OWN * own
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pw_oracle():
    """(frequency_hz [71], panel [5, 71, 4096] complex128): the oracle's order-12 CWT of every record, computed once."""
    from oracle import tfr_oracle as orc

    panels = [orc.cwt_fft(PW_ORDER, r, bc.PW_FS) for r in pw_records()]
    f, z = panels[0][0], np.stack([p[2] for p in panels])
    z.setflags(write=False)
    return f, z


@functools.lru_cache(maxsize=None)
def pw_asserted_bands():
    """The bands (of those that fit) that the GPU test asserts, chosen on the CPU from the oracle's panel."""
    f, z = pw_oracle()
    off, power = pw_power(z, f, pw_geometry(f))
    return tuple(pw_asserted(pw_margins(off, power)))


def pw_asserted(rows):
    """The bands of pw_margins' rows that the tests assert: every window at the source, by at least beam_cases.PW_MARGIN."""
    return [b for b, (ok, margin) in enumerate(rows) if ok and margin >= bc.PW_MARGIN]


def pw_geometry(frequency_hz, max_terms=PW_MAX_TERMS):
    from quantum_inferno_amd import beamform

    return beamform.constant_q_windows(frequency_hz, bc.PW_FS, PW_N, PW_CYCLES, PW_HOP_FRACTION, max_terms)


def pw_power(panel, frequency_hz, geometry):
    """(offsets, semblance [total, G] float64) of a panel [5, bands, 4096]: restate with weight 1 / terms, then
    beam_cases.restate with every matrix its own band and the band's frequency repeated per window."""
    bins, terms, hop, stride = geometry
    off, s = restate(panel, bins[0], terms, hop, stride, 1.0 / terms)
    f_all = np.repeat(np.asarray(frequency_hz)[bins[0]:bins[0] + bins[1]], np.diff(off))
    return off, bc.restate(s, f_all, pw_delays(), normalize=True)


def pw_margins(offsets, power):
    """Per band: (every window peaks at the source's grid point, the smallest peak less its runner-up over the windows)."""
    order = np.sort(power, axis=1)
    margin = order[:, -1] - order[:, -2]
    at = np.argmax(power, axis=1) == bc.pw_true_index()
    return [(bool(at[a:b].all()), float(margin[a:b].min())) for a, b in zip(offsets[:-1], offsets[1:])]
