"""Cases and NumPy restatements of the synchrosqueezing tests (a plain helper module, not collected; imports without a GPU).

The restatements state include/qi_squeeze.h in NumPy:
  valid_mask      which elements have a frequency at all, in the PANEL's precision (the device's mask must be exactly this)
  ifreq_restated  the frequencies in float64 (the device's are held to a tolerance, as wrapped phase)
  bins_of         the bin rule, in the precision of the frequencies it is handed
  squeeze_restated  the reassignment in the PANEL's precision, band by band in ascending order: exact given the frequencies
  synchro_restated  the whole chain in float64, with the frequencies, for the fused call's tolerance test
  bin_edges_restated  scales_dyadic.squeeze_bin_edges, value by value
and the method on the repository's own CPU panels (the tone and the chirp of the issue's experiment): concentration, ridges.

CASES: the shapes at which the kernel can go wrong -- n around the tile of 256 columns, one column and its partner alone,
several tiles with a ragged last one; one band and more bands than a wave; one bin, a few, bin counts around 32 and around 64
(a wave's lanes, and where an earlier form of the kernel changed chunks of LDS rows: the kernel that is kept sums in the
result itself and has one path for every bin count) and 568 = 71 x 8; one record and three.
"""
import collections
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float32", "float64")
COMPLEX = {"float32": np.complex64, "float64": np.complex128}
# the kernel's sizes (include/qi_squeeze.h: QI_SQUEEZE_TILE, QI_SQUEEZE_MAX_*)
TILE = 256
MAX_BINS, MAX_BANDS = 4096, 65536
FS = 800.0
# the project's coefficient tolerances: the frequency as wrapped phase, and the fused result against float64 as a fraction
# of the largest modulus, away from the edges by EDGE_GUARD * fs
PHASE_TOL = {"float32": 2e-5, "float64": 1e-11}
FUSED_TOL = {"float32": 1e-4, "float64": 1e-10}
EDGE_GUARD = {"float32": 1e-5, "float64": 1e-12}
EXCLUDED_CAP = 0.25

Case = collections.namedtuple("Case", "id C nb n nbin")


def _case(C, nb, n, nbin):
    return Case(f"c{C}_b{nb}_n{n}_k{nbin}", C, nb, n, nbin)


CASES = (
    _case(1, 1, 2, 1), _case(3, 5, 3, 7), _case(1, 24, 255, 31), _case(3, 24, 256, 32), _case(1, 24, 257, 33),
    _case(1, 71, 700, 568), _case(1, 24, 3001, 64), _case(3, 24, 700, 65), _case(1, 71, 3001, 7), _case(3, 5, 700, 1),
    _case(3, 71, 257, 568), _case(1, 71, 2, 568), _case(1, 1, 700, 7), _case(1, 5, 3001, 568), _case(1, 71, 256, 65),
    _case(3, 24, 3, 64),
)


def ids():
    return [c.id for c in CASES]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def bins(case, dtype=None):
    return case.nbin


def header_text():
    with open(os.path.join(ROOT, "include", "qi_squeeze.h")) as fh:
        return fh.read()


def real_of(z):
    return np.float32 if z.dtype == np.complex64 else np.float64


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
def partners(n):
    """(u, last): the partner column of every column, and which column swaps the roles."""
    u = np.arange(n) + 1
    u[-1] = n - 2
    last = np.zeros(n, dtype=bool)
    last[-1] = True
    return u, last


def power_of(z):
    """re^2 + im^2 in the panel's precision, every product and the sum rounded on their own."""
    with np.errstate(over="ignore", invalid="ignore"):
        re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        return re * re + im * im


def valid_mask(z, floor):
    p = power_of(z)
    with np.errstate(invalid="ignore"):
        ok = (p >= real_of(z)(floor)) & (p < np.inf)
    return ok & ok[..., partners(z.shape[-1])[0]]


def ifreq_restated(z, fs, carrier=None, floor=0.0):
    """float64 frequencies [C, nb, n] of a panel of either precision; the carrier and the rate as the panel's precision holds
    them; NaN exactly where valid_mask says."""
    r = real_of(z)
    zw = z.astype(np.complex128)
    u, last = partners(z.shape[-1])
    later, earlier = np.where(last, zw, zw[..., u]), np.where(last, zw[..., u], zw)
    with np.errstate(over="ignore", invalid="ignore"):
        dr = later.real * earlier.real + later.imag * earlier.imag
        di = later.imag * earlier.real - later.real * earlier.imag
        car = np.zeros(z.shape[1]) if carrier is None else np.asarray(carrier, dtype=np.float64).astype(r).astype(np.float64)
        f = car[:, None] + float(r(fs)) * np.arctan2(di, dr) / (2.0 * np.pi)
    f[~valid_mask(z, floor)] = np.nan
    return f


def bins_of(f, edges):
    """k(f) = (number of edges <= f) - 1 where 0 <= k < nbin, else -1; `edges` in the precision of f."""
    edges = np.asarray(edges).astype(f.dtype)
    k = np.searchsorted(edges, f, side="right").astype(np.int64) - 1  # (NaN sorts behind every edge: nbin, dropped)
    k[(k < 0) | (k >= len(edges) - 1)] = -1
    return k


def squeeze_restated(z, f, edges, weight=None):
    """out [C, nbin, n] in the panel's precision: band by band in ascending order, product rounded per component, then
    added, from +0."""
    r = real_of(z)
    C, nb, n = z.shape
    nbin = len(edges) - 1
    k = bins_of(np.asarray(f).astype(r), edges)
    w = np.ones(nb, dtype=r) if weight is None else np.asarray(weight, dtype=np.float64).astype(r)
    re, im = np.zeros((C, nbin, n), dtype=r), np.zeros((C, nbin, n), dtype=r)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(nb):
            cc, tt = np.nonzero(k[:, b, :] >= 0)
            kk = k[cc, b, tt]
            re[cc, kk, tt] = re[cc, kk, tt] + w[b] * z.real[cc, b, tt]
            im[cc, kk, tt] = im[cc, kk, tt] + w[b] * z.imag[cc, b, tt]
    return _join(re, im, z.dtype)


def _join(re, im, cdtype):
    out = np.empty(re.shape, dtype=cdtype)
    out.real, out.imag = re, im  # (no arithmetic: NaN and the sign of a zero stay as they are)
    return out


def synchro_restated(z, fs, edges, carrier=None, weight=None, floor=0.0):
    """(out complex128, f float64): the whole chain in float64 on the panel's values -- the mask, the carrier, the rate, the
    edges and the weights as the panel's precision holds them."""
    r = real_of(z)
    f = ifreq_restated(z, fs, carrier, floor)
    e = np.asarray(edges, dtype=np.float64).astype(r).astype(np.float64)
    w = None if weight is None else np.asarray(weight, dtype=np.float64).astype(r).astype(np.float64)
    return squeeze_restated(z.astype(np.complex128), f, e, w), f


def near_edges(f, edges, guard_hz):
    """[C, nbin, n] bool: the output elements a frequency within guard_hz of an edge could have gone to or stayed out of --
    the two bins beside that edge, in that element's column.  And the share of the panel's elements that lie so near."""
    C, nb, n = f.shape
    e = np.asarray(edges, dtype=np.float64)
    nbin = len(e) - 1
    with np.errstate(invalid="ignore"):
        j = np.clip(np.searchsorted(e, f), 0, nbin)  # the edge at or above f; the one below is j - 1
        hit_up = np.abs(e[j] - f) <= guard_hz
        hit_dn = np.abs(f - e[np.clip(j - 1, 0, nbin)]) <= guard_hz
    touched = np.zeros((C, nbin, n), dtype=bool)
    for hit, edge in ((hit_up, j), (hit_dn, np.clip(j - 1, 0, nbin))):
        cc, bb, tt = np.nonzero(hit)
        ee = edge[cc, bb, tt]
        for side in (ee - 1, ee):
            ok = (side >= 0) & (side < nbin)
            touched[cc[ok], side[ok], tt[ok]] = True
    return touched, float((hit_up | hit_dn).mean())


def bin_edges_restated(frequency_hz, per=1):
    """scales_dyadic.squeeze_bin_edges value by value: log2 f linear in the band index, the end slopes extended, the edges
    at the indices m / per - 1/2 and the centres half a bin further."""
    l = np.log2(np.asarray(frequency_hz, dtype=np.float64))
    B = len(l)

    def at(x):
        i = min(max(int(np.floor(x)), 0), B - 2)
        return np.exp2(l[i] + (x - i) * (l[i + 1] - l[i]))

    edges = np.array([at(m / per - 0.5) for m in range(B * per + 1)])
    centre = np.array([at((m + 0.5) / per - 0.5) for m in range(B * per)])
    return edges, centre


# ---- inputs of the cases ------------------------------------------------------------------------------------------------------------------
def case_edges(nbin):
    """nbin bins over the inner nine tenths of (-fs / 2, fs / 2): a random phase difference falls out of range on both sides."""
    return np.linspace(-0.45 * FS, 0.45 * FS, nbin + 1)


@functools.lru_cache(maxsize=None)
def panel(cid, dtype, whole=False):
    """The case's panel [C, nb, n] of the precision: complex normal values (whole: Gaussian integers of up to 8); read-only."""
    c = by_id(cid)
    rng = np.random.default_rng([53, c.C, c.nb, c.n, int(whole)])
    if whole:
        z = rng.integers(-8, 9, (c.C, c.nb, c.n)) + 1j * rng.integers(-8, 9, (c.C, c.nb, c.n))
    else:
        z = rng.standard_normal((c.C, c.nb, c.n)) + 1j * rng.standard_normal((c.C, c.nb, c.n))
    z = z.astype(COMPLEX[dtype])
    z.setflags(write=False)
    return z


def carrier_of(nb):
    return np.linspace(-30.0, 40.0, nb) if nb > 1 else np.array([12.5])


def weight_of(nb):
    return np.linspace(0.5, 2.0, nb) if nb > 1 else np.array([1.5])


TABLE_KINDS = ("random", "one_bin", "planted")


def given_frequencies(cid, dtype, kind):
    """A frequency table [C, nb, n] of the precision for qi_tfr_squeeze: random and not monotone in the band, past the edges
    on both sides; every element in one bin (the longest chain of additions); or random with planted values -- exactly on
    every edge in turn, NaN, both infinities, just below the first edge, exactly the last."""
    c = by_id(cid)
    r = np.dtype(dtype).type
    nbin = bins(c, dtype)
    e = case_edges(nbin).astype(r)
    rng = np.random.default_rng([59, c.C, c.nb, c.n, TABLE_KINDS.index(kind)])
    span = float(e[-1] - e[0])
    f = rng.uniform(float(e[0]) - 0.1 * span, float(e[-1]) + 0.1 * span, (c.C, c.nb, c.n)).astype(r)
    if kind == "one_bin":
        k = nbin // 2
        f[:] = r(0.5) * (e[k] + e[k + 1])
    elif kind == "planted":
        flat = f.reshape(-1)
        special = np.concatenate([e, [np.nan, np.inf, -np.inf, np.nextafter(e[0], r(-np.inf)), e[-1], np.nextafter(e[-1], r(-np.inf))]]).astype(r)
        where = rng.permutation(flat.size)[: min(flat.size, 4 * len(special))]
        flat[where] = np.resize(special, len(where))
    return f


# ---- the method on the repository's own CPU panels ----------------------------------------------------------------------------------------
METHOD_N, TONE_HZ, CHIRP_HZ = 4096, 37.3, (10.0, 120.0)
ORDERS = (3, 12)


def inner(n):
    """The inner three quarters of a record."""
    return slice(n // 8, n - n // 8)


def tone(n=METHOD_N, fs=FS):
    return np.sin(2 * np.pi * TONE_HZ * np.arange(n) / fs)


def chirp(n=METHOD_N, fs=FS):
    """A linear chirp CHIRP_HZ[0] -> CHIRP_HZ[1] over the record -> (signal, its frequency at every sample)."""
    t = np.arange(n) / fs
    f0, f1 = CHIRP_HZ
    rate = (f1 - f0) / t[-1]
    return np.sin(2 * np.pi * (f0 * t + 0.5 * rate * t * t)), f0 + rate * t


@functools.lru_cache(maxsize=None)
def cpu_panel(kind, order, signal, n=METHOD_N):
    """(frequency_hz, panel [1, B, n] complex128, carrier_hz or None) from the repository's CPU transforms."""
    from oracle import tfr_oracle as orc

    from quantum_inferno_amd import scales_dyadic as scales

    sig = tone(n) if signal == "tone" else chirp(n)[0]
    f, _, z = (orc.cwt_fft if kind == "cwt" else orc.stx_fft)(order, sig, FS)
    carrier = None if kind == "cwt" else scales.stx_shift_indices(f, n, FS) * FS / n
    return f, z[None], carrier


def bin_share(power, k, cols):
    """The share of the columns' power that lies in bin k."""
    return float(power[k, cols].sum() / power[:, cols].sum())


def ridge_error_octaves(power, centre_hz, truth_hz, cols):
    """Median over the columns of |log2(centre of the strongest bin / truth)|."""
    ridge = centre_hz[np.argmax(power[:, cols], axis=0)]
    return float(np.median(np.abs(np.log2(ridge / truth_hz[cols]))))


def share_near_truth(power, centre_hz, truth_hz, cols, octaves):
    """Mean over the columns of the share of a column's power whose bin centre lies within `octaves` of the truth."""
    p = power[:, cols]
    near = np.abs(np.log2(centre_hz[:, None] / truth_hz[cols][None, :])) <= octaves
    return float(np.mean((p * near).sum(axis=0) / p.sum(axis=0)))
