"""Cases and references of the streamed STFT (qi_stft_out_range, styx_fft.StftRangePlan, stream.StftStream / StftRecord; a
plain helper module beside stft_cases.py and stft_reduced_cases.py).  Used by tests/test_gpu_stft_stream.py (GPU) and
tests/test_stft_stream_cpu.py (CPU).

An STFT segment depends on its own samples only, so every reference is the float64 oracle panel of the WHOLE record
(stft_cases' records and orc.stft_spectral): an item's coefficients are the matching columns of that panel, the assembled
reductions are stft_reduced_cases.reduce_reference of it (bounds: check_reduced, RED_TOL), and the pooled spectrogram is
P = power_scale |Z|^2 of it reshaped into windows of F segments, `mean` / `max` in float64 (the ragged tail dropped), held
to RED_TOL of the channel's largest value.
"""
import collections

import numpy as np

import stft_cases as sc
import stft_reduced_cases as rc

# name, FromSig (stft_from_sig's geometry through an explicit Hann window) or the name of a SPECTRAL_CASES row, segments per item
Shape = collections.namedtuple("Shape", "name case per_item")

RECORD = sc.FromSig(512, 10757)  # 44 segments: items of 16, 16, 12; launch groups of 16
SHAPES = (
    Shape("seg512_n10757", RECORD, 16),
    Shape("seg201_hop101", rc.spectral_case("seg201_hop101"), 15),  # 31 segments in 15, 15, 1: odd sample0s leave the aligned loaders
    Shape("seg200_nfft300", rc.spectral_case("seg200_nfft300"), 3),  # hipFFT: 8 segments, items of 3, 3, 2
)
LONG = sc.FromSig(4096, 23 * 2048 - 1000)  # 24 segments of 4096: launch group 2 in float32, hipFFT in float64

# (n_total, seg, hop, segments_per_item) of segment_items
ITEM_CASES = ((10757, 512, 256, 16), (2561, 64, 64, 7), (5000, 201, 101, 5), (600, 512, 500, 1), (385, 128, 64, 100))

# pooling factors: 512-point transforms (launch group 16: G' = 4, 16, 16, 4) and 4096-point ones (G' = 2, 2, 1)
POOL_512 = (4, 16, 32, 12)
POOL_4096 = (2, 8, 3)


def geometry(shape):
    """(seg, hop, nfft) as they reach the kernel"""
    if isinstance(shape.case, sc.FromSig):
        return shape.case.seg, shape.case.seg // 2, shape.case.seg
    seg, overlap, nfft = sc.spectral_geometry(shape.case)
    return seg, seg - overlap, nfft


def record(shape, dtype):
    return sc.from_sig_record(shape.case, dtype) if isinstance(shape.case, sc.FromSig) else sc.spectral_record(shape.case, dtype)


def reference(shape, dtype):
    """The float64 oracle panel [C, f, t] of the whole record (cached by stft_cases)"""
    return (sc.from_sig_reference if isinstance(shape.case, sc.FromSig) else sc.spectral_reference)(shape.case, dtype)[2]


def plan_arguments(shape):
    """Keyword arguments of styx_fft.StftRangePlan(n_total, FS, **kw) for the shape: the window and scale of the wrappers"""
    from quantum_inferno_amd import styx_fft

    seg, hop, nfft = geometry(shape)
    if isinstance(shape.case, sc.FromSig):
        return dict(window=styx_fft.tukey_window_periodic(seg, 1.0), overlap_points=seg - hop, nfft_points=nfft,
                    extra_scale=2 * np.sqrt(np.pi) / seg)
    return dict(window=sc.spectral_window(shape.case), overlap_points=seg - hop, nfft_points=nfft)


def brute_interval(n_total, seg, hop, first, count):
    """(lo, hi) of the record samples inside [0, n_total) that the segments first .. first + count - 1 cover, by listing
    them; (None, None) when there are none"""
    covered = set()
    for m in range(first, first + count):
        a = m * hop - seg // 2
        covered.update(range(max(0, a), min(n_total, a + seg)))
    return (min(covered), max(covered) + 1) if covered else (None, None)


def pooled_reference(z_ref, factor, power_scale=1.0):
    """(mean, max) [C, f, windows] of P = power_scale |z_ref|^2 over windows of `factor` columns, float64"""
    p = power_scale * (z_ref.real ** 2 + z_ref.imag ** 2)
    windows = p.shape[-1] // factor
    w = p[..., : windows * factor].reshape(p.shape[:-1] + (windows, factor))
    return w.mean(-1), w.max(-1)


def check_pooled(got, ref, dtype, what):
    """A pooled array [C, f, windows] against its float64 reference: per channel, max |error| / max |reference| <= RED_TOL"""
    assert got.shape == ref.shape and got.dtype == dtype, (what, got.shape, ref.shape, got.dtype)
    for c in range(ref.shape[0]):
        err = np.max(np.abs(got[c].astype(np.float64) - ref[c])) / ref[c].max()
        assert err <= rc.RED_TOL[dtype], (what, c, err)


class FakeResult:
    """What an assembler reads of an item's TfrResult"""

    def __init__(self, power_band, stats, power_time=None, pooled=None):
        self.power_band, self.stats, self.power_time, self.pooled = power_band, stats, power_time, pooled
        self.frequency_hz, self.power_scale = np.arange(power_band.shape[1], dtype=np.float64), 1.0
