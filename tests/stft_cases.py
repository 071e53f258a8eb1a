"""Case table of the short-time Fourier family (a plain helper module: deterministic, data and reference helpers only).

Every shape of qi_stft_fused.hip's forward kernel (seven <LOG2R, LOG2C> instantiations per precision, PLAIN or not, three
loader paths), of its Welch form, of the fused inverse, and of the three-kernel hipFFT path behind the same entry points,
as (wrapper arguments, record length) rows -- used by tests/test_gpu_stft_shapes.py (GPU) and
tests/test_stft_cases_cpu.py (CPU: the oracle against SciPy on the same rows, and what the table claims to reach).

Records.  C = 3 channels, channel c = (0.5 + c) standard_normal(n) + (1 + 0.5 c) (-1)^c, seeded per case: energies
differ, DC offsets are non-zero and of both signs (a value from the wrong channel or a wrong segment mean shows).  Record
lengths are odd unless a case says otherwise, n = 3 seg + 1 by default: channels 1 of 3 then start on an odd sample (they
leave the kernel's aligned vector loads), and the panel has segments inside the record and at both ends.

References.  The oracle (oracle/tfr_oracle.py) in float64.  For float32 the record is rounded to float32 first and the
reference is the oracle on that record widened again, with its window rounded to float32 and widened, exactly as the
wrappers round the window before they sum it (`run_window`).

The last segment.  scipy.signal.stft(padded=True) appends zeros up to a whole number of hops.  At half overlap
(stft_from_sig, every default-overlap row) the last segment starts before the record ends -- the first start k hop >= n
is < n + seg / 2 -- so it is never all zeros: with n = 3 seg + 1 it holds exactly ONE record sample, under the window's
zero, and the column is -x[n - 1] / seg times the window's spectrum: the segment mean alone, 1 / seg below its
neighbours.  The per-column bound of the GPU tests therefore pins the mean (divisor seg, zero extension counted) on that
column.  An all-zero last segment needs hop > seg - seg // 2; `last_segment_all_zero` says where one exists (the
hop = seg rows).
"""
import collections
import functools

import numpy as np

from oracle import tfr_oracle as orc

FS = 1000.0
CHANNELS = 3
DTYPES = (np.float64, np.float32)


# ---- records and windows ------------------------------------------------------------------------------------------------
def record(n, seed, dtype, channels=CHANNELS):
    """[channels, n]: channel c = (0.5 + c) standard_normal + (1 + 0.5 c) (-1)^c, rounded to `dtype`."""
    rng = np.random.default_rng(seed)
    rows = [(0.5 + c) * rng.standard_normal(n) + (1.0 + 0.5 * c) * (-1.0) ** c for c in range(channels)]
    return np.stack(rows).astype(dtype)


def run_window(win64, dtype):
    """The window as a run in `dtype` uses it, in float64: float32 runs round it before summing it."""
    win64 = np.asarray(win64, dtype=np.float64)
    return win64 if np.dtype(dtype) == np.float64 else win64.astype(np.float32).astype(np.float64)


def next_pow2(m):
    return int(2 ** np.ceil(np.log2(m)))


# ---- geometry (restated from the reference's call of scipy.signal.stft, no library involved) ----------------------------
def frame_count(n, seg, hop):
    """Segments of scipy.signal.stft(boundary="zeros", padded=True): seg // 2 zeros at both ends, then zeros up to a whole
    number of hops (orc.stft_spectral's own arithmetic)."""
    length = n + 2 * (seg // 2)
    length += (-(length - seg) % hop) % seg
    return (length - seg) // hop + 1


def last_segment_all_zero(n, seg, hop):
    """The last segment starts at or past the end of the record (seg // 2 + n in the extended record)."""
    return (frame_count(n, seg, hop) - 1) * hop >= seg // 2 + n


def fused_transform(nfft, seg, dtype):
    """stft_fused_supported (qi_stft_fused.hip): a power of two 64 .. 4096 (float64: .. 2048: M = nfft / 2 = R x C with
    C <= 32) that holds the segment."""
    top = 2048 if np.dtype(dtype) == np.float64 else 4096
    return 64 <= nfft <= top and nfft & (nfft - 1) == 0 and 2 <= seg <= nfft


FUSED_LENGTHS = {np.float32: (64, 128, 256, 512, 1024, 2048, 4096), np.float64: (64, 128, 256, 512, 1024, 2048)}


# ---- 1. stft_from_sig ---------------------------------------------------------------------------------------------------
# segment length -> (band_order_nth, center_frequency_hz, octaves_below_center) at FS (orc.stft_segment_points)
SEGMENT_ARGS = collections.OrderedDict([
    (32, (1, None, 1)), (64, (1, None, 2)), (128, (1, None, 4)), (256, (1, 37.5, 4)), (512, (1, 20.0, 4)),
    (1024, (1, 10.0, 4)), (2048, (2, 10.0, 4)), (4096, (3, 10.0, 4)), (8192, (6, 10.0, 4))])
# lengths the default centre frequency reaches through the order alone (StftPlan takes no other argument): order -> seg
PLAN_ORDERS = {1: 128, 12: 2048}

FromSig = collections.namedtuple("FromSig", "seg n")


def from_sig_cases():
    out = [FromSig(seg, 3 * seg + 1) for seg in SEGMENT_ARGS]
    out += [FromSig(seg, seg) for seg in (64, 1024, 4096)]  # the shortest record accepted: no segment inside it, n even
    out.append(FromSig(2048, 4 * 2048))  # every channel aligned: the half-overlap pair loader
    return out


def from_sig_id(case):
    return f"seg{case.seg}_n{case.n}"


def from_sig_record(case, dtype):
    return record(case.n, [1, case.seg, case.n], dtype)


@functools.lru_cache(maxsize=None)
def from_sig_reference(case, dtype):
    """(f, t, z [C, seg / 2 + 1, segments]) of orc.stft_from_sig's arithmetic with the run's window."""
    x = from_sig_record(case, dtype).astype(np.float64)
    win = run_window(orc.tukey_periodic(case.seg, 1.0), dtype)
    f, t, z = orc.stft_spectral(x, FS, win, case.seg, case.seg // 2, case.seg)
    return f, t, z * (2 * np.sqrt(np.pi) / case.seg)


# ---- 2. stft_complex_pow2 / gtx_complex_pow2 ----------------------------------------------------------------------------
# fn: "stft" (Tukey 0.25) or "gtx" (Gaussian, sigma = seg // 4); overlap / nfft None: the wrappers' defaults
Spectral = collections.namedtuple("Spectral", "name fn seg overlap nfft n")

SPECTRAL_CASES = (
    Spectral("seg200", "stft", 200, None, None, 601),
    Spectral("seg201_hop101", "stft", 201, 100, None, 3001),  # odd segment, odd hop
    Spectral("seg100_hop1", "stft", 100, 99, None, 777),
    Spectral("seg96_hop96", "stft", 96, 0, None, 289),  # hop = seg: an all-zero last segment
    Spectral("seg64_nfft512", "stft", 64, None, 512, 193),  # zero padding 8 x
    Spectral("seg1000", "stft", 1000, None, None, 3001),
    Spectral("seg3000", "stft", 3000, None, None, 9001),  # nfft 4096: fused in float32, hipFFT in float64
    Spectral("seg200_nfft300", "stft", 200, None, 300, 601),  # not a power of two: hipFFT
    Spectral("seg1024_n1000", "stft", 1024, None, None, 1000),  # the record is shorter: the segment shrinks to it
    Spectral("gtx_seg201", "gtx", 201, None, None, 3001),
    Spectral("gtx_seg1000", "gtx", 1000, None, None, 3001),
)


def spectral_geometry(case):
    """(seg, overlap, nfft) as they reach the kernel: defaults from the requested segment, which then shrinks to a
    shorter record (scipy.signal.stft's _triage_segments; overlap and nfft stay)."""
    nfft = next_pow2(case.seg) if case.nfft is None else case.nfft
    overlap = int(case.seg / 2) if case.overlap is None else case.overlap
    return min(case.seg, case.n), overlap, nfft


def spectral_window(case):
    seg = spectral_geometry(case)[0]
    return orc.tukey_periodic(seg, 0.25) if case.fn == "stft" else orc.gaussian_periodic(seg, int(case.seg / 4))


def spectral_record(case, dtype):
    return record(case.n, [2, case.seg, case.n], dtype)


@functools.lru_cache(maxsize=None)
def spectral_reference(case, dtype):
    seg, overlap, nfft = spectral_geometry(case)
    x = spectral_record(case, dtype).astype(np.float64)
    return orc.stft_spectral(x, FS, run_window(spectral_window(case), dtype), seg, overlap, nfft)


# ---- 3. Welch -----------------------------------------------------------------------------------------------------------
Welch = collections.namedtuple("Welch", "name seg overlap nfft n")

WELCH_CASES = tuple(Welch(f"nfft{m}", m, None, None, 3 * m + 1) for m in (64, 128, 1024, 2048, 4096)) + (
    Welch("one_segment", 256, None, None, 256),  # one segment, one group
    Welch("41_segments", 512, None, None, 512 + 40 * 256 + 5),  # three groups of 16 per record, the last one of 9
    Welch("seg300_nfft512", 300, 225, 512, 901),
    Welch("seg8192", 8192, None, None, 3 * 8192 + 1),  # hipFFT
)


def welch_geometry(case):
    return (case.seg, int(case.seg / 2) if case.overlap is None else case.overlap,
            next_pow2(case.seg) if case.nfft is None else case.nfft)


def welch_record(case, dtype):
    return record(case.n, [3, case.seg, case.n], dtype)


def welch_with_window(x, fs, win, seg, overlap, nfft):
    """orc.welch_power_pow2 with the window handed in (bit-equal to it on its own window: test_stft_cases_cpu.py)."""
    x = np.asarray(x, dtype=np.float64)
    frames = np.lib.stride_tricks.sliding_window_view(x, seg, axis=-1)[..., 0 :: seg - overlap, :]
    frames = frames - np.mean(frames, axis=-1, keepdims=True)
    spec = orc._rfft(win * frames, n=nfft, axis=-1)
    p = (np.conjugate(spec) * spec * (1.0 / win.sum() ** 2)).real
    p[..., 1:-1 if nfft % 2 == 0 else None] *= 2
    return np.fft.rfftfreq(nfft, 1 / fs), p.mean(axis=-2)


@functools.lru_cache(maxsize=None)
def welch_reference(case, dtype):
    seg, overlap, nfft = welch_geometry(case)
    win = run_window(orc.tukey_periodic(seg, 0.25), dtype)
    return welch_with_window(welch_record(case, dtype), FS, win, seg, overlap, nfft)


# ---- 4. ShortTimeFFT convention -----------------------------------------------------------------------------------------
ALPHA = 0.25
PADDINGS = ("zeros", "edge", "even", "odd")
# overlap 3 / 4 of the segment; 24 (nfft 32, below every fused shape: 73 samples, 15 slices) takes the hipFFT path in both precisions
SLIDING_SEGS = (24, 64, 200, 512, 1000, 2048, 4096)
BOTH_SCALINGS_AT = (200, 2048)  # "magnitude" and "psd" there, "magnitude" elsewhere
# the complex output: its roll phase exp(2 pi i k (seg // 2) / nfft) is (-1)^k when seg = nfft (512, 2048: a conjugated ramp is the
# same ramp there) and a ramp with an imaginary part below it (200 in 256, 1000 in 1024; 3000 in 4096: fused in float32,
# the rotation of the framing kernel before hipFFT in float64; 24 in 32: hipFFT in both)
SLIDING_COMPLEX_SEGS = (24, 200, 512, 1000, 2048, 3000)
# (seg, hop) of the inverse.  Halo ceil(seg / hop) - 1 = 1, 3, 7, 15; launch_istft_fused holds
# G = min(16, (80 KiB / sizeof(complex) - M - 1) / tile) slices per workgroup and needs G - halo >= 1:
#   nfft   64,  512: G = 16 in both precisions                  -> every hop fused
#   nfft 2048      : G = 8 float32 (fused to halo 7), 3 float64 (fused at halo 1 only)
#   nfft 4096      : G = 3 float32 (fused at halo 1 only); float64 has no 4096-point shape -> never fused
ISTFT_SHAPES = tuple((seg, seg // d) for seg in (64, 512, 2048, 4096) for d in (2, 4, 8, 16)) + ((200, 75),)


def sliding_scalings(seg):
    return ("magnitude", "psd") if seg in BOTH_SCALINGS_AT else ("magnitude",)


def sliding_record(seg, dtype):
    return record(3 * seg + 1, [4, seg], dtype)


def sliding_object(seg, overlap, scaling, dtype=np.float64):
    """orc.SlidingStft with the window as a run in `dtype` holds it (the wrappers round the scaled window)."""
    obj = orc.SlidingStft(FS, ALPHA, seg, overlap, scaling)
    obj.win = run_window(obj.win, dtype)
    return obj


@functools.lru_cache(maxsize=None)
def sliding_reference(seg, scaling, padding, dtype):
    """(f, t, |stft_detrend| [C, f, p], |stft|^2 [C, f, p], stft [C, f, p]) at overlap 3 / 4 seg."""
    obj = sliding_object(seg, 3 * seg // 4, scaling, dtype)
    x = sliding_record(seg, dtype).astype(np.float64)
    det = np.stack([obj.stft(row, padding, detrend=True) for row in x])
    raw = np.stack([obj.stft(row, padding, detrend=False) for row in x])
    t = np.arange(start=0, stop=obj.delta_t * raw.shape[-1], step=obj.delta_t)
    return obj.f, t, np.abs(det), raw.real ** 2 + raw.imag ** 2, raw


def istft_spectrum(seg, hop, dtype):
    """A spectrum no forward transform made: [2, f_pts, p_max(n) - p_min] complex normal, channel 1 at half the scale of
    channel 0 and from its own draws; rows 0 and M keep their imaginary parts (irfft drops them)."""
    obj = orc.SlidingStft(FS, ALPHA, seg, seg - hop)
    slices = obj.p_max(3 * seg + 1) - obj.p_min
    rng = np.random.default_rng([5, seg, hop])
    s = rng.standard_normal((2, len(obj.f), slices)) + 1j * rng.standard_normal((2, len(obj.f), slices))
    s[1] *= 0.5
    return s.astype(np.complex128 if np.dtype(dtype) == np.float64 else np.complex64)


@functools.lru_cache(maxsize=None)
def istft_reference(seg, hop, dtype):
    obj = orc.SlidingStft(FS, ALPHA, seg, seg - hop)
    s = istft_spectrum(seg, hop, dtype).astype(np.complex128)
    return np.stack([obj.istft(s[c], (s.shape[-1] - 1) * hop) for c in range(2)])
