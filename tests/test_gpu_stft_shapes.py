"""The short-time Fourier family at every transform shape against the CPU oracle (-m gpu).

tests/stft_cases.py holds the rows and their references (the oracle in float64 on the same three-channel record; for
float32 on the rounded record, widened, with the window rounded as the wrappers round it).  Which branch of
qi_stft_fused.hip / qi_stft_hipfft.hip / qi_api_ops.hip each group is there for:

  test_stft_from_sig_every_segment_length
      k_stft_fused<T, R, C, PLAIN = true>, all seven <2,3> .. <5,6> (float64: six) -- nfft 64 with NP * kWave != M (half a
      wave idle in the loaders and the `j < M` guards); nfft 4096 float32 / 2048 float64 with kFast false (scalar loads
      only, no pair loader).  Odd n: channel 1's `x + base` is not 2-sample aligned -> `whole` false there and the pair
      loader falls back to one_segment, channels 0 and 2 take them.  n = 3 seg + 1: interior segments (`whole`), segments
      cut by both record ends (guarded scalar path, zeros counted in the mean) and a last segment holding ONE record sample
      under the window's zero -- the column is the segment mean alone (divisor seg, not nfft, not the samples inside).
      n = seg: no segment inside the record, `nseg` 3 < G (tiles past the last segment zero-filled, never stored).
      n = 4 * 2048: every channel aligned, pairs on every interior pair.  seg 32 / 8192 (both precisions) and 4096
      (float64): qi_stft's frames -> hipFFT R2C -> transpose path.
  test_stft_plan_matches_wrapper_and_keeps_no_state
      StftPlan's kept buffers (the same kernels through the plan's own scale / scratch).
  test_spectral_wrappers_general_kernel
      PLAIN = false store loop (`bits` null) and the guarded scalar loader with seg < nfft (`i0 < a.seg`, window and
      samples), odd seg (the last pair half empty), odd hop (alignment alternates by segment), hop 1 (778 segments: 49
      workgroups per record, the last with 10 of 16), hop = seg (the all-zero padded segment: exact zeros), 8 x zero
      padding, nfft 4096 float32 fused / float64 hipFFT, nfft 300 (not a power of two: hipFFT), _shrunk_segment.
  test_zero_segment_bits
      PLAIN = true with seg < nfft and hop = seg: the all-zero last segment's coefficients and bits.
  test_welch_every_shape
      the `welch_part` branch at <2,3>, <3,3>, <4,5>, <5,5>, <5,6> (+ <3,4>, <4,4> below), one segment in one group,
      k_welch_reduce over three partials with a last group of 9, seg < nfft with 3 / 4 overlap, qi_welch's hipFFT path
      (8192; 4096 in float64).
  test_sliding_forward_vs_oracle / test_sliding_complex_vs_oracle
      PLAIN = false with pad_mode 0 .. 3 (stft_sample), detrend on / off, real_kind 1 / 2, the roll phase ramp
      (`a.roll`: complex output compared directly, not through the inverse -- at seg = nfft the ramp is (-1)^k and a
      conjugated ramp passes, so the complex rows include seg 200 / 1000 / 3000 below nfft), at <2,3> .. <5,6>; float64 at
      4096 and seg 24 (nfft 32) in both precisions: the request through launch_hipfft_frames (every padding, detrend on /
      off, its rotation in time) -> hipFFT -> launch_hipfft_transpose (real_kind 1 / 2, the complex panel).
  test_istft_random_spectrum_vs_oracle
      k_istft_fused at halo 1, 3, 7, 15 where G - halo >= 1 and the three-kernel path (untranspose -> hipFFT C2R ->
      overlap-add) past it (stft_cases.ISTFT_SHAPES has the table), a hop that does not divide the segment, and the
      imaginary parts of X[0] and X[M], which both paths must drop as irfft does.

Bounds: TOL of test_gpu_parity.py (1e-11 / 2e-5 coefficients of the channel's panel maximum, bits by check_bits), and the
same number for every time column against that column's own maximum -- the interior columns of these records sit up to
30 x below the edge columns, the last one (the mean alone) up to 4e4 x, and the panel bound alone lets them be wrong.
The float32 pipeline itself (scipy.fft.rfft in float32 on the same frames) is within 2.0e-6 per column and 2.2e-7 of the
panel at seg 64 .. 4096, so 2e-5 leaves 10 x.
"""
import numpy as np
import pytest
import torch

import stft_cases as sc
from oracle import tfr_oracle as orc
from test_gpu_parity import TOL, check_bits

from quantum_inferno_amd import _lib, styx_fft
from quantum_inferno_amd.utilities import short_time_fft as stf

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
COMPLEX = {np.float64: np.complex128, np.float32: np.complex64}


def check_panels(z, ref, tol, what):
    """Per channel: every coefficient within tol of the panel maximum AND within tol of its time column's maximum; a
    column the reference has exactly zero is exactly zero."""
    assert z.shape == ref.shape, (what, z.shape, ref.shape)
    for c in range(ref.shape[0]):
        err = np.abs(z[c] - ref[c])
        assert err.max() <= tol * np.abs(ref[c]).max(), (what, c, err.max() / np.abs(ref[c]).max())
        col = np.abs(ref[c]).max(axis=0)
        live = col > 0
        worst = np.max(err.max(axis=0)[live] / col[live])
        assert worst <= tol, (what, c, int(np.argmax(err.max(axis=0)[live] / col[live])), worst)
        assert np.all(z[c][:, ~live] == 0), (what, c)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", sc.from_sig_cases(), ids=sc.from_sig_id)
def test_stft_from_sig_every_segment_length(case, dtype):
    tol = TOL[dtype]
    order, center, octaves = sc.SEGMENT_ARGS[case.seg]
    x = sc.from_sig_record(case, dtype)
    z, bits, t, f = styx_fft.stft_from_sig(x, sc.FS, order, center, octaves)
    ref_f, ref_t, ref = sc.from_sig_reference(case, dtype)
    assert z.shape == ref.shape == (sc.CHANNELS, case.seg // 2 + 1, sc.frame_count(case.n, case.seg, case.seg // 2))
    assert np.array_equal(t, ref_t) and np.array_equal(f, ref_f)
    assert z.dtype == COMPLEX[dtype] and bits.shape == z.shape
    check_panels(z, ref, tol["coef"], sc.from_sig_id(case))
    for c in range(sc.CHANNELS):
        check_bits(bits[c], ref[c], tol)
    # (no all-zero column exists at half overlap -- stft_cases' docstring; test_zero_segment_bits has one)
    assert np.all(np.abs(ref).max(axis=1) > 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("order", sorted(sc.PLAN_ORDERS))
def test_stft_plan_matches_wrapper_and_keeps_no_state(order, dtype):
    """StftPlan.run is bit-equal to stft_from_sig on the same tensor, and again after a run on another record."""
    seg = sc.PLAN_ORDERS[order]
    case = sc.FromSig(seg, 3 * seg + 1)
    x = torch.from_numpy(sc.from_sig_record(case, dtype)).cuda()
    other = torch.from_numpy(sc.record(case.n, [6, seg], dtype)).cuda()
    plan = styx_fft.StftPlan(case.n, sc.CHANNELS, sc.FS, order, x.dtype)
    assert plan.seg == seg
    want_z, want_bits, t, f = styx_fft.stft_from_sig(x, sc.FS, order)
    assert np.array_equal(plan.time_s, t) and np.array_equal(plan.frequency_hz, f)
    z, bits = plan.run(x)
    assert torch.equal(z, want_z) and torch.equal(bits, want_bits)
    z2, _ = plan.run(other)
    assert not torch.equal(z2, want_z)
    z, bits = plan.run(x)
    assert torch.equal(z, want_z) and torch.equal(bits, want_bits)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", sc.SPECTRAL_CASES, ids=lambda case: case.name)
def test_spectral_wrappers_general_kernel(case, dtype):
    x = sc.spectral_record(case, dtype)
    fn = styx_fft.stft_complex_pow2 if case.fn == "stft" else styx_fft.gtx_complex_pow2
    kw = dict(overlap_points=case.overlap, nfft_points=case.nfft)
    if case.seg > case.n:
        with pytest.warns(UserWarning, match="using nperseg"):
            f, t, z = fn(x, sc.FS, case.seg, **kw)
    else:
        f, t, z = fn(x, sc.FS, case.seg, **kw)
    ref_f, ref_t, ref = sc.spectral_reference(case, dtype)
    assert np.array_equal(t, ref_t) and np.array_equal(f, ref_f)
    assert z.dtype == COMPLEX[dtype]
    check_panels(z, ref, TOL[dtype]["coef"], case.name)
    seg, overlap, _ = sc.spectral_geometry(case)
    if sc.last_segment_all_zero(case.n, seg, seg - overlap):
        assert np.all(z[:, :, -1] == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_segment_bits(dtype):
    """The all-zero segment that padded=True appends, through the kernel that also writes bits (qi_stft with both panels:
    PLAIN): coefficients exactly zero, bits log2(eps).  stft_from_sig cannot reach one (half overlap), so the call is the
    wrappers' common one at hop = seg."""
    tol = TOL[dtype]
    case = next(c for c in sc.SPECTRAL_CASES if c.name == "seg96_hop96")
    seg, overlap, nfft = sc.spectral_geometry(case)
    assert sc.last_segment_all_zero(case.n, seg, seg - overlap)
    x = sc.spectral_record(case, dtype)
    f, t, z, bits = styx_fft._stft_windowed(x, sc.FS, sc.spectral_window(case), seg, overlap, nfft, want_bits=True)
    ref = sc.spectral_reference(case, dtype)[2]
    check_panels(z, ref, tol["coef"], case.name)
    assert np.all(z[:, :, -1] == 0) and np.all(ref[:, :, -1] == 0)
    assert np.all(np.abs(bits[:, :, -1] - np.log2(orc.EPS64)) <= tol["bits"])
    for c in range(sc.CHANNELS):
        check_bits(bits[c], ref[c], tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", sc.WELCH_CASES, ids=lambda case: case.name)
def test_welch_every_shape(case, dtype):
    tol = 1e-11 if dtype == np.float64 else 2e-5
    seg, overlap, nfft = sc.welch_geometry(case)
    f, p = styx_fft.welch_power_pow2(sc.welch_record(case, dtype), sc.FS, case.seg, case.nfft, case.overlap)
    ref_f, ref = sc.welch_reference(case, dtype)
    assert np.array_equal(f, ref_f) and p.dtype == dtype and p.shape == ref.shape == (sc.CHANNELS, nfft // 2 + 1)
    for c in range(sc.CHANNELS):
        err = np.max(np.abs(p[c] - ref[c])) / np.max(ref[c])
        assert err <= tol, (case.name, c, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("seg", sc.SLIDING_SEGS)
def test_sliding_forward_vs_oracle(seg, dtype):
    """stft_tukey (detrended magnitude) and spectrogram_tukey, every padding mode, channel by channel."""
    tol = 1e-11 if dtype == np.float64 else 2e-5
    x = sc.sliding_record(seg, dtype)
    for scaling in sc.sliding_scalings(seg):
        for padding in sc.PADDINGS:
            ref_f, ref_t, ref_mag, ref_sxx, _ = sc.sliding_reference(seg, scaling, padding, dtype)
            f, t, mag = stf.stft_tukey(x, sc.FS, sc.ALPHA, seg, 3 * seg // 4, scaling, padding)
            assert np.array_equal(f, ref_f) and np.array_equal(t, ref_t)
            assert mag.dtype == dtype and mag.shape == ref_mag.shape
            _, _, sxx = stf.spectrogram_tukey(x, sc.FS, sc.ALPHA, seg, 3 * seg // 4, scaling, padding)
            for c in range(sc.CHANNELS):
                err = np.max(np.abs(mag[c] - ref_mag[c])) / np.max(ref_mag[c])
                assert err <= tol, (seg, scaling, padding, c, err)
                err = np.max(np.abs(sxx[c] - ref_sxx[c])) / np.max(ref_sxx[c])
                assert err <= 2 * tol, (seg, scaling, padding, c, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("seg", sc.SLIDING_COMPLEX_SEGS)
def test_sliding_complex_vs_oracle(seg, dtype):
    """qi_sliding_stft's complex output (it carries the roll phase ramp) against ShortTimeFFT.stft restated, directly:
    a consistent phase or scale error would cancel in a forward -> inverse round trip."""
    lib = _lib.require_gpu()
    obj = stf.get_stft_object_tukey(sc.FS, sc.ALPHA, seg, 3 * seg // 4, "magnitude")
    x = torch.from_numpy(sc.sliding_record(seg, dtype)).cuda()
    n_ch, n = x.shape
    p0, p1 = obj.p_min, obj.p_max(n)
    n_slices, first = p1 - p0, p0 * obj.hop - obj.m_num_mid
    code = _lib.QI_F32 if dtype == np.float32 else _lib.QI_F64
    win = torch.from_numpy(obj.win).to(device="cuda", dtype=x.dtype)
    z = torch.empty((n_ch, obj.f_pts, n_slices), dtype=torch.complex64 if dtype == np.float32 else torch.complex128, device="cuda")
    nbytes = int(lib.qi_sliding_scratch_bytes(code, n_ch, obj.mfft, n_slices))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.qi_sliding_stft(code, 0, _lib.ptr(x), n_ch, n, _lib.ptr(win), obj.m_num, obj.hop, obj.mfft, first, n_slices, 0, 0,
                                   obj.m_num_mid, _lib.ptr(z), None, 1, _lib.ptr(scratch), nbytes, _lib.stream_ptr(x.device)))
    ref = sc.sliding_reference(seg, "magnitude", "zeros", dtype)[4]
    check_panels(z.cpu().numpy(), ref, TOL[dtype]["coef"], f"sliding seg {seg}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("seg,hop", sc.ISTFT_SHAPES)
def test_istft_random_spectrum_vs_oracle(seg, hop, dtype):
    tol = 1e-11 if dtype == np.float64 else 2e-5
    s = sc.istft_spectrum(seg, hop, dtype)
    assert np.all(s[:, 0].imag != 0) and np.all(s[:, -1].imag != 0)
    ts, x = stf.istft_tukey(s, sc.FS, sc.ALPHA, seg, seg - hop, "magnitude")
    ref = sc.istft_reference(seg, hop, dtype)
    last = (s.shape[-1] - 1) * hop
    assert x.shape == ref.shape == (2, last) and np.array_equal(ts, np.arange(start=0, stop=last / sc.FS, step=1 / sc.FS))
    for c in range(2):
        err = np.max(np.abs(x[c] - ref[c])) / np.max(np.abs(ref[c]))
        assert err <= 10 * tol, (seg, hop, c, err)
