"""CPU checks on the short-time case table (tests/stft_cases.py): (a) its references against SciPy itself, (b) the bits
floors of the GPU tests keep most of every panel, (c) the table reaches the kernel shapes it claims to -- from the case
geometry, no device."""
import warnings

import numpy as np
import pytest

import stft_cases as sc
from conftest import relmax
from oracle import tfr_oracle as orc
from test_gpu_parity import TOL

from quantum_inferno_amd import _lib, styx_fft


# ---- (a) the oracle against SciPy ---------------------------------------------------------------------------------------
def test_from_sig_references_match_scipy():
    ss = pytest.importorskip("scipy.signal")
    for case in sc.from_sig_cases():
        for dtype in sc.DTYPES:
            x = sc.from_sig_record(case, dtype).astype(np.float64)
            win = sc.run_window(orc.tukey_periodic(case.seg, 1.0), dtype)
            f, t, z = ss.stft(x, sc.FS, window=win, nperseg=case.seg, noverlap=case.seg // 2, nfft=case.seg, detrend="constant",
                              return_onesided=True, boundary="zeros", padded=True)
            ref_f, ref_t, ref = sc.from_sig_reference(case, dtype)
            assert np.array_equal(f, ref_f) and np.allclose(t, ref_t, rtol=0, atol=1e-12)
            assert relmax(z * (2 * np.sqrt(np.pi) / case.seg), ref) <= 1e-12, sc.from_sig_id(case)
            if dtype == np.float64:  # the helper is orc.stft_from_sig with the window handed in
                for c in range(sc.CHANNELS):
                    assert np.array_equal(orc.stft_from_sig(x[c], sc.FS, *sc.SEGMENT_ARGS[case.seg])[0], ref[c])


def test_spectral_references_match_scipy():
    ss = pytest.importorskip("scipy.signal")
    for case in sc.SPECTRAL_CASES:
        seg, overlap, nfft = sc.spectral_geometry(case)
        for dtype in sc.DTYPES:
            x = sc.spectral_record(case, dtype).astype(np.float64)
            win = sc.run_window(sc.spectral_window(case), dtype)
            f, t, z = ss.stft(x, sc.FS, window=win, nperseg=seg, noverlap=overlap, nfft=nfft, detrend="constant",
                              return_onesided=True, boundary="zeros", padded=True)
            ref_f, ref_t, ref = sc.spectral_reference(case, dtype)
            assert np.array_equal(f, ref_f) and np.allclose(t, ref_t, rtol=0, atol=1e-12)
            assert z.shape == ref.shape and relmax(z, ref) <= 1e-12, case.name
        # the requested arguments as the reference hands them to SciPy (window by name, a segment longer than the record)
        x = sc.spectral_record(case, np.float64)
        window = ("tukey", 0.25) if case.fn == "stft" else ("gaussian", int(case.seg / 4))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, _, z = ss.stft(x, sc.FS, window=window, nperseg=case.seg, noverlap=overlap, nfft=nfft, detrend="constant",
                              return_onesided=True, boundary="zeros", padded=True)
        assert relmax(z, sc.spectral_reference(case, np.float64)[2]) <= 1e-12, case.name


def test_welch_references_match_scipy():
    ss = pytest.importorskip("scipy.signal")
    for case in sc.WELCH_CASES:
        seg, overlap, nfft = sc.welch_geometry(case)
        for dtype in sc.DTYPES:
            x = sc.welch_record(case, dtype).astype(np.float64)
            win = sc.run_window(orc.tukey_periodic(seg, 0.25), dtype)
            f, p = ss.welch(x, sc.FS, window=win, nperseg=seg, noverlap=overlap, nfft=nfft, detrend="constant",
                            return_onesided=True, scaling="spectrum", average="mean")
            ref_f, ref = sc.welch_reference(case, dtype)
            assert np.array_equal(f, ref_f) and relmax(p, ref) <= 1e-12, case.name
        x = sc.welch_record(case, np.float64)
        f, p = orc.welch_power_pow2(x, sc.FS, seg, nfft, overlap)
        assert np.array_equal(p, sc.welch_reference(case, np.float64)[1])


def test_sliding_references_match_scipy():
    """The ShortTimeFFT-convention rows: orc.SlidingStft against scipy.signal.ShortTimeFFT (forward with every padding,
    detrended or not, and the inverse of a spectrum no forward transform made)."""
    ss = pytest.importorskip("scipy.signal")
    for seg in sc.SLIDING_SEGS:
        x = sc.sliding_record(seg, np.float64)
        for scaling in sc.sliding_scalings(seg):
            obj = sc.sliding_object(seg, 3 * seg // 4, scaling)
            ref = ss.ShortTimeFFT(win=ss.windows.tukey(seg, alpha=sc.ALPHA), hop=seg // 4, fs=sc.FS, mfft=obj.mfft,
                                  fft_mode="onesided", scale_to=scaling)
            for padding in sc.PADDINGS:
                _, _, mag, sxx, raw = sc.sliding_reference(seg, scaling, padding, np.float64)
                assert relmax(raw, ref.stft(x, padding=padding)) <= 1e-12
                assert relmax(mag, np.abs(ref.stft_detrend(x, "constant", padding=padding))) <= 1e-12
                assert relmax(sxx, ref.spectrogram(x, padding=padding)) <= 1e-12
    for seg in sc.SLIDING_COMPLEX_SEGS:
        ref = ss.ShortTimeFFT(win=ss.windows.tukey(seg, alpha=sc.ALPHA), hop=seg // 4, fs=sc.FS, mfft=sc.next_pow2(seg),
                              fft_mode="onesided", scale_to="magnitude")
        raw = sc.sliding_reference(seg, "magnitude", "zeros", np.float64)[4]
        assert relmax(raw, ref.stft(sc.sliding_record(seg, np.float64))) <= 1e-12
        roll = np.exp(2j * np.pi * (seg // 2) / sc.next_pow2(seg))  # the phase step per bin: real only when seg = nfft
        assert (abs(roll.imag) > 1e-2) == (seg != sc.next_pow2(seg))
    for seg, hop in sc.ISTFT_SHAPES:
        ref = ss.ShortTimeFFT(win=ss.windows.tukey(seg, alpha=sc.ALPHA), hop=hop, fs=sc.FS, mfft=sc.next_pow2(seg),
                              fft_mode="onesided", scale_to="magnitude")
        s = sc.istft_spectrum(seg, hop, np.float64)
        assert s.shape[1:] == (ref.f_pts, ref.p_max(3 * seg + 1) - ref.p_min)
        assert np.all(s[:, 0].imag != 0) and np.all(s[:, -1].imag != 0) and not np.array_equal(2 * s[1], s[0])
        want = ref.istft(s, k0=0, k1=(s.shape[-1] - 1) * hop, f_axis=-2, t_axis=-1)
        assert relmax(sc.istft_reference(seg, hop, np.float64), want) <= 1e-12, (seg, hop)


# ---- (b) the bits floors keep most of every panel -----------------------------------------------------------------------
def test_bits_floors_keep_most_coefficients():
    """check_bits compares above a magnitude floor: per channel of every stft_from_sig row the strict floor keeps >= 40 %
    of the coefficients and the wide one (1e-6 float64, 1e-3 float32 of the maximum) >= 85 % (measured: 0.476 at seg 8192
    channel 0, 0.873; what the wide floor drops is the last column, the mean alone: two bins of a Hann spectrum)."""
    wide = {np.float64: TOL[np.float64]["bits_wide"][1], np.float32: 1e-3}
    assert wide[np.float64] == 1e-6
    for case in sc.from_sig_cases():
        for dtype in sc.DTYPES:
            ref = sc.from_sig_reference(case, dtype)[2]
            for c in range(sc.CHANNELS):
                mag = np.abs(ref[c])
                assert np.mean(mag >= TOL[dtype]["bits_floor"] * mag.max()) >= 0.40, (sc.from_sig_id(case), dtype, c)
                assert np.mean(mag >= wide[dtype] * mag.max()) >= 0.85, (sc.from_sig_id(case), dtype, c)


# ---- (c) the table reaches what it claims -------------------------------------------------------------------------------
def _forward_rows():
    """(group, n, seg, hop, nfft) of every forward row, as the kernel sees it."""
    rows = [("from_sig", c.n, c.seg, c.seg // 2, c.seg) for c in sc.from_sig_cases()]
    for c in sc.SPECTRAL_CASES:
        seg, overlap, nfft = sc.spectral_geometry(c)
        rows.append(("spectral", c.n, seg, seg - overlap, nfft))
    for c in sc.WELCH_CASES:
        seg, overlap, nfft = sc.welch_geometry(c)
        rows.append(("welch", c.n, seg, seg - overlap, nfft))
    rows += [("sliding", 3 * seg + 1, seg, seg // 4, sc.next_pow2(seg)) for seg in sc.SLIDING_SEGS]
    return rows


def test_table_reaches_every_transform_shape():
    rows = _forward_rows()
    for seg, args in sc.SEGMENT_ARGS.items():
        assert orc.stft_segment_points(sc.FS, *args) == seg
    for order, seg in sc.PLAN_ORDERS.items():
        assert orc.stft_segment_points(sc.FS, order) == seg and seg in sc.SEGMENT_ARGS
    for dtype in sc.DTYPES:
        for group in ("from_sig", "welch", "sliding"):  # PLAIN, the Welch sums, the general store loop
            fused = {nfft for g, n, seg, hop, nfft in rows if g == group and sc.fused_transform(nfft, seg, dtype)}
            want = set(sc.FUSED_LENGTHS[dtype])
            if group == "sliding":  # 200 -> 256, 1000 -> 1024 beside the powers of two; 128 is not asked of this group, 24 -> 32 is hipFFT's
                want -= {128}
            assert fused == want, (group, dtype, sorted(fused))
        for group in ("from_sig", "welch"):
            unfused = {nfft for g, n, seg, hop, nfft in rows if g == group and not sc.fused_transform(nfft, seg, dtype)}
            assert any(nfft > 4096 for nfft in unfused), (group, dtype)
        unfused = {nfft for g, n, seg, hop, nfft in rows if not sc.fused_transform(nfft, seg, dtype)}
        assert any(nfft < 64 for nfft in unfused) and any(nfft > 4096 for nfft in unfused)
        assert any(nfft & (nfft - 1) for nfft in unfused)
        assert (4096 in unfused) == (dtype == np.float64)
        assert ("sliding", 73, 24, 6, 32) in rows and not sc.fused_transform(32, 24, dtype)  # every padding on hipFFT in float32 too
    assert len(sc.FUSED_LENGTHS[np.float32]) == 7 and len(sc.FUSED_LENGTHS[np.float64]) == 6
    styx = [r for r in rows if r[0] in ("from_sig", "spectral")]
    assert any(n % 2 for g, n, seg, hop, nfft in styx) and any(n == seg for g, n, seg, hop, nfft in styx)
    assert any(n % 2 == 0 and n > seg for g, n, seg, hop, nfft in styx if g == "from_sig")
    assert any(sc.last_segment_all_zero(n, seg, hop) for g, n, seg, hop, nfft in styx)
    # at half overlap the last segment always holds a record sample; with n = 3 seg + 1 exactly one
    for g, n, seg, hop, nfft in styx:
        if g == "from_sig":
            assert not sc.last_segment_all_zero(n, seg, hop)
            if n == 3 * seg + 1:
                assert (sc.frame_count(n, seg, hop) - 1) * hop == seg // 2 + n - 1
    # the frame count of every styx row is the oracle's
    for case in sc.from_sig_cases():
        assert sc.from_sig_reference(case, np.float64)[2].shape[-1] == sc.frame_count(case.n, case.seg, case.seg // 2)
    for case in sc.SPECTRAL_CASES:
        seg, overlap, _ = sc.spectral_geometry(case)
        assert sc.spectral_reference(case, np.float64)[2].shape[-1] == sc.frame_count(case.n, seg, seg - overlap)
        if sc.last_segment_all_zero(case.n, seg, seg - overlap):
            assert np.all(sc.spectral_reference(case, np.float64)[2][..., -1] == 0)
    # Welch: one segment; >= 40 segments in >= 3 groups of 16 with a last group that is not full
    counts = [(n - seg) // hop + 1 for g, n, seg, hop, nfft in rows if g == "welch"]
    assert 1 in counts and any(c >= 40 and c > 32 and c % 16 for c in counts)
    # hop 1: a segment count that is no multiple of the workgroup's 16 segments
    assert any(hop == 1 and sc.frame_count(n, seg, hop) % 16 for g, n, seg, hop, nfft in styx)


def test_istft_shapes_straddle_the_fused_limit():
    """launch_istft_fused: G = min(16, (80 KiB / sizeof(complex) - (M + 1)) / tile) slices, tile = R (C + 1) + 1, fused
    while G - halo >= 1.  Both sides of that point are in the table, per precision."""
    for dtype, esz in ((np.float32, 8), (np.float64, 16)):
        sides = set()
        for seg, hop in sc.ISTFT_SHAPES:
            nfft = sc.next_pow2(seg)
            lm = int(np.log2(nfft // 2))
            lr, lc = lm // 2, lm - lm // 2
            tile = (1 << lr) * ((1 << lc) + 1) + 1
            g = min(16, (80 * 1024 // esz - (nfft // 2 + 1)) // tile)
            halo = -(-seg // hop) - 1
            sides.add((nfft, sc.fused_transform(nfft, seg, dtype) and g - halo >= 1))
        assert {(2048, True), (2048, False), (4096, False), (64, True), (512, True), (256, True)} <= sides, sides
        assert ((4096, True) in sides) == (dtype == np.float32)
    assert sorted({-(-seg // hop) - 1 for seg, hop in sc.ISTFT_SHAPES}) == [1, 2, 3, 7, 15]


def test_segment_count_of_the_library_matches_the_oracle():
    """qi_stft_segments (a pure-host entry point) and styx_fft._frame_count (what StftGeometry counts with) over n 1 .. 300 x
    seg {2, 3, 7, 8, 64, 201} x every hop <= seg against the frame count of scipy.signal.stft's geometry as the oracle
    restates it -- the restatement itself against the oracle's own output on every 17th combination."""
    lib = _lib.load()
    k = 0
    for seg in (2, 3, 7, 8, 64, 201):
        for hop in range(1, seg + 1):
            for n in range(1, 301):
                want = sc.frame_count(n, seg, hop)
                assert lib.qi_stft_segments(n, seg, hop) == want, (n, seg, hop)
                assert styx_fft._frame_count(n, seg, hop) == want, (n, seg, hop)
                k += 1
                if k % 17 == 0:
                    assert orc.stft_spectral(np.zeros(n), 1.0, np.ones(seg), seg, seg - hop, seg)[2].shape[-1] == want


def _assert_geometry(g, dtype, ref_f, ref_t, win64, seg, hop, nfft, n_seg, extra, what):
    run = sc.run_window(win64, dtype)
    assert (g.seg, g.hop, g.nfft, g.n_seg, g.n_f) == (seg, hop, nfft, n_seg, nfft // 2 + 1), what
    assert np.array_equal(g.time_s, ref_t) and np.array_equal(g.frequency_hz, ref_f), what
    assert g.window.dtype == dtype and np.array_equal(g.window.astype(np.float64), run), what
    assert g.scale == float(np.sqrt(1.0 / run.sum() ** 2)) * extra, what


def test_geometry_object_matches_the_oracle():
    """styx_fft.StftGeometry (host arithmetic: the one place the wrappers and plans take their numbers from) against
    orc.stft_spectral on every FromSig and Spectral row in both precisions: segment, hop, transform length, segment count,
    both axes and the rounded window are equal; the scale is, as floats, the oracle's sqrt(1 / win.sum() ** 2) times the
    wrapper's factor."""
    for dtype in sc.DTYPES:
        for case in sc.from_sig_cases():
            ref_f, ref_t, ref = sc.from_sig_reference(case, dtype)
            g = styx_fft.StftGeometry.from_order(case.n, sc.FS, *sc.SEGMENT_ARGS[case.seg], rdtype=dtype)
            _assert_geometry(g, dtype, ref_f, ref_t, orc.tukey_periodic(case.seg, 1.0), case.seg, case.seg // 2, case.seg, ref.shape[-1],
                             2 * np.sqrt(np.pi) / case.seg, sc.from_sig_id(case))
        for case in sc.SPECTRAL_CASES:
            seg, overlap, nfft = sc.spectral_geometry(case)
            ref_f, ref_t, ref = sc.spectral_reference(case, dtype)
            g = styx_fft.StftGeometry.from_window(case.n, sc.FS, sc.spectral_window(case), overlap, nfft, rdtype=dtype)
            _assert_geometry(g, dtype, ref_f, ref_t, sc.spectral_window(case), seg, seg - overlap, nfft, ref.shape[-1], 1.0, case.name)
