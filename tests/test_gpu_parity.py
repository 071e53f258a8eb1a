"""GPU parity tests (-m gpu): the HIP path, called through the C ABI by the reference-signature
wrappers, against (1) golden vectors captured from the reference itself, (2) the CPU oracle on the
same seeded inputs, (3) size-independent properties at the benchmark size.

Stated tolerances (max|delta| relative to max|reference| of the panel unless noted):
  float64 path : 1e-11 coefficients, 1e-9 log2 bits, 1e-10 reductions.  A bits tolerance needs a magnitude
                 floor -- log2 of a coefficient far below the panel maximum amplifies ANY absolute error, the reference's
                 own FFT rounding (~2e-15 max) and the 1.8e-12 amplitude rounding of its cwt_atoms path
                 included.  1e-9 bits are asserted from the floor the coefficient contract itself implies,
                 |z| >= 1e-11 / (1e-9 ln 2) = 1.5e-2 max (BITS_FLOOR64); beside it round 4's wider check stays: 1e-8 bits
                 from 1e-6 max on the hipFFT engine (the reference's algorithm) and from 1e-3 max on the native engines
  float32 path : 2e-5 coefficients, 1e-3 log2 bits where |z| >= 1e-3 max, 1e-4 reductions; at the benchmark
                 length every band is also held to 1e-5 of ITS OWN maximum (weak bands included)
Band tables, shift indices, STFT shapes / time / frequency axes: bit-exact.
"""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, relmax
from oracle import tfr_oracle as orc

import quantum_inferno_amd as qi
from quantum_inferno_amd import cwt_atoms, engine, scales_dyadic, styx_cwt, styx_fft, styx_stx, tfr_info

pytestmark = pytest.mark.gpu

TOL = {np.float64: dict(coef=1e-11, bits=1e-9, bits_floor=1.5e-2, bits_wide=(1e-8, 1e-6), red=1e-10),
       np.float32: dict(coef=2e-5, bits=1e-3, bits_floor=1e-3, red=1e-4, row=1e-5)}
BITS_FLOOR64 = 1.5e-2  # coef / (bits ln 2): where the 1e-11 coefficient contract implies 1e-9 bits
# (measured at 2^20 samples against the reference, tools/measure_parity.py: panel-relative error < 1e-6, every band
# within 2.4e-6 of its own maximum at orders 3 and 12, bits within 3e-4 above 1e-3 of the panel maximum)


# The medium / large fixtures were captured from a float32 record: SciPy then evaluates the signal's
# FFT in single precision inside the reference (complex64 spectrum times complex128 atoms), so the
# reference output itself carries ~1e-7 of rounding.  The float64 path is compared at that level.
TOL_F32_RECORD = {np.float64: dict(coef=5e-7, bits=1e-5, bits_floor=1e-3, red=1e-6), np.float32: TOL[np.float32]}


def check_bits(bits, ref_coef, tol):
    mag = np.abs(ref_coef)
    sel = mag >= tol["bits_floor"] * mag.max()
    ref_bits = np.log2(mag + orc.EPS64)
    assert np.max(np.abs(bits - ref_bits)[sel]) <= tol["bits"]
    if "bits_wide" in tol:  # a second, looser tolerance over a wider range of magnitudes
        wide_tol, wide_floor = tol["bits_wide"]
        assert np.max(np.abs(bits - ref_bits)[mag >= wide_floor * mag.max()]) <= wide_tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("key,order,fs", [("o3_fs1000", 3, 1000.0), ("o12_fs800", 12, 800.0)])
def test_small_panels_vs_reference(golden, key, order, fs, dtype):
    g = golden("small_n1024.npz")
    tol = TOL[dtype]
    sig = g[f"sig_{key}"].astype(dtype)
    f, t, cwt = styx_cwt.cwt_complex_any_scale_pow2(order, sig, fs)
    assert np.array_equal(f, g[f"f_{key}"]) and np.array_equal(t, g[f"t_{key}"])
    assert cwt.dtype == np.complex128  # as the reference returns it, whatever the record's dtype (styx_cwt.py:195-198)
    assert relmax(cwt, g[f"cwt_norm_{key}"]) <= tol["coef"]
    f2, t2, stx = styx_stx.stx_complex_any_scale_pow2(order, sig, fs)
    assert np.array_equal(f2, f) and np.array_equal(t2, t) and stx.dtype == np.complex128  # styx_stx.py:228
    assert relmax(stx, g[f"stx_{key}"]) <= tol["coef"]
    c, bits, tc, fc = cwt_atoms.cwt_chirp_from_sig(sig, fs, order)
    assert c.dtype == np.complex128 and bits.dtype == np.float64  # cwt_atoms.py:408,442
    assert np.array_equal(fc, g[f"chirp_f_{key}"]) and np.array_equal(tc, t)
    assert relmax(c, g[f"chirp_cwt_{key}"]) <= tol["coef"]
    check_bits(bits, g[f"chirp_cwt_{key}"], tol)
    if order == 3:
        _, _, spect = styx_cwt.cwt_complex_any_scale_pow2(order, sig, fs, dictionary_type="spect")
        assert relmax(spect, g[f"cwt_spect_{key}"]) <= tol["coef"]
        c2 = cwt_atoms.cwt_chirp_from_sig(sig, fs, order, dictionary_type="spect")[0]
        assert relmax(c2, g[f"chirp_cwt_spect_{key}"]) <= tol["coef"]
        c3 = cwt_atoms.cwt_chirp_from_sig(sig, fs, order, cwt_type="conv")[0]
        assert relmax(c3, g[f"chirp_cwt_conv_{key}"]) <= tol["coef"]


def test_atom_bank_rows_vs_reference(golden):
    g = golden("small_n1024.npz")
    for key, order, fs in (("o3_fs1000", 3, 1000.0), ("o12_fs800", 12, 800.0)):
        f = g[f"f_{key}"]
        atoms, t_c, scale, omega, amp = styx_cwt.wavelet_centered_4cwt(order, 1024, f, fs, "norm")
        sel = [0, len(f) // 2, len(f) - 1]
        assert relmax(atoms[sel], g[f"atoms_{key}"]) <= 1e-12
        assert scale.shape == atoms.shape and np.array_equal(scale[:, 0], g[f"atom_scale_{key}"])
        assert np.array_equal(amp[:, 7], g[f"atom_amp_{key}"])
        one, _, s1, w1, a1 = styx_cwt.wavelet_centered_4cwt(order, 1024, float(f[3]), fs, "norm")
        assert one.shape == (1024,) and relmax(one, atoms[3]) <= 1e-15
        ref_chirp = orc.chirp_atom(order, 1024, f[3], fs)
        got, _ = cwt_atoms.chirp_centered_4cwt(order, np.zeros(1024), f[3], fs)
        assert relmax(got, ref_chirp) <= 1e-12


@pytest.mark.parametrize("tag", ["n13_fs1000", "n13_fs800", "n16_fs1000"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("order", [3, 12])
def test_stft_vs_reference(golden, tag, dtype, order):
    g = golden("stft.npz")
    tol = TOL[np.dtype(dtype).type]
    fs = float(tag.split("fs")[1])
    sig = g[f"sig_{tag}_{dtype}"]
    z, bits, t, f = styx_fft.stft_from_sig(sig, fs, order)
    key = f"{tag}_{dtype}_o{order}"
    assert np.array_equal(np.array(z.shape), g[f"shape_{key}"])
    assert np.array_equal(t, g[f"t_{key}"]) and np.array_equal(f, g[f"f_{key}"])
    gz = g[f"z_{key}"]
    step = 1 if gz.shape[1] == z.shape[1] else 8
    assert z.dtype == gz.dtype
    assert relmax(z[:, ::step], gz) <= tol["coef"]
    check_bits(bits[:, ::step], gz, tol)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_stft_benchmark_shape_vs_reference(golden, dtype):
    """The STFT of BASELINE configs[2] (2^20 samples, order 12, 2048-sample segments: the fused kernel's <5,5> shape)
    against sampled rows and columns of the reference's 1025 x 1025 panel, axes bit-exact."""
    g = golden("stft_n1048576_o12.npz")
    n, fs, order = 1 << 20, 1000.0, 12
    sig = orc.synth_chirp(n, fs, dtype=np.dtype(dtype).type)
    assert np.array_equal(sig[:: n // 4096], g[f"sig_samples_{dtype}"])  # the fixture's record
    z, bits, t, f = styx_fft.stft_from_sig(sig, fs, order)
    assert np.array_equal(np.array(z.shape), g[f"shape_{dtype}"])
    assert np.array_equal(t, g[f"t_{dtype}"]) and np.array_equal(f, g[f"f_{dtype}"])
    rows, cols = g[f"rows_{dtype}"], g[f"cols_{dtype}"]
    tol = 2e-6 if dtype == "float32" else 1e-12
    zmax = float(g[f"zmax_{dtype}"])
    assert np.max(np.abs(z[rows] - g[f"z_rows_{dtype}"])) <= tol * zmax
    assert np.max(np.abs(z[:, cols] - g[f"z_cols_{dtype}"])) <= tol * zmax
    big = np.abs(g[f"z_cols_{dtype}"]) >= 1e-3 * zmax
    assert np.max(np.abs(bits[:, cols] - g[f"bits_cols_{dtype}"])[big]) <= (2e-3 if dtype == "float32" else 1e-9)


def test_stft_2d_batch_and_errors(golden):
    g = golden("stft.npz")
    f, t, z = styx_fft.stft_complex_pow2(g["sig_2d"], 1000.0, 256)
    assert np.array_equal(f, g["f_2d"]) and np.array_equal(t, g["t_2d"])
    assert z.shape == g["z_2d_alpha025"].shape and relmax(z, g["z_2d_alpha025"]) <= 1e-11
    with pytest.raises(ValueError):
        styx_fft.stft_from_sig(np.zeros(1024), 1000.0, 12)  # ref styx_fft.py:42-45
    # Gaussian-window variant against the oracle's spectral helper
    sig = g["sig_2d"][0]
    f2, t2, zg = styx_fft.gtx_complex_pow2(sig, 1000.0, 256)
    k = np.arange(0, 257) - 128.0
    ref = orc.stft_spectral(sig, 1000.0, np.exp(-(k ** 2) / (2 * 64.0 * 64.0))[:-1], 256, 128, 256)
    assert np.array_equal(t2, ref[1]) and relmax(zg, ref[2]) <= 1e-11


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_corner_cases_vs_reference(golden, dtype):
    """Gaussian-window STFT (styx_fft.py:190-227), chirped atoms index_shift = +-1 (cwt_atoms.py:202-211) and the
    unit-amplitude dictionary (styx_cwt.py:139) against the reference's own outputs."""
    g = golden("corners_n2048.npz")
    tol = TOL[dtype]
    tag = np.dtype(dtype).name
    sig = g[f"sig_{tag}"]
    f, t, z = styx_fft.gtx_complex_pow2(sig, 1000.0, 256)
    assert np.array_equal(f, g[f"gtx_f_{tag}"]) and np.array_equal(t, g[f"gtx_t_{tag}"]) and z.dtype == g[f"gtx_z_{tag}"].dtype
    assert relmax(z, g[f"gtx_z_{tag}"]) <= tol["coef"]
    f, t, z = styx_fft.gtx_complex_pow2(sig, 1000.0, 200, gaussian_sigma=30, overlap_points=150, nfft_points=512)
    assert np.array_equal(t, g[f"gtx2_t_{tag}"]) and relmax(z, g[f"gtx2_z_{tag}"]) <= tol["coef"]
    x = g["sig_float64"].astype(dtype)
    for shift, key in ((1.0, "p1"), (-1.0, "m1")):
        c, bits, _, fc = cwt_atoms.cwt_chirp_from_sig(x, 1000.0, 3, index_shift=shift)
        assert np.array_equal(fc, g[f"shift_f_{key}"])
        assert np.array_equal(np.array(cwt_atoms.chirp_mqg_from_n(3, shift)), g[f"shift_mqg_{key}"])
        assert relmax(c, g[f"shift_cwt_{key}"]) <= tol["coef"], key
        if shift > 0:
            check_bits(bits, g[f"shift_cwt_{key}"], tol)
    c6 = cwt_atoms.cwt_chirp_from_sig(x, 1000.0, 6, index_shift=1.0, dictionary_type="spect")[0]
    assert relmax(c6[::3], g["shift_cwt_o6_spect_p1"]) <= tol["coef"]
    f, _, unit = styx_cwt.cwt_complex_any_scale_pow2(3, x, 1000.0, dictionary_type="unit")
    assert np.array_equal(f, g["unit_f_o3"]) and relmax(unit, g["unit_cwt_o3"]) <= tol["coef"]
    atoms, _, _, _, amp = styx_cwt.wavelet_centered_4cwt(3, len(x), f[:4], 1000.0, "unit")
    assert relmax(atoms, g["unit_atoms"]) <= 1e-12 and np.array_equal(amp[:, 0], g["unit_amp"])


def test_atoms_on_any_time_axis_log2_of_tensors_and_short_records():
    """Behind matching signatures the reference also (a) evaluates atoms on any time axis / offset (styx_cwt.py:68-110,
    cwt_atoms.py:16-50), (b) takes log2 of anything array-like (rescaling.py:13-20), (c) lets SciPy shorten the STFT
    segment to a shorter record (styx_fft.py:175-187)."""
    import warnings
    import scipy.signal

    fs, order = 800.0, 6
    t = np.sort(np.random.default_rng(3).uniform(0.0, 2.0, 777))  # irregular axis, arbitrary offset
    f = np.array([5.0, 40.0, 123.0])
    atoms, x, omega, scale, _, a_norm, a_spect = styx_cwt.wavelet_complex(order, t, 0.7321, f, fs)
    xs = fs * (t - 0.7321)
    s_ref, w_ref = orc.scale_omega(order, f, fs)
    ref = np.exp(-0.5 * (xs[None, :] / s_ref[:, None]) ** 2) * np.exp(1j * w_ref[:, None] * xs[None, :])
    assert np.array_equal(x, xs) and relmax(atoms, ref) <= 1e-12
    atom, tc, an, asp = cwt_atoms.chirp_complex(3, t, 0.7321, 40.0, fs, index_shift=1.0)
    m_q, _, gamma = orc.chirp_mqg_from_n(3, 1.0)
    sc = m_q * fs / 40.0 / (2 * np.pi)
    pp = (1 - 1j * gamma / np.pi) / (2 * sc ** 2)
    assert relmax(atom, np.exp(-pp * xs ** 2) * np.exp(1j * m_q * xs / sc)) <= 1e-12
    # log2(|x| + eps) of device tensors goes through the library's kernel
    from quantum_inferno_amd.utilities import rescaling
    z = torch.randn(3, 1000, dtype=torch.complex128, device="cuda")
    assert np.allclose(rescaling.to_log2_with_epsilon(z).cpu().numpy(), np.log2(np.abs(z.cpu().numpy()) + orc.EPS64), rtol=0, atol=1e-12)
    r32 = torch.randn(4096, dtype=torch.float32, device="cuda")
    got = rescaling.to_log2_with_epsilon(r32)
    assert got.dtype == torch.float32 and np.allclose(got.cpu().numpy(), np.log2(np.abs(r32.cpu().numpy()) + orc.EPS64), atol=2e-6)
    # a record shorter than the segment: SciPy (and the reference through it) shortens the segment to the record
    sig = np.random.default_rng(5).standard_normal(300)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f1, t1, z1 = styx_fft.stft_complex_pow2(sig, fs, 512, overlap_points=100)
        f0, t0, z0 = scipy.signal.stft(sig, fs, window=("tukey", 0.25), nperseg=512, noverlap=100, nfft=512, detrend="constant",
                                       return_onesided=True, boundary="zeros", padded=True)
    assert np.array_equal(f1, f0) and np.allclose(t1, t0, rtol=0, atol=1e-12) and relmax(z1, z0) <= 1e-11


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tfr_info_vs_reference(golden, dtype):
    g = golden("small_n1024.npz")
    tol = TOL[dtype]
    p = g["info_power"].astype(dtype)
    bits, per_time, per_freq = tfr_info.power_dynamics_scaled_bits(p)
    atol = 1e-9 if dtype == np.float64 else 1e-3  # bits within 1e-9 (float64) / 1e-3 (float32)
    assert np.max(np.abs(bits - g["info_bits"])) <= atol
    assert np.max(np.abs(per_time - g["info_bits_time"])) <= atol
    assert np.max(np.abs(per_freq - g["info_bits_freq"])) <= atol
    assert np.max(np.abs(tfr_info.scale_power_bits(p) - g["info_bits"])) <= atol
    for nm, obj in (("tot", tfr_info.shannon_stft_from_tfr_power(p)), ("time", tfr_info.ShannonStftPerTime(p)),
                    ("freq", tfr_info.ShannonStftPerFreq(p))):
        assert np.max(np.abs(obj.info - g[f"sh_{nm}_info"])) <= atol, nm
        assert relmax(obj.shannon_bits, g[f"sh_{nm}_bits"]) <= tol["red"], nm
        assert obj.ref_bits == float(g[f"sh_{nm}_ref"])
        assert np.max(np.abs(obj.isnr - g[f"sh_{nm}_isnr"])) <= atol, nm
        assert relmax(obj.esnr, g[f"sh_{nm}_esnr"]) <= tol["red"], nm
    # 1-D marginal input and a pdf handed in directly
    assert np.max(np.abs(tfr_info.scale_power_bits(p.sum(axis=0)) - g["info_bits_time"])) <= atol
    direct = tfr_info.ShannonStft((g["info_power"] / g["info_power"].sum()).astype(dtype), p.size)
    assert relmax(direct.shannon_bits, g["sh_tot_bits"]) <= tol["red"]


def _plan_with_all(n, fs, order, dtype, channels=1, workspace=None):
    f = qi.scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order)
    ws = workspace or engine.TfrPlan.workspace_for(n, len(f), dtype, channels)
    plan = engine.TfrPlan(n, dtype, None, ws)
    plan.set_styx_bank(order, fs)
    plan.set_stx_bands(order, fs)
    return plan


def check_digest(res, g, prefix, order, tol, rows, channel=0):
    """One record's result against a reference digest: sampled (or whole) panel rows, per-band and per-time power,
    maximum, total and entropy."""
    tsel = g[f"{prefix}_tsel_o{order}"]
    ref_rows = g[f"{prefix}_rows_o{order}"]
    panel = res.coef[channel]
    n_b, n = panel.shape
    sel = panel[torch.from_numpy(np.asarray(rows)).to(panel.device)]
    if ref_rows.shape[1] != n:
        sel = sel[:, torch.from_numpy(tsel).to(panel.device)]
    got = sel.cpu().numpy()
    scale = np.sqrt(float(g[f"{prefix}_pmax_o{order}"]))
    assert np.max(np.abs(got - ref_rows)) / scale <= tol["coef"]
    if "row" in tol and len(rows) == n_b:  # every band kept: each is held to its own maximum
        rel_row = np.max(np.abs(got - ref_rows), axis=1) / np.max(np.abs(ref_rows), axis=1)
        assert rel_row.max() <= tol["row"], (prefix, int(np.argmax(rel_row)), float(rel_row.max()))
    if res.bits is not None:
        bsel = res.bits[channel][torch.from_numpy(np.asarray(rows)).to(panel.device)]
        if ref_rows.shape[1] != n:
            bsel = bsel[:, torch.from_numpy(tsel).to(panel.device)]
        check_bits(bsel.cpu().numpy(), ref_rows, tol)
    pb = res.power_band[channel].cpu().numpy()
    ref_pb = g[f"{prefix}_psum_band_o{order}"]
    assert np.max(np.abs(pb - ref_pb)) / ref_pb.max() <= tol["red"]
    if "row" in tol and len(rows) == n_b:
        assert np.max(np.abs(pb - ref_pb) / ref_pb) <= 10 * tol["red"]  # every band's own power, weak bands included
    pt = res.power_time[channel].cpu().numpy().astype(np.float64)
    ref_pt = g[f"{prefix}_psum_time_o{order}"]
    pt = pt[tsel] if ref_pt.shape[0] != pt.shape[0] else pt
    assert np.max(np.abs(pt - ref_pt)) / ref_pt.max() <= tol["red"]
    st = res.stats[channel].cpu().numpy()
    assert abs(st[0] - float(g[f"{prefix}_pmax_o{order}"])) / st[0] <= 10 * tol["coef"]
    assert abs(st[1] - float(g[f"{prefix}_ptot_o{order}"])) / st[1] <= tol["red"]
    ent = float(res.entropy_bits[channel])
    # (the fused entropy is H = log2 S - sum(P log2 P) / S; the reference's eps64 inside its logarithm moves H by up to
    # ~2e-8 bits, so a float64 caller states that allowance as tol["ent"])
    assert abs(ent - float(g[f"{prefix}_entropy_bits_o{order}"])) <= tol.get("ent", tol["red"] * 20)


@pytest.mark.parametrize("name,n,fs,orders", [("medium_n8192.npz", 8192, 1000.0, (3, 12)),
                                               ("large_n65536.npz", 65536, 800.0, (3, 12))])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_reductions_vs_reference(golden, name, n, fs, orders, dtype):
    g = golden(name)
    tol = TOL_F32_RECORD[dtype]
    sig = torch.from_numpy(g["sig"].astype(dtype)).cuda().unsqueeze(0)
    for order in orders:
        plan = _plan_with_all(n, fs, order, dtype)
        assert np.array_equal(plan.freq[0], g[f"f_o{order}"])
        rows = g[f"rows_o{order}"]
        check_digest(plan.cwt(sig, coef=True, reductions=True), g, "cwt", order, tol, rows)
        check_digest(plan.stx(sig, coef=True, reductions=True), g, "stx", order, tol, rows)
        plan.close()
        c, bits, _, fc = cwt_atoms.cwt_chirp_from_sig(sig[0], fs, order)
        assert np.array_equal(fc, g[f"chirp_f_o{order}"])
        got = c[torch.from_numpy(g[f"chirp_rowsel_o{order}"]).cuda()].cpu().numpy()
        ref = g[f"chirp_rows_o{order}"]
        got = got[:, g[f"chirp_tsel_o{order}"]] if ref.shape[1] != got.shape[1] else got
        assert np.max(np.abs(got - ref)) / np.sqrt(float(g[f"chirp_pmax_o{order}"])) <= tol["coef"]
        engine.clear_plans()


def test_benchmark_size_vs_reference_and_properties(golden):
    """Config 2 of BASELINE.json: 1 channel, 2^20 samples, order 3, float32."""
    g = golden("large_n1048576.npz")
    n, fs, order = 1 << 20, 1000.0, 3
    tol = TOL[np.float32]
    x = orc.synth_chirp(n, fs, dtype=np.float32)
    assert np.max(np.abs(x[:: n // 4096] - g["sig_samples"])) <= 1e-6  # same seeded input as the fixture
    sig = torch.from_numpy(x).cuda().unsqueeze(0)
    plan = _plan_with_all(n, fs, order, np.float32)
    rows = g["rows_o3"]
    assert len(rows) == len(plan.freq[0])  # the fixture holds every band: each sub-engine's rows are reference-pinned
    res_c = plan.cwt(sig, coef=True, bits=True, reductions=True)
    check_digest(res_c, g, "cwt", order, tol, rows)
    res_c.bits = None
    res_s = plan.stx(sig, coef=True, bits=True, reductions=True)
    check_digest(res_s, g, "stx", order, tol, rows)
    res_s.bits = None
    fus_c, fus_s = plan.cwt_stx(sig, coef=True, reductions=True)  # the benchmark's call: joint launches
    check_digest(fus_c, g, "cwt", order, tol, rows)
    check_digest(fus_s, g, "stx", order, tol, rows)
    del fus_c, fus_s
    # cwt_atoms (circular CWT, 49 bands) on the native engine, every band against the reference
    c_atoms, bits_atoms, _, fc = cwt_atoms.cwt_chirp_from_sig(sig[0], fs, order)
    assert np.array_equal(fc, g["chirp_f_o3"])
    got = c_atoms[:, torch.from_numpy(g["chirp_tsel_o3"]).cuda()].cpu().numpy()
    ref = g["chirp_rows_o3"]
    assert np.max(np.abs(got - ref)) / np.sqrt(float(g["chirp_pmax_o3"])) <= tol["coef"]
    rel_row = np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)
    assert rel_row.max() <= tol["row"], ("chirp", int(np.argmax(rel_row)), float(rel_row.max()))
    del c_atoms, bits_atoms
    engine.clear_plans()
    # fused reductions agree with a direct reduction of the stored panel
    p = (res_s.coef[0].abs() ** 2).double()
    assert torch.allclose(p.sum(dim=1), res_s.power_band[0], rtol=1e-5)
    assert torch.allclose(p.sum(dim=0), res_s.power_time[0].double(), rtol=1e-4, atol=1e-6 * float(p.sum(dim=0).max()))
    # linearity: T(a x + b y) = a T(x) + b T(y)
    y = torch.from_numpy(orc.synth_chirp(n, fs, channel=1, n_channels=2, dtype=np.float32)).cuda().unsqueeze(0)
    mix = 0.75 * sig - 1.5 * y
    for fn in (plan.cwt, plan.stx):
        a, b, m = fn(sig).coef, fn(y).coef, fn(mix).coef
        lin = 0.75 * a - 1.5 * b
        assert float((m - lin).abs().max() / lin.abs().max()) <= 4 * tol["coef"]
        del a, b, m, lin
    # Stockwell is covariant to circular time shifts: |STX(x shifted by s)| = |STX(x)| shifted by s
    s = 12345
    shifted = plan.stx(torch.roll(sig, s, dims=1)).coef
    assert float((shifted.abs() - torch.roll(res_s.coef, s, dims=2).abs()).abs().max() / res_s.coef.abs().max()) <= 4 * tol["coef"]
    plan.close()


def test_order6_table_at_2e19_vs_reference(golden):
    """An order-6 table at 2^19 samples (other zoom classes and reach groups than orders 3 / 12 at 2^20) on the native
    engines, every band of both panels against reference rows -- not against the hipFFT engine."""
    g = golden("large_n524288_o6.npz")
    n, fs, order = 1 << 19, 1000.0, 6
    tol = TOL[np.float32]
    x = orc.synth_chirp(n, fs, dtype=np.float32)
    assert np.max(np.abs(x[:: n // 4096] - g["sig_samples"])) <= 1e-6
    sig = torch.from_numpy(x).cuda().unsqueeze(0)
    plan = _plan_with_all(n, fs, order, np.float32)
    rows = g["rows_o6"]
    assert np.array_equal(plan.freq[0], g["f_o6"]) and len(rows) == len(plan.freq[0])
    for which in (0, 2):
        assert plan.stage_bands("zoom")[which] + plan.stage_bands("block")[which] == len(rows)  # native engines only
    res_c, res_s = plan.cwt_stx(sig, coef=True, reductions=True)
    check_digest(res_c, g, "cwt", order, tol, rows)
    check_digest(res_s, g, "stx", order, tol, rows)
    for c in (4,):  # and as a batch (the batch cut of the block items, the short zoom classes)
        xb = torch.from_numpy(np.stack([x] + [orc.synth_chirp(n, fs, k, c, np.float32) for k in range(1, c)])).cuda()
        bc, bs = plan.cwt_stx(xb, coef=True, reductions=True)
        check_digest(bc, g, "cwt", order, tol, rows)
        check_digest(bs, g, "stx", order, tol, rows)
    plan.close()


def test_config3_64_channels_order12_vs_reference(golden):
    """Config 3 of BASELINE.json (configs[2]): 64 channels x 2^20 samples, order 12 (167 bands), float32, the full
    stack -- STFT + CWT + STX + entropy -- in one batch on one GPU.  Channel 0 is the record of the reference fixture
    (every band of both panels at ~1250 sampled times, all reductions); every other channel's batch result is checked
    against the same plan run on that record alone (sampled rows, all reductions); the STFT against the oracle."""
    from quantum_inferno_amd import synth

    g = golden("large_n1048576_o12.npz")
    n, fs, order, n_ch = 1 << 20, 1000.0, 12, 64
    tol = TOL[np.float32]
    x = synth.channels(n, fs, 0, n_ch, n_ch, np.float32)
    assert np.max(np.abs(x[0, :: n // 4096] - g["sig_samples"])) <= 1e-6  # channel 0 = the fixture's record
    sig = torch.from_numpy(x).cuda()
    plan = _plan_with_all(n, fs, order, np.float32, channels=n_ch)  # (8 GiB of scratch: the batch goes through in tiles)
    assert np.array_equal(plan.freq[0], g["f_o12"]) and len(plan.freq[0]) == 167
    rows = g["rows_o12"]
    assert len(rows) == 167
    res_c, res_s = plan.cwt_stx(sig, coef=True, reductions=True)
    torch.cuda.synchronize()
    assert res_c.coef.shape == (n_ch, 167, n) and res_s.coef.shape == (n_ch, 167, n)
    check_digest(res_c, g, "cwt", order, tol, rows)
    check_digest(res_s, g, "stx", order, tol, rows)
    # the last record of the batch against the reference too (Stockwell panel, every band): pins the batch indexing
    g63 = golden("large_n1048576_o12_ch63_stx.npz")
    assert np.max(np.abs(x[63, :: n // 4096] - g63["sig_samples"])) <= 1e-6 and np.array_equal(g63["f_o12"], g["f_o12"])
    check_digest(res_s, g63, "stx", order, tol, g63["rows_o12"], channel=63)
    # every channel of the batch against its single-record run (other tiling, same kernels)
    tsel = torch.from_numpy(g["cwt_tsel_o12"]).cuda()
    one = None
    for c in range(n_ch):
        one = plan.cwt_stx(sig[c : c + 1], coef=True, reductions=True, out=one)
        for batch, single in ((res_c, one[0]), (res_s, one[1])):
            a, b = batch.coef[c][:, tsel], single.coef[0][:, tsel]
            assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max()), c
            assert torch.allclose(batch.power_band[c], single.power_band[0], rtol=1e-5), c
            assert torch.allclose(batch.power_time[c], single.power_time[0], rtol=1e-4, atol=1e-7 * float(single.power_time.max())), c
            assert torch.allclose(batch.stats[c, :3], single.stats[0, :3], rtol=1e-5), c
    del res_c, res_s, one
    plan.close()
    torch.cuda.empty_cache()
    # cwt_atoms at order 12 (170 bands, circular) for the fixture's record
    c_atoms, _, _, fc = cwt_atoms.cwt_chirp_from_sig(sig[0], fs, order)
    assert np.array_equal(fc, g["chirp_f_o12"])
    got = c_atoms[:, torch.from_numpy(g["chirp_tsel_o12"]).cuda()].cpu().numpy()
    ref = g["chirp_rows_o12"]
    assert np.max(np.abs(got - ref)) / np.sqrt(float(g["chirp_pmax_o12"])) <= tol["coef"]
    del c_atoms
    engine.clear_plans()
    # the STFT of the stack: order 12 -> 2048-sample segments, (1025 x 1025) per channel
    stft = styx_fft.StftPlan(n, n_ch, fs, order, torch.float32)
    z, bits = stft.run(sig)
    assert z.shape == (n_ch, 1025, 1025)
    for c in (0, 17, 63):
        ref_z, ref_bits, ref_t, ref_f = orc.stft_from_sig(x[c], fs, order)
        assert np.array_equal(stft.time_s, ref_t) and np.array_equal(stft.frequency_hz, ref_f)
        assert relmax(z[c].cpu().numpy(), ref_z) <= tol["coef"]
        check_bits(bits[c].cpu().numpy(), ref_z, tol)
    zw, bw, tw, fw = styx_fft.stft_from_sig(sig[5], fs, order)  # the reference-signature wrapper: the same kernels
    assert float((zw - z[5]).abs().max()) <= 1e-6 * float(z[5].abs().max()) and np.array_equal(tw, stft.time_s)


def test_batches_tiles_and_oracle_on_noise():
    """Ragged cases: several channels, a workspace that forces band tiles and channel tiles,
    a record length that is not a power of two, all-zero input."""
    rng = np.random.default_rng(7)
    n, fs, order = 4096, 1000.0, 6
    x = rng.standard_normal((5, n))
    ref_c = np.stack([orc.cwt_fft(order, xi, fs)[2] for xi in x])
    ref_s = np.stack([orc.stx_fft(order, xi, fs)[2] for xi in x])
    f, _, c = styx_cwt.cwt_complex_any_scale_pow2(order, x, fs)
    assert c.shape == ref_c.shape and relmax(c, ref_c) <= 1e-11
    _, _, s = styx_stx.stx_complex_any_scale_pow2(order, x, fs)
    assert relmax(s, ref_s) <= 1e-11
    # tiny workspace: 1 channel x 5 bands per tile
    small = 7 * 2 * n * 16 + len(f) * 4 * 32 + 8192
    plan = _plan_with_all(n, fs, order, np.float64, workspace=small)
    xt = torch.from_numpy(x).cuda()
    r = plan.cwt(xt, coef=True, bits=True, reductions=True)
    assert relmax(r.coef.cpu().numpy(), ref_c) <= 1e-11
    p = np.abs(ref_c) ** 2
    assert np.allclose(r.power_band.cpu().numpy(), p.sum(axis=2), rtol=1e-10)
    assert np.allclose(r.power_time.cpu().numpy(), p.sum(axis=1), rtol=1e-10)
    assert np.allclose(r.stats[:, 0].cpu().numpy(), p.max(axis=(1, 2)), rtol=1e-10)
    ent = [np.sum(orc.shannon_from_power(pi).shannon_bits) for pi in p]
    assert np.allclose(r.entropy_bits.cpu().numpy(), ent, rtol=1e-10)
    r2 = plan.stx(xt, coef=True, reductions=True)
    assert relmax(r2.coef.cpu().numpy(), ref_s) <= 1e-11
    zero = plan.cwt(torch.zeros((1, n), dtype=torch.float64, device="cuda"), coef=True, reductions=True)
    assert float(zero.coef.abs().max()) == 0.0 and float(zero.stats[0, 1]) == 0.0
    plan.close()
    # n not a power of two goes through the same path with hipFFT sizes
    m = 3000
    xm = rng.standard_normal(m)
    assert relmax(styx_cwt.cwt_complex_any_scale_pow2(3, xm, fs)[2], orc.cwt_fft(3, xm, fs)[2]) <= 1e-11
    assert relmax(styx_stx.stx_complex_any_scale_pow2(3, xm, fs)[2], orc.stx_fft(3, xm, fs)[2]) <= 1e-11
    assert relmax(cwt_atoms.cwt_chirp_from_sig(xm, fs, 3)[0], orc.cwt_chirp_fft(xm, fs, 3)[0]) <= 1e-11
    # index_shift != 0 (chirped atoms, complex p)
    ref = orc.cwt_chirp_fft(x[0], fs, 3, index_shift=1.0)[0]
    assert relmax(cwt_atoms.cwt_chirp_from_sig(x[0], fs, 3, index_shift=1.0)[0], ref) <= 1e-11
    with pytest.raises(ValueError):
        styx_cwt.cwt_complex_any_scale_pow2(3, x[0], fs, cwt_type="morlet2")
    with pytest.raises(ValueError):
        cwt_atoms.cwt_chirp_from_sig(x[0], fs, 3, cwt_type="nope")
    # CUDA tensor in -> CUDA tensor out
    out = styx_stx.stx_complex_any_scale_pow2(order, xt[0], fs)[2]
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.shape == ref_s[0].shape


def test_native_engine_batches_match_single_records():
    """Native engine (float32, n = 2^20 and 2^19): a 3-channel batch equals the three single-record results and the
    hipFFT engine on the same input; also with a workspace that forces channel tiling."""
    from quantum_inferno_amd import _lib

    fs, order = 1000.0, 3
    for n in (1 << 20, 1 << 19):
        x = torch.from_numpy(np.stack([orc.synth_chirp(n, fs, c, 3, np.float32) for c in range(3)])).cuda()
        plan = _plan_with_all(n, fs, order, np.float32, channels=3)
        ref = engine.TfrPlan(n, np.float32, None, engine.TfrPlan.workspace_for(n, len(plan.freq[0]), np.float32, 1),
                             _lib.QI_ENGINE_HIPFFT)
        ref.set_styx_bank(order, fs)
        ref.set_stx_bands(order, fs)
        for name in ("cwt", "stx"):
            batch = getattr(plan, name)(x, coef=True, bits=(n == 1 << 19), reductions=True)
            for c in range(3):
                one = getattr(plan, name)(x[c : c + 1], coef=True, reductions=True)
                assert torch.equal(one.coef[0], batch.coef[c]), (name, n, c)
                assert torch.equal(one.power_band[0], batch.power_band[c])
                # the band-chunking (hence the summation order over bands) depends on the channel count
                assert torch.allclose(one.power_time[0], batch.power_time[c], rtol=1e-5, atol=1e-7 * float(one.power_time.max()))
                assert torch.allclose(one.stats[0], batch.stats[c], rtol=1e-5)
            # reductions without a stored panel (the short-atom bands hand their edge samples over in scratch)
            lean = getattr(plan, name)(x, coef=False, reductions=True)
            assert lean.coef is None
            assert torch.equal(lean.power_band, batch.power_band), (name, n)
            assert torch.equal(lean.power_time, batch.power_time) and torch.equal(lean.stats, batch.stats)
            gold = getattr(ref, name)(x[1:2], coef=True, bits=(n == 1 << 19), reductions=True)
            scale = float(gold.coef.abs().max())
            assert float((gold.coef[0] - batch.coef[1]).abs().max()) / scale <= 2e-5, (name, n)
            assert torch.allclose(gold.power_band[0], batch.power_band[1], rtol=1e-4)
            assert torch.allclose(gold.power_time[0], batch.power_time[1], rtol=1e-3, atol=1e-6 * float(gold.power_time.max()))
            assert torch.allclose(gold.stats[0, :3], batch.stats[1, :3], rtol=1e-4)
            if batch.bits is not None:
                big = gold.coef[0].abs() >= 1e-2 * scale
                assert float((gold.bits[0] - batch.bits[1]).abs()[big].max()) <= 1e-3
            del batch, gold
        ref.close()
        plan.close()
    # channel tiling: workspace for one record only
    n = 1 << 20
    x = torch.from_numpy(np.stack([orc.synth_chirp(n, fs, c, 2, np.float32) for c in range(2)])).cuda()
    big = _plan_with_all(n, fs, order, np.float32, channels=2)
    small = _plan_with_all(n, fs, order, np.float32, channels=1)
    for name in ("cwt", "stx"):
        a, b = getattr(big, name)(x, coef=True, reductions=True), getattr(small, name)(x, coef=True, reductions=True)
        assert torch.equal(a.coef, b.coef) and torch.allclose(a.stats, b.stats, rtol=1e-5)
        assert torch.allclose(a.power_time, b.power_time, rtol=1e-5, atol=1e-7 * float(a.power_time.max()))
    big.close()
    small.close()
    # cwt_atoms on the native engine (circular bank, roll by n/2) against the hipFFT engine
    sig = x[0].cpu().numpy()
    c_nat = cwt_atoms.cwt_chirp_from_sig(sig, fs, 3)[0]
    import os
    engine.clear_plans()
    os.environ["QI_FORCE_HIPFFT"] = "1"
    try:
        c_ref = cwt_atoms.cwt_chirp_from_sig(sig, fs, 3)[0]
    finally:
        del os.environ["QI_FORCE_HIPFFT"]
        engine.clear_plans()
    assert relmax(c_nat, c_ref) <= 2e-5


@pytest.mark.parametrize("order", [3, 12])
def test_float64_native_engine_vs_oracle(golden, order):
    """float64 records of 2^20 samples run on the native engines in double arithmetic (float64 zoom, block engine, split
    bands; the exact two-pass kernels for whatever those leave).  Against the oracle (pinned to the reference at this length by
    tests/test_oracle_golden.py::test_benchmark_length_rows) on a sample of bands of every kind, at the float64
    tolerance; every band and every fused reduction against the hipFFT engine (the reference's algorithm on the GPU);
    and every band against the reference's own rows at this length (captured from a float32 record, so the reference
    output carries ~1e-7 of SciPy's single-precision FFT: compared at 5e-7)."""
    from quantum_inferno_amd import _lib

    n, fs = 1 << 20, 1000.0
    tol = TOL[np.float64]
    x = orc.synth_chirp(n, fs, dtype=np.float64)
    xt = torch.from_numpy(x).cuda().unsqueeze(0)
    f = scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order)
    nb = len(f)
    ws = engine.TfrPlan.workspace_for(n, nb, np.float64, 1)
    nat = engine.TfrPlan(n, np.float64, None, ws, _lib.QI_ENGINE_NATIVE)
    ref = engine.TfrPlan(n, np.float64, None, ws, _lib.QI_ENGINE_HIPFFT)
    for plan in (nat, ref):
        plan.set_styx_bank(order, fs)
        plan.set_stx_bands(order, fs)
    for which in (0, 2):  # the narrow-spectrum bands on the float64 zoom engine, short atoms with wide spectra on the
        # block engine in double arithmetic, what is left on the two-pass kernels
        assert nat.stage_bands("pass2")[which] + nat.stage_bands("zoom")[which] + nat.stage_bands("block")[which] == nb
        assert nat.stage_bands("zoom")[which] >= nb // 2 and nat.stage_bands("block")[which] > 0
    if not any(k in os.environ for k in ("QI_NATIVE_SPLIT", "QI_NATIVE_SPLIT64", "QI_NATIVE_Z64", "QI_NATIVE_BLOCK64")):
        # the styx bands with atoms longer than the record are split between the float64 zoom (tapered part) and the block
        # engine's edge items (k_block64_edge): nothing of either table is left on the two-pass kernels
        assert nat.stage_bands("pass2")[0] == 0 and nat.stage_bands("pass2")[2] == 0
    pick = sorted({0, 1, nb // 5, nb // 2, (3 * nb) // 4, nb - 2, nb - 1})
    for name, fn in (("cwt", orc.cwt_fft), ("stx", orc.stx_fft)):
        a = getattr(nat, name)(xt, coef=True, bits=True, reductions=True)
        _, _, want = fn(order, x, fs, bands=pick)
        got = a.coef[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        scale = float(a.coef.abs().max())
        assert np.max(np.abs(got - want)) <= tol["coef"] * scale, (name, order)
        for i, j in enumerate(pick):  # each sampled band also to its own maximum (weak bands carry the rounding of the strong ones)
            assert np.max(np.abs(got[i] - want[i])) <= 5e-9 * np.max(np.abs(want[i])), (name, order, j)
        # (at 2^20 samples the float64 transforms carry ~1e-12 of the panel maximum: 1e-9 bits where the coefficient
        # tolerance implies them, and 1e-8 from 1e-3 of the maximum as in round 4)
        got_bits = a.bits[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        check_bits(got_bits, want, dict(bits=tol["bits"], bits_floor=BITS_FLOOR64, bits_wide=(1e-8, 1e-3)))
        b = getattr(ref, name)(xt, coef=True, reductions=True)
        worst = float((a.coef - b.coef).abs().amax(dim=2).max()) / scale
        assert worst <= tol["coef"], (name, order, worst)
        assert torch.allclose(a.power_band, b.power_band, rtol=1e-9, atol=1e-12 * float(b.power_band.max()))
        assert torch.allclose(a.power_time, b.power_time, rtol=1e-8, atol=1e-11 * float(b.power_time.max()))
        assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=1e-9)
        # (reductions only: the float64 kernels leave out the unit-modulus carrier / demodulation factor of every output --
        # the powers are those of the envelope, equal to a rounding)
        lean = getattr(nat, name)(xt[:, :], coef=False, reductions=True)
        assert torch.allclose(lean.reduced, a.reduced, rtol=1e-12, atol=1e-14 * float(a.reduced.abs().max()))
        del a, b, lean
    if order == 3:
        # the float64 record against the REFERENCE run on the same float64 record (every band of both panels, all
        # reductions): the float64 tolerances, no allowance for a single-precision spectrum inside the reference
        g64 = golden("large_n1048576_f64.npz")
        assert np.max(np.abs(x[:: n // 4096] - g64["sig_samples"])) == 0.0 and np.array_equal(f, g64["f_o3"])
        for name in ("cwt", "stx"):
            res = getattr(nat, name)(xt, coef=True, bits=True, reductions=True)
            check_digest(res, g64, name, order, dict(tol, bits_floor=1e-3, bits_wide=(1e-8, 1e-3), row=5e-9, ent=5e-8), g64["rows_o3"])
            del res
    g = golden("large_n1048576.npz" if order == 3 else "large_n1048576_o12.npz")
    x32 = torch.from_numpy(orc.synth_chirp(n, fs, dtype=np.float32).astype(np.float64)).cuda().unsqueeze(0)
    rows = g[f"rows_o{order}"]
    assert len(rows) == nb
    for name in ("cwt", "stx"):
        res = getattr(nat, name)(x32, coef=True, reductions=True)
        check_digest(res, g, name, order, TOL_F32_RECORD[np.float64], rows)
        del res
    if order == 3:
        # cwt_atoms (circular CWT: the float64 zoom engine's rolled kind) on the native engine, every band against the
        # reference's rows and against the hipFFT engine
        c_atoms, _, _, fc = cwt_atoms.cwt_chirp_from_sig(x32[0], fs, order)
        assert np.array_equal(fc, g["chirp_f_o3"])
        got = c_atoms[:, torch.from_numpy(g["chirp_tsel_o3"]).cuda()].cpu().numpy()
        refc = g["chirp_rows_o3"]
        assert np.max(np.abs(got - refc)) / np.sqrt(float(g["chirp_pmax_o3"])) <= TOL_F32_RECORD[np.float64]["coef"]
        del c_atoms
        engine.clear_plans()
    # a batch of three records (tiles of the scratch) equals the single-record runs
    xb = torch.from_numpy(np.stack([orc.synth_chirp(n, fs, c, 3, np.float64) for c in range(3)])).cuda()
    if order == 3:
        batch = nat.cwt(xb, coef=True, reductions=True)
        for c in range(3):
            one = nat.cwt(xb[c : c + 1], coef=True, reductions=True)
            assert torch.equal(one.coef[0], batch.coef[c]) and torch.equal(one.power_band[0], batch.power_band[c])
            assert torch.allclose(one.stats[0], batch.stats[c], rtol=1e-12)
    nat.close()
    ref.close()


@pytest.mark.parametrize("channels,fs,ws_cap", [(4, 1000.0, 48 << 30), (16, 800.0, 32 << 30)])
def test_float64_order12_batches_at_timed_shape(golden, channels, fs, ws_cap):
    """The float64 engines at the shapes that are TIMED: 4 records x order 12 x 2^20 through `cwt_stx` (bench.py's f64 leg,
    1 kHz, 48 GiB scratch cap) and 16 records at 800 Hz with a 32 GiB cap (one item of the configs[4] streaming leg: the records
    pass in tiles), with the panels stored and with `coef=False` (streaming keeps the reduced product only).
      * every record against its single-record run (coefficients bit for bit: the same kernels; the reductions to 1e-12 --
        the per-time planes of a batch are cut differently);
      * record 0 against the oracle at 1e-10 on bands of every engine: all 14 split bands (float64 zoom + k_block64_edge),
        zoom bands of several grids, block bands of both k_block64 variants (styx / Stockwell demodulation);
      * at 1 kHz record 0 against the REFERENCE run on the same float64 record, every band of both panels and every
        reduction (large_n1048576_o12_f64.npz; the reference is complex128 throughout: styx_stx.py:228, styx_cwt.py:195-198);
      * the reductions of `coef=False` equal those of the stored-panel call to 1e-12 (the streaming kernels skip the unit-modulus
        carrier / demodulation factor), and the per-band powers equal a direct
        sum over the stored panel (tfr_info.py:82-94)."""
    n, order = 1 << 20, 12
    tol = TOL[np.float64]
    f = scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order)
    nb = len(f)
    assert nb == 167
    recs = [orc.synth_chirp(n, fs, dtype=np.float64)] + [orc.synth_chirp(n, fs, c, channels, np.float64) for c in range(1, channels)]
    x = torch.from_numpy(np.stack(recs)).cuda()
    plan = engine.TfrPlan(n, np.float64, None, engine.TfrPlan.workspace_for(n, nb, np.float64, channels, cap_bytes=ws_cap))
    plan.set_styx_bank(order, fs)
    plan.set_stx_bands(order, fs)
    knobs = ("QI_NATIVE_SPLIT", "QI_NATIVE_SPLIT64", "QI_NATIVE_Z64", "QI_NATIVE_BLOCK64")
    if not any(k in os.environ for k in knobs):
        assert plan.stage_bands("pass2")[0] == 0 and plan.stage_bands("pass2")[2] == 0
        assert plan.stage_bands("block")[0] >= 20 and plan.stage_bands("block")[2] >= 20
        assert plan.stage_bands("block")[0] + plan.stage_bands("zoom")[0] == nb  # (the 14 split bands count with the zoom engine)
    full = plan.cwt_stx(x, coef=True, reductions=True)
    lean = plan.cwt_stx(x, coef=False, reductions=True)
    torch.cuda.synchronize()
    for a, b in zip(full, lean):  # (no carrier / demodulation factor when nothing is stored: equal to a rounding)
        assert b.coef is None
        assert torch.allclose(a.power_band, b.power_band, rtol=1e-12, atol=0.0)
        assert torch.allclose(a.power_time, b.power_time, rtol=1e-12, atol=1e-14 * float(a.power_time.max()))
        assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=1e-12)
    # every record against its single-record run
    for c in range(channels):
        one = plan.cwt_stx(x[c : c + 1], coef=True, reductions=True)
        for a, b, name in zip(full, one, ("cwt", "stx")):
            assert torch.equal(a.coef[c], b.coef[0]), (name, c)
            assert torch.allclose(a.power_band[c], b.power_band[0], rtol=1e-12, atol=0.0), (name, c)
            assert torch.allclose(a.power_time[c], b.power_time[0], rtol=1e-11, atol=1e-13 * float(b.power_time.max())), (name, c)
            assert torch.allclose(a.stats[c, :3], b.stats[0, :3], rtol=1e-12), (name, c)
        del one
    # the fused reductions against a direct reduction of the stored panels (one record at a time: 2.8 GB each)
    for a, name in zip(full, ("cwt", "stx")):
        for c in (0, channels - 1):
            p = a.coef[c].real ** 2 + a.coef[c].imag ** 2
            assert torch.allclose(a.power_band[c], p.sum(dim=1), rtol=1e-10), name
            assert torch.allclose(a.power_time[c], p.sum(dim=0), rtol=1e-9, atol=1e-12 * float(p.sum(dim=0).max())), name
            assert abs(float(a.stats[c, 0]) - float(p.max())) <= 1e-12 * float(p.max())
            assert abs(float(a.stats[c, 1]) - float(p.sum())) <= 1e-10 * float(p.sum())
            del p
    # record 0 against the oracle on bands of every engine
    picks = {"cwt": list(range(14)) + [14, 40, 90, 130, nb - 23, nb - 12, nb - 1],
             "stx": [0, 1, 30, 90, 130, nb - 23, nb - 12, nb - 2, nb - 1]}
    for a, name, fn in zip(full, ("cwt", "stx"), (orc.cwt_fft, orc.stx_fft)):
        pick = picks[name]
        _, _, want = fn(order, recs[0], fs, bands=pick)
        got = a.coef[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        scale = float(a.coef[0].abs().max())
        assert np.max(np.abs(got - want)) <= tol["coef"] * scale, name
        for i, j in enumerate(pick):
            assert np.max(np.abs(got[i] - want[i])) <= 5e-9 * np.max(np.abs(want[i])), (name, j)
        pb = a.power_band[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        assert np.allclose(pb, (np.abs(want) ** 2).sum(axis=1), rtol=tol["red"]), name
        # the last record too (another tile of the scratch at 16 records), on one band of each engine
        last = [pick[0], pick[len(pick) // 2], pick[-1]]
        _, _, want = fn(order, recs[-1], fs, bands=last)
        got = a.coef[channels - 1][torch.tensor(last, device="cuda")].cpu().numpy()
        assert np.max(np.abs(got - want)) <= tol["coef"] * scale, (name, "last record")
    if fs == 1000.0:
        g = golden("large_n1048576_o12_f64.npz")
        assert np.max(np.abs(recs[0][:: n // 4096] - g["sig_samples"])) == 0.0 and np.array_equal(f, g["f_o12"])
        assert len(g["rows_o12"]) == nb
        # (entropy: the reference adds eps64 to every pdf value inside its logarithm (tfr_info.py:203-228), which lowers H by
        # sum pdf log2(1 + eps / pdf) <= D eps / ln 2 = 5.6e-8 bits for the D = 167 x 2^20 points of this panel; the fused
        # H = log2 S - sum(P log2 P) / S has no such term)
        ent_tol = 1.05 * nb * n * float(orc.EPS64) / np.log(2.0) + 1e-9
        for a, name in zip(full, ("cwt", "stx")):
            check_digest(a, g, name, order, dict(tol, bits_floor=1e-3, bits_wide=(1e-8, 1e-3), row=5e-9, ent=ent_tol), g["rows_o12"])
    del full, lean
    plan.close()


@pytest.mark.parametrize("log2n,name,order", [(19, "cwt", 6), (21, "stx", 6), (16, "cwt", 12), (16, "stx", 3), (18, "cwt", 3),
                                              (18, "stx", 12), (22, "cwt", 6), (22, "stx", 6), (15, "cwt", 6),
                                              (16, "cwt", 1), (18, "cwt", 2), (20, "cwt", 1)])
def test_float64_native_engine_other_lengths(log2n, name, order):
    """The float64 engines (float64 zoom, block engine in double, split bands) at other record lengths than 2^20: every
    power of two from 2^15 to 2^22 whose band table leaves nothing for the two-pass kernels (round 3 ran these on the hipFFT
    engine, 13-25 x slower, except the two shapes with 2^20 / 2^21-point transforms).  Against the ORACLE on bands of every
    engine at the float64 tolerance, and against the hipFFT engine: every row to its own maximum, and the fused reductions.
    Orders 1 and 2 (round 4): their top band's atom is shorter than 2.75 samples -- the block engine in double takes it with the
    aliases of its Gaussian spectrum summed in the weight table."""
    from quantum_inferno_amd import _lib

    n, fs = 1 << log2n, 1000.0
    x = torch.from_numpy(orc.synth_chirp(n, fs, dtype=np.float64)).cuda().unsqueeze(0)
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order))
    ws = engine.TfrPlan.workspace_for(n, nb, np.float64, 1)
    nat = engine.TfrPlan(n, np.float64, None, ws, _lib.QI_ENGINE_AUTO)
    ref = engine.TfrPlan(n, np.float64, None, ws, _lib.QI_ENGINE_HIPFFT)
    for plan in (nat, ref):
        (plan.set_styx_bank if name == "cwt" else plan.set_stx_bands)(order, fs)
    which = 0 if name == "cwt" else 2
    assert nat.stage_bands("zoom")[which] + nat.stage_bands("pass2")[which] + nat.stage_bands("block")[which] == nb
    assert nat.stage_bands("zoom")[which] > 0 and nat.stage_bands("block")[which] > 0  # (zero would mean: the hipFFT engine ran it)
    a = getattr(nat, name)(x, coef=True, reductions=True)
    b = getattr(ref, name)(x, coef=True, reductions=True)
    pick = sorted({0, 1, nb // 4, nb // 2, (3 * nb) // 4, nb - 2, nb - 1})
    _, _, want = (orc.cwt_fft if name == "cwt" else orc.stx_fft)(order, x[0].cpu().numpy(), fs, bands=pick)
    got = a.coef[0][torch.tensor(pick, device="cuda")].cpu().numpy()
    assert np.max(np.abs(got - want)) <= TOL[np.float64]["coef"] * float(b.coef.abs().max()), (log2n, name)
    for i, j in enumerate(pick):
        assert np.max(np.abs(got[i] - want[i])) <= 5e-9 * np.max(np.abs(want[i])), (log2n, name, j)
    assert np.allclose(a.power_band[0][torch.tensor(pick, device="cuda")].cpu().numpy(), (np.abs(want) ** 2).sum(axis=1), rtol=1e-10)
    peak = b.coef[0].abs().amax(dim=1)
    err = (a.coef[0] - b.coef[0]).abs().amax(dim=1) / peak
    assert float(err.max()) <= 5e-9, (int(err.argmax()), float(err.max()))
    assert float((a.coef - b.coef).abs().max()) <= TOL[np.float64]["coef"] * float(b.coef.abs().max())
    assert torch.allclose(a.power_band, b.power_band, rtol=1e-9, atol=1e-12 * float(b.power_band.max()))
    assert torch.allclose(a.power_time, b.power_time, rtol=1e-8, atol=1e-11 * float(b.power_time.max()))
    assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=1e-9)
    nat.close()
    ref.close()


def test_streaming_chunks_float64():
    """Config-5 shape in miniature: a long float64 record as overlapped chunks; every chunk's reduced product equals
    the transform of that chunk alone, and a run restarted at a chunk boundary reproduces the rest."""
    from quantum_inferno_amd import stream

    rng = np.random.default_rng(11)
    n, hop, fs, order = 4096, 2048, 800.0, 12
    x = rng.standard_normal((2, 3 * n + 777))
    plan = _plan_with_all(n, fs, order, np.float64, channels=2)
    seen = {}
    for i, start, res in stream.stream_reduced(plan, x, hop, "cwt"):
        seen[i] = (start, res.power_band.clone(), res.entropy_bits.clone())
    assert len(seen) == len(stream.chunk_starts(x.shape[1], n, hop))
    for i, (start, band, ent) in seen.items():
        ref = np.stack([orc.cwt_fft(order, x[c, start : start + n], fs)[2] for c in range(2)])
        p = np.abs(ref) ** 2
        assert np.allclose(band.cpu().numpy(), p.sum(axis=2), rtol=1e-10)
        assert np.allclose(ent.cpu().numpy(), [np.sum(orc.shannon_from_power(pc).shannon_bits) for pc in p], rtol=1e-10)
    resumed = {i: r.power_band.clone() for i, _, r in stream.stream_reduced(plan, x, hop, "cwt", first_chunk=3)}
    assert sorted(resumed) == [k for k in sorted(seen) if k >= 3]
    for i, band in resumed.items():
        assert torch.equal(band, seen[i][1])
    plan.close()


def test_stream_pipeline_full_chunks_float64():
    """Config 5 at its real chunk length: float64 records on the host, chunks of 2^20 samples with a hop of 2^19 (three
    hops and the flush chunk), moved through the double-buffered pipeline (pinned staging, copy stream) in channel
    blocks; every item's reduced product equals the same chunk handed to the plan directly; two ranks' shares make
    up the whole; a run restarted at an item reproduces the rest."""
    from quantum_inferno_amd import stream

    n, hop, fs, order = 1 << 20, 1 << 19, 800.0, 3
    rng = np.random.default_rng(19)
    total = n + 2 * hop + 777
    host = np.stack([orc.synth_chirp(total, fs, c, 3, np.float64) for c in range(3)]) + 0.01 * rng.standard_normal((3, total))
    plan = _plan_with_all(n, fs, order, np.float64, channels=2)
    pipe = stream.StreamPipeline(plan, host, hop, block=2, transforms=("cwt", "stx"))
    assert len(pipe.items) == 2 * 4 and [it[3] for it in pipe.items[:4]] == [0, hop, 2 * hop, total - n]
    got = list(pipe.run())
    assert [g.index for g in got] == list(range(8))
    for g in got:
        x = torch.from_numpy(host[g.first_channel : g.first_channel + g.channels, g.start : g.start + n]).cuda()
        ref_c, ref_s = plan.cwt_stx(x, coef=False, reductions=True)
        for mine, ref in ((g.cwt, ref_c), (g.stx, ref_s)):
            assert torch.equal(mine.power_band, ref.power_band) and torch.equal(mine.stats, ref.stats)
            assert torch.equal(mine.power_time, ref.power_time)
    # against the oracle for one item (chunk 1 of channel 2, a few bands)
    g = got[5]
    assert (g.first_channel, g.chunk) == (2, 1)
    pick = [0, 20, 47]
    _, _, want = orc.cwt_fft(order, host[2, g.start : g.start + n], fs, bands=pick)
    assert np.allclose(g.cwt.power_band[0, pick].cpu().numpy(), (np.abs(want) ** 2).sum(axis=1), rtol=1e-9)
    # two ranks: contiguous shares of the item list; a restarted run
    a = [(i.first_channel, i.chunk) for i in pipe.run(rank=0, world=2)]
    b = [(i.first_channel, i.chunk) for i in pipe.run(rank=1, world=2)]
    assert a + b == [(i.first_channel, i.chunk) for i in got] and len(a) == 4
    again = list(pipe.run(first_item=6))
    assert [i.index for i in again] == [6, 7] and torch.equal(again[1].stx.power_band, got[7].stx.power_band)
    lean = stream.StreamPipeline(plan, host, hop, block=3, transforms=("stx",), keep_time=False)
    first = next(iter(lean.run()))
    assert first.cwt is None and first.stx.power_time is None and first.stx.power_band.shape == (3, 48)
    plan.close()


@pytest.mark.parametrize("name,kw", [
    ("lin", dict(frequency_min=20.0, frequency_max=400.0, frequency_step=20.0)),
    ("geo", dict(scale_order_input=3.0, frequency_min=10.0, frequency_max=450.0, is_geometric=True)),
    ("inferno", dict(scale_order_input=3.0, frequency_min=8.0, frequency_max=400.0, is_geometric=True, is_inferno=True)),
    ("qpr", dict(frequency_min=25.0, frequency_max=300.0, frequency_step=25.0, factor_q=0.5, power_p=1.0, power_r=0.75)),
])
def test_general_stockwell_vs_reference(golden, name, kw):
    """styx_stx.tfr_stx_fft: band / bin selection bit-exact, coefficients to the float64 tolerance."""
    g = golden("stx_general_n1024.npz")
    tfr, psd, f, f_fft, win = styx_stx.tfr_stx_fft(g["sig"], 1 / 1000.0, n_fft_in=1024, **kw)
    assert np.array_equal(f, g[f"{name}_f"]) and np.array_equal(f_fft, g[f"{name}_ffft"])
    assert relmax(tfr, g[f"{name}_tfr"]) <= 1e-11
    assert np.allclose(psd[0], g[f"{name}_psd_row0"], rtol=1e-8, atol=1e-12 * psd.max())
    assert relmax(win[[0, len(f) - 1]], g[f"{name}_win_rows"]) <= 1e-12
    # the padding path the reference documents but cannot run (TypeError upstream): 1000 samples padded to 1024
    short = g["sig"][:1000]
    t2 = styx_stx.tfr_stx_fft(short, 1 / 1000.0, n_fft_in=1024, **kw)[0]
    ref = orc.stx_general(np.concatenate([short, np.zeros(24)]), 1 / 1000.0, **{
        dict(scale_order_input="order", frequency_min="f_min", frequency_max="f_max", frequency_step="f_step",
             factor_q="q", power_p="p", power_r="r", is_geometric="geometric", is_inferno="inferno")[k]: v
        for k, v in kw.items()})[0][:, :1000]
    assert t2.shape == ref.shape and relmax(t2, ref) <= 1e-11


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_welch_vs_reference(golden, dtype):
    """styx_fft.welch_power_pow2."""
    g = golden("stft.npz")
    sig = g[f"sig_n13_fs1000_{dtype}"]
    tol = 1e-11 if dtype == "float64" else 2e-5
    f, p = styx_fft.welch_power_pow2(sig, 1000.0, 512)
    assert np.array_equal(f, g[f"welch_f_{dtype}"]) and p.dtype == g[f"welch_p_{dtype}"].dtype
    assert relmax(p, g[f"welch_p_{dtype}"]) <= tol
    _, p2 = styx_fft.welch_power_pow2(sig, 1000.0, 300, nfft_points=512, overlap_points=100, alpha=0.5)
    assert relmax(p2, g[f"welch2_p_{dtype}"]) <= tol
    _, pb = styx_fft.welch_power_pow2(np.stack([sig, 2 * sig]), 1000.0, 512)
    assert pb.shape == (2, 257) and relmax(pb[1], 4 * g[f"welch_p_{dtype}"]) <= tol
    with pytest.raises(ValueError):
        styx_fft.welch_power_pow2(sig[:100], 1000.0, 512)


@pytest.mark.parametrize("order,fs", [(6, 800.0), (12, 1000.0), (1, 1000.0)])
def test_native_engines_other_band_tables(order, fs):
    """Band tables with other populations of the three native sub-engines (zoom classes, block reach groups, two-pass)
    than the benchmark's order 3: the native engine against the hipFFT engine on the same noise + chirp record,
    n = 2^20, coefficients, bits and every fused reduction; per-band power also as a direct sum of the stored panel; nine
    bands spread over each table against the oracle."""
    from quantum_inferno_amd import _lib

    n = 1 << 20
    rng = np.random.default_rng(1234 + int(order))
    x = (orc.synth_chirp(n, fs, 0, 1, np.float32) + 0.25 * rng.standard_normal(n).astype(np.float32))[None, :]
    xt = torch.from_numpy(x).cuda()
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order))
    ws = engine.TfrPlan.workspace_for(n, nb, np.float32, 1)
    nat = engine.TfrPlan(n, np.float32, None, ws, _lib.QI_ENGINE_NATIVE)
    ref = engine.TfrPlan(n, np.float32, None, ws, _lib.QI_ENGINE_HIPFFT)
    for plan in (nat, ref):
        plan.set_styx_bank(order, fs)
        plan.set_stx_bands(order, fs)
    for name in ("cwt", "stx"):
        a = getattr(nat, name)(xt, coef=True, bits=True, reductions=True)
        b = getattr(ref, name)(xt, coef=True, bits=True, reductions=True)
        scale = float(b.coef.abs().max())
        worst = float((a.coef - b.coef).abs().amax(dim=2).max()) / scale
        assert worst <= 2e-5, (name, order, worst)
        big = b.coef.abs() >= 1e-2 * scale
        assert float((a.bits - b.bits).abs()[big].max()) <= 1e-3, (name, order)
        assert torch.allclose(a.power_band, b.power_band, rtol=1e-4, atol=1e-9 * float(b.power_band.max()))
        assert torch.allclose(a.power_time, b.power_time, rtol=1e-3, atol=1e-6 * float(b.power_time.max()))
        assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=1e-4)
        direct = (a.coef.abs().double() ** 2).sum(dim=2)
        assert torch.allclose(a.power_band, direct, rtol=1e-5, atol=1e-9 * float(direct.max()))
        # ... and against the ORACLE on bands spread over the table (every engine's share of it)
        pick = sorted({0, 1, nb // 5, (2 * nb) // 5, nb // 2, (3 * nb) // 5, (4 * nb) // 5, nb - 2, nb - 1})
        _, _, want = (orc.cwt_fft if name == "cwt" else orc.stx_fft)(order, x[0].astype(np.float64), fs, bands=pick)
        got = a.coef[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        for i, j in enumerate(pick):
            assert np.max(np.abs(got[i] - want[i])) <= 2e-5 * np.max(np.abs(want[i])), (name, order, j)
        del a, b
    nat.close()
    ref.close()


def test_native_split_bands_of_the_benchmark_table():
    """The two lowest bands of the order-3 styx table at n = 2^20 have atoms longer than the record (the reference cuts
    them off at |x| = n / 2, styx_cwt.py:113-144).  The native engine runs them as a tapered band on the zoom engine
    plus edge items in the block launch, and nothing of the table is left for the two-pass kernels: every row against
    the hipFFT engine (the reference's own algorithm), with and without a stored panel."""
    from quantum_inferno_amd import _lib

    n, fs, order = 1 << 20, 1000.0, 3
    rng = np.random.default_rng(77)
    # noise up to the record ends: the edge pieces weigh the samples half a record away from each output
    x = (orc.synth_chirp(n, fs, 0, 1, np.float32) + 0.5 * rng.standard_normal(n).astype(np.float32))[None, :]
    xt = torch.from_numpy(x).cuda()
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order))
    ws = engine.TfrPlan.workspace_for(n, nb, np.float32, 1)
    nat = engine.TfrPlan(n, np.float32, None, ws, _lib.QI_ENGINE_NATIVE)
    ref = engine.TfrPlan(n, np.float32, None, ws, _lib.QI_ENGINE_HIPFFT)
    for plan in (nat, ref):
        plan.set_styx_bank(order, fs)
    if "QI_NATIVE_SPLIT" not in os.environ and "QI_NATIVE_ZOOM" not in os.environ and "QI_NATIVE_BLOCK" not in os.environ:
        assert nat.stage_bands("pass2")[0] == 0  # zoom + block engines produce all 48 bands
        assert nat.stage_bands("zoom")[0] + nat.stage_bands("block")[0] == nb
    a = nat.cwt(xt, coef=True, bits=True, reductions=True)
    b = ref.cwt(xt, coef=True, bits=True, reductions=True)
    for row in range(nb):  # per row: the two split bands are the weakest rows of the panel
        scale = float(b.coef[0, row].abs().max())
        assert float((a.coef[0, row] - b.coef[0, row]).abs().max()) <= 2e-5 * scale, row
    big = b.coef.abs() >= 1e-2 * float(b.coef.abs().max())
    assert float((a.bits - b.bits).abs()[big].max()) <= 1e-3
    assert torch.allclose(a.power_band, b.power_band, rtol=1e-4, atol=1e-9 * float(b.power_band.max()))
    assert torch.allclose(a.power_time, b.power_time, rtol=1e-3, atol=1e-6 * float(b.power_time.max()))
    assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=1e-4)
    r = nat.cwt(xt, coef=False, bits=False, reductions=True)  # reductions only: the split bands still meet in a scratch row
    assert torch.equal(r.power_band, a.power_band) and torch.equal(r.power_time, a.power_time)
    assert torch.equal(r.stats, a.stats)
    nat.close()
    ref.close()


def test_fused_cwt_stx_call_matches_separate_calls():
    """qi_cwt_stx (both transforms of the same records in one call, the Stockwell bands formed from the even bins of
    the CWT's zero-padded spectrum, the block bands of both from one forward transform per block in a joint launch)
    against qi_cwt followed by qi_stx: both panels agree to float rounding (the zoom bands of the CWT are the same
    launches: bit-equal); a second fused call reproduces the first bit for bit."""
    n, fs, order = 1 << 20, 1000.0, 3
    x = torch.from_numpy(np.stack([orc.synth_chirp(n, fs, c, 2, np.float32) for c in range(2)])).cuda()
    plan = _plan_with_all(n, fs, order, np.float32, channels=2)
    sep_c = plan.cwt(x, coef=True, reductions=True)
    sep_s = plan.stx(x, coef=True, reductions=True)
    fus_c, fus_s = plan.cwt_stx(x, coef=True, reductions=True)
    for fus, sep in ((fus_c, sep_c), (fus_s, sep_s)):
        scale = float(sep.coef.abs().max())
        assert float((fus.coef - sep.coef).abs().max()) / scale <= 2e-6
        assert torch.allclose(fus.power_band, sep.power_band, rtol=1e-5)
        assert torch.allclose(fus.power_time, sep.power_time, rtol=1e-4, atol=1e-7 * float(sep.power_time.max()))
        assert torch.allclose(fus.stats[:, :3], sep.stats[:, :3], rtol=1e-5)
    assert torch.equal(fus_c.coef[:, 2:8], sep_c.coef[:, 2:8])  # zoom bands of the CWT: the same launches
    again_c, again_s = plan.cwt_stx(x, coef=True, reductions=True)
    assert torch.equal(again_s.coef, fus_s.coef) and torch.equal(again_s.reduced, fus_s.reduced)
    assert torch.equal(again_c.coef, fus_c.coef) and torch.equal(again_c.reduced, fus_c.reduced)
    # a plain Stockwell call after the fused one stands on its own forward transform again
    sep2 = plan.stx(x, coef=True, reductions=True)
    assert torch.equal(sep2.coef, sep_s.coef)
    plan.close()


def test_staged_result_copy_is_bit_equal(monkeypatch):
    """engine.finish for results above PINNED_RESULT_MAX_BYTES: the copy through the two fixed page-locked staging buffers
    (many pieces, an odd tail) equals a plain device-to-host copy bit for bit, for every result dtype; two threads at once do
    not disturb each other (the staging buffers are shared under a lock)."""
    import threading

    monkeypatch.setattr(engine, "PINNED_RESULT_MAX_BYTES", 1 << 20)
    monkeypatch.setattr(engine, "STAGE_PIECE_BYTES", 3 << 20)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for dtype in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        t = torch.randn((3, 7, 100003), dtype=dtype, device="cuda", generator=gen)
        got = engine.finish(t, True, False)
        assert isinstance(got, np.ndarray) and got.shape == tuple(t.shape) and np.array_equal(got, t.cpu().numpy())
    wide = engine.finish(torch.randn((2, 5, 70001), dtype=torch.complex64, device="cuda", generator=gen), True, True, widen=True)
    assert wide.dtype == np.complex128 and wide.shape == (5, 70001)
    with pytest.raises(TypeError):
        engine._staged_copy(torch.zeros(4, dtype=torch.bfloat16, device="cuda"))
    a = torch.randn((4, 1 << 20), dtype=torch.float64, device="cuda", generator=gen)
    b = torch.randn((4, 1 << 20), dtype=torch.float64, device="cuda", generator=gen)
    out = {}

    def work(key, t):
        torch.cuda.set_device(0)
        out[key] = [engine.finish(t, True, False) for _ in range(3)]

    threads = [threading.Thread(target=work, args=(k, t)) for k, t in (("a", a), ("b", b))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for key, t in (("a", a), ("b", b)):
        ref = t.cpu().numpy()
        assert all(np.array_equal(r, ref) for r in out[key])


def test_plan_desc_flags_are_reserved():
    """qi_plan_desc.flags is reserved (round 4's experimental graph mode left the library): anything but 0 is refused, so a C
    caller that leaves garbage in the field gets an error instead of a silent mode switch."""
    import ctypes as C

    from quantum_inferno_amd import _lib

    lib = _lib.require_gpu()
    handle = C.c_void_p()
    for flags, ok in ((0, True), (1, False), (0x40000000, False)):
        desc = _lib.PlanDesc(n=4096, dtype=_lib.QI_F32, device=torch.cuda.current_device(), engine=_lib.QI_ENGINE_AUTO, flags=flags,
                             workspace_bytes=1 << 24)
        rc = lib.qi_plan_create(C.byref(handle), C.byref(desc))
        assert (rc == 0) == ok, (flags, rc)
        if ok:
            assert lib.qi_plan_destroy(handle) == 0
        else:
            with pytest.raises(_lib.QiError, match="reserved"):
                _lib.check(rc)


def test_plan_ring_matches_single_plan():
    """PlanRing: independent records on alternating plans / streams give the results of one plan on one stream, bit for
    bit, and every result carries the event that follows its launches."""
    n, fs, order = 1 << 18, 1000.0, 3
    recs = [torch.from_numpy(orc.synth_chirp(n, fs, c, 5, np.float32)).cuda().unsqueeze(0) for c in range(5)]
    plan = _plan_with_all(n, fs, order, np.float32)
    want = []
    for r in recs:
        c, s = plan.cwt_stx(r, coef=True, reductions=True)
        want.append((c.coef.clone(), s.coef.clone(), c.reduced.clone(), s.reduced.clone()))
    plan.close()
    ring = qi.PlanRing(n, torch.float32, setup=lambda p: (p.set_styx_bank(order, fs), p.set_stx_bands(order, fs)), depth=2)
    for i, r in enumerate(recs):
        c, s, done = ring.cwt_stx(r, coef=True, reductions=True)
        done.synchronize()
        assert torch.equal(c.coef, want[i][0]) and torch.equal(s.coef, want[i][1]), i
        assert torch.equal(c.reduced, want[i][2]) and torch.equal(s.reduced, want[i][3]), i
    # two calls in flight: both slots' results are intact after their events
    c0, s0, d0 = ring.cwt_stx(recs[0], coef=True, reductions=True)
    c1, s1, d1 = ring.cwt_stx(recs[1], coef=True, reductions=True)
    d0.synchronize()
    d1.synchronize()
    assert torch.equal(c0.coef, want[0][0]) and torch.equal(s1.coef, want[1][1])
    ring.close()


def test_fused_call_other_requests_and_tiles():
    """qi_cwt_stx beyond the benchmark's request: reductions only and coefficients + bits through the joint launches
    (the reductions do not depend on which panels are stored: bit-equal), the two transforms asking for different
    panels (joint launches where the kernels allow, else one after the other), and a workspace that holds one record
    at a time (no joint launches: the plain sequence)."""
    n, fs, order = 1 << 20, 1000.0, 3
    x = torch.from_numpy(np.stack([orc.synth_chirp(n, fs, c, 2, np.float32) for c in range(2)])).cuda()
    plan = _plan_with_all(n, fs, order, np.float32, channels=2)
    full_c, full_s = plan.cwt_stx(x, coef=True, bits=True, reductions=True)
    red_c, red_s = plan.cwt_stx(x, coef=False, bits=False, reductions=True)
    for full, red in ((full_c, red_c), (full_s, red_s)):
        assert torch.equal(full.reduced, red.reduced)
    sep_c = plan.cwt(x, coef=True, bits=True, reductions=True)
    big = sep_c.coef.abs() >= 1e-2 * float(sep_c.coef.abs().max())
    assert float((full_c.bits - sep_c.bits).abs()[big].max()) <= 1e-5
    assert float((full_c.coef - sep_c.coef).abs().max()) <= 2e-6 * float(sep_c.coef.abs().max())
    # different requests on the two sides of one call (C ABI only: the wrapper passes the same flags to both)
    import ctypes as C
    from quantum_inferno_amd import _lib
    res_c, desc_c = plan._outputs(_lib.QI_BANK_STYX, 2, True, False, True, 1.0, 0.0, None, None)
    res_s, desc_s = plan._outputs(_lib.QI_TABLE_STX, 2, False, False, True, 1.0, 0.0, None, None)
    _lib.check(plan._lib.qi_cwt_stx(plan._handle, _lib.QI_BANK_STYX, _lib.ptr(x), 2, C.byref(desc_c), C.byref(desc_s),
                                    plan._stream()))
    torch.cuda.synchronize()
    for res, full in ((res_c, full_c), (res_s, full_s)):  # (other kernels than the joint ones: float rounding)
        assert torch.allclose(res.power_band, full.power_band, rtol=1e-5)
        assert torch.allclose(res.power_time, full.power_time, rtol=1e-4, atol=1e-7 * float(full.power_time.max()))
        assert torch.allclose(res.stats[:, :3], full.stats[:, :3], rtol=1e-5)
    assert float((res_c.coef - full_c.coef).abs().max()) <= 2e-6 * float(full_c.coef.abs().max())
    plan.close()
    small = _plan_with_all(n, fs, order, np.float32, workspace=260 << 20)  # one record's scratch, not two
    one_c, one_s = small.cwt_stx(x, coef=True, reductions=True)
    for one, full in ((one_c, full_c), (one_s, full_s)):
        assert float((one.coef - full.coef).abs().max()) <= 2e-6 * float(full.coef.abs().max())
        assert torch.allclose(one.power_band, full.power_band, rtol=1e-5)
        assert torch.allclose(one.stats[:, :3], full.stats[:, :3], rtol=1e-5)
    small.close()


@pytest.mark.parametrize("log2n,order", [(14, 3), (14, 12), (15, 3), (15, 12), (16, 3), (17, 3), (16, 12), (17, 6), (18, 3), (19, 3), (21, 3), (22, 3), (19, 12), (21, 12), (21, 6)])
def test_native_engine_other_lengths(log2n, order):
    """Stockwell transform and styx CWT at the other power-of-two lengths the native engine takes (their order-3 band
    tables need only the zoom and block engines -- the CWT's longest atoms as split bands -- which are not tied to the
    two-pass kernels' 2^20 / 2^21) against the hipFFT engine: every row, the fused reductions, and the fused call; seven
    bands of each table (split / zoom / block engine) against the oracle."""
    from quantum_inferno_amd import _lib

    n, fs = 1 << log2n, 1000.0
    rng = np.random.default_rng(log2n)
    x = orc.synth_chirp(n, fs, 0, 1, np.float32) + 0.25 * rng.standard_normal(n).astype(np.float32)
    x = torch.from_numpy(x[None, :]).cuda()
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order))
    ws = engine.TfrPlan.workspace_for(n, nb, np.float32, 1)
    nat = engine.TfrPlan(n, np.float32, None, ws, _lib.QI_ENGINE_AUTO)
    ref = engine.TfrPlan(n, np.float32, None, ws, _lib.QI_ENGINE_HIPFFT)
    for plan in (nat, ref):
        plan.set_stx_bands(order, fs)
        plan.set_styx_bank(order, fs)
    knobs = any(k in os.environ for k in ("QI_NATIVE_ZOOM", "QI_NATIVE_BLOCK", "QI_NATIVE_SPLIT"))  # (they move bands to the two-pass kernels)
    for which, name in ((2, "stx"), (0, "cwt")):
        a = getattr(nat, name)(x, coef=True, reductions=True)
        b = getattr(ref, name)(x, coef=True, reductions=True)
        for row in range(nb):
            scale = float(b.coef[0, row].abs().max())
            assert float((a.coef[0, row] - b.coef[0, row]).abs().max()) <= 2e-5 * scale, (name, row)
        assert torch.allclose(a.power_band, b.power_band, rtol=1e-4, atol=1e-9 * float(b.power_band.max()))
        assert torch.allclose(a.power_time, b.power_time, rtol=1e-3, atol=1e-6 * float(b.power_time.max()))
        assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=1e-4)
        # ... and against the ORACLE (float64 arithmetic on the same float32 record) on bands of every engine: the
        # lowest (split / zoom), the middle (zoom) and the highest (block) of the table
        pick = sorted({0, 1, nb // 3, nb // 2, (2 * nb) // 3, nb - 2, nb - 1})
        _, _, want = (orc.cwt_fft if name == "cwt" else orc.stx_fft)(order, x[0].cpu().numpy().astype(np.float64), fs, bands=pick)
        got = a.coef[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        for i, j in enumerate(pick):
            assert np.max(np.abs(got[i] - want[i])) <= 2e-5 * np.max(np.abs(want[i])), (log2n, name, j)
        assert np.allclose(a.power_band[0][torch.tensor(pick, device="cuda")].cpu().numpy(), (np.abs(want) ** 2).sum(axis=1), rtol=2e-4)
        if not knobs:
            assert nat.stage_bands("zoom")[which] + nat.stage_bands("block")[which] == nb  # the native engine did run
        if name == "cwt":
            fc, fs_ = nat.cwt_stx(x, coef=True, reductions=True)
            assert float((fc.coef - a.coef).abs().max()) <= 2e-6 * float(a.coef.abs().max())  # (joint block launch)
            assert float((fs_.coef - nat.stx(x, coef=True).coef).abs().max()) <= 2e-5 * float(fs_.coef.abs().max())
        del a, b
    nat.close()
    ref.close()


@pytest.mark.parametrize("log2n,order", [(19, 3), (19, 12), (21, 3)])
def test_native_engine_batch_launches_other_lengths(log2n, order):
    """Calls of four (order 3: eight) records and more use other launch geometry than single records: 8192-sample long blocks for the
    1024-reach block bands, twelve bands per block workgroup, the 6- / 4-tap zoom classes, the gather inside the coarse
    kernel.  At lengths other than the benchmark's: a five-record joint call against the single-record call of one of
    its records (the other geometry of the same arithmetic) and against the hipFFT engine, every row."""
    from quantum_inferno_amd import _lib

    n, fs = 1 << log2n, 800.0
    C = 9 if order == 3 else 5  # (the batch geometry starts at 8 records for the few block bands of an order-3 table, at 4 otherwise)
    rng = np.random.default_rng(100 + log2n + order)
    x = np.stack([orc.synth_chirp(n, fs, c, C, np.float32) for c in range(C)]) + 0.1 * rng.standard_normal((C, n)).astype(np.float32)
    x = torch.from_numpy(x).cuda()
    nat = _plan_with_all(n, fs, order, np.float32, channels=C)
    nb = len(nat.freq[0])
    ref = engine.TfrPlan(n, np.float32, None, engine.TfrPlan.workspace_for(n, nb, np.float32, 1), _lib.QI_ENGINE_HIPFFT)
    ref.set_styx_bank(order, fs)
    ref.set_stx_bands(order, fs)
    pick = 3
    batch = nat.cwt_stx(x, coef=True, reductions=True)
    one = nat.cwt_stx(x[pick : pick + 1], coef=True, reductions=True)
    for name, b, o in (("cwt", batch[0], one[0]), ("stx", batch[1], one[1])):
        gold = getattr(ref, name)(x[pick : pick + 1], coef=True, reductions=True)
        peak = gold.coef[0].abs().amax(dim=1)
        err_one = (b.coef[pick] - o.coef[0]).abs().amax(dim=1) / peak
        err_ref = (b.coef[pick] - gold.coef[0]).abs().amax(dim=1) / peak
        assert float(err_one.max()) <= 1e-5, (name, int(err_one.argmax()), float(err_one.max()))
        assert float(err_ref.max()) <= 2e-5, (name, int(err_ref.argmax()), float(err_ref.max()))
        assert torch.allclose(b.power_band[pick], gold.power_band[0], rtol=1e-4, atol=1e-9 * float(gold.power_band.max()))
        assert torch.allclose(b.power_time[pick], gold.power_time[0], rtol=1e-3, atol=1e-6 * float(gold.power_time.max()))
        assert torch.allclose(b.stats[pick, :3], gold.stats[0, :3], rtol=1e-4)
        del gold
    nat.close()
    ref.close()


@pytest.mark.parametrize("tag,dtype", [("f64", np.float64), ("f32", np.float32), ("f64_odd", np.float64)])
def test_shannon_1d_family_vs_reference(golden, tag, dtype):
    """1-D Shannon TDR / FFT (tfr_info.py:97-200) against the reference's outputs (tests/golden/shannon1d.npz)."""
    g = golden("shannon1d.npz")
    sig = g[f"sig_{tag}"]
    assert sig.dtype == dtype
    tdr, fft = tfr_info.shannon_tdr_fft(sig)
    rel = 1e-12 if dtype == np.float64 else 2e-6
    assert tdr.sig.dtype == dtype and fft.marginal.dtype == dtype
    np.testing.assert_allclose(tdr.sig, g[f"tdr_sig_{tag}"], rtol=rel, atol=rel * np.abs(g[f"tdr_sig_{tag}"]).max())
    np.testing.assert_allclose(fft.sig, g[f"fft_sig_{tag}"], rtol=0, atol=rel * 10 * np.abs(g[f"fft_sig_{tag}"]).max())
    np.testing.assert_array_equal(fft.frequency, g[f"fft_frequency_{tag}"])
    # unwrapped phase: every bin of the chirp + noise record is far above rounding, so the 2 pi decisions agree
    np.testing.assert_allclose(fft.angle_rads, g[f"fft_angle_{tag}"], rtol=0, atol=1e-8 if dtype == np.float64 else 2e-2)
    if dtype == np.float32:  # the reference's float32 cumulative sum drifts; modulo 2 pi the phases agree closely
        d = np.angle(np.exp(1j * (fft.angle_rads.astype(np.float64) - g[f"fft_angle_{tag}"].astype(np.float64))))
        assert np.abs(d).max() <= 2e-3
    for name, obj in (("tdr", tdr), ("fft", fft)):
        m = g[f"{name}_marginal_{tag}"]
        np.testing.assert_allclose(obj.marginal, m, rtol=10 * rel, atol=rel * m.max())
        # info = -log2(m + eps32): compared where the marginal is not below the epsilon floor's rounding
        np.testing.assert_allclose(obj.info, g[f"{name}_info_{tag}"], rtol=0, atol=1e-9 if dtype == np.float64 else 2e-4)
        np.testing.assert_allclose(obj.entropy, g[f"{name}_entropy_{tag}"], rtol=1e-9 if dtype == np.float64 else 1e-4,
                                   atol=rel * g[f"{name}_entropy_{tag}"].max())
        assert obj.ref_entropy == float(g[f"{name}_ref_entropy_{tag}"])
        np.testing.assert_allclose(obj.isnr, g[f"{name}_isnr_{tag}"], rtol=0, atol=1e-9 if dtype == np.float64 else 2e-4)
        np.testing.assert_allclose(obj.esnr, g[f"{name}_esnr_{tag}"], rtol=1e-9 if dtype == np.float64 else 1e-4,
                                   atol=10 * rel * g[f"{name}_esnr_{tag}"].max())
    # batched records through the same kernels: every record equals its single-record run (records of different energy,
    # so a partial sum or an unwrap carry taken from the wrong record shows)
    other = 0.5 * sig[::-1] + 0.25 * sig
    assert other.dtype == dtype
    both_t, both_f = tfr_info.ShannonTDR(np.stack([sig, other])), tfr_info.ShannonFFT(np.stack([sig, other]))
    one_t, one_f = tfr_info.ShannonTDR(other), tfr_info.ShannonFFT(other)
    for k, (t_ref, f_ref) in enumerate(((tdr, fft), (one_t, one_f))):
        np.testing.assert_array_equal(both_t.marginal[k], t_ref.marginal)
        np.testing.assert_array_equal(both_t.sig[k], t_ref.sig)
        np.testing.assert_array_equal(both_f.marginal[k], f_ref.marginal)
        np.testing.assert_array_equal(both_f.angle_rads[k], f_ref.angle_rads)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_short_time_fft_wrappers_vs_reference(golden, dtype):
    """utilities/short_time_fft.py: stft_tukey, spectrogram_tukey (every padding mode, both scalings) and istft_tukey
    against the reference's outputs (tests/golden/short_time_fft.npz)."""
    from quantum_inferno_amd.utilities import short_time_fft as stf

    g = golden("short_time_fft.npz")
    sig = g["sig"].astype(dtype)
    tol = 1e-11 if dtype == np.float64 else 2e-5
    for line in g["cases"]:
        tag, fs, alpha, seg, ov, scaling, padding = str(line).split(",")
        fs, alpha, seg, ov = float(fs), float(alpha), int(seg), int(ov)
        obj = stf.get_stft_object_tukey(fs, alpha, seg, ov, scaling)
        assert [obj.p_min, obj.p_max(len(sig)), obj.hop, obj.mfft, obj.m_num_mid] == list(g[f"geom_{tag}"])
        f, t, mag = stf.stft_tukey(sig, fs, alpha, seg, ov, scaling, padding)
        assert np.array_equal(f, g[f"f_{tag}"]) and np.array_equal(t, g[f"t_{tag}"])
        assert mag.dtype == dtype and relmax(mag, g[f"mag_{tag}"]) <= tol, (tag, relmax(mag, g[f"mag_{tag}"]))
        _, _, sxx = stf.spectrogram_tukey(sig, fs, alpha, seg, ov, scaling, padding)
        assert relmax(sxx, g[f"sxx_{tag}"]) <= 2 * tol, tag
        cdt = np.complex128 if dtype == np.float64 else np.complex64
        ts, x = stf.istft_tukey(g[f"S_{tag}"].astype(cdt), fs, alpha, seg, ov, scaling)
        assert np.array_equal(ts, g[f"ts_{tag}"]) and relmax(x, g[f"x_{tag}"]) <= 10 * tol, (tag, relmax(x, g[f"x_{tag}"]))
    # a batch of records (of different energy) through the same kernels: every record equals its single-record run
    other = 0.5 * sig[::-1] + 0.25 * sig
    two = stf.stft_tukey(np.stack([sig, other]), 800.0, 0.25, 256, 128)[2]
    assert np.array_equal(two[0], stf.stft_tukey(sig, 800.0, 0.25, 256, 128)[2])
    assert np.array_equal(two[1], stf.stft_tukey(other, 800.0, 0.25, 256, 128)[2])

@pytest.mark.parametrize("dtype,seg,ov,log2n", [(np.float32, 2048, 1024, 17), (np.float32, 1024, 768, 16), (np.float32, 4096, 2048, 17),
                                                (np.float64, 2048, 1024, 16), (np.float64, 512, 384, 15), (np.float32, 300, 150, 15)])
def test_sliding_stft_istft_round_trip(dtype, seg, ov, log2n):
    """ShortTimeFFT's convention, forward then inverse (qi_sliding_stft with the complex output, istft_tukey): with the
    canonical dual window the record comes back, at shapes of the benchmark's size -- the fused inverse kernel's halo of 1
    and 3 slices, both precisions, 4096-point transforms, and a transform length that is not a power of two (the
    three-kernel path) for comparison."""
    from quantum_inferno_amd import _lib
    from quantum_inferno_amd.utilities import short_time_fft as stf

    lib = _lib.require_gpu()
    n, fs = 1 << log2n, 1000.0
    rng = np.random.default_rng(seg + ov)
    x = (orc.synth_chirp(n, fs, 0, 1, np.float64) + 0.3 * rng.standard_normal(n)).astype(dtype)
    obj = stf.get_stft_object_tukey(fs, 0.25, seg, ov, "magnitude")
    xt = torch.from_numpy(np.stack([x, x[::-1].copy()])).cuda()
    p0, p1 = obj.p_min, obj.p_max(n)
    n_slices, first = p1 - p0, p0 * obj.hop - obj.m_num_mid
    cdt = torch.complex64 if dtype == np.float32 else torch.complex128
    code = _lib.QI_F32 if dtype == np.float32 else _lib.QI_F64
    win = torch.from_numpy(obj.win).to(device="cuda", dtype=xt.dtype)
    z = torch.empty((2, obj.f_pts, n_slices), dtype=cdt, device="cuda")
    nbytes = int(lib.qi_sliding_scratch_bytes(code, 2, obj.mfft, n_slices))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.qi_sliding_stft(code, 0, _lib.ptr(xt), 2, n, _lib.ptr(win), obj.m_num, obj.hop, obj.mfft, first, n_slices, 0, 0,
                                   obj.m_num_mid, _lib.ptr(z), None, 1, _lib.ptr(scratch), nbytes, _lib.stream_ptr(xt.device)))
    ts, back = stf.istft_tukey(z, fs, 0.25, seg, ov, "magnitude")
    k1 = back.shape[1]
    assert k1 == (n_slices - 1) * obj.hop and k1 >= n - seg
    m = min(k1, n)
    err = float((back[:, :m] - xt[:, :m]).abs().max()) / float(xt.abs().max())
    assert err <= (2e-5 if dtype == np.float32 else 1e-12), (seg, ov, err)

@pytest.mark.parametrize("dtype,log2n,order", [(np.float32, 16, 1), (np.float32, 18, 2), (np.float64, 16, 1), (np.float64, 17, 2)])
def test_stockwell_rows_behind_the_native_run(dtype, log2n, order):
    """Order-1 / order-2 Stockwell tables at lengths other than 2^19 / 2^20: the top band's frequency window is cut at the
    Nyquist bins, no native engine takes it there, and (round 4) the native run leaves that row to a pass of the hipFFT
    engine over just it -- the whole table had gone to the hipFFT engine before.  Every row and every reduction against the
    hipFFT engine, the last rows against the oracle, through stx, cwt_stx and the reductions-only call."""
    from quantum_inferno_amd import _lib

    n, fs = 1 << log2n, 1000.0
    rng = np.random.default_rng(log2n + int(order))
    x = np.stack([orc.synth_chirp(n, fs, c, 2, np.float64) for c in range(2)]) + 0.2 * rng.standard_normal((2, n))
    x = x.astype(dtype)
    xt = torch.from_numpy(x).cuda()
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order))
    ws = engine.TfrPlan.workspace_for(n, nb, dtype, 2)
    nat = engine.TfrPlan(n, dtype, None, ws, _lib.QI_ENGINE_AUTO)
    ref = engine.TfrPlan(n, dtype, None, ws, _lib.QI_ENGINE_HIPFFT)
    for plan in (nat, ref):
        plan.set_styx_bank(order, fs)
        plan.set_stx_bands(order, fs)
    native_rows = nat.stage_bands("zoom")[2] + nat.stage_bands("block")[2]
    assert 0 < native_rows < nb and nb - native_rows <= 4  # (the zoom and block engines ran all but the last rows)
    a = nat.stx(xt, coef=True, bits=True, reductions=True)
    b = ref.stx(xt, coef=True, bits=True, reductions=True)
    f64 = dtype == np.float64
    for row in range(nb):
        scale = float(b.coef[:, row].abs().max())
        assert float((a.coef[:, row] - b.coef[:, row]).abs().max()) <= (5e-9 if f64 else 2e-5) * scale, row
    assert torch.allclose(a.power_band, b.power_band, rtol=1e-9 if f64 else 1e-4)
    assert torch.allclose(a.power_time, b.power_time, rtol=1e-8 if f64 else 1e-3, atol=(1e-11 if f64 else 1e-6) * float(b.power_time.max()))
    assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=1e-9 if f64 else 1e-4)
    big = b.coef.abs() >= 1e-2 * float(b.coef.abs().max())
    assert float((a.bits - b.bits).abs()[big].max()) <= (1e-9 if f64 else 1e-3)
    pick = [nb - 3, nb - 2, nb - 1]
    _, _, want = orc.stx_fft(order, x[1].astype(np.float64), fs, bands=pick)
    got = a.coef[1][torch.tensor(pick, device="cuda")].cpu().numpy()
    for i, j in enumerate(pick):
        assert np.max(np.abs(got[i] - want[i])) <= (5e-9 if f64 else 2e-5) * np.max(np.abs(want[i])), j
    # the joint call and the reductions-only call take the same route
    fc, fs_ = nat.cwt_stx(xt, coef=True, reductions=True)
    assert float((fs_.coef - a.coef).abs().max()) <= (1e-12 if f64 else 2e-6) * float(a.coef.abs().max())
    assert torch.allclose(fs_.power_band, a.power_band, rtol=1e-12 if f64 else 1e-5)
    lean = nat.stx(xt, coef=False, reductions=True)
    assert lean.coef is None and torch.allclose(lean.power_band, a.power_band, rtol=1e-12 if f64 else 1e-5)
    assert torch.allclose(lean.stats[:, :3], a.stats[:, :3], rtol=1e-12 if f64 else 1e-5)
    nat.close()
    ref.close()


@pytest.mark.parametrize("dtype,n,order", [(np.float32, 1 << 18, 3), (np.float64, 1 << 16, 6), (np.float32, 3000, 3), (np.float64, 1 << 20, 12)])
def test_band_only_reductions_match_full(dtype, n, order):
    """reductions="band" (what the streaming pipeline asks for when no per-time power is kept: band powers, maximum, total
    and entropy sums, NO per-time marginal -- the kernels then write no per-time planes and the tail sums none) against the
    full reductions, on the native engines in both precisions and on the hipFFT engine, stored and streaming, separate and
    joint calls."""
    fs, C = 800.0, 3
    rng = np.random.default_rng(n % 1000 + order)
    x = np.stack([orc.synth_chirp(n, fs, c, C, dtype) for c in range(C)]) + (0.1 * rng.standard_normal((C, n))).astype(dtype)
    x = torch.from_numpy(x).cuda()
    plan = _plan_with_all(n, fs, order, dtype, channels=C)
    rt = 1e-5 if dtype == np.float32 else 1e-11
    for coef in (True, False):
        full = {"cwt": plan.cwt(x, coef=coef, reductions=True), "stx": plan.stx(x, coef=coef, reductions=True)}
        lean = {"cwt": plan.cwt(x, coef=coef, reductions="band"), "stx": plan.stx(x, coef=coef, reductions="band")}
        joint = dict(zip(("cwt", "stx"), plan.cwt_stx(x, coef=coef, reductions="band")))
        for name in ("cwt", "stx"):
            for got in (lean[name], joint[name]):
                assert got.power_time is None and got.reduced is None
                assert torch.allclose(got.power_band, full[name].power_band, rtol=rt, atol=0.0), (name, coef)
                assert torch.allclose(got.stats[:, :3], full[name].stats[:, :3], rtol=rt, atol=0.0), (name, coef)
                assert torch.allclose(got.entropy_bits, full[name].entropy_bits, rtol=rt)
                if coef:
                    assert float((got.coef - full[name].coef).abs().max()) <= 2e-6 * float(full[name].coef.abs().max())
    plan.close()
