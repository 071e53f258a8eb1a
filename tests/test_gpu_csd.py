"""Cross-spectra and coherence between records on the device (-m gpu): qi_cross_spectra on exact integer panels, the
contract of include/qi_array.h on noise records (mirror, diagonal, run-to-run and batch-position independence, bit for bit),
qi_csd against the SciPy fixture tests/golden/csd.npz in both precisions, and the styx_fft / engine wrappers."""
import functools

import numpy as np
import pytest
import torch

import csd_cases as cc

from quantum_inferno_amd import engine, styx_fft

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float64")
# SURVEY s8d, the project's reduction contract: |dS| <= CSD_TOL max |S|
CSD_TOL = {"float32": 1e-4, "float64": 1e-10}
# float64: 4 eps / m with eps = 1e-10 and m = csd_cases.FLOOR.  float32: csd_cases.COH32_TOL = 16 x 5.84e-07, the largest
# deviation from the fixture of the float32 NumPy restatement's coherence over all cases as measured on the CPU (provenance
# at the constant; tests/test_csd_cpu.py holds it to the measurement), times 16 for the per-stage rounding of a float32 FFT.
COH_TOL = {"float32": cc.COH32_TOL, "float64": 4e-8}
assert COH_TOL["float32"] <= 4e-2


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(cc.GOLDEN, allow_pickle=False)


def records(case, dtype):
    return golden()[cc.key(case, "records")].astype(dtype)


def args(case):
    return dict(segment_points=case.seg, nfft_points=case.nfft, overlap_points=case.overlap, alpha=cc.ALPHA)


@functools.lru_cache(maxsize=None)
def device_results(cid, dtype):
    """(csd spectrum, csd density, coherence) [nf, C, C] NumPy arrays of one case: computed once, shared, left unchanged."""
    case = cc.by_id(cid)
    x = records(case, dtype)
    f, s = styx_fft.csd_matrix_pow2(x, cc.FS, scaling="spectrum", **args(case))
    f2, d = styx_fft.csd_matrix_pow2(x, cc.FS, scaling="density", **args(case))
    f3, coh = styx_fft.coherence_matrix_pow2(x, cc.FS, **args(case))
    for got in (f, f2, f3):
        assert np.array_equal(got, np.fft.rfftfreq(case.nfft, 1 / cc.FS))
    for a in (s, d, coh):
        a.setflags(write=False)
    return s, d, coh


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- qi_cross_spectra on exact panels -------------------------------------------------------------------------------------------
def integer_panel(C, nf, nseg):
    """Small integers, asymmetric in the record index: every product and every sum is exact in float32."""
    i, f, s = np.arange(C)[:, None, None], np.arange(nf)[None, :, None], np.arange(nseg)[None, None, :]
    zr = (3 * i + s + 0 * f) % 7 - 3
    zi = (5 * i + 2 * s + f) % 5 - 2
    return zr.astype(np.int64), zi.astype(np.int64)


def integer_csd(zr, zi):
    """conj(Z_i) Z_j summed over the segments, in integers -> (re, im) [nf, C, C]."""
    re = np.einsum("ifs,jfs->fij", zr, zr) + np.einsum("ifs,jfs->fij", zi, zi)
    im = np.einsum("ifs,jfs->fij", zr, zi) - np.einsum("ifs,jfs->fij", zi, zr)
    return re, im


@pytest.mark.parametrize("weighted", (False, True), ids=("unit", "weighted"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_integer_panels(dtype, weighted):
    """A row / column swap, the conjugation sign, the float64 C/D map, ragged tiles, the ragged end of the segments and the
    mirror all show as a wrong integer."""
    ctype = np.complex64 if dtype == "float32" else np.complex128
    for C in (1, 2, 15, 16, 17, 33):
        for nseg in (1, 3, 4, 5, 67):
            for nf in (1, 3):
                zr, zi = integer_panel(C, nf, nseg)
                panel = torch.from_numpy((zr + 1j * zi).astype(ctype)).cuda()
                weight = 0.25 * (1 + np.arange(nf)) if weighted else None  # (exact in float32, and so is every product with it)
                csd, coh = engine.cross_spectra(panel, weight=weight, coherence=True)
                assert csd.dtype == panel.dtype and coh.dtype == (torch.float32 if dtype == "float32" else torch.float64)
                re, im = integer_csd(zr, zi)
                w = (weight if weighted else np.ones(nf))[:, None, None]
                want = (re * w + 1j * (im * w)).astype(ctype)
                got = csd.cpu().numpy()
                assert np.array_equal(got, want), (C, nseg, nf, np.argwhere(got != want)[:4])
                assert np.array_equal(got.imag[:, np.arange(C), np.arange(C)], np.zeros((nf, C))), (C, nseg, nf)
                # the coherence of exact matrices is one correctly rounded double quotient, rounded to the panel's precision
                d = (re * w)[:, np.arange(C), np.arange(C)]
                with np.errstate(all="ignore"):
                    den = d[:, :, None] * d[:, None, :]
                    num = den if nseg == 1 else (re * w) ** 2 + (im * w) ** 2
                    want_coh = (num / den).astype(dtype)
                assert np.array_equal(coh.cpu().numpy(), want_coh, equal_nan=True), (C, nseg, nf)
                if nseg == 1:
                    assert np.all((want_coh == 1) | np.isnan(want_coh))


@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_of_more_than_one_upload_chunk(dtype):
    """257 host weights go to the device in two chunks of kernel arguments, 256 values and one.  A bin's matrix depends on its
    own rows and weight alone, so the call has the bits of the calls on bins 0 .. 255 and on bin 256."""
    C, nf, nseg = 5, 257, 12
    rng = np.random.default_rng([41, C, nf, nseg])
    panel = (rng.standard_normal((C, nf, nseg)) + 1j * rng.standard_normal((C, nf, nseg))).astype(np.complex64 if dtype == "float32" else np.complex128)
    weight = rng.uniform(0.5, 1.5, nf)  # (no two alike: a value of the wrong chunk shows)
    whole = engine.cross_spectra(panel, weight=weight, coherence=True)
    head = engine.cross_spectra(panel[:, :256], weight=weight[:256], coherence=True)
    last = engine.cross_spectra(panel[:, 256:], weight=weight[256:], coherence=True)
    assert whole[0].shape == (nf, C, C) and np.isfinite(whole[0]).all()
    for w, h, t in zip(whole, head, last):
        assert same_bits(w, np.concatenate([h, t]))


def test_cross_spectra_without_matrices_or_without_coherence():
    """Either output alone: the coherence alone goes through the scratch matrices and has the same bits."""
    zr, zi = integer_panel(17, 3, 67)
    panel = torch.from_numpy((zr + 1j * zi).astype(np.complex64)).cuda()
    csd, coh = engine.cross_spectra(panel, coherence=True)
    assert torch.equal(engine.cross_spectra(panel), csd)
    from quantum_inferno_amd import _lib

    lib = _lib.require_gpu()
    alone = torch.full_like(coh, 0.3125)
    scratch, nbytes = _lib.scratch(lib.qi_cross_spectra_scratch_bytes, panel.device, _lib.QI_F32, 17, 3, 67)
    _lib.call(lib.qi_cross_spectra, panel.device, _lib.QI_F32, panel.device.index, _lib.ptr(panel), 17, 3, 67, None, None,
              _lib.ptr(alone), _lib.ptr(scratch), nbytes)
    assert same_bits(alone.cpu().numpy(), coh.cpu().numpy())
    with pytest.raises(_lib.QiError):
        _lib.call(lib.qi_cross_spectra, panel.device, _lib.QI_F32, panel.device.index, _lib.ptr(panel), 17, 3, 67, None, None,
                  None, _lib.ptr(scratch), nbytes)


# ---- the contract on the results, on noise records ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", cc.ids())
def test_mirror_and_diagonal(cid, dtype):
    s, d, coh = device_results(cid, dtype)
    i, j = np.triu_indices(s.shape[1], 1)
    for m in (s, d):
        assert same_bits(m[:, j, i], np.conj(m[:, i, j]))
        diag = m[:, np.arange(m.shape[1]), np.arange(m.shape[1])]
        assert np.array_equal(bits(diag.imag), bits(np.zeros_like(diag.imag)))  # +0, bit for bit
        assert np.all(diag.real >= 0)
    assert same_bits(coh, np.swapaxes(coh, 1, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_on_a_second_call(dtype):
    case = cc.by_id("c33_n1024_seg64")
    s, _, coh = device_results(case.id, dtype)
    x = records(case, dtype)
    assert same_bits(styx_fft.csd_matrix_pow2(x, cc.FS, **args(case))[1], s)
    assert same_bits(styx_fft.coherence_matrix_pow2(x, cc.FS, **args(case))[1], coh)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_entry_depends_on_its_two_records_alone(dtype):
    """Records 3 and 20 of the C = 33 case (tiles 0 and 1 of the full run): alone as C = 2 (one diagonal tile), and inside
    another batch at the positions (0, 1) and (14, 31)."""
    case = cc.by_id("c33_n1024_seg64")
    s, _, coh = device_results(case.id, dtype)
    x = records(case, dtype)
    _, pair = styx_fft.csd_matrix_pow2(x[[3, 20]], cc.FS, **args(case))
    _, pair_coh = styx_fft.coherence_matrix_pow2(x[[3, 20]], cc.FS, **args(case))
    for (a, b), (i, j) in (((0, 1), (3, 20)), ((0, 0), (3, 3)), ((1, 1), (20, 20)), ((1, 0), (20, 3))):
        assert same_bits(pair[:, a, b], s[:, i, j]), (a, b)
        assert same_bits(pair_coh[:, a, b], coh[:, i, j]), (a, b)
    for pos in ((0, 1), (14, 31)):
        order = [k for k in range(case.C) if k not in (3, 20)][::-1]  # the other records, in another order
        order.insert(pos[0], 3)
        order.insert(pos[1], 20)
        assert order[pos[0]] == 3 and order[pos[1]] == 20
        _, moved = styx_fft.csd_matrix_pow2(x[order], cc.FS, **args(case))
        _, moved_coh = styx_fft.coherence_matrix_pow2(x[order], cc.FS, **args(case))
        assert same_bits(moved[:, pos[0], pos[1]], s[:, 3, 20]), pos
        assert same_bits(moved_coh[:, pos[0], pos[1]], coh[:, 3, 20]), pos


# ---- against the fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", cc.ids())
def test_against_scipy(cid, dtype):
    case = cc.by_id(cid)
    s, d, coh = device_results(cid, dtype)
    assert s.dtype == (np.complex64 if dtype == "float32" else np.complex128) and coh.dtype == np.dtype(dtype)
    for name, got in (("spectrum", s), ("density", d)):
        ref, select = cc.expected(golden(), case, f"csd_{name}")
        err = np.abs(select(got) - ref).max() / np.abs(ref).max()
        print(f"{cid} {dtype} {name}: max |dS| / max |S| = {err:.3g} (bound {CSD_TOL[dtype]:g})")
        assert err <= CSD_TOL[dtype], (name, err)
    # the diagonal is the Welch spectrum of each record
    _, welch = styx_fft.welch_power_pow2(records(case, dtype), cc.FS, case.seg, case.nfft, case.overlap, cc.ALPHA)
    diag = s[:, np.arange(case.C), np.arange(case.C)].real.T
    err = np.abs(diag - welch).max() / np.abs(s).max()
    print(f"{cid} {dtype}: diagonal against welch_power_pow2, / max |S| = {err:.3g}")
    assert err <= CSD_TOL[dtype], err
    ref, select = cc.expected(golden(), case, "coherence")
    if cc.segments(case) > 1:
        assert cc.auto_power_floor(s.astype(np.complex128)) >= 0.99 * cc.FLOOR  # the condition the tolerance rests on
        assert np.all(np.isfinite(coh))
    err = np.nanmax(np.abs(select(coh) - ref))
    print(f"{cid} {dtype}: coherence against scipy.signal.coherence: {err:.3g} (bound {COH_TOL[dtype]:g})")
    assert err <= COH_TOL[dtype], err
    if cc.segments(case) == 1:
        assert np.isfinite(coh).any() and np.all(coh[np.isfinite(coh)] == 1)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_forms_are_the_matrix_entries(dtype):
    case = cc.by_id("c5_n4096_seg256")
    s, d, coh = device_results(case.id, dtype)
    x = records(case, dtype)
    f, one = styx_fft.csd_pow2(x[1], x[4], cc.FS, **args(case))
    assert isinstance(one, np.ndarray) and one.shape == (case.nfft // 2 + 1,) and np.array_equal(f, np.fft.rfftfreq(case.nfft, 1 / cc.FS))
    assert same_bits(one, s[:, 1, 4])
    assert same_bits(styx_fft.csd_pow2(x[1], x[4], cc.FS, scaling="density", **args(case))[1], d[:, 1, 4])
    assert same_bits(styx_fft.coherence_pow2(x[1], x[4], cc.FS, **args(case))[1], coh[:, 1, 4])
    # two batches paired row by row, tensors in -> tensors out on the device
    xa, xb = torch.from_numpy(x[[0, 1, 2]]).cuda(), torch.from_numpy(x[[4, 3, 2]]).cuda()
    _, rows = styx_fft.csd_pow2(xa, xb, cc.FS, **args(case))
    _, rows_coh = styx_fft.coherence_pow2(xa, xb, cc.FS, **args(case))
    assert isinstance(rows, torch.Tensor) and rows.is_cuda and rows.shape == (3, case.nfft // 2 + 1)
    assert rows.dtype == (torch.complex64 if dtype == "float32" else torch.complex128) and rows_coh.dtype == xa.dtype
    for r, (i, j) in enumerate(((0, 4), (1, 3), (2, 2))):
        assert same_bits(rows[r].cpu().numpy(), s[:, i, j]), r
        assert same_bits(rows_coh[r].cpu().numpy(), coh[:, i, j]), r
    _, on_device = styx_fft.csd_matrix_pow2(torch.from_numpy(x).cuda(), cc.FS, **args(case))
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and same_bits(on_device.cpu().numpy(), s)


def test_defaults_are_welch_s():
    """nfft_points and overlap_points default as welch_power_pow2's: the next power of two and half the segment."""
    case = cc.by_id("c3_n1000_seg100_nfft128")
    x = records(case, "float64")
    f, got = styx_fft.csd_matrix_pow2(x, cc.FS, case.seg)
    assert same_bits(got, device_results(case.id, "float64")[0]) and len(f) == 65


def test_refusals():
    x = np.zeros((2, 100), dtype=np.float32)
    with pytest.raises(ValueError, match="less than the segment"):
        styx_fft.csd_matrix_pow2(x, cc.FS, 128)
    with pytest.raises(ValueError, match="noverlap must be less than nperseg"):
        styx_fft.coherence_matrix_pow2(x, cc.FS, 64, overlap_points=64)
    with pytest.raises(ValueError, match="noverlap must be less than nperseg"):
        styx_fft.csd_pow2(x[0], x[1], cc.FS, 64, overlap_points=65)
    with pytest.raises(ValueError, match="same shape"):
        styx_fft.csd_pow2(x[0], x[1, :99], cc.FS, 64)
    with pytest.raises(ValueError, match="same shape"):
        styx_fft.coherence_pow2(x, x[0], cc.FS, 64)
    with pytest.raises(ValueError, match="Unknown scaling"):
        styx_fft.csd_matrix_pow2(x, cc.FS, 64, scaling="power")
    with pytest.raises(ValueError, match="one value per band"):
        engine.cross_spectra(np.ones((2, 3, 4), dtype=np.complex64), weight=np.ones(4))
    with pytest.raises(ValueError, match="complex"):
        engine.cross_spectra(np.ones((2, 3, 4), dtype=np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_spectra_of_a_stored_stft_panel(dtype):
    case = cc.by_id("c5_n4096_seg256")
    x = torch.from_numpy(records(case, dtype)).cuda()
    _, _, z = styx_fft.stft_complex_pow2(x, cc.FS, case.seg, case.overlap, case.nfft, cc.ALPHA)
    weight = np.linspace(0.5, 1.5, z.shape[1])
    csd, coh = engine.cross_spectra(z, weight=weight, coherence=True)
    assert csd.is_cuda and csd.shape == (z.shape[1], case.C, case.C) and csd.dtype == z.dtype
    zn = z.cpu().numpy().astype(np.complex128)
    wt = weight.astype(dtype).astype(np.float64)  # (the weight is rounded to the panel's precision)
    want = np.einsum("ifs,jfs->fij", np.conj(zn), zn) * wt[:, None, None]
    err = np.abs(csd.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"{dtype}: cross-spectra of a stored STFT panel against einsum: {err:.3g}")
    assert err <= CSD_TOL[dtype]
    # the coherence is the quotient of the stored matrices' own entries, formed in double and rounded once
    own = cc.coherence_of(csd.cpu().numpy())
    assert np.nanmax(np.abs(coh.cpu().numpy() - own) / own) <= 2 * np.finfo(dtype).eps
    # NumPy in -> NumPy out
    host = engine.cross_spectra(z.cpu().numpy(), weight=weight)
    assert isinstance(host, np.ndarray) and same_bits(host, csd.cpu().numpy())
