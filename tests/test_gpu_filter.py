"""The zero-phase filter on the GPU: qi_filtfilt through ctypes with the fixture's tables against the reference's results
bit for bit (every design, length and dtype of tests/golden/filter.npz, 1, 3 and 65 records), its argument checks and its
determinism, and the reference-signature wrappers end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import filter_cases as fc
from quantum_inferno_amd import _lib, engine, styx_fft
from quantum_inferno_amd.utilities import picker

pytestmark = pytest.mark.gpu


def filtfilt(x, form, coef, zi, edge, taper=None, n=None, extra_scratch=0, expect=0):
    """qi_filtfilt on a device tensor x [C, n] -> out [C, n] float64 (device); `expect`: the status the call must return."""
    lib = _lib.require_gpu()
    dev = x.device
    n_ch = x.shape[0]
    n = x.shape[1] if n is None else n
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    zi = np.ascontiguousarray(zi, dtype=np.float64)
    sections, order = (coef.shape[0], 2) if form == fc.QI_IIR_SOS else (1, coef.shape[1] - 1)
    need = int(lib.qi_filtfilt_scratch_bytes(n_ch, n, edge))
    words = (need // 8 if need > 0 else n_ch * (n + 2 * edge)) + extra_scratch
    scratch = torch.full((words,), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((n_ch, n), float("nan"), dtype=torch.float64, device=dev)
    tp = None if taper is None else torch.from_numpy(np.ascontiguousarray(taper, dtype=np.float64)).to(dev)
    with torch.cuda.device(dev):
        rc = lib.qi_filtfilt(_lib.QI_F64 if x.dtype == torch.float64 else _lib.QI_F32, dev.index, _lib.ptr(x), n_ch, n, _lib.ptr(tp),
                             form, sections, order, coef.ctypes.data_as(_lib._D), zi.ctypes.data_as(_lib._D), edge, _lib.ptr(out),
                             _lib.ptr(scratch), words * 8, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc == expect, (rc, lib.qi_last_error())
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def case_taper(form, n):
    return None if form == fc.QI_IIR_SOS else fc.tukey_symmetric(n, fc.TUKEY_ALPHA)


@pytest.mark.parametrize("name", list(fc.DESIGNS))
def test_filtfilt_equals_the_reference_bit_for_bit(golden, name):
    g = golden("filter.npz")
    form, coef, zi, edge = fc.tables(g, name)
    seen = 0
    for cname, dtype, n in fc.cases(g):
        if cname != name:
            continue
        x = torch.from_numpy(g[fc.key(name, dtype, n, "x")]).cuda()
        y = torch.from_numpy(g[fc.key(name, dtype, n, "y")]).cuda()
        for records in (1, fc.RECORDS):
            out = filtfilt(x[:records].contiguous(), form, coef, zi, edge, case_taper(form, n))
            assert out.dtype == torch.float64
            diff = (out - y[:records]).abs().max().item()
            print(f"{name} {dtype} n={n} records={records}: max |difference| {diff:.3e}")
            assert same_bits(out, y[:records]), (name, dtype, n, records, diff)
        seen += 1
    assert seen == (6 if name in fc.F32_DESIGNS else 3)


@pytest.mark.parametrize("name", list(fc.DESIGNS))
def test_batch_across_a_wavefront(golden, name):
    """65 records, the fixture's three cyclically, row r scaled by 2^(r mod 4): every row is the fixture's result times the
    same power of two, bit for bit (a lane, tile or row-stride mistake shows)."""
    g = golden("filter.npz")
    form, coef, zi, edge = fc.tables(g, name)
    rows = torch.arange(65, device="cuda")
    for cname, dtype, n in fc.cases(g):
        if cname != name:
            continue
        x = torch.from_numpy(g[fc.key(name, dtype, n, "x")]).cuda()
        y = torch.from_numpy(g[fc.key(name, dtype, n, "y")]).cuda()
        gain = torch.pow(2.0, (rows % 4).to(torch.float64))[:, None]
        xb = (x[rows % fc.RECORDS].to(torch.float64) * gain).to(x.dtype).contiguous()
        out = filtfilt(xb, form, coef, zi, edge, case_taper(form, n))
        want = y[rows % fc.RECORDS] * gain
        bad = [r for r in range(65) if not same_bits(out[r], want[r])]
        assert not bad, (name, dtype, n, bad)


def test_taper_given_and_null(golden):
    g = golden("filter.npz")
    for name, n in (("bp4", 300), ("sos3", 1031), ("lp4", 16)):
        form, coef, zi, edge = fc.tables(g, name)
        for dtype in ("float64", "float32") if name == "bp4" else ("float64",):
            x = g[fc.key(name, dtype, n, "x")]
            for taper in (None, fc.tukey_symmetric(n, 0.25)):
                want = torch.from_numpy(fc.filtfilt_ref(x, form, coef, zi, edge, taper)).cuda()
                out = filtfilt(torch.from_numpy(x).cuda(), form, coef, zi, edge, taper)
                assert same_bits(out, want), (name, dtype, taper is None)


def test_same_bits_when_repeated_and_with_more_scratch(golden):
    g = golden("filter.npz")
    for name in ("bp8", "sos7"):
        form, coef, zi, edge = fc.tables(g, name)
        x = torch.from_numpy(g[fc.key(name, "float64", 1031, "x")]).cuda()
        y = torch.from_numpy(g[fc.key(name, "float64", 1031, "y")]).cuda()
        taper = case_taper(form, 1031)
        first = filtfilt(x, form, coef, zi, edge, taper)
        assert same_bits(first, y)
        assert same_bits(filtfilt(x, form, coef, zi, edge, taper), first)
        assert same_bits(filtfilt(x, form, coef, zi, edge, taper, extra_scratch=4099), first)


def test_bad_arguments_are_refused(golden):
    g = golden("filter.npz")
    lib = _lib.load()
    form, coef, zi, edge = fc.tables(g, "bp4")
    x = torch.from_numpy(g[fc.key("bp4", "float64", 300, "x")]).cuda()
    filtfilt(x, form, coef, zi, edge, n=edge, expect=-1)  # n == edge: QI_ERR_ARG
    assert b"longer than the extension" in lib.qi_last_error()
    filtfilt(x, form, coef, zi, edge, n=edge + 1)  # the shortest legal record (of the same buffer)
    bad = coef.copy()
    bad[1, 0] = 2.0
    filtfilt(x, form, bad, zi, edge, expect=-1)  # a[0] != 1
    filtfilt(x, 2, coef, zi, edge, expect=-1)  # unknown form
    filtfilt(x, form, np.ones((2, 18)), np.zeros(17), 54, expect=-1)  # order 17
    sform, sos, szi, sedge = fc.tables(g, "sos7")
    filtfilt(x, sform, np.tile(sos, (3, 1))[:17], np.zeros((17, 2)), sedge, expect=-1)  # 17 sections
    sbad = sos.copy()
    sbad[2, 3] = 0.5
    filtfilt(x, sform, sbad, szi, sedge, expect=-1)
    with torch.cuda.device(x.device):  # scratch one byte short
        need = int(lib.qi_filtfilt_scratch_bytes(3, 300, edge))
        scratch = torch.empty(need // 8, dtype=torch.float64, device=x.device)
        out = torch.empty((3, 300), dtype=torch.float64, device=x.device)
        rc = lib.qi_filtfilt(_lib.QI_F64, x.device.index, _lib.ptr(x), 3, 300, None, form, 1, coef.shape[1] - 1,
                             coef.ctypes.data_as(_lib._D), zi.ctypes.data_as(_lib._D), edge, _lib.ptr(out), _lib.ptr(scratch),
                             need - 1, _lib.stream_ptr(x.device))
    assert rc == -1


def wrapper_call(name, x):
    kind, order, band = fc.DESIGNS[name]
    if kind == "sos":
        return picker.apply_bandpass(x, band, fc.FS_SOS, order)
    if kind == "bandpass":
        return styx_fft.butter_bandpass(x, fc.FS_BA, band[0], band[1], order, fc.TUKEY_ALPHA)
    if kind == "highpass":
        return styx_fft.butter_highpass(x, fc.FS_BA, band[0], order, fc.TUKEY_ALPHA)
    return styx_fft.butter_lowpass(x, fc.FS_BA, band[0], order, fc.TUKEY_ALPHA)


@pytest.mark.parametrize("name", list(fc.DESIGNS))
def test_wrappers_end_to_end(golden, name):
    """Design on this host, filter on the device, against the reference's results: within 4 sens + 16 * 2^-52 of each
    record's largest value (sens: what one ulp in every table entry does to the reference's own result; 0 is expected
    where NumPy reproduces the tables' bits)."""
    g = golden("filter.npz")
    for cname, dtype, n in fc.cases(g):
        if cname != name:
            continue
        x = g[fc.key(name, dtype, n, "x")]
        y = g[fc.key(name, dtype, n, "y")]
        tol = (4.0 * g[fc.key(name, dtype, n, "sens")] + 16.0 * 2.0 ** -52) * np.max(np.abs(y), axis=1)
        rows = wrapper_call(name, x)  # NumPy [C, n] in
        assert isinstance(rows, np.ndarray) and rows.dtype == np.float64 and rows.shape == y.shape
        one = wrapper_call(name, x[1])  # NumPy [n] in
        assert isinstance(one, np.ndarray) and one.shape == (n,)
        dev = wrapper_call(name, torch.from_numpy(x).cuda())  # CUDA tensor in
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64 and tuple(dev.shape) == y.shape
        err = np.max(np.abs(rows - y), axis=1)
        print(f"{name} {dtype} n={n}: max |difference| {err.max():.3e}, bound {tol.min():.3e}")
        assert np.all(err <= tol), (name, dtype, n, err, tol)
        assert np.array_equal(one, rows[1])
        assert np.array_equal(dev.cpu().numpy(), rows)


def test_zero_phase_filter_checks_its_tables():
    x = torch.ones((2, 64), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        engine.zero_phase_filter(x, "zpk", np.ones((2, 3)), np.zeros(2), 9)
    with pytest.raises(ValueError):
        engine.zero_phase_filter(x, "ba", np.ones((2, 3)), np.zeros(3), 9)
    with pytest.raises(ValueError):
        engine.zero_phase_filter(x, "sos", np.ones((2, 5)), np.zeros((2, 2)), 9)
    with pytest.raises(ValueError, match="padlen"):
        engine.zero_phase_filter(x, "ba", np.array([[0.5, 0.5], [1.0, 0.0]]), np.zeros(1), 64)
    with pytest.raises(ValueError):
        engine.zero_phase_filter(x, "ba", np.array([[0.5, 0.5], [1.0, 0.0]]), np.zeros(1), 6, taper=np.ones(63))
    out = engine.zero_phase_filter(x, "ba", np.array([[0.5, 0.5], [1.0, 0.0]]), np.zeros(1), 6)  # a two-point mean of ones
    assert torch.equal(out, x)
