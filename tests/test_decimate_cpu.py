"""Decimation without a GPU: the fixture is complete; the NumPy restatement of qi_decimate's semantics
(tests/decimate_cases.py) equals the reference's results bit for bit, in float64 and in float32; the host design
(utilities/iir_design.py) reproduces the tables SciPy made for the fixture bit for bit in both precisions; the wrappers'
argument checks; the new symbols of the library and its host-only size queries."""
import os

import numpy as np
import pytest

import decimate_cases as dc
import filter_cases as fc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import iir_design, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_holds_every_case(golden):
    g = golden("decimate.npz")
    cs = dc.cases()
    assert len(cs) == 4 * 2 * 4
    for q, dtype, n in cs:
        x, y, sens = (g[dc.key(q, dtype, n, w)] for w in ("x", "y", "sens"))
        assert x.shape == (dc.RECORDS, n) and x.dtype == np.dtype(dtype)
        assert y.shape == (dc.RECORDS, dc.columns(n, q)) and y.dtype == np.dtype(dtype)  # the dtype is kept
        assert sens.shape == (dc.RECORDS,) and np.all(sens < 1e-3)
        assert abs(x.mean()) > 0.25  # records with a drift
        assert np.array_equal(x * fc.GRID, np.round(x * fc.GRID))
    for q in dc.FACTORS:
        for dtype in dc.DTYPES:
            sos, zi, edge = dc.tables(g, q, dtype)
            assert sos.shape == (dc.SECTIONS, 6) and zi.shape == (dc.SECTIONS, 2) and edge == dc.EDGE == 27
            assert sos.dtype == zi.dtype == np.dtype(dtype)
            assert np.all(sos[:, 3] == 1) and np.all(sos[:, 2] != 0) and np.all(sos[:, 5] != 0)
        # SciPy casts the float64 design: the float32 sections are the rounded float64 ones
        assert np.array_equal(g[dc.table_key(q, "float32", "sos")], g[dc.table_key(q, "float64", "sos")].astype(np.float32))
    assert dc.LENGTHS[0] == dc.EDGE + 1 and (266 + 2 * dc.EDGE) % 64 == 0


def test_restatement_equals_the_reference(golden):
    g = golden("decimate.npz")
    for q, dtype, n in dc.cases():
        sos, zi, edge = dc.tables(g, q, dtype)
        mine = dc.decimate_ref(g[dc.key(q, dtype, n, "x")], q, sos, zi, edge)
        assert mine.dtype == np.dtype(dtype)
        assert np.array_equal(mine, g[dc.key(q, dtype, n, "y")]), (q, dtype, n)


def test_design_reproduces_the_fixture_tables(golden):
    g = golden("decimate.npz")
    for q in dc.FACTORS:
        wide = iir_design.cheby1_sos(8, 0.05, 0.8 / q)
        assert wide.dtype == np.float64 and np.array_equal(wide, g[dc.table_key(q, "float64", "sos")]), q
        for dtype in dc.DTYPES:
            want_sos, want_zi, want_edge = dc.tables(g, q, dtype)
            sos, zi, edge = iir_design.decimator(q, np.dtype(dtype))
            assert sos.dtype == zi.dtype == np.dtype(dtype)
            assert np.array_equal(sos, want_sos), (q, dtype)
            assert np.array_equal(zi, want_zi), (q, dtype)
            assert edge == want_edge == 27
            assert np.array_equal(iir_design.sosfilt_zi(want_sos), want_zi) and iir_design.sosfilt_zi(want_sos).dtype == np.dtype(dtype)


def test_float64_callers_of_the_design_keep_their_types():
    sos = iir_design.butter_sos(3, (0.02, 0.8), "bandpass")
    assert iir_design.sosfilt_zi(sos).dtype == np.float64
    assert iir_design.sosfilt_zi(sos.tolist()).dtype == np.float64
    assert np.array_equal(iir_design.sosfilt_zi(sos.tolist()), iir_design.sosfilt_zi(sos))
    ints = [[1, 2, 1, 1, 0, 0]]
    assert iir_design.sosfilt_zi(ints).dtype == np.float64
    with pytest.raises(TypeError):
        iir_design.decimator(4, np.float16)
    with pytest.raises(ValueError):
        iir_design.cheby1_sos(8, 0.05, 1.0)


def test_wrappers_raise_their_errors():
    x = np.ones(300)
    for call, arg in ((sampling.decimate_timeseries, x), (sampling.decimate_timeseries_collection, np.ones((2, 300)))):
        with pytest.raises(TypeError):
            call(arg, 2.5)  # as operator.index
        with pytest.raises(TypeError):
            call(arg, "4")
        with pytest.raises(ValueError):
            call(arg, 0)
        with pytest.raises(ValueError):
            call(arg, -3)
    # a record no longer than the extension: SciPy's error, before anything reaches the device
    with pytest.raises(ValueError, match="padlen, which is 27"):
        sampling.decimate_timeseries(np.ones(27), 4)
    with pytest.raises(ValueError, match="padlen"):
        sampling.decimate_timeseries_collection(np.ones((3, 27), dtype=np.float32), 4)
    with pytest.raises(ValueError, match="padlen"):
        sampling.decimate_timeseries(np.ones(5, dtype=np.int16), 1)
    # the reference's functions take one rank each
    with pytest.raises(ValueError):
        sampling.decimate_timeseries(np.ones((2, 300)), 4)
    with pytest.raises(ValueError):
        sampling.decimate_timeseries_collection(x, 4)


def test_zero_phase_decimate_checks_its_arguments():
    sos, zi, edge = iir_design.decimator(4)
    x = np.ones((2, 64))
    with pytest.raises(TypeError):
        engine.zero_phase_decimate(x, 2.0, sos, zi, edge)
    with pytest.raises(ValueError):
        engine.zero_phase_decimate(x, 0, sos, zi, edge)
    with pytest.raises(ValueError, match="padlen"):
        engine.zero_phase_decimate(x, 4, sos, zi, 64)
    with pytest.raises(ValueError):
        engine.zero_phase_decimate(x, 4, sos[:, :5], zi, edge)
    with pytest.raises(ValueError):
        engine.zero_phase_decimate(x, 4, sos, zi[:3], edge)
    with pytest.raises(ValueError):
        engine.zero_phase_decimate(x, 4, np.tile(sos, (5, 1)), np.tile(zi, (5, 1)), edge)  # 20 sections
    bad = sos.copy()
    bad[1, 3] = 0.5
    with pytest.raises(ValueError):
        engine.zero_phase_decimate(x, 4, bad, zi, edge)
    with pytest.raises(ValueError):
        engine.zero_phase_decimate(np.ones((2, 2, 64)), 4, sos, zi, edge)


def test_no_cpu_fallback(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (the check of _lib.require_gpu)
    sos, zi, edge = iir_design.decimator(4)
    with pytest.raises(_lib.QiError):
        sampling.decimate_timeseries(np.ones(300), 4)
    with pytest.raises(_lib.QiError):
        sampling.decimate_timeseries_collection(np.ones((2, 300), dtype=np.float32), 4)
    with pytest.raises(_lib.QiError):
        engine.zero_phase_decimate(np.ones(300), 4, sos, zi, edge)


def test_header_declares_and_library_exports_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    lib = _lib.load()
    assert lib.qi_abi_version() == 1
    assert "#define QI_TFR_ABI_VERSION 1" in header
    for name in ("qi_decimate", "qi_decimate_columns", "qi_decimate_scratch_bytes"):
        assert name + "(" in header
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    # host-only size queries
    assert lib.qi_decimate_columns(28, 1) == 28
    assert lib.qi_decimate_columns(28, 13) == 3
    assert lib.qi_decimate_columns(26, 13) == 2
    assert lib.qi_decimate_columns(1031, 5) == 207
    assert lib.qi_decimate_columns(5, 1 << 40) == 1
    assert lib.qi_decimate_columns(0, 2) < 0
    assert lib.qi_decimate_columns(100, 0) < 0
    assert lib.qi_decimate_columns(100, -2) < 0
    # [C][n + 2 edge] in the record's type: float32 needs half the bytes
    assert lib.qi_decimate_scratch_bytes(_lib.QI_F64, 3, 1031, 27) == 3 * (1031 + 54) * 8
    assert lib.qi_decimate_scratch_bytes(_lib.QI_F32, 3, 1031, 27) == 3 * (1031 + 54) * 4
    assert lib.qi_decimate_scratch_bytes(_lib.QI_F64, 3, 1031, 27) == lib.qi_filtfilt_scratch_bytes(3, 1031, 27)
    assert lib.qi_decimate_scratch_bytes(_lib.QI_F32, 1, 28, 27) == 82 * 4
    assert lib.qi_decimate_scratch_bytes(2, 1, 100, 27) < 0  # unknown dtype
    assert lib.qi_decimate_scratch_bytes(_lib.QI_F32, 0, 100, 27) < 0
    assert lib.qi_decimate_scratch_bytes(_lib.QI_F32, 1, 27, 27) < 0
    assert lib.qi_decimate_scratch_bytes(_lib.QI_F64, 1, 100, -1) < 0
