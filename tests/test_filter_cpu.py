"""The zero-phase filter without a GPU: the NumPy restatement of qi_filtfilt's semantics (tests/filter_cases.py) against
the reference's results in the fixture, bit for bit; the host design (utilities/iir_design.py) against the tables SciPy
made for the fixture, bit for bit; the wrappers' argument checks; the new symbols of the library."""
import os

import numpy as np
import pytest

import filter_cases as fc
from quantum_inferno_amd import _lib, styx_fft
from quantum_inferno_amd.utilities import iir_design, picker
from quantum_inferno_amd.utilities.short_time_fft import tukey_window_symmetric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_holds_every_case(golden):
    g = golden("filter.npz")
    cs = fc.cases(g)
    assert len(cs) == 3 * (len(fc.DESIGNS) + len(fc.F32_DESIGNS))
    for name, dtype, n in cs:
        x, y, sens = (g[fc.key(name, dtype, n, w)] for w in ("x", "y", "sens"))
        assert x.shape == y.shape == (fc.RECORDS, n) and x.dtype == np.dtype(dtype) and y.dtype == np.float64
        assert sens.shape == (fc.RECORDS,) and np.all(sens < 1e-3)
        assert abs(x.mean()) > 0.25  # records with a drift
        assert np.array_equal(x * fc.GRID, np.round(x * fc.GRID))
    assert int(g["sos7_edge"]) == 45 and g["sos7_sos"].shape == (7, 6)  # "at least 46 values" (picker.py:61)
    assert len(g["bp8_a"]) == 17


def test_restatement_equals_the_reference(golden):
    g = golden("filter.npz")
    for name, dtype, n in fc.cases(g):
        form, coef, zi, edge = fc.tables(g, name)
        x = g[fc.key(name, dtype, n, "x")]
        taper = None if form == fc.QI_IIR_SOS else tukey_window_symmetric(n, fc.TUKEY_ALPHA)
        mine = fc.filtfilt_ref(x, form, coef, zi, edge, taper)
        assert mine.dtype == np.float64
        assert np.array_equal(mine, g[fc.key(name, dtype, n, "y")]), (name, dtype, n)


def test_tukey_restatement():
    for n in (10, 16, 300, 1031):
        assert np.array_equal(fc.tukey_symmetric(n, fc.TUKEY_ALPHA), tukey_window_symmetric(n, fc.TUKEY_ALPHA))


def test_design_reproduces_the_fixture_tables(golden):
    g = golden("filter.npz")
    for name, (kind, order, band) in fc.DESIGNS.items():
        if kind == "sos":
            sos = iir_design.butter_sos(order, [2 * f / fc.FS_SOS for f in band], "bandpass")
            assert np.array_equal(sos, g[f"{name}_sos"]), name
            assert np.array_equal(iir_design.sosfilt_zi(sos), g[f"{name}_zi"]), name
            assert iir_design.sosfiltfilt_edge(sos) == int(g[f"{name}_edge"]), name
        else:
            b, a = iir_design.butter_ba(order, band, kind)
            assert b.dtype == a.dtype == np.float64
            assert np.array_equal(b, g[f"{name}_b"]) and np.array_equal(a, g[f"{name}_a"]), name
            assert a[0] == 1.0
            assert np.array_equal(iir_design.lfilter_zi(b, a), g[f"{name}_zi"]), name
            assert iir_design.filtfilt_edge(b, a) == int(g[f"{name}_edge"]), name


def test_design_rejects_bad_requests():
    for wn in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            iir_design.butter_ba(4, wn, "lowpass")
    with pytest.raises(ValueError):
        iir_design.butter_ba(4, (0.2, 0.1), "bandpass")
    with pytest.raises(ValueError):
        iir_design.butter_ba(4, 0.1, "bandpass")
    with pytest.raises(ValueError):
        iir_design.butter_sos(0, (0.1, 0.2), "bandpass")
    with pytest.raises(ValueError):
        iir_design.butter_ba(4, 0.1, "bandstop")
    iir_design.check_length(46, 45)
    with pytest.raises(ValueError):
        iir_design.check_length(45, 45)


def test_wrappers_raise_the_reference_errors(capsys):
    x = np.ones(300)
    with pytest.raises(ValueError, match="greater than Nyquist"):
        styx_fft.butter_highpass(x, 100.0, 50.0)
    with pytest.raises(ValueError, match="greater than Nyquist"):
        styx_fft.butter_lowpass(x, 100.0, 60.0)
    with pytest.raises(ValueError, match="Invalid bandpass filter band"):
        picker.apply_bandpass(x, (-1.0, 20.0), 100.0)
    with pytest.raises(ValueError, match="Invalid bandpass filter band"):
        picker.apply_bandpass(x, (10.0, 60.0), 100.0)
    with pytest.raises(ValueError, match="lower bound must be less"):
        picker.apply_bandpass(x, (20.0, 20.0), 100.0)
    # a record no longer than the extension: SciPy's error, before anything reaches the device
    with pytest.raises(ValueError, match="padlen"):
        picker.apply_bandpass(np.ones(45), (100.0, 200.0), 1000.0)
    with pytest.raises(ValueError, match="padlen"):
        styx_fft.butter_bandpass(np.ones(27), 2.0, 0.05, 0.2)
    with pytest.raises(ValueError, match="padlen"):
        styx_fft.butter_lowpass(np.ones((2, 15)), 2.0, 0.1)
    with pytest.raises(ValueError):
        styx_fft.butter_lowpass(np.ones((2, 2, 64)), 2.0, 0.1)


def test_bandpass_above_nyquist_warns_and_uses_half_nyquist(capsys):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.QiError):  # (no CPU fallback: the design and the warning come first)
        styx_fft.butter_bandpass(np.ones(300), 100.0, 5.0, 60.0)
    assert "greater than Nyquist" in capsys.readouterr().out


def test_no_cpu_fallback():
    import torch

    from quantum_inferno_amd import engine

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.QiError):
        picker.apply_bandpass(np.ones(300), (100.0, 200.0), 1000.0)
    with pytest.raises(_lib.QiError):
        engine.zero_phase_filter(np.ones(300), "ba", np.array([[0.5, 0.5], [1.0, 0.0]]), np.zeros(1), 6)


def test_header_declares_and_library_exports_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    lib = _lib.load()
    assert lib.qi_abi_version() == 1
    for name in ("qi_filtfilt", "qi_filtfilt_scratch_bytes"):
        assert name + "(" in header
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert "QI_IIR_BA = 0, QI_IIR_SOS = 1" in header
    assert (_lib.QI_IIR_BA, _lib.QI_IIR_SOS) == (fc.QI_IIR_BA, fc.QI_IIR_SOS) == (0, 1)
    # host-only size query: [C][n + 2 edge] float64
    assert lib.qi_filtfilt_scratch_bytes(3, 1031, 27) == 3 * (1031 + 54) * 8
    assert lib.qi_filtfilt_scratch_bytes(1, 46, 45) == 136 * 8
    assert lib.qi_filtfilt_scratch_bytes(0, 100, 9) < 0
    assert lib.qi_filtfilt_scratch_bytes(1, 9, 9) < 0
    assert lib.qi_filtfilt_scratch_bytes(1, 100, -1) < 0
