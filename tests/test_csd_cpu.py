"""Cross-spectra without a GPU: the NumPy restatement of qi_csd (tests/csd_cases.py) against the SciPy fixture
tests/golden/csd.npz, the condition the tolerances rest on, the float32 coherence tolerance's provenance, the exports of
include/qi_array.h and the census of tests/array_stream_cases.py against that header."""
import numpy as np
import pytest

import array_stream_cases as asc
import csd_cases as cc
from stream_table import header_functions, stream_functions

COH32_RESTATEMENT, COH32_TOL = cc.COH32_RESTATEMENT, cc.COH32_TOL
HEADER = "qi_array.h"


@pytest.fixture(scope="module")
def golden():
    return np.load(cc.GOLDEN, allow_pickle=False)


def test_case_table_is_the_issue_s():
    assert [(c.C, c.n, c.seg, c.overlap, c.nfft, c.path) for c in cc.CASES] == [
        (5, 4096, 256, 128, 256, "fused"), (17, 2048, 64, 48, 128, "fused"), (3, 1000, 100, 50, 128, "hipfft"),
        (33, 1024, 64, 32, 64, "fused"), (2, 256, 256, 0, 256, "fused")]
    assert cc.by_id("c33_n1024_seg64").rows == (0, 15, 16, 32)
    assert cc.segments(cc.by_id("c2_n256_one_segment")) == 1


@pytest.mark.parametrize("cid", cc.ids())
def test_records_are_the_fixture_s(golden, cid):
    case = cc.by_id(cid)
    x = golden[cc.key(case, "records")]
    assert x.dtype == np.float32 and x.shape == (case.C, case.n)
    assert np.array_equal(x, cc.records(case))


@pytest.mark.parametrize("scaling", cc.SCALINGS)
@pytest.mark.parametrize("cid", cc.ids())
def test_restatement_matches_scipy(golden, cid, scaling):
    case = cc.by_id(cid)
    x = golden[cc.key(case, "records")].astype(np.float64)
    ref, select = cc.expected(golden, case, f"csd_{scaling}")
    got = cc.restate(x, case, scaling)
    assert got.shape == (case.nfft // 2 + 1, case.C, case.C)
    err = np.abs(select(got) - ref).max() / np.abs(ref).max()
    print(f"{cid} {scaling}: restatement against SciPy, max |dS| / max |S| = {err:.3g}")
    assert err <= 1e-13
    # Hermitian, with a real diagonal
    assert np.array_equal(got, np.conj(np.swapaxes(got, 1, 2)))


@pytest.mark.parametrize("cid", cc.ids())
def test_auto_powers_keep_the_floor_and_coherence_matches(golden, cid):
    case = cc.by_id(cid)
    x = golden[cc.key(case, "records")].astype(np.float64)
    s = cc.restate(x, case, "spectrum")
    if cc.segments(case) > 1:  # (one segment: bin 0 is what the mean removal leaves -- and the coherence is 1 whatever the power)
        assert cc.auto_power_floor(s) >= cc.FLOOR, cc.auto_power_floor(s)
    ref, select = cc.expected(golden, case, "coherence")
    err = np.nanmax(np.abs(select(cc.coherence_of(s)) - ref))
    print(f"{cid}: coherence of the spectrum-scaled restatement against scipy.signal.coherence: {err:.3g}")
    assert err <= 1e-13
    if cc.segments(case) == 1:
        assert np.nanmax(np.abs(ref - 1.0)) <= 1e-13


def test_float32_coherence_tolerance(golden):
    worst = 0.0
    for case in cc.CASES:
        x = golden[cc.key(case, "records")]
        ref, select = cc.expected(golden, case, "coherence")
        err = float(np.nanmax(np.abs(select(cc.coherence_of(cc.restate(x, case, "spectrum", np.float32))) - ref)))
        print(f"{case.id}: float32 restatement's coherence against the fixture: {err:.4g}")
        worst = max(worst, err)
    print(f"largest: {worst:.4g}; the constant {COH32_RESTATEMENT:g}; tolerance {COH32_TOL:g}")
    assert worst <= COH32_RESTATEMENT <= 1.05 * worst, worst  # the constant is the measurement, rounded up
    assert COH32_TOL == 16 * COH32_RESTATEMENT and COH32_TOL <= 4e-2


def test_bin_weights():
    assert np.array_equal(cc.bin_weights(8, 2, 1.0), [0.5, 1, 1, 1, 0.5])
    assert np.array_equal(cc.bin_weights(7, 1, 1.0), [1, 2, 2, 2])


def test_library_exports_the_array_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == {"qi_cross_spectra_scratch_bytes", "qi_cross_spectra", "qi_csd_scratch_bytes", "qi_csd"}
    assert declared == set(_lib.ARRAY_PROTOTYPES) and not declared & set(_lib.PROTOTYPES)
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_array.h but not exported"
    # the size queries are host only: refusals and sizes without a GPU
    assert lib.qi_cross_spectra_scratch_bytes(_lib.QI_F32, 0, 4, 4) < 0 and lib.qi_cross_spectra_scratch_bytes(7, 2, 4, 4) < 0
    assert lib.qi_csd_scratch_bytes(_lib.QI_F32, 2, 100, 256, 128, 256) < 0  # a record shorter than the segment
    small = lib.qi_cross_spectra_scratch_bytes(_lib.QI_F64, 3, 5, 9)
    assert small >= 5 * 8 + 5 * 9 * 16 and small % 256 == 0
    assert lib.qi_csd_scratch_bytes(_lib.QI_F64, 3, 1000, 100, 50, 128) > lib.qi_csd_scratch_bytes(_lib.QI_F32, 3, 1000, 100, 50, 128) > 0


# ---- the census of tests/array_stream_cases.py against include/qi_array.h ----------------------------------------------------
def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert asc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_cross_spectra", "qi_csd"]
    assert asc.TABLE.named_functions() == stream_functions(HEADER)


def test_stream_case_table():
    assert asc.TABLE.ids() == ["csd-fused", "csd-hipfft", "cross_spectra-coherence", "cross_spectra-matrices"]
    for case in asc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous, case.id
