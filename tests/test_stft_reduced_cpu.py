"""The STFT reduced product's public surface and its references, without a GPU: the two appended symbols, the unchanged
ABI version, what qi_stft_out_scratch_bytes promises (a pure host function), and the references of
tests/test_gpu_stft_reduced.py themselves."""
import os
import re

import numpy as np
import pytest

import stft_cases as sc
import stft_reduced_cases as rc
from conftest import ROOT

from quantum_inferno_amd import _lib, styx_fft


def _header():
    return open(os.path.join(ROOT, "include", "qi_tfr.h")).read()


def test_header_declares_and_library_exports_the_new_symbols():
    header = _header()
    assert re.search(r"#define\s+QI_TFR_ABI_VERSION\s+1\b", header)
    lib = _lib.load()
    assert lib.qi_abi_version() == 1
    for name in ("qi_stft_out_scratch_bytes", "qi_stft_out"):
        assert re.search(r"\b%s\s*\(int dtype" % name, header), f"{name} is not declared in include/qi_tfr.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES
    # appended: nothing is declared behind them
    assert header.rindex("qi_stft_out(") > max(header.rindex(f"{n}(") for n in ("qi_pool_strip_stats", "qi_stft", "qi_welch"))


def test_python_surface():
    assert callable(styx_fft.StftPlan.reduce) and callable(styx_fft.stft_reductions_from_sig)


@pytest.mark.parametrize("code,esz", [(_lib.QI_F32, 4), (_lib.QI_F64, 8)], ids=["f32", "f64"])
def test_scratch_bytes(code, esz):
    lib = _lib.load()
    channels = 3
    # fused shapes: at least one float64 partial per (record, group of 16 segments, bin)
    for seg, hop, nfft, n in ((2048, 1024, 2048, 1 << 16), (64, 32, 64, 40 * 64 + 1), (64, 32, 512, 193), (100, 1, 128, 777)):
        n_seg = int(lib.qi_stft_segments(n, seg, hop))
        assert n_seg == sc.frame_count(n, seg, hop)
        for want_coef in (0, 1):
            got = int(lib.qi_stft_out_scratch_bytes(code, channels, n, seg, hop, nfft, want_coef, 0))
            assert got >= channels * -(-n_seg // 16) * (nfft // 2 + 1) * 8, (seg, nfft, want_coef, got)
    # hipFFT shapes without `coef`: the panel is formed in scratch, beside what qi_stft needs for the same shape
    for seg, hop, nfft, n in ((200, 100, 300, 601), (8192, 4096, 8192, 3 * 8192 + 1), (32, 16, 32, 97)):
        n_seg = int(lib.qi_stft_segments(n, seg, hop))
        panel = channels * (nfft // 2 + 1) * n_seg * 2 * esz
        base = int(lib.qi_stft_scratch_bytes(code, channels, n, seg, hop, nfft))
        without = int(lib.qi_stft_out_scratch_bytes(code, channels, n, seg, hop, nfft, 0, 0))
        with_coef = int(lib.qi_stft_out_scratch_bytes(code, channels, n, seg, hop, nfft, 1, 1))
        assert without >= base + panel and with_coef >= base and without >= with_coef + panel, (seg, nfft)
    # a geometry with no segment has no scratch
    assert int(lib.qi_stft_out_scratch_bytes(code, channels, 0, 64, 32, 64, 0, 0)) == 0


def test_references_are_usable():
    """Every reference the GPU tests divide by: finite, positive maxima, sum |P log2 P| > 0."""
    count = 0
    for what, ref in rc.every_reference():
        assert all(np.all(np.isfinite(a)) for a in ref), what
        assert np.all(ref.power_band.max(axis=-1) > 0) and np.all(ref.power_time.max(axis=-1) > 0), what
        assert np.all(ref.stats[:, 0] > 0) and np.all(ref.stats[:, 1] > 0) and np.all(ref.abs_plogp > 0), what
        assert np.all(ref.entropy_bits > 0) and np.all(ref.entropy_bits <= np.log2(ref.power_band.shape[-1] * ref.power_time.shape[-1])), what
        count += 1
    assert count == 2 * (len(rc.GROUP_CASES) + 1 + len(rc.GENERAL_NAMES)) + sum(len(rc.plain_cases(d)) for d in sc.DTYPES) + 3


def test_group_cases_keep_several_groups():
    """More than two groups of 16 and a ragged last one, whatever G the kernel picks (G <= 16 divides 16)."""
    for case in rc.GROUP_CASES:
        n_seg = sc.frame_count(case.n, case.seg, case.seg // 2)
        assert n_seg > 32 and n_seg % 16 != 0, (case, n_seg)


def test_zero_segment_case():
    case = rc.spectral_case("seg96_hop96")
    seg, overlap, _ = sc.spectral_geometry(case)
    assert sc.last_segment_all_zero(case.n, seg, seg - overlap)
    for dtype in sc.DTYPES:
        assert np.all(rc.spectral_reduced(case, dtype).power_time[:, -1] == 0)
