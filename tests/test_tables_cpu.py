"""CPU tests of the synthetic band tables (tests/band_tables.py) that tests/test_gpu_tables.py runs on the native engines."""
import concurrent.futures

import numpy as np
import pytest

import band_tables as bt
from oracle import tfr_oracle as orc

ROW32 = 2e-5  # the float32 tolerance of the GPU tests: of each row's own maximum
FS = 1000.0


def _record32(n, seed):
    x = orc.synth_chirp(n, FS, 0, 1, np.float64) + 0.25 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


def _worst_rows(n, nb, single, double, workers=8):
    """max over time of |single - double| / max |double| per row, the rows dealt to a few threads."""
    def part(rows):
        a, b = single(rows), double(rows)
        return np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)

    chunks = [list(range(nb))[k::workers] for k in range(workers)]
    chunks = [c for c in chunks if c]
    with concurrent.futures.ThreadPoolExecutor(len(chunks)) as pool:
        parts = list(pool.map(part, chunks))
    out = np.empty(nb)
    for k, p in enumerate(parts):
        out[k::workers][: len(p)] = p
    return out


def _f32_tables():
    out = []
    for name, log2n, f64, bank, table, _ in bt.gabor_cases():
        if not f64:
            out.append(pytest.param("gabor", log2n, bank, table, id=name))
    for name, log2n, f64, table, _ in bt.stx_cases():
        if not f64:
            out.append(pytest.param("stx", log2n, 2, table, id=name))
    out.append(pytest.param("stx", 16, 2, bt.linear_stx_table(1 << 16)[1:], id="linear_2000"))
    for k, where in ((4, "last"), (5, "last"), (4, "middle")):
        out.append(pytest.param("stx", 16, 2, bt.stx_two_pass_population(1 << 16, k, where), id=f"two_pass_{k}_{where}"))
    from quantum_inferno_amd import styx_stx

    for name, kw in sorted(bt.GENERAL_SETS.items()):  # tfr_stx_fft's tables at 2^16 (test_general_stockwell_at_a_native_length)
        out.append(pytest.param("stx", 16, 2, styx_stx.stx_general_table(1 << 16, 1 / FS, **kw)[1:3], id=f"general_{name}"))
    return out


@pytest.mark.parametrize("kind,log2n,bank,table", _f32_tables())
def test_single_precision_restatement_stays_within_half_the_float32_tolerance(kind, log2n, bank, table):
    """The arithmetic is not the limit of the float32 tolerance on these tables: the oracle's own algorithm in single
    precision (scipy.fft on float32 / complex64) stays within HALF of 2e-5 of each row's maximum on EVERY band of the
    sweep, linear, two-pass-row and tfr_stx_fft tables the GPU tests run in float32 (their joint, replacement, population
    and single-band tables are subsets or coarser samplings of these sweeps), on the kind of record they use (chirp +
    0.25 noise).  Measured on the
    Gabor sweep at 2^16: worst row 1.3e-6, median 3e-7.  A GPU failure on one of these tables therefore points at the
    engine, not at the table."""
    n = 1 << log2n
    x32 = _record32(n, 300 + log2n)
    x64 = x32.astype(np.float64)
    if kind == "gabor":
        nb = len(table["p_re"])
        single = lambda rows: bt.gabor_table_fft32(x32, table, rows, circular=bank == 1)
        double = lambda rows: orc.gabor_table_fft(x64, table["p_re"], table["p_im"], table["omega"], table["amp"], bands=rows,
                                                  circular=bank == 1)
    else:
        nb = len(table[1])
        single = lambda rows: bt.stx_table_fft32(x32, table[0], table[1], rows)
        double = lambda rows: orc.stx_table_fft(x64, table[0], table[1], bands=rows)
    worst = _worst_rows(n, nb, single, double)
    print(f"worst row {worst.max():.2e} (row {int(worst.argmax())}), median {np.median(worst):.2e}")
    assert worst.max() <= 0.5 * ROW32, (int(worst.argmax()), float(worst.max()))


def test_join_rule_mirror():
    """band_tables.join_zoom_classes on hand-worked cases of upload_native_table's rule."""
    assert bt.join_zoom_classes([8, 8, 6, 0, 0, 8, 1]) == [8, 8, 6, 0, 0, 9, 0]
    assert bt.join_zoom_classes([8, 8, 6, 0, 0, 5, 0]) == [13, 8, 6, 0, 0, 0, 0]
    assert bt.join_zoom_classes([8, 8, 6, 0, 0, 3, 2]) == [13, 8, 6, 0, 0, 0, 0]  # 6 -> 5 (5 bands: still few) -> 0
    assert bt.join_zoom_classes([5, 8, 6, 0, 0, 0, 0]) == [0, 13, 6, 0, 0, 0, 0]
    assert bt.join_zoom_classes([5, 0, 6, 0, 0, 0, 0]) == [0, 0, 11, 0, 0, 0, 0]  # two levels up
    assert bt.join_zoom_classes([5, 0, 0, 6, 0, 0, 0]) == [5, 0, 0, 6, 0, 0, 0]   # three up: stays
    assert bt.join_zoom_classes([0, 0, 1, 0, 0, 0, 0]) == [0, 0, 1, 0, 0, 0, 0]
    assert bt.join_zoom_classes([2, 3, 8, 0, 0, 0, 0]) == [0, 0, 13, 0, 0, 0, 0]  # 0 -> 1 (5 bands) -> 2
    # the float64 fine classes: fewer than four join the next longer interpolator, class 2 the 16-tap class
    assert bt.join_fine_classes([6, 9, 6, 6, 6, 4]) == [6, 9, 6, 6, 6, 4]
    assert bt.join_fine_classes([6, 9, 6, 6, 6, 3]) == [6, 9, 6, 6, 9, 0]
    assert bt.join_fine_classes([6, 9, 1, 6, 6, 6]) == [7, 9, 0, 6, 6, 6]
    assert bt.join_fine_classes([6, 0, 6, 6, 1, 1]) == [6, 0, 6, 8, 0, 0]  # 5 -> 4 (2 bands: still few) -> 3
    assert bt.join_fine_classes([1, 0, 3, 0, 0, 0]) == [4, 0, 0, 0, 0, 0]


def test_sweeps_are_deterministic_and_not_constant_q():
    n = 1 << 16
    a, b = bt.gabor_sweep(n, 20, outside=False), bt.gabor_sweep(n, 20, outside=False)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # atom length and centre frequency are independent: every centre frequency meets every reach
    for om in bt.OMEGAS:
        sel = a["omega"] == om * np.pi
        assert sel.sum() == 20 and np.allclose(np.sqrt(30 * bt.LN2 / a["p_re"][sel]), np.geomspace(3.0, 3.0 * n, 20))
    idx, sigma = bt.stx_sweep(n, 10)
    perm = bt.shuffle_permutation(len(idx))
    si, ss = bt.stx_sweep(n, 10, "shuffled")
    assert np.array_equal(si, idx[perm]) and np.array_equal(ss, sigma[perm]) and not np.array_equal(perm, np.arange(len(idx)))
    di, ds = bt.stx_sweep(n, 10, "duplicates")
    assert len(di) == len(idx) + 2 and ds[-2] == sigma[1] and di[-1] == idx[len(idx) // 2]
    assert set(idx) == set(bt.stx_shifts(n)) and idx.min() >= 0 and idx.max() < n
