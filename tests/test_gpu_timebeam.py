"""Time-domain delay-and-sum on the device (include/qi_timebeam.h): engine.time_beam_power and engine.time_beam_traces on
every case of tests/timebeam_cases.py against the float64 NumPy restatement, in both precisions and both normalisations;
whole-number cases bit for bit; the header's contract (the row's position and the row count, the number of windows, a record
and its copy from a later sample on, either side of the LDS bound, two runs); NaN masks, samples no tap reads, guarded rows;
beamform.fisher_timeline and beamform.beam_traces_delay on the plane wave of tests/beam_cases.py; the two stream-order cases
of tests/timebeam_stream_cases.py."""
import numpy as np
import pytest
import torch

import stream_order as so
import timebeam_cases as tb
import timebeam_stream_cases as tsc

from quantum_inferno_amd import beamform, engine

pytestmark = pytest.mark.gpu
TORCH = {"float32": torch.float32, "float64": torch.float64}


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases' arrays are read-only)
    return t if dtype is None else t.to(TORCH[dtype])


def host(t):
    return t.detach().cpu().numpy()


def call_power(x, taps, shift, phase, reach, win, hop, normalize):
    return engine.time_beam_power(x, shift, phase, taps, win, hop, reach, normalize=normalize, peaks=True)


def case_tensors(cid, dtype):
    x, taps, shift, phase = tb.inputs(cid)
    return dev(x, dtype), dev(taps, dtype), dev(shift), dev(phase)


def deviation(got, want):
    """The largest |got - want| as a fraction of the largest |want|; the NaN masks must agree."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return float(np.nanmax(np.abs(got - want), initial=0.0)) / tb.largest(want)


# ---- against the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tb.DTYPES)
@pytest.mark.parametrize("cid", tb.ids())
def test_power_and_traces_against_the_restatement(cid, dtype):
    case, want, tol = tb.by_id(cid), tb.restated(cid), tb.TOL[dtype]
    x, taps, shift, phase = case_tensors(cid, dtype)
    for normalize, ref in ((False, want.mean_square), (True, want.semblance)):
        power, index, value = call_power(x, taps, shift, phase, case.reach, case.win, case.hop, normalize)
        assert power.dtype == TORCH[dtype] and tuple(power.shape) == ref.shape and index.dtype == torch.int64
        err = deviation(host(power).astype(np.float64), ref)
        w_index, w_value = tb.peaks_of(ref)
        sure = tb.margins(ref) > tol * tb.largest(ref)
        v_err = deviation(host(value).astype(np.float64), w_value)
        print(f"timebeam {cid} {dtype} normalize {int(normalize)}: power {err:.3g}, peak value {v_err:.3g}, {int(sure.sum())} of {len(sure)} peaks held")
        assert err <= tol and v_err <= tol
        assert np.array_equal(host(index)[sure], w_index[sure])
        assert case.win == 1 or sure.all()
        # the peak outputs are the power's own: the value is the entry at the index
        assert so.same_bits(value, power[torch.arange(power.shape[0], device=power.device), index])
    traces = engine.time_beam_traces(x, shift, phase, taps, case.reach)
    assert traces.dtype == TORCH[dtype] and tuple(traces.shape) == (case.G, case.n)
    t_err = deviation(host(traces).astype(np.float64), want.traces)
    print(f"timebeam {cid} {dtype}: traces {t_err:.3g}")
    assert t_err <= tol


def test_numpy_in_numpy_out_and_outputs_alone():
    cid = "n700_c5_g65_w100h37_p64t2_r60"
    case = tb.by_id(cid)
    x, taps, shift, phase = tb.inputs(cid)
    power, index, value = engine.time_beam_power(x.astype(np.float32), shift, phase, taps, case.win, case.hop, case.reach)
    assert isinstance(power, np.ndarray) and power.dtype == np.float32 and index.dtype == np.int64 and isinstance(value, np.ndarray)
    alone = engine.time_beam_power(x.astype(np.float32), shift, phase, taps, case.win, case.hop, case.reach, peaks=False)
    assert isinstance(alone, np.ndarray) and np.array_equal(alone, power, equal_nan=True)
    traces = engine.time_beam_traces(x, shift, phase, taps, case.reach)
    assert isinstance(traces, np.ndarray) and traces.dtype == np.float64 and traces.shape == (case.G, case.n)


# ---- exact cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tb.DTYPES)
@pytest.mark.parametrize("C", (2, 4, 16))
def test_whole_numbers_bit_for_bit(C, dtype):
    x, shift, phase = tb.exact_inputs(C)
    n = x.shape[1]
    for taps in (np.ones((1, 1)), tb.bank(1, 8)):  # the impulse, alone and among seven zero taps
        for win, hop in ((64, 32), (256, 256), (512, 1)):
            w_traces, w_power = tb.exact_restate(x, shift, win, hop)
            for reach in (n, tb.LDS_MAX_SHIFT + 1):
                power, index, value = call_power(dev(x, dtype), dev(taps, dtype), dev(shift), dev(phase), reach, win, hop, False)
                assert np.array_equal(host(power), w_power.astype(dtype)), (taps.shape, win, hop, reach)
                assert not host(power)[:, -1].any()  # wholly off the record: exactly zero
                sem = host(call_power(dev(x, dtype), dev(taps, dtype), dev(shift), dev(phase), reach, win, hop, True)[0])
                assert np.isnan(sem[:, -1]).all() and not np.isnan(sem[:, :-1]).any()
                traces = host(engine.time_beam_traces(dev(x, dtype), dev(shift), dev(phase), dev(taps, dtype), reach))
                assert np.array_equal(traces, w_traces.astype(dtype)), (taps.shape, reach)
                assert np.array_equal(traces[0], x.mean(axis=0).astype(dtype))  # zero delays: the mean of the records


@pytest.mark.parametrize("dtype", tb.DTYPES)
def test_zero_delays_give_the_mean_of_the_records(dtype):
    x = tb.inputs("n3001_c5_g65_w100h37_p256t8_r60")[0]
    zeros = np.zeros((3, x.shape[0]), dtype=np.int32)
    traces = host(engine.time_beam_traces(dev(x, dtype), dev(zeros), dev(zeros), dev(tb.bank(64, 8), dtype), 0))
    mean = x.astype(dtype).astype(np.float64).mean(axis=0)
    assert np.abs(traces - mean).max() <= 4 * np.finfo(dtype).eps * np.abs(x).sum(axis=0).max()
    assert np.array_equal(traces[0], traces[1]) and np.array_equal(traces[0], traces[2])


# ---- the contract ------------------------------------------------------------------------------------------------------------------------
CONTRACT_SHAPES = ((64, 32, 8, 64), (100, 37, 4, 64), (512, 256, 8, 64), (256, 256, 16, 256))  # (win, hop, T, P)


def contract_inputs(dtype, T, P, C=5, n=2048, G=257, seed=0):
    rng = np.random.default_rng([43, T, P, seed])
    x = rng.standard_normal((C, n))
    shift = rng.integers(-tb.SHIFT, tb.SHIFT + 1, (G, C)).astype(np.int32)
    phase = rng.integers(0, P, (G, C)).astype(np.int32)
    return x, dev(x, dtype), dev(tb.bank(P, T), dtype), shift, phase


@pytest.mark.parametrize("dtype", tb.DTYPES)
@pytest.mark.parametrize("win,hop,T,P", CONTRACT_SHAPES)
def test_a_row_has_the_same_bits_wherever_it_stands(win, hop, T, P, dtype):
    """One row alone, and at positions 0, 64 and 256 of a grid of 257; either side of the LDS bound; K = 1 against K = 65 for the
    traces; two runs."""
    _, x, taps, shift, phase = contract_inputs(dtype, T, P)
    row = np.array([17, -60, 0, 33, 60], dtype=np.int32), np.array([5 % P, P - 1, 0, P // 2, 1 % P], dtype=np.int32)
    alone = [call_power(x, taps, dev(row[0][None]), dev(row[1][None]), tb.SHIFT, win, hop, nz)[0] for nz in (False, True)]
    trace_alone = engine.time_beam_traces(x, dev(row[0][None]), dev(row[1][None]), taps, tb.SHIFT)
    for position in (0, 64, 256):
        s, p = shift.copy(), phase.copy()
        s[position], p[position] = row
        for nz in (False, True):
            for reach in (tb.SHIFT, tb.LDS_MAX_SHIFT, tb.LDS_MAX_SHIFT + 1):
                power = call_power(x, taps, dev(s), dev(p), reach, win, hop, nz)[0]
                assert so.same_bits(power[:, position:position + 1].contiguous(), alone[int(nz)]), (position, nz, reach)
            again = call_power(x, taps, dev(s), dev(p), tb.SHIFT, win, hop, nz)
            first = call_power(x, taps, dev(s), dev(p), tb.SHIFT, win, hop, nz)
            assert all(so.same_bits(a, b) for a, b in zip(again, first))
        traces = engine.time_beam_traces(x, dev(s[:65] if position < 65 else s[-65:]), dev(p[:65] if position < 65 else p[-65:]), taps, tb.SHIFT)
        where = position if position < 65 else 64
        assert so.same_bits(traces[where:where + 1].contiguous(), trace_alone), position
        slow = engine.time_beam_traces(x, dev(s[:65] if position < 65 else s[-65:]), dev(p[:65] if position < 65 else p[-65:]), taps, tb.MAX_SHIFT)
        assert so.same_bits(slow, traces)


@pytest.mark.parametrize("dtype", tb.DTYPES)
@pytest.mark.parametrize("win,hop,T,P", CONTRACT_SHAPES)
def test_windows_do_not_depend_on_the_record_around_them(win, hop, T, P, dtype):
    """The record cut after a window (fewer windows), and the record's copy from sample k hop on (window w becomes w - k)."""
    x64, x, taps, shift, phase = contract_inputs(dtype, T, P, G=17, seed=1)
    n = x64.shape[1]
    s, p = dev(shift), dev(phase)
    reach_back = tb.SHIFT + T  # no read of a window starts further before it, or ends further behind it
    for nz in (False, True):
        whole = call_power(x, taps, s, p, tb.SHIFT, win, hop, nz)[0]
        nwin = whole.shape[0]
        # cut after window `last`: the windows whose reads end inside the shorter record keep their bits
        last = nwin // 2
        cut = last * hop + win
        short = call_power(x[:, :cut].contiguous(), taps, s, p, tb.SHIFT, win, hop, nz)[0]
        assert short.shape[0] == last + 1 < nwin
        keep = [w for w in range(last + 1) if w * hop + win + reach_back <= cut]
        assert len(keep) >= 2 and so.same_bits(short[keep].contiguous(), whole[keep].contiguous())
        # the copy from k hop on
        k = max(1, 300 // hop)
        moved = call_power(x[:, k * hop:].contiguous(), taps, s, p, tb.SHIFT, win, hop, nz)[0]
        assert moved.shape[0] == nwin - k
        keep = [w for w in range(k, nwin) if w * hop - reach_back >= k * hop]
        assert len(keep) >= 2 and so.same_bits(moved[[w - k for w in keep]].contiguous(), whole[keep].contiguous())
    assert n == 2048


# ---- NaN, unread samples, guarded rows ------------------------------------------------------------------------------------------------------
NAN_CASE = "n2048_c3_g17_w512h256_p64t8_r60"
NAN_PLACES = ((0, 0), (1, 255), (2, 256), (0, 511), (1, 2047), (2, 1100))  # (sensor, sample): the record's ends, a chunk's edges


@pytest.mark.parametrize("dtype", tb.DTYPES)
@pytest.mark.parametrize("win,hop", ((64, 32), (512, 256)))
def test_a_nan_poisons_exactly_what_its_taps_touch(win, hop, dtype):
    case = tb.by_id(NAN_CASE)
    x, taps, shift, phase = tb.inputs(case.id)
    shift, phase = shift.copy(), phase.copy()
    phase[0] = 0  # the impulse: a NaN under a zero tap poisons too
    for sensor, sample in NAN_PLACES:
        xn = x.copy()
        xn[sensor, sample] = np.nan
        want = tb.restate(xn, taps, shift, phase, case.reach, win, hop)
        assert np.isnan(want.semblance).any() and not np.isnan(want.semblance).all(axis=0).any()  # some windows of every row, never all
        assert case.G <= np.isnan(want.traces).sum() <= case.G * case.T
        for reach in (case.reach, tb.LDS_MAX_SHIFT + 1):
            for nz, ref in ((False, want.mean_square), (True, want.semblance)):
                power = host(call_power(dev(xn, dtype), dev(taps, dtype), dev(shift), dev(phase), reach, win, hop, nz)[0])
                assert np.array_equal(np.isnan(power), np.isnan(ref)), (sensor, sample, reach, nz)
            traces = host(engine.time_beam_traces(dev(xn, dtype), dev(shift), dev(phase), dev(taps, dtype), reach))
            assert np.array_equal(np.isnan(traces), np.isnan(want.traces)), (sensor, sample, reach)


@pytest.mark.parametrize("dtype", tb.DTYPES)
def test_samples_no_tap_reads_are_never_looked_at(dtype):
    rng = np.random.default_rng(47)
    C, n, T, P, win, hop = 4, 700, 8, 64, 100, 37
    x = rng.standard_normal((C, n))
    shift = np.array([[10, -10, 25, -31], [12, -14, 20, -40]], dtype=np.int32)
    phase = np.array([[3, 60, 0, 17], [0, 1, 63, 32]], dtype=np.int32)
    taps = tb.bank(P, T)
    covered = (tb.windows(n, win, hop) - 1) * hop + win
    for t_count, run in ((covered, lambda r: call_power(dev(r, dtype), dev(taps, dtype), dev(shift), dev(phase), 40, win, hop, True)[0]),
                         (n, lambda r: engine.time_beam_traces(dev(r, dtype), dev(shift), dev(phase), dev(taps, dtype), 40))):
        unread = ~tb.samples_read(n, T, shift, phase, P, 40, t_count)
        assert unread[0, :7].all() and unread[1, -6:].all() and 20 <= unread.sum() < 120
        planted = x.copy()
        planted[unread] = 1e30
        assert so.same_bits(run(planted), run(x))


@pytest.mark.parametrize("dtype", tb.DTYPES)
def test_a_row_beyond_its_bounds_is_nan_and_alone(dtype):
    """|shift| = max_shift + 1, phase -1 and phase P: guarded reads with ordinary results -- that row NaN, the others untouched."""
    cid = "n700_c5_g17_w100h37_p64t8_r1025"
    case = tb.by_id(cid)
    x, taps, shift, phase = case_tensors(cid, dtype)
    for reach in (tb.SHIFT, tb.LDS_MAX_SHIFT + 1):
        clean_power = call_power(x, taps, shift, phase, reach, case.win, case.hop, True)[0]
        clean_traces = engine.time_beam_traces(x, shift, phase, taps, reach)
        for row, sensor, table, value in ((3, 0, "shift", reach + 1), (16, 4, "shift", -reach - 1), (0, 2, "phase", -1), (15, 1, "phase", case.P),
                                          (8, 3, "shift", -2 ** 31), (9, 0, "phase", 2 ** 31 - 1)):
            s, p = shift.clone(), phase.clone()
            (s if table == "shift" else p)[row, sensor] = value
            others = [g for g in range(case.G) if g != row]
            for nz in (False, True):
                power = call_power(x, taps, s, p, reach, case.win, case.hop, nz)[0]
                assert torch.isnan(power[:, row]).all(), (row, table, value)
                if nz:
                    assert so.same_bits(power[:, others].contiguous(), clean_power[:, others].contiguous())
            traces = engine.time_beam_traces(x, s, p, taps, reach)
            assert torch.isnan(traces[row]).all() and so.same_bits(traces[others].contiguous(), clean_traces[others].contiguous())


# ---- the wrappers on the plane wave -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tb.DTYPES)
@pytest.mark.parametrize("win,hop", tb.PW_WINDOWS)
def test_fisher_timeline_on_the_plane_wave(win, hop, dtype):
    records = tb.pw_records().astype(dtype)
    time_s, semblance, index, value, fisher = beamform.fisher_timeline(records, tb.PW_FS, tb.PW_POSITIONS_M, tb.pw_slowness(), win, hop)
    want = tb.pw_restated(win, hop).semblance
    assert all(isinstance(a, np.ndarray) for a in (time_s, semblance, index, value, fisher))  # NumPy in, NumPy out
    assert semblance.dtype == np.dtype(dtype) and semblance.shape == want.shape and index.dtype == np.int64
    margin = float(tb.margins(semblance).min())
    print(f"timebeam fisher_timeline {win}/{hop} {dtype}: margin {margin:.3f}, deviation {deviation(semblance.astype(np.float64), want):.3g}, "
          f"F {fisher.min():.1f} .. {fisher.max():.1f}")
    assert (index == tb.pw_true_index()).all() and margin >= tb.PW_MARGIN
    assert deviation(semblance.astype(np.float64), want) <= tb.TOL[dtype]
    assert np.array_equal(value, semblance[np.arange(len(index)), index])
    assert np.allclose(fisher, 4 * value.astype(np.float64) / (1 - value.astype(np.float64)), rtol=1e-5)
    assert np.allclose(time_s, (np.arange(len(index)) * hop + 0.5 * (win - 1)) / tb.PW_FS)
    if (win, hop) == tb.PW_WINDOWS[0]:
        half = beamform.fisher_timeline(records, tb.PW_FS, tb.PW_POSITIONS_M, tb.pw_slowness(), win)  # the default hop
        assert np.array_equal(half[1], semblance)
        on_device = beamform.fisher_timeline(dev(records), tb.PW_FS, tb.PW_POSITIONS_M, tb.pw_slowness(), win, hop)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in on_device[1:]) and np.array_equal(host(on_device[1]), semblance)
        whole, _, w_index, _, _ = beamform.fisher_timeline(records, tb.PW_FS, tb.PW_POSITIONS_M, tb.pw_slowness(), win, hop, phases=1, taps=1)
        assert (w_index == tb.pw_true_index()).all()
        banded = beamform.fisher_timeline(records, tb.PW_FS, tb.PW_POSITIONS_M, tb.pw_slowness(), win, hop, band_hz=(25.0, 225.0))
        assert banded[1].dtype == np.float64 and (banded[2] == tb.pw_true_index()).all()


@pytest.mark.parametrize("dtype", tb.DTYPES)
def test_beam_traces_delay_on_the_plane_wave(dtype):
    rows, (shift, phase, reach) = tb.pw_steer_tables(tb.PW_BANK[0])
    records, source = tb.pw_low_passed()
    traces = beamform.beam_traces_delay(records.astype(dtype), tb.PW_FS, tb.PW_POSITIONS_M, rows)
    assert isinstance(traces, np.ndarray) and traces.dtype == np.dtype(dtype) and traces.shape == (2, tb.PW_N)
    at_source, at_centre = tb.rms_from(traces[0].astype(np.float64), source), tb.rms_from(traces[1].astype(np.float64), source)
    want = tb.restate(records, tb.bank(*tb.PW_BANK), shift, phase, reach, tb.PW_N, 1).traces
    white = beamform.beam_traces_delay(dev(tb.pw_records(), dtype), tb.PW_FS, tb.PW_POSITIONS_M, rows)
    assert isinstance(white, torch.Tensor) and white.is_cuda
    print(f"timebeam beam_traces_delay {dtype}: low-passed {at_source:.4f} at the source, {at_centre:.3f} at the centre, deviation "
          f"{deviation(traces.astype(np.float64), want):.3g}; white records {tb.relative_rms(host(white)[0].astype(np.float64), tb.PW_INTERIOR):.3f}")
    assert at_source <= 0.05 and at_centre >= 0.8
    assert deviation(traces.astype(np.float64), want) <= tb.TOL[dtype]


# ---- stream order ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", tsc.TABLE.ids())
def test_ordered_behind_a_delayed_producer(cid):
    assert tsc.TABLE.by_id(cid).asynchronous
    so.ordered_behind_producer(tsc.TABLE, cid)


def teardown_module(module):
    so.clear_cases()
