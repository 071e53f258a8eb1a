"""Scaling and peak picking on the GPU: qi_find_peaks through ctypes against the reference's recorded results
(tests/golden/peaks.npz: every case, 1 and 3 records, both dtypes), across a batch of 65 records, its determinism, small
capacities, absent outputs and argument checks, plateaus longer than one step of the summary walk, and the
reference-signature wrappers end to end.  Every buffer is pre-filled with a sentinel and carries a guard column."""
import numpy as np
import pytest
import torch

import peak_cases as pc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import picker

pytestmark = pytest.mark.gpu

GUARD = 1  # elements behind each buffer that the call must leave alone
POS_FILL, VAL_FILL, SCALED_FILL, COUNT_FILL = -7, -3.0e300, 2.0 ** 100, -9  # (2^100: exact in float32 too)
LOG2_TOL = 1e-9  # bits: the project's float64 log2 tolerance


def find(x, kind, height_kind=pc.HEIGHT_NONE, height=0.0, capacity=None, scaled=True, positions=True, values=True,
         extra_scratch=0, short_scratch=0, expect=0, scale=None):
    """qi_find_peaks on a device tensor x [C, n] -> dict of the whole buffers (device), after checking the guards.
    `expect`: the status the call must return."""
    lib = _lib.require_gpu()
    dev = x.device
    n_ch, n = x.shape
    code = _lib.QI_F64 if x.dtype == torch.float64 else _lib.QI_F32
    cap = max((n - 1) // 2, 1) if capacity is None else capacity  # (n < 3 holds no peak: one column stays the sentinel)
    need = int(lib.qi_peaks_scratch_bytes(code, n_ch, n))
    words = need // 8 + extra_scratch
    sdtype = torch.float64 if kind in ("log2", "log2max") else x.dtype
    scratch = torch.full((words,), float("nan"), dtype=torch.float64, device=dev)
    out = {
        "scaled": torch.full((n_ch * n + GUARD,), SCALED_FILL, dtype=sdtype, device=dev) if scaled else None,
        "positions": torch.full((n_ch * max(cap, 0) + GUARD,), POS_FILL, dtype=torch.int64, device=dev) if positions else None,
        "values": torch.full((n_ch * max(cap, 0) + GUARD,), VAL_FILL, dtype=torch.float64, device=dev) if values else None,
        "counts": torch.full((n_ch + GUARD,), COUNT_FILL, dtype=torch.int64, device=dev),
    }
    with torch.cuda.device(dev):
        rc = lib.qi_find_peaks(code, dev.index, _lib.ptr(x), n_ch, n, pc.SCALE[kind] if scale is None else scale, 0.0, height_kind,
                               float(height), _lib.ptr(out["scaled"]), _lib.ptr(out["positions"]), _lib.ptr(out["values"]), cap,
                               _lib.ptr(out["counts"]), _lib.ptr(scratch), words * 8 - short_scratch, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc == expect, (rc, lib.qi_last_error())
    for name, fill in (("scaled", SCALED_FILL), ("positions", POS_FILL), ("values", VAL_FILL), ("counts", COUNT_FILL)):
        if out[name] is not None:
            assert out[name][-1].item() == fill, f"the guard of {name} was written"
    out["cap"] = cap
    return out


def rows_of(out, n_ch):
    """(counts [C], [positions of record r], [values of record r], scaled [C, n] or None) on the host, after checking that
    every column behind a record's peaks still holds the sentinel."""
    cap = out["cap"]
    counts = out["counts"][:-GUARD].cpu().numpy()
    assert (counts >= 0).all()
    pos = out["positions"][:-GUARD].view(n_ch, cap).cpu().numpy() if out["positions"] is not None else None
    val = out["values"][:-GUARD].view(n_ch, cap).cpu().numpy() if out["values"] is not None else None
    prow, vrow = [], []
    for r in range(n_ch):
        k = min(int(counts[r]), cap)
        if pos is not None:
            assert (pos[r, k:] == POS_FILL).all(), "a column behind the peaks was written"
            prow.append(pos[r, :k])
        if val is not None:
            assert (val[r, k:] == VAL_FILL).all(), "a column behind the peaks was written"
            vrow.append(val[r, :k])
    scaled = None
    if out["scaled"] is not None:
        scaled = out["scaled"][:-GUARD].view(n_ch, -1).cpu().numpy()
        assert not (scaled == SCALED_FILL).any(), "a sample of the scaled record was not written"
    return counts, prow, vrow, scaled


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(bits)[~nan], b.view(bits)[~nan])  # (any NaN is a NaN)


def check_scaled(got, want, x, kind, where):
    """sig*: bit for bit.  log2: within 1e-9 bits; log2max: within 1e-9 (1 + |s|) / |max| (the quotient of two values that
    are each within 1e-9 bits); what is infinite or NaN in the reference is the same here."""
    if kind in pc.SIG_TYPES:
        with np.errstate(invalid="ignore"):
            diff = np.nanmax(np.abs(np.where(np.isfinite(want), got.astype(np.float64) - want, 0.0)), initial=0.0)
        print(f"{where}: scaled max |difference| {diff:.3e} (bit for bit asked)")
        assert same_bits(got, want), where
        return
    assert got.dtype == np.float64
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), where
    tol = np.full(want.shape, LOG2_TOL)
    if kind == "log2max":
        top = np.array([np.nanmax(u) if np.isfinite(u).any() else np.nan for u in pc.transform_ref(x, "log2")])
        tol = LOG2_TOL * (1.0 + np.abs(want)) / np.abs(top)[:, None]
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    print(f"{where}: scaled max |difference| {np.max(err[fin], initial=0.0):.3e}, smallest bound {np.min(tol[fin], initial=np.inf):.3e}")
    assert np.all(err[fin] <= tol[fin]), where


@pytest.fixture(scope="module")
def g(golden):
    return golden("peaks.npz")


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_every_case_equals_the_reference(g, dtype):
    for tag in pc.tags(dtype):
        x_host = g[pc.x_key(dtype, tag)]
        x = torch.from_numpy(x_host).cuda()
        want = pc.unpack(g[pc.peaks_key(dtype, tag)], pc.case_ids(tag))
        for records in (1, pc.RECORDS):
            xr = x[:records].contiguous()
            for kind in pc.types_of(tag):
                for h in pc.HEIGHTS:
                    out = find(xr, kind, pc.HEIGHT_NONE if h is None else pc.HEIGHT_ABS, 0.0 if h is None else h)
                    counts, pos, val, scaled = rows_of(out, records)
                    where = f"{dtype} {tag} {kind} height {h} records {records}"
                    if h is None:
                        check_scaled(scaled, g[pc.scaled_key(dtype, tag, kind)][:records], x_host[:records], kind, where)
                    for r in range(records):
                        ref = want["ext", kind, h][r]
                        assert counts[r] == len(ref) and np.array_equal(pos[r], ref), (where, r)
                        assert np.array_equal(val[r], scaled[r][pos[r]].astype(np.float64)), (where, r)
            if not pc.has_bits(tag):
                continue
            for scaling in pc.BITS_SCALINGS:
                for t in pc.BITS_THRESHOLDS:
                    kind_h = (pc.HEIGHT_BELOW_MAX, float(t)) if scaling == "log2" else (pc.HEIGHT_BELOW_RAW_MAX, float(2 ** t))
                    counts, pos, val, _ = rows_of(find(xr, "log2", *kind_h), records)
                    for d in pc.BITS_DISTANCES:
                        for r in range(records):
                            keep = picker.select_by_distance(pos[r], val[r], d)
                            assert np.array_equal(pos[r][keep], want["bits", scaling, t, d][r]), (dtype, tag, scaling, t, d, records, r)


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_batch_of_65_records(g, dtype):
    """65 records, the fixture's three cyclically, row r scaled by 2^(r mod 4) (exact): the positions of a row are the
    fixture's, and for the sig* kinds the scaled values are too, bit for bit -- the power of two cancels in the division.
    (log2max: without the gain, which moves the sign of the maximum of the log2 values and with it the order.)"""
    rows = torch.arange(65, device="cuda")
    for tag in pc.tags(dtype):
        x = torch.from_numpy(g[pc.x_key(dtype, tag)]).cuda()
        want = pc.unpack(g[pc.peaks_key(dtype, tag)], pc.case_ids(tag))
        for kind in pc.types_of(tag):
            gain = torch.pow(2.0, (rows % 4).to(x.dtype))[:, None] if kind != "log2max" else 1.0
            xb = (x[rows % pc.RECORDS] * gain).contiguous()
            for h in (None, 0.7) if kind in pc.SIG_TYPES else (None,):
                out = find(xb, kind, pc.HEIGHT_NONE if h is None else pc.HEIGHT_ABS, 0.0 if h is None else h)
                counts, pos, val, scaled = rows_of(out, 65)
                bad = [r for r in range(65) if not np.array_equal(pos[r], want["ext", kind, h][r % pc.RECORDS])]
                assert not bad, (dtype, tag, kind, h, bad)
                if kind in pc.SIG_TYPES:
                    rec = g[pc.scaled_key(dtype, tag, kind)]
                    bad = [r for r in range(65) if not same_bits(scaled[r], rec[r % pc.RECORDS])]
                    assert not bad, (dtype, tag, kind, bad)


def test_same_bits_when_repeated_and_with_more_scratch(g):
    for dtype, kind in (("float64", "log2max"), ("float32", "sigmin"), ("float32", "log2")):
        x = torch.from_numpy(g[pc.x_key(dtype, f"n{3 * pc.TILE + 17}")]).cuda()
        first = find(x, kind, pc.HEIGHT_BELOW_MAX, 0.5)
        for again in (find(x, kind, pc.HEIGHT_BELOW_MAX, 0.5), find(x, kind, pc.HEIGHT_BELOW_MAX, 0.5, extra_scratch=4099)):
            assert torch.equal(first["positions"], again["positions"]) and torch.equal(first["counts"], again["counts"])
            assert same_bits(first["values"].cpu().numpy(), again["values"].cpu().numpy())
            assert same_bits(first["scaled"].cpu().numpy(), again["scaled"].cpu().numpy())


def test_capacity_smaller_than_the_count(g):
    for dtype in pc.DTYPES:
        tag = f"n{3 * pc.TILE + 17}"
        x = torch.from_numpy(g[pc.x_key(dtype, tag)]).cuda()
        want = pc.unpack(g[pc.peaks_key(dtype, tag)], pc.case_ids(tag))["ext", "sigabs", None]
        assert len(want[0]) > 70 and len(want[1]) > 5
        for cap in (1, 5, 70):
            counts, pos, val, scaled = rows_of(find(x, "sigabs", capacity=cap), pc.RECORDS)  # (rows_of: the rest of a row is untouched)
            for r in range(pc.RECORDS):
                assert counts[r] == len(want[r])  # the total, whatever the capacity
                assert np.array_equal(pos[r], want[r][:cap])
                assert np.array_equal(val[r], scaled[r][pos[r]].astype(np.float64))


def test_absent_outputs(g):
    tag = f"n{pc.TILE + 1}"
    x = torch.from_numpy(g[pc.x_key("float32", tag)]).cuda()
    full = rows_of(find(x, "sigmax", pc.HEIGHT_ABS, 0.3), pc.RECORDS)
    counts, pos, val, scaled = rows_of(find(x, "sigmax", pc.HEIGHT_ABS, 0.3, scaled=False), pc.RECORDS)
    assert scaled is None and np.array_equal(counts, full[0])
    assert all(np.array_equal(a, b) for a, b in zip(pos, full[1])) and all(np.array_equal(a, b) for a, b in zip(val, full[2]))
    counts, pos, val, scaled = rows_of(find(x, "sigmax", pc.HEIGHT_ABS, 0.3, values=False), pc.RECORDS)
    assert val == [] and all(np.array_equal(a, b) for a, b in zip(pos, full[1])) and same_bits(scaled, full[3])
    counts, pos, val, scaled = rows_of(find(x, "sigmax", pc.HEIGHT_ABS, 0.3, positions=False), pc.RECORDS)
    assert pos == [] and all(np.array_equal(a, b) for a, b in zip(val, full[2]))
    # the scaling alone: no positions, no values, no capacity; the counts are still the counts
    counts, pos, val, scaled = rows_of(find(x, "sigmax", pc.HEIGHT_ABS, 0.3, capacity=0, positions=False, values=False), pc.RECORDS)
    assert np.array_equal(counts, full[0]) and same_bits(scaled, g[pc.scaled_key("float32", tag, "sigmax")])
    counts, _, val, _ = rows_of(find(x, "sigmax", capacity=0, positions=False), pc.RECORDS)  # values with no room: nothing stored
    assert all(len(v) == 0 for v in val)


def test_bad_arguments_are_refused(g):
    lib = _lib.load()
    x = torch.from_numpy(g[pc.x_key("float64", f"n{pc.TILE}")]).cuda()
    find(x, "sigmax", scale=5, expect=-1)
    assert b"scaling" in lib.qi_last_error()
    find(x, "sigmax", scale=-1, expect=-1)
    find(x, "sigmax", height_kind=4, expect=-1)
    assert b"height" in lib.qi_last_error()
    find(x, "sigmax", height_kind=-1, expect=-1)
    find(x, "sigmax", short_scratch=1, expect=-1)
    assert b"scratch" in lib.qi_last_error()
    find(x, "sigmax", capacity=-1, positions=False, values=False, expect=-1)
    assert b"capacity" in lib.qi_last_error()
    find(x, "sigmax", capacity=0, expect=-1)  # positions with a capacity of 0
    assert b"capacity of 0" in lib.qi_last_error()
    rows_of(find(x.to(torch.float32), "sigmax"), pc.RECORDS)


def plateau_record(n, start, stop, dtype):
    x = np.sin(0.37 * np.arange(n)).astype(dtype) * dtype(0.5)
    x[start:stop] = 2.0
    return x


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_plateaus_longer_than_one_walk_step(dtype):
    """Runs over more than 64 whole tiles (the wave follows the tile summaries 64 at a time), and over a tile count that is
    no multiple of the tiles a workgroup owns: one that ends inside a later tile, one that ends exactly on a tile boundary,
    one that reaches the last sample, against the restatement."""
    t = pc.TILE
    real = np.float64 if dtype == "float64" else np.float32
    n = 135 * t + 3
    x = np.stack([plateau_record(n, 5, 131 * t + 9, real), plateau_record(n, t + 2, 70 * t, real), plateau_record(n, 3 * t - 1, n, real),
                  plateau_record(n, 2, 64 * t + 1, real)])
    assert pc.log2_neighbours_clear(x)
    for kind in ("sigmax", "log2"):
        _, want, want_val = pc.peaks_ref(x, kind)
        assert (5 + 131 * t + 8) // 2 in want[0] and (t + 2 + 70 * t - 1) // 2 in want[1] and not any(p >= 3 * t - 1 for p in want[2])
        counts, pos, val, scaled = rows_of(find(torch.from_numpy(x).cuda(), kind), 4)
        for r in range(4):
            assert counts[r] == len(want[r]) and np.array_equal(pos[r], want[r]), (dtype, kind, r)
            assert np.array_equal(val[r], scaled[r][pos[r]].astype(np.float64))


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_relative_heights_of_every_scaling_equal_the_restatement(g, dtype):
    """max(s) - h and max(x) - h with every scaling (the reference uses them with log2 only): the thresholds are formed per
    record on the device.  h keeps the candidates of the restatement 1e-6 away from the threshold (asserted here)."""
    for tag in (f"n{pc.TILE + 1}", f"n{3 * pc.TILE + 17}"):
        x_host = g[pc.x_key(dtype, tag)]
        x = torch.from_numpy(x_host).cuda()
        for kind in pc.TYPES:
            for hk, h in ((pc.HEIGHT_BELOW_MAX, 0.40625), (pc.HEIGHT_BELOW_RAW_MAX, 2.5)):
                scaled, all_pos, _ = pc.peaks_ref(x_host, kind)
                _, want, _ = pc.peaks_ref(x_host, kind, hk, h)
                for row, s, p in zip(x_host, scaled, all_pos):
                    thr = pc.threshold_ref(row, s, hk, h)
                    assert not np.any(np.abs(s[p].astype(np.float64) - thr) <= pc.MARGIN), (dtype, tag, kind, hk)
                counts, pos, _, _ = rows_of(find(x, kind, hk, h), pc.RECORDS)
                for r in range(pc.RECORDS):
                    assert counts[r] == len(want[r]) and np.array_equal(pos[r], want[r]), (dtype, tag, kind, hk, r)


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_wrappers_end_to_end(g, dtype, capsys):
    tdtype = torch.float64 if dtype == "float64" else torch.float32
    for tag in (f"n{3 * pc.TILE + 17}", f"n{pc.TILE + 1}", "n4", "n1") + (("div",) if dtype == "float32" else ()):
        x = g[pc.x_key(dtype, tag)]
        want = pc.unpack(g[pc.peaks_key(dtype, tag)], pc.case_ids(tag))
        dev = torch.from_numpy(x).cuda()
        for kind in pc.types_of(tag):
            rec = g[pc.scaled_key(dtype, tag, kind)]
            s = picker.scale_signal_by_extraction_type(x, kind)  # NumPy [C, n] in
            assert isinstance(s, np.ndarray) and s.dtype == rec.dtype and s.shape == rec.shape
            check_scaled(s, rec, x, kind, f"wrapper {dtype} {tag} {kind}")
            one = picker.scale_signal_by_extraction_type(x[1], kind)  # NumPy [n] in
            assert isinstance(one, np.ndarray) and one.shape == (x.shape[1],) and same_bits(one, s[1])
            sd = picker.scale_signal_by_extraction_type(dev, kind)  # CUDA in
            assert isinstance(sd, torch.Tensor) and sd.is_cuda and tuple(sd.shape) == x.shape and same_bits(sd.cpu().numpy(), s)
            for h in pc.HEIGHTS:
                ref = want["ext", kind, h]
                rows = picker.find_peaks_by_extraction_type(x, kind, h)
                assert isinstance(rows, list) and len(rows) == pc.RECORDS
                assert all(isinstance(p, np.ndarray) and p.dtype == np.int64 and np.array_equal(p, w) for p, w in zip(rows, ref))
                one = picker.find_peaks_by_extraction_type(x[2], kind, h)
                assert isinstance(one, np.ndarray) and one.dtype == np.int64 and np.array_equal(one, ref[2])
                rows = picker.find_peaks_by_extraction_type(dev, kind, h)
                assert isinstance(rows, list) and all(isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.int64 for p in rows)
                assert all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(rows, ref))
                one = picker.find_peaks_by_extraction_type(dev[0], kind, h)
                assert isinstance(one, torch.Tensor) and one.is_cuda and np.array_equal(one.cpu().numpy(), ref[0])
        if not pc.has_bits(tag):
            continue
        for scaling in pc.BITS_SCALINGS:
            for t in pc.BITS_THRESHOLDS:
                for d in pc.BITS_DISTANCES:
                    ref = want["bits", scaling, t, d]
                    rows = picker.find_peaks_with_bits(x, pc.SAMPLE_RATE_HZ, scaling, t, float(d))
                    assert all(isinstance(p, np.ndarray) and p.dtype == np.int64 and np.array_equal(p, w) for p, w in zip(rows, ref))
                    one = picker.find_peaks_with_bits(dev[1], pc.SAMPLE_RATE_HZ, scaling, t, float(d))
                    assert isinstance(one, torch.Tensor) and one.is_cuda and one.dtype == torch.int64
                    assert np.array_equal(one.cpu().numpy(), ref[1])
    x = g[pc.x_key(dtype, "n4")]
    assert np.array_equal(picker.find_peaks_by_extraction_type(x[1], "sigmoid", None),  # an unknown type is read as sigmax
                          picker.find_peaks_by_extraction_type(x[1], "sigmax", None))
    assert "Invalid extraction type.  Defaulting to sigmax." in capsys.readouterr().out
    ints = np.array([[0, 3, 1, 4, 4, 2, 9, 0], [5, 1, 1, 7, 2, 2, 8, 3]], dtype=np.int16)  # integers are read as float64
    s = picker.scale_signal_by_extraction_type(ints, "sigmax")
    assert s.dtype == np.float64 and np.array_equal(s, ints / np.max(ints, axis=1, keepdims=True))
    assert [p.tolist() for p in picker.find_peaks_by_extraction_type(ints, "sigmax", None)] == [[1, 3, 6], [3, 6]]
    pos, val, counts, scaled = engine.find_peaks(torch.from_numpy(x).cuda(), "sigabs", want_scaled=True)
    assert pos.dtype == torch.int64 and val.dtype == torch.float64 and counts.dtype == torch.int64 and scaled.dtype == tdtype
    assert tuple(pos.shape) == tuple(val.shape) == (pc.RECORDS, 1) and tuple(counts.shape) == (pc.RECORDS,) and pos.is_cuda


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_bandpass_wrapper(g, dtype):
    """find_peaks_by_extraction_type_with_bandpass is find_peaks_by_extraction_type(apply_bandpass(..)) exactly, and the
    reference's recorded picks: the generator kept 1e-6 between every candidate and its height, and the device's filtered
    record is the reference's to a few ulp (test_gpu_filter.py)."""
    x = g[pc.x_key(dtype, "bp")]
    ids = pc.bp_ids(g, dtype)
    want = pc.unpack(g[pc.peaks_key(dtype, "bp")], ids)
    for name, kind, h in ids:
        band, order = pc.BP_DESIGNS[name]
        rows = picker.find_peaks_by_extraction_type_with_bandpass(x, band, pc.FS_BP, order, kind, h)
        two = picker.find_peaks_by_extraction_type(picker.apply_bandpass(x, band, pc.FS_BP, order), kind, h)
        assert len(rows) == len(two) == pc.RECORDS
        for r in range(pc.RECORDS):
            assert isinstance(rows[r], np.ndarray) and rows[r].dtype == np.int64
            assert np.array_equal(rows[r], two[r]), (dtype, name, kind, h, r)
            assert np.array_equal(rows[r], want[name, kind, h][r]), (dtype, name, kind, h, r)
    name, kind, h = ids[0]
    band, order = pc.BP_DESIGNS[name]
    one = picker.find_peaks_by_extraction_type_with_bandpass(torch.from_numpy(x[1]).cuda(), band, pc.FS_BP, order, kind, h)
    assert isinstance(one, torch.Tensor) and one.is_cuda and np.array_equal(one.cpu().numpy(), want[name, kind, h][1])
