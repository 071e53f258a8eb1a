"""GPU tests (-m gpu) of the native engines on band tables that are NOT constant-Q (tests/band_tables.py): sweeps of atom
length against centre frequency and chirp rate on both Gabor banks, sweeps of window width against shift index on the
Stockwell table (ascending, shuffled, with duplicates), population tables around the "few bands join the next class"
rules, single-band tables, a 2000-band linear table, tfr_stx_fft's general tables at a native length, and tables replaced
on a live plan.  Which kernels produce a row is read from the plan (TfrPlan.band_route), never assumed.

References: the float64 table-driven oracle (oracle.gabor_table_fft / stx_table_fft: include/qi_tfr.h's own definition)
-- every row at 2^16 / 2^17 samples, at 2^20 the rows next to a route change --, and the hipFFT engine on the same table,
every row.  Tolerances are the project's (test_gpu_requests / test_gpu_parity.TOL): float32 2e-5 of each row's own
maximum; float64 1e-11 of the panel maximum and 5e-9 of each row's own maximum; bits and reductions as there.
"""
import collections
import concurrent.futures

import numpy as np
import pytest
import torch

import band_tables as bt
from oracle import tfr_oracle as orc
from test_gpu_requests import ATOMS, STX, STYX, _knobs, check_bits, check_direct, check_reductions, check_rows, record

from quantum_inferno_amd import _lib, engine, styx_stx

pytestmark = pytest.mark.gpu

AUTO, HIPFFT = _lib.QI_ENGINE_AUTO, _lib.QI_ENGINE_HIPFFT
BATCH = 8  # records of a batch call: at least the plan's batch_from (4, or 8 for tables with few block bands)


def real(f64):
    return np.float64 if f64 else np.float32


def gabor_plan(n, f64, bank, table, eng=AUTO, channels=1, plan=None):
    nb = len(table["p_re"])
    if plan is None:
        plan = engine.TfrPlan(n, real(f64), None, engine.TfrPlan.workspace_for(n, nb, real(f64), channels), eng)
    plan.set_gabor_bank(bank, np.arange(nb, dtype=np.float64), table["p_re"], table["p_im"], table["omega"], table["amp"])
    return plan


def stx_plan(n, f64, table, eng=AUTO, channels=1, plan=None):
    idx, sigma = table
    if plan is None:
        plan = engine.TfrPlan(n, real(f64), None, engine.TfrPlan.workspace_for(n, len(sigma), real(f64), channels), eng)
    plan.set_stx_table(np.arange(len(sigma), dtype=np.float64), idx, sigma)
    return plan


def category(route):
    """One name per route category of qi_plan_band_route."""
    stage, cls, run_cls, flags = route
    if stage == "block":
        return (f"block/reach{cls}/analytic{_lib.route_analytic(flags)}/narrow{_lib.route_narrow(flags)}/"
                f"{'nowrap' if flags & _lib.ROUTE_NOWRAP else 'wrap'}")
    if stage == "zoom":
        if flags & _lib.ROUTE_F64_ZOOM:
            return f"zoom64/level{cls}/fine{run_cls}" + ("/split" if flags & _lib.ROUTE_SPLIT else "")
        return f"zoom/class{cls}" + ("/split" if flags & _lib.ROUTE_SPLIT else "")
    if stage == "pass2":
        return "pass2/" + ("one-pass", "general", "short-atom")[_lib.route_pass2_kind(flags)]
    assert stage == "inverse", route
    return "hipfft/behind" if flags & _lib.ROUTE_BEHIND else "hipfft/table"


def routes(plan, which, records=1):
    return [plan.band_route(which, j, records) for j in range(len(plan.freq[which]))]


def check_expect(plan, which, expect):
    """The table came out as it was built to: "native" no row on the hipFFT engine, "fallback" every row, "behind" some
    last rows on the hipFFT pass behind the native run."""
    if _knobs() or expect is None:
        return
    nb = len(plan.freq[which])
    inv = plan.stage_bands("inverse")[which]
    cats = [category(r) for r in routes(plan, which)]
    assert {"native": inv == 0, "fallback": inv == nb and set(cats) == {"hipfft/table"},
            "behind": 0 < inv <= 4 and cats[-inv:] == ["hipfft/behind"] * inv and "hipfft/table" not in cats}[expect], (expect, inv, nb)
    assert sum(plan.stage_bands(s)[which] for s in ("zoom", "block", "pass2", "inverse")) == nb


def route_neighbours(cats):
    """Rows next to a route change (the last band of one category and the first of the next), and both ends."""
    rows = {0, len(cats) - 1}
    for j in range(1, len(cats)):
        if cats[j] != cats[j - 1]:
            rows |= {j - 1, j}
    return sorted(rows)


def oracle_rows(fn, rows, workers=8):
    """fn(bands=[...]) -> [len(bands), n] for `rows`, the rows dealt to a few threads (the FFTs release the GIL)."""
    rows = list(rows)
    chunks = [rows[k::workers] for k in range(workers) if rows[k::workers]]
    with concurrent.futures.ThreadPoolExecutor(len(chunks)) as pool:
        parts = list(pool.map(lambda c: fn(bands=c), chunks))
    out = np.empty((len(rows), parts[0].shape[1]), dtype=np.complex128)
    for k, part in enumerate(parts):
        out[k::workers][: len(part)] = part
    return out


def gabor_oracle(x64, table, circular):
    return lambda bands: orc.gabor_table_fft(x64, table["p_re"], table["p_im"], table["omega"], table["amp"], bands=bands,
                                             circular=circular)


def stx_oracle(x64, table):
    return lambda bands: orc.stx_table_fft(x64, table[0], table[1], bands=bands)


def check_requests(nat, ref, name, xt, f64, oracle, rows, what):
    """One table through `coef + bits + reductions`, `coef=False` and `reductions="band"` on the native plan: every row,
    the bits and the reductions against the hipFFT engine, `rows` against the oracle, the reductions against direct sums
    of the stored panel; the lean requests give the same reductions.  Returns the stored panel."""
    a = getattr(nat, name)(xt, coef=True, bits=True, reductions=True)
    b = getattr(ref, name)(xt, coef=True, reductions=True)
    check_rows(a.coef, b.coef, f64, (what, "hipfft"))
    check_bits(a.bits, b.coef, f64, what)
    check_reductions(a, b, f64, what)
    check_direct(a, f64, what)
    if len(rows):
        want = oracle_rows(oracle, rows)
        check_rows(a.coef[0, rows], want, f64, (what, "oracle"))
        check_rows(b.coef[0, rows], want, f64, (what, "hipfft engine against the oracle"))
    a.bits = None
    lean = getattr(nat, name)(xt, coef=False, reductions=True)
    assert lean.coef is None
    check_reductions(lean, b, f64, (what, "coef=False"))
    band = getattr(nat, name)(xt, coef=True, reductions="band")
    assert band.power_time is None
    check_rows(band.coef, b.coef, f64, (what, 'reductions="band"'))
    check_reductions(band, b, f64, (what, 'reductions="band"'))
    del b, lean, band
    return a.coef


# ---- (a) Gabor sweeps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bt.gabor_cases(), ids=lambda c: c[0])
def test_gabor_sweep(case):
    """Reach 3 samples .. 3 n at four centre frequencies (and, at 2^20, chirped rows; six rows outside the block engine's
    analytic domain) on the styx bank and the atoms bank."""
    name, log2n, f64, bank, table, expect = case
    n, nb = 1 << log2n, len(table["p_re"])
    x = record(n, real(f64), 300 + log2n)
    xt = torch.from_numpy(x).cuda()
    nat = gabor_plan(n, f64, bank, table)
    check_expect(nat, bank, expect)
    cats = [category(r) for r in routes(nat, bank)]
    print(name, sorted(collections.Counter(cats).items()))
    ref = gabor_plan(n, f64, bank, table, HIPFFT)
    rows = list(range(nb)) if log2n < 20 else route_neighbours(cats)
    call = "cwt" if bank == STYX else "cwt_atoms"
    check_requests(nat, ref, call, xt, f64, gabor_oracle(x[0].astype(np.float64), table, bank == ATOMS), rows, name)
    nat.close()
    ref.close()


# ---- (b) Stockwell sweeps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bt.stx_cases(), ids=lambda c: c[0])
def test_stx_sweep(case):
    """sigma 1 .. n / 4 at six shift indices, in ascending order, shuffled and with two duplicated rows: each against
    the hipFFT engine (every row) and the oracle; the shuffled panel is the ascending one with its rows permuted (another
    launch order of the same arithmetic: float rounding), the duplicated rows equal their originals."""
    name, log2n, f64, table, expect = case
    n, nb = 1 << log2n, len(table[1])
    x = record(n, real(f64), 400 + log2n)
    xt = torch.from_numpy(x).cuda()
    x64 = x[0].astype(np.float64)
    nat = stx_plan(n, f64, table)
    check_expect(nat, STX, expect)
    cats = [category(r) for r in routes(nat, STX)]
    print(name, sorted(collections.Counter(cats).items()))
    ref = stx_plan(n, f64, table, HIPFFT)
    rows = list(range(nb)) if log2n < 20 else route_neighbours(cats)
    asc = check_requests(nat, ref, "stx", xt, f64, stx_oracle(x64, table), rows, name)
    # shuffled: set on the same (live) plans
    perm = bt.shuffle_permutation(nb)
    shuffled = (table[0][perm], table[1][perm])
    stx_plan(n, f64, shuffled, plan=nat)
    stx_plan(n, f64, shuffled, plan=ref)
    check_expect(nat, STX, expect)
    assert sorted(category(r) for r in routes(nat, STX)) == sorted(cats)  # the same bands, the same routes
    got = check_requests(nat, ref, "stx", xt, f64, stx_oracle(x64, shuffled), rows if log2n < 20 else rows[:8], (name, "shuffled"))
    d = (got[0] - asc[0, torch.from_numpy(perm).cuda()]).abs().amax(dim=1).double()
    worst = float((d / asc[0, torch.from_numpy(perm).cuda()].abs().amax(dim=1).double().clamp_min(1e-300)).max())
    assert worst <= (1e-12 if f64 else 1e-6), (name, "shuffled against ascending", worst)
    del got
    # duplicates
    dup = [1, nb // 2]
    twice = (np.concatenate([table[0], table[0][dup]]), np.concatenate([table[1], table[1][dup]]))
    stx_plan(n, f64, twice, plan=nat)
    check_expect(nat, STX, expect)
    res = nat.stx(xt, coef=True, reductions=True)
    check_direct(res, f64, (name, "duplicates"))
    for k, j in enumerate(dup):  # (a duplicate sits elsewhere in its engine's band list: the same arithmetic, to float rounding)
        d = float((res.coef[0, nb + k] - res.coef[0, j]).abs().max()) / float(res.coef[0, j].abs().max())
        assert d <= (1e-12 if f64 else 1e-6), (name, "duplicate of row", j, d)
    d = (res.coef[0, :nb] - asc[0]).abs().amax(dim=1).double()
    worst = float((d / asc[0].abs().amax(dim=1).double().clamp_min(1e-300)).max())
    assert worst <= (1e-12 if f64 else 1e-6), (name, "duplicates against ascending", worst)
    nat.close()
    ref.close()


# ---- joint call, single record and batch --------------------------------------------------------------------------------
@pytest.mark.parametrize("f64,log2n", [(False, 16), (False, 20), (True, 16)])
def test_joint_call_single_and_batch(f64, log2n):
    """qi_cwt_stx on synthetic tables: a single record against the separate calls; a batch of eight records (the other
    block item cut, twelve bands per workgroup, the 8192-sample long blocks, the short-interpolator zoom classes) against
    the single-record run of one of its records and against the hipFFT engine, every row -- as
    test_native_engine_batch_launches_other_lengths does for the dyadic tables."""
    n = 1 << log2n
    full = bt.gabor_sweep(n, 14)
    gab = full if log2n == 20 else bt.take(full, bt.split_gabor(full, n, f64)[0])
    idx, sigma = bt.stx_sweep(n, 12)
    keep = np.arange(len(sigma)) if log2n == 20 else bt.split_stx(idx, sigma, n)[0]
    stx = (idx[keep], sigma[keep])
    nb = max(len(gab["p_re"]), len(stx[1]))
    x = record(n, real(f64), 500 + log2n, channels=BATCH)
    xt = torch.from_numpy(x).cuda()
    ws = engine.TfrPlan.workspace_for(n, nb, real(f64), BATCH)
    nat = engine.TfrPlan(n, real(f64), None, ws)
    ref = engine.TfrPlan(n, real(f64), None, engine.TfrPlan.workspace_for(n, nb, real(f64), 1), HIPFFT)
    for plan in (nat, ref):
        gabor_plan(n, f64, STYX, gab, plan=plan)
        stx_plan(n, f64, stx, plan=plan)
    check_expect(nat, STYX, "native")
    check_expect(nat, STX, "native")
    if not _knobs():  # the batch takes other routes than the single record where the tables have such bands
        one_r = [category(r) for w in (STYX, STX) for r in routes(nat, w, 1)]
        many_r = [category(r) for w in (STYX, STX) for r in routes(nat, w, BATCH)]
        print("single", sorted(collections.Counter(one_r).items()), "batch", sorted(collections.Counter(many_r).items()))
    pick = 5
    batch = nat.cwt_stx(xt, coef=True, reductions=True)
    one = nat.cwt_stx(xt[pick : pick + 1], coef=True, reductions=True)
    sep = (nat.cwt(xt[pick : pick + 1], coef=True, reductions=True), nat.stx(xt[pick : pick + 1], coef=True, reductions=True))
    tight = 1e-12 if f64 else 1e-5
    for name, b, o, s in (("cwt", batch[0], one[0], sep[0]), ("stx", batch[1], one[1], sep[1])):
        gold = getattr(ref, name)(xt[pick : pick + 1], coef=True, reductions=True)
        peak = gold.coef[0].abs().amax(dim=1).double().clamp_min(1e-300)
        for what, u, v in (("batch against single", b.coef[pick], o.coef[0]), ("joint against separate", o.coef[0], s.coef[0])):
            err = (u - v).abs().amax(dim=1).double() / peak
            assert float(err.max()) <= tight, (name, what, int(err.argmax()), float(err.max()))
        check_rows(b.coef[pick : pick + 1], gold.coef, f64, (name, "batch against hipfft"))
        check_rows(o.coef, gold.coef, f64, (name, "single against hipfft"))
        sliced = engine.TfrResult(frequency_hz=b.frequency_hz, power_band=b.power_band[pick : pick + 1],
                                  power_time=b.power_time[pick : pick + 1], stats=b.stats[pick : pick + 1])
        check_reductions(sliced, gold, f64, (name, "batch"))
        check_reductions(o, gold, f64, (name, "single"))
        del gold
    nat.close()
    ref.close()


# ---- (c) population and single-band tables ------------------------------------------------------------------------------
def zoom_counts(cats, prefix="zoom/class"):
    c = [0] * 7
    for name in cats:
        if name.startswith(prefix):
            c[int(name[len(prefix)])] += 1
    return c


@pytest.mark.parametrize("k", [1, 5, 6, 7])
def test_zoom_class_populations_float32(k):
    """upload_native_table's join rules: tables that keep exactly k bands of one zoom class (before the joins) plus a
    fixed rest (eight bands of every other occupied class, every block band of one centre frequency).  The classes come
    from the plan's own routes of the Stockwell sweep at 2^20 (all of whose occupied classes hold at least six bands, so
    no join has moved them); the population after the joins is what band_tables.join_zoom_classes says, and every row
    agrees with the oracle."""
    n = 1 << 20
    idx, sigma = bt.stx_sweep(n, 30)
    probe = stx_plan(n, False, (idx, sigma))
    cats = [category(r) for r in routes(probe, STX)]
    probe.close()
    before = zoom_counts(cats)
    occupied = [c for c in range(7) if before[c] > 0]
    assert all(before[c] >= 6 for c in occupied) and len(occupied) >= 4, before
    by_class = {c: [j for j, name in enumerate(cats) if name == f"zoom/class{c}"] for c in occupied}
    block = [j for j, name in enumerate(cats) if name.startswith("block/")][:12]
    x = record(n, np.float32, 600 + k)
    xt = torch.from_numpy(x).cuda()
    for chosen in occupied:
        rows = sorted(by_class[chosen][:k] + [j for c in occupied if c != chosen for j in by_class[c][:8]] + block)
        table = (idx[rows], sigma[rows])
        want = [0] * 7
        for c in occupied:
            want[c] = min(k if c == chosen else 8, before[c])
        plan = stx_plan(n, False, table)
        check_expect(plan, STX, "native")
        got = zoom_counts([category(r) for r in routes(plan, STX)])
        if not _knobs():
            assert got == bt.join_zoom_classes(want), (chosen, k, want, got)
        res = plan.stx(xt, coef=True, reductions=True)
        check_rows(res.coef[0], oracle_rows(stx_oracle(x[0].astype(np.float64), table), range(len(rows))), False, (chosen, k))
        check_direct(res, False, (chosen, k))
        big = plan.stx(xt.expand(4, n).contiguous(), coef=True)  # four records: classes 5 and 6 run with their own interpolators
        assert float((big.coef[3] - res.coef[0]).abs().amax(dim=1).div(res.coef[0].abs().amax(dim=1)).max()) <= 1e-5, (chosen, k)
        plan.close()
        del res, big


def fine_counts(cats):
    c = [0] * 6
    for name in cats:
        if name.startswith("zoom64/level0/fine"):
            c[int(name[len("zoom64/level0/fine"):])] += 1
    return c


@pytest.mark.parametrize("k", [1, 3, 4])
def test_fine_class_populations_float64(k):
    """The float64 zoom's fine classes ("fewer than four bands join the next longer interpolator"): tables that keep
    exactly k bands of one fine class of the coarsest grid (before the joins) plus six of every other and six block bands.
    The classes come from the plan's routes of the Stockwell sweep at 2^16 (every fine class of which holds at least four
    bands, so no join has moved them); the population after the joins is exactly what band_tables.join_fine_classes says
    -- k = 4 stays, k = 1 / 3 land in the next longer interpolator and nowhere else --, and every row agrees with the
    oracle."""
    n = 1 << 16
    idx, sigma = bt.stx_sweep(n, 60, sigma_lo=3.0)
    probe = stx_plan(n, True, (idx, sigma))
    cats = [category(r) for r in routes(probe, STX)]
    probe.close()
    before = fine_counts(cats)
    occupied = [c for c in (0, 2, 3, 4, 5) if before[c] > 0]
    assert occupied == [0, 2, 3, 4, 5] and all(before[c] >= 6 for c in occupied), before
    by_class = {c: [j for j, name in enumerate(cats) if name == f"zoom64/level0/fine{c}"] for c in occupied}
    block = [j for j, name in enumerate(cats) if name.startswith("block/")][:6]
    x = record(n, np.float64, 700 + k)
    xt = torch.from_numpy(x).cuda()
    for chosen in occupied:
        rows = sorted(by_class[chosen][:k] + [j for c in occupied if c != chosen for j in by_class[c][:6]] + block)
        table = (idx[rows], sigma[rows])
        want = [0] * 6
        for c in occupied:
            want[c] = k if c == chosen else 6
        plan = stx_plan(n, True, table)
        check_expect(plan, STX, "native")
        after = [category(r) for r in routes(plan, STX)]
        if not _knobs():
            assert fine_counts(after) == bt.join_fine_classes(want), (chosen, k, want, fine_counts(after))
            assert sum(fine_counts(after)) + len(block) == len(rows) and sum(a.startswith("block/") for a in after) == len(block)
        res = plan.stx(xt, coef=True, reductions=True)
        check_rows(res.coef[0], oracle_rows(stx_oracle(x[0], table), range(len(rows))), True, (chosen, k))
        check_direct(res, True, (chosen, k))
        plan.close()


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("k,where,expect", [(0, "last", "native"), (4, "last", "behind"), (5, "last", "fallback"), (4, "middle", "fallback")])
def test_stockwell_two_pass_row_populations(f64, k, where, expect):
    """build_stx_tables at 2^16 samples: up to four LAST rows that need the two-pass kernels get a hipFFT pass behind the
    native run; five, or four in the middle, send the whole table to the hipFFT engine.  Every row against the oracle."""
    n = 1 << 16
    table = bt.stx_two_pass_population(n, k, where)
    x = record(n, real(f64), 800 + k)
    plan = stx_plan(n, f64, table)
    check_expect(plan, STX, expect)
    res = plan.stx(torch.from_numpy(x).cuda(), coef=True, bits=True, reductions=True)
    want = oracle_rows(stx_oracle(x[0].astype(np.float64), table), range(len(table[1])))
    check_rows(res.coef[0], want, f64, (k, where))
    check_bits(res.bits[0], torch.from_numpy(want).cuda(), f64, (k, where))
    check_direct(res, f64, (k, where))
    plan.close()


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("log2n", [16, 20])
@pytest.mark.parametrize("kind", ["zoom", "block", "split"])
def test_single_band_tables(kind, log2n, f64):
    """B = 1: one zoom band, one block band, one atom cut by the record.  A split band needs a block band in its table
    (its edge items ride in the block launch): alone it is a two-pass band at 2^20 and a hipFFT band elsewhere.  So is the
    long atom in float64 (band_tables.split_gabor: the 2^-50 support of a long atom at 0.3 pi is the whole row); the float64
    zoom's single band is the Stockwell one below."""
    n = 1 << log2n
    table = bt.single_band(kind, n)
    x = record(n, real(f64), 900 + log2n)
    plan = gabor_plan(n, f64, STYX, table)
    cat = category(plan.band_route(STYX, 0))
    if not _knobs():
        if kind == "split" or (kind == "zoom" and f64):
            assert cat == ("pass2/general" if log2n == 20 else "hipfft/table"), cat
        else:
            assert cat.startswith("zoom/" if kind == "zoom" else "block/"), cat
    res = plan.cwt(torch.from_numpy(x).cuda(), coef=True, bits=True, reductions=True)
    want = gabor_oracle(x[0].astype(np.float64), table, False)([0])
    check_rows(res.coef[0], want, f64, (kind, cat))
    check_bits(res.bits[0], torch.from_numpy(want).cuda(), f64, kind)
    check_direct(res, f64, kind)
    plan.close()


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("log2n", [16, 20])
@pytest.mark.parametrize("kind", ["zoom", "block"])
def test_single_band_stockwell_tables(kind, log2n, f64):
    """B = 1 on the Stockwell side: one zoom band (float64: the float64 zoom), one block band; a single record and a batch."""
    n = 1 << log2n
    table = bt.single_stx_band(kind, n)
    x = record(n, real(f64), 950 + log2n, channels=BATCH)
    plan = stx_plan(n, f64, table, channels=BATCH)
    cat = category(plan.band_route(STX, 0))
    if not _knobs():
        assert cat.startswith(("zoom/", "zoom64/") if kind == "zoom" else "block/"), cat
    res = plan.stx(torch.from_numpy(x).cuda(), coef=True, bits=True, reductions=True)
    for c in (0, BATCH - 1):
        want = stx_oracle(x[c].astype(np.float64), table)([0])
        check_rows(res.coef[c], want, f64, (kind, cat, c))
        check_bits(res.bits[c], torch.from_numpy(want).cuda(), f64, kind)
    check_direct(res, f64, kind)
    one = plan.stx(torch.from_numpy(x[:1]).cuda(), coef=True, reductions=True)
    check_rows(one.coef, res.coef[:1], f64, (kind, "single against batch"))
    check_direct(one, f64, kind)
    plan.close()


# ---- (d) a large linear table -------------------------------------------------------------------------------------------
def test_large_linear_stockwell_table():
    """2000 bands by tfr_stx_fft's linear rule at 2^16 samples, float32 (hundreds of bands per block reach group and zoom
    class: plane, slot and partial indexing): no row on the hipFFT engine, every row against the hipFFT engine, every
    50th against the oracle."""
    n = 1 << 16
    f, idx, sigma = bt.linear_stx_table(n)
    assert len(f) == 2000
    x = record(n, np.float32, 1000)
    xt = torch.from_numpy(x).cuda()
    nat = stx_plan(n, False, (idx, sigma))
    assert nat.stage_bands("inverse")[STX] == 0
    check_expect(nat, STX, "native")
    print(sorted(collections.Counter(category(r) for r in routes(nat, STX)).items()))
    ref = stx_plan(n, False, (idx, sigma), HIPFFT)
    check_requests(nat, ref, "stx", xt, False, stx_oracle(x[0].astype(np.float64), (idx, sigma)), list(range(0, 2000, 50)) + [1999],
                   "linear")
    nat.close()
    ref.close()


# ---- tfr_stx_fft at a native length -------------------------------------------------------------------------------------
# what the plan must make of each of band_tables.GENERAL_SETS at 2^16 samples
GENERAL_EXPECT = {
    "lin": "native", "inferno": "native", "qpr": "native", "const_width": "native", "q2p1": "native",
    "geo": "behind",  # (order 3: the top band's window, sigma = 2.60 samples, is the one row for the hipFFT pass behind the run)
    "short_windows": "fallback",  # (order 2: ten windows shorter than 2.75 samples -> the whole table on the hipFFT engine)
}
ORACLE_KW = dict(scale_order_input="order", frequency_min="f_min", frequency_max="f_max", frequency_step="f_step", factor_q="q",
                 power_p="p", power_r="r", is_geometric="geometric", is_inferno="inferno")


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name", sorted(bt.GENERAL_SETS))
def test_general_stockwell_at_a_native_length(golden, name, f64):
    """styx_stx.tfr_stx_fft at n_fft = 2^16 (its plan is QI_ENGINE_AUTO: the native engines classify the table): linear,
    geometric, inferno, q/p/r-tuned, constant-width (power_r = 0) and q = 2, p = 1 tables -- widths that are not ~ 1 / f --
    against orc.stx_general and the reference's own rows (tests/golden/stx_general_n65536.npz); the route is read from a
    plan built with the same table (styx_stx.stx_general_table) and asserted."""
    g = golden("stx_general_n65536.npz")
    kw, expect = bt.GENERAL_SETS[name], GENERAL_EXPECT[name]
    n, fs = 1 << 16, 1000.0
    sig = orc.synth_chirp(n, fs, dtype=np.float64) + 0.25 * np.random.default_rng(65536).standard_normal(n)
    assert np.array_equal(sig[:: n // 4096], g["sig_samples"])
    x = sig.astype(real(f64))
    f, idx, sigma, f_fft, _ = styx_stx.stx_general_table(n, 1 / fs, **kw)
    assert np.array_equal(f, g[f"{name}_f"]) and np.array_equal(f_fft, g[f"{name}_ffft"])
    plan = stx_plan(n, f64, (idx, sigma))
    check_expect(plan, STX, expect)
    plan.close()
    tfr, psd, f2, f_fft2, win = styx_stx.tfr_stx_fft(x, 1 / fs, n_fft_in=n, **kw)
    assert np.array_equal(f2, f) and np.array_equal(f_fft2, f_fft) and tfr.dtype == np.complex128
    want = orc.stx_general(x.astype(np.float64), 1 / fs, **{ORACLE_KW[k]: v for k, v in kw.items()})[0]
    check_rows(torch.from_numpy(tfr), want, f64, name)
    if f64:  # the reference's own rows (its record is the float64 one)
        rows, tsel = g[f"{name}_rowsel"], g["tsel"]
        ref = g[f"{name}_rows"]
        assert np.max(np.abs(tfr[rows][:, tsel] - ref)) <= 1e-11 * np.abs(want).max(), name
        assert np.allclose((np.abs(tfr) ** 2).sum(axis=1), g[f"{name}_psum_band"], rtol=1e-9), name


# ---- tables replaced on a live plan -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64,log2n", [(False, 16), (False, 20), (True, 16)])
def test_tables_replaced_on_a_live_plan(f64, log2n):
    """Set tables A, run the joint call (single record and batch: the joint item lists of both cuts are built); replace
    the Stockwell table by B, run; replace the styx table by B, run; set A again, run: the last run equals the first bit
    for bit, and every B run equals a fresh plan's (table_gen, dual_valid, d_band_slots)."""
    n = 1 << log2n
    def tables(steps, widths, lo):
        full = bt.gabor_sweep(n, steps)
        gab = full if log2n == 20 else bt.take(full, bt.split_gabor(full, n, f64)[0])
        idx, sigma = bt.stx_sweep(n, widths, sigma_lo=lo)
        return gab, (idx, sigma)
    a_gab, a_stx = tables(12, 10, 3.0)
    b_gab, b_stx = tables(7, 5, 4.0)
    b_gab = bt.take(b_gab, np.arange(len(b_gab["p_re"]))[::-1])  # (another order as well)
    x = record(n, real(f64), 1100 + log2n, channels=BATCH)
    xt = torch.from_numpy(x).cuda()
    nb = max(len(a_gab["p_re"]), len(a_stx[1]))
    ws = engine.TfrPlan.workspace_for(n, nb, real(f64), BATCH)

    def fresh(gab, stx):
        plan = engine.TfrPlan(n, real(f64), None, ws)
        gabor_plan(n, f64, STYX, gab, plan=plan)
        stx_plan(n, f64, stx, plan=plan)
        return plan

    def run(plan):
        out = []
        for sig in (xt[:1], xt):
            c, s = plan.cwt_stx(sig, coef=True, reductions=True)
            out += [c.coef.clone(), s.coef.clone(), c.reduced.clone(), s.reduced.clone()]
        return out

    def same(u, v, what):
        for k, (p, q) in enumerate(zip(u, v)):
            assert torch.equal(p, q), (what, k)

    live = fresh(a_gab, a_stx)
    first = run(live)
    stx_plan(n, f64, b_stx, plan=live)
    other = fresh(a_gab, b_stx)
    same(run(live), run(other), "Stockwell table replaced")
    other.close()
    gabor_plan(n, f64, STYX, b_gab, plan=live)
    other = fresh(b_gab, b_stx)
    same(run(live), run(other), "styx table replaced")
    other.close()
    gabor_plan(n, f64, STYX, a_gab, plan=live)
    stx_plan(n, f64, a_stx, plan=live)
    same(run(live), first, "tables A again")
    live.close()


# ---- (e) coverage census ------------------------------------------------------------------------------------------------
# Route categories some table of this file must reach (qi_plan_band_route's stage / class / flag combinations), by prefix.
REQUIRED = [
    "block/reach1/", "block/reach2/", "block/reach4/", "block/reach8/",
    "/analytic0/", "/analytic1/", "/analytic2/", "/narrow0/", "/narrow1/", "/narrow2/", "/nowrap", "/wrap",
    "zoom/class0", "zoom/class1", "zoom/class2", "zoom/class3", "zoom/class4", "zoom/class5", "zoom/class6", "/split",
    "zoom64/level0/", "zoom64/level1/", "zoom64/level2/", "zoom64/level3/", "zoom64/level4/",
    "zoom64/level0/fine0", "zoom64/level0/fine2", "zoom64/level0/fine3", "zoom64/level0/fine4", "zoom64/level0/fine5",
    "zoom64/level1/fine1", "/fine-1",
    "pass2/general", "pass2/short-atom", "hipfft/table", "hipfft/behind",
]
# A category no table can reach, with the reason from the plan code (qi_plan_build.hip): dead code as the library is configured.
UNREACHABLE = {
    "pass2/one-pass": "make_native_table marks a band for the one-pass loader when its support is <= kOnePassMax = 12288 bins and "
                      "zoom_class refuses it; at the lengths where pass 2 runs (Lf = 2^20, 2^21) the zoom grids of levels 0..3 take "
                      "any support up to Lf / 32 >= 32768 bins, and in float64 upload_native_table gives every such band to the "
                      "float64 zoom (support <= Lf / 16).  Only the short-atom table (zoom_class returns -1 for it) still uses the "
                      "loader, and its rows are reported as pass2/short-atom.  Reachable with QI_NATIVE_ZOOM=0 / QI_NATIVE_Z64=0 only.",
}
def test_coverage_census():
    """Every route category of qi_plan_band_route holds at least one band in some table of this file (single-record and
    batch routes, both precisions); what no table reaches is named in UNREACHABLE with the reason, and the test asserts that it stays unreached.
    (zoom/class4, the finest float32 grid, is reached by the chirped rows of reach 1100 .. 1300 at 2^16 / 2^17 only: a
    Gaussian with such a support is a block band, and where the two-pass kernels exist zoom_class stops at level 3.)  Plans are built, no
    transform runs."""
    if _knobs():  # (engine knobs move bands between the engines on purpose)
        return
    seen = collections.Counter()
    per_table = {}

    def tally(name, plan, which):
        for records in (1, BATCH):
            cats = collections.Counter(category(r) for r in routes(plan, which, records))
            seen.update(cats)
            per_table[(name, records)] = dict(cats)

    for name, log2n, f64, bank, table, _ in bt.gabor_cases():
        plan = gabor_plan(1 << log2n, f64, bank, table)
        tally(name, plan, bank)
        plan.close()
    for name, log2n, f64, table, _ in bt.stx_cases():
        plan = stx_plan(1 << log2n, f64, table)
        tally(name, plan, STX)
        plan.close()
    for f64 in (False, True):
        for k, where in ((4, "last"), (5, "last")):
            plan = stx_plan(1 << 16, f64, bt.stx_two_pass_population(1 << 16, k, where))
            tally(f"two_pass_rows_{k}_{where}_{'f64' if f64 else 'f32'}", plan, STX)
            plan.close()
    plan = stx_plan(1 << 16, False, bt.linear_stx_table(1 << 16)[1:])
    tally("linear_2000", plan, STX)
    plan.close()
    for (name, records), cats in sorted(per_table.items()):
        print(f"{name} x{records}: {sorted(cats.items())}")
    print("census:", sorted(seen.items()))
    missing = [want for want in REQUIRED if not any(want in name for name in seen)]
    assert not missing, missing
    for name in UNREACHABLE:  # (a category declared unreachable that a table does reach must move to REQUIRED)
        assert not any(name in got for got in seen), name
