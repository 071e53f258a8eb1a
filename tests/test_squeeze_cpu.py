"""Synchrosqueezing without a GPU: the exports of include/qi_squeeze.h and the census of tests/squeeze_stream_cases.py against
that header, every refusal of the three calls and the size query's verdicts, the case table's coverage and the condition
the GPU test of the fused call relies on (the share of elements near an edge), scales_dyadic.squeeze_bin_edges against its
restatement, the restatements of tests/squeeze_cases.py against a dense contraction and on planted values, and the method
through the restatement on the repository's own CPU panels: the tone's concentration, the chirp's ridge, and what the
Stockwell panel's carrier has to be."""
import ctypes
import os
import re

import numpy as np
import pytest

import squeeze_cases as sq
import squeeze_stream_cases as ssc
from stream_table import header_functions, stream_functions

from quantum_inferno_amd._lib import SQUEEZE_PROTOTYPES  # noqa: F401  (the feature's table: without it nothing here has a subject)

ROOT = sq.ROOT
HEADER = "qi_squeeze.h"
OTHER_HEADERS = ("qi_tfr.h", "qi_array.h", "qi_beam.h", "qi_adaptive.h", "qi_subspace.h", "qi_steer.h", "qi_windows.h", "qi_lags.h",
                 "qi_bands.h", "qi_timebeam.h")
NAMES = {"qi_tfr_squeeze_scratch_bytes", "qi_tfr_ifreq", "qi_tfr_squeeze", "qi_tfr_synchrosqueeze"}


# ---- the header, the exports, the stream census ---------------------------------------------------------------------------------------
def test_library_exports_the_squeeze_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == NAMES
    assert declared == set(_lib.SQUEEZE_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.ADAPTIVE_PROTOTYPES, _lib.SUBSPACE_PROTOTYPES,
                  _lib.STEER_PROTOTYPES, _lib.WINDOW_PROTOTYPES, _lib.LAG_PROTOTYPES, _lib.BAND_PROTOTYPES, _lib.TIMEBEAM_PROTOTYPES):
        assert not declared & set(table)
    for other in OTHER_HEADERS:
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_squeeze.h but not exported"
        assert getattr(lib, name).argtypes == _lib.SQUEEZE_PROTOTYPES[name][1], f"{name}: load() did not attach the table"
        assert len(_lib.SQUEEZE_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    text = sq.header_text()
    assert '#include "qi_tfr.h"' in text and "Contract on the results" in text and "Out of scope" in text
    for name, value in (("QI_SQUEEZE_MAX_BINS", _lib.SQUEEZE_MAX_BINS), ("QI_SQUEEZE_MAX_BANDS", _lib.SQUEEZE_MAX_BANDS),
                        ("QI_SQUEEZE_TILE", _lib.SQUEEZE_TILE)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert sq.TILE == _lib.SQUEEZE_TILE
    assert (sq.MAX_BINS, sq.MAX_BANDS) == (_lib.SQUEEZE_MAX_BINS, _lib.SQUEEZE_MAX_BANDS)
    with open(os.path.join(ROOT, "quantum_inferno_amd", "_build.py")) as fh:
        build = fh.read()
    assert '"qi_squeeze.h"' in build and '"qi_squeeze.hip"' in build
    assert re.search(r'"qi_squeeze\.hip": \("-ffp-contract=off",\)', build)  # a product is rounded before it is added
    with open(os.path.join(ROOT, "quantum_inferno_amd", "csrc", "qi_api_ops.hip")) as fh:
        assert '#include "qi_squeeze.h"' in fh.read()  # included where the other plan-less headers are


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    import stream_order as so

    assert ssc.TABLE.header == HEADER and ssc.TABLE.complex_input
    assert stream_functions(HEADER) == ["qi_tfr_ifreq", "qi_tfr_squeeze", "qi_tfr_synchrosqueeze"]
    assert ssc.TABLE.named_functions() == stream_functions(HEADER)
    assert ssc.TABLE.ids() == ["tfr_ifreq-f32-carriers", "tfr_squeeze-f64-given", "tfr_synchrosqueeze-f32-tables"]
    for case in ssc.TABLE.cases:
        assert len(case.functions) == 1 and callable(case.build) and case.asynchronous and case.engine is None, case.id
    assert ssc.COLUMNS % sq.TILE and ssc.COLUMNS > 4 * sq.TILE
    assert ssc.BINS["squeeze"] > 1 and ssc.BINS["synchrosqueeze"] > 1
    assert ssc.TABLE not in so.TABLES  # (that tuple's census is pinned elsewhere; these cases run in tests/test_gpu_squeeze.py)


def test_case_table_covers_what_the_kernel_branches_on(capsys):
    cases = sq.CASES
    assert {c.n for c in cases} == {2, 3, sq.TILE - 1, sq.TILE, sq.TILE + 1, 700, 3001}
    assert {c.nb for c in cases} == {1, 5, 24, 71} and {c.C for c in cases} == {1, 3}
    assert len(set(sq.ids())) == len(cases) <= 16 and max(c.n for c in cases) <= 3001  # (x two precisions: about 30 runs)
    counts = {c.nbin for c in cases}
    assert counts == {1, 7, 31, 32, 33, 64, 65, 568} and max(counts) <= sq.MAX_BINS
    # more than one tile, a ragged tile, more bands than a wave has lanes, three records and a column with its partner alone,
    # each with few bins and with many
    for few in (True, False):
        mine = [c for c in cases if (c.nbin <= 64) == few]
        assert any(c.n > sq.TILE and c.n % sq.TILE for c in mine) and any(c.nb > 64 for c in mine) and any(c.C == 3 for c in mine)
        assert any(c.n <= 3 for c in mine)
    for dtype in sq.DTYPES:
        # what the fused call's tolerance test needs: few elements so near an edge that the two precisions may disagree
        for c in cases:
            z = sq.panel(c.id, dtype)
            edges = sq.case_edges(sq.bins(c, dtype))
            _, f = sq.synchro_restated(z, sq.FS, edges, sq.carrier_of(c.nb), sq.weight_of(c.nb))
            _, share = sq.near_edges(f, edges.astype(dtype).astype(np.float64), sq.EDGE_GUARD[dtype] * sq.FS)
            with capsys.disabled():
                print(f"squeeze case {c.id:28s} {dtype}: {share:.4f} of the elements within {sq.EDGE_GUARD[dtype]:g} fs of an edge")
            assert share <= sq.EXCLUDED_CAP, (c.id, dtype)
            for kind in sq.TABLE_KINDS:
                f = sq.given_frequencies(c.id, dtype, kind)
                k = sq.bins_of(f, edges)
                assert f.dtype == np.dtype(dtype) and f.shape == z.shape
                if kind == "one_bin":
                    assert (k == sq.bins(c, dtype) // 2).all()
                elif f.size > 200:
                    assert (k < 0).any() and (k >= 0).any()
                if kind == "planted" and f.size > 8 * (sq.bins(c, dtype) + 7):
                    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
                    assert all((f == e).any() for e in edges.astype(dtype))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
GOOD = dict(dtype=None, C=2, nb=5, n=300, nbin=7, rate=800.0, floor=0.0)
SHAPE_REFUSALS = (
    (dict(dtype=7), "dtype"), (dict(C=0), "bad shape"), (dict(nb=0), "bad shape"), (dict(nbin=0), "bad shape"), (dict(C=-1), "bad shape"),
    (dict(n=1), "panel length"), (dict(n=0), "panel length"), (dict(nbin=sq.MAX_BINS + 1), "bins"),
    (dict(nb=sq.MAX_BANDS + 1), "too large"), (dict(C=1 << 20, nb=1 << 10, n=(1 << 10) + 1), "too large"),  # the panel: above 2^40
    (dict(C=1 << 20, nb=1, n=1 << 20, nbin=2), "too large"),                                                # the result: above 2^40
    (dict(C=1 << 21, nb=1 << 10, n=2), "too large"),                                                       # 2^31 workgroups
)


def test_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (a host without a GPU runs this test).  The size
    query gives the calls' status and message."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)

    def at(offset):
        return ctypes.c_void_p(base + offset)

    def tables(a, **kw):
        edges = kw.get("edges", np.linspace(-300.0, 300.0, max(a["nbin"], 1) + 1) if a["nbin"] <= sq.MAX_BINS else np.zeros(2))
        out = []
        for name, default in (("carrier", None), ("edges", edges), ("weight", None)):
            v = kw.get(name, default)
            out.append((None, None) if v is None else _lib.darr(v))
        return out

    def ifreq(a, z=p, out=p, scratch=p, nbytes=1 << 40, **kw):
        (c_host, c_ptr), _, _ = tables(a, **kw)
        return lib.qi_tfr_ifreq(a["dtype"], 0, z, a["C"], a["nb"], a["n"], c_ptr, a["rate"], a["floor"], out, scratch, nbytes, None)

    def squeeze(a, z=p, f=p, out=p, scratch=p, nbytes=1 << 40, **kw):
        _, (e_host, e_ptr), (w_host, w_ptr) = tables(a, **kw)
        return lib.qi_tfr_squeeze(a["dtype"], 0, z, f, a["C"], a["nb"], a["n"], e_ptr, a["nbin"], w_ptr, out, scratch, nbytes, None)

    def fused(a, z=p, out=p, scratch=p, nbytes=1 << 40, **kw):
        (c_host, c_ptr), (e_host, e_ptr), (w_host, w_ptr) = tables(a, **kw)
        return lib.qi_tfr_synchrosqueeze(a["dtype"], 0, z, a["C"], a["nb"], a["n"], c_ptr, a["rate"], a["floor"], e_ptr, a["nbin"], w_ptr,
                                         out, scratch, nbytes, None)

    def query(a):
        return lib.qi_tfr_squeeze_scratch_bytes(a["dtype"], a["C"], a["nb"], a["n"], a["nbin"])

    for code, name in ((_lib.QI_F32, "float32"), (_lib.QI_F64, "float64")):
        good = {**GOOD, "dtype": code}
        e = 4 if code == _lib.QI_F32 else 8
        for change, what in SHAPE_REFUSALS:
            bad = {**good, **change}
            got = query(bad)
            msg = lib.qi_last_error()
            assert got < 0 and what in msg.decode(), (change, msg)
            for call in (squeeze, fused):
                assert call(bad) == got and lib.qi_last_error() == msg, (change, call.__name__)
            if "nbin" not in change:  # qi_tfr_ifreq has no bins: the query's verdict for one
                got, msg = query({**bad, "nbin": 1}), lib.qi_last_error()
                assert got < 0 and what in msg.decode() and ifreq(bad) == got and lib.qi_last_error() == msg, change
        # the size query's verdicts: nbin + 1 edges and two tables of nb values, each region on 16 bytes, the whole on 256
        need = query(good)
        assert (good["nbin"] + 1 + 2 * good["nb"]) * e <= need <= (good["nbin"] + 1 + 2 * good["nb"]) * e + 32 + 256 and need % 256 == 0
        assert query({**good, "C": 9, "n": 2}) == need and query({**good, "nbin": 1}) <= need
        assert query({**good, "nbin": sq.MAX_BINS, "nb": sq.MAX_BANDS}) >= (sq.MAX_BINS + 1 + 2 * sq.MAX_BANDS) * e
        # the values of the host tables and the scalars, as the panel's precision holds them
        up = np.linspace(-300.0, 300.0, good["nbin"] + 1)
        for call in (squeeze, fused):
            for edges, what in ((up[::-1].copy(), "ascending"), (np.where(np.arange(8) == 3, up[2], up), "ascending"),
                                (np.where(np.arange(8) == 3, np.nan, up), "not finite"), (np.where(np.arange(8) == 7, np.inf, up), "not finite")):
                assert call(good, edges=edges) < 0 and what in lib.qi_last_error().decode(), (call.__name__, edges)
            for weight in (np.array([1, 1, np.nan, 1, 1.0]), np.array([1, 1, 1, 1, -np.inf])):
                assert call(good, weight=weight) < 0 and b"weight" in lib.qi_last_error(), call.__name__
            assert call(good, edges=None) < 0 and b"null" in lib.qi_last_error()
        if name == "float32":  # two edges one float32 value apart in float64 only; an edge beyond float32's range
            close = up.copy()
            close[4] = close[3] * (1 + 1e-9)
            assert squeeze(good, edges=close) < 0 and b"ascending" in lib.qi_last_error()
            assert fused(good, edges=np.where(np.arange(8) == 7, 1e39, up)) < 0 and b"not finite" in lib.qi_last_error()
            assert ifreq({**good, "rate": 1e-50}) < 0 and b"sample_rate_hz" in lib.qi_last_error()
            assert ifreq({**good, "floor": 1e39}) < 0 and b"power_floor" in lib.qi_last_error()
        for call in (ifreq, fused):
            for carrier in (np.array([0, 0, np.nan, 0, 0.0]), np.array([np.inf, 0, 0, 0, 0.0])):
                assert call(good, carrier=carrier) < 0 and b"carrier" in lib.qi_last_error(), call.__name__
            for rate in (0.0, -800.0, np.nan, np.inf):
                assert call({**good, "rate": rate}) < 0 and b"sample_rate_hz" in lib.qi_last_error(), (call.__name__, rate)
            for floor in (-1e-30, np.nan, np.inf):
                assert call({**good, "floor": floor}) < 0 and b"power_floor" in lib.qi_last_error(), (call.__name__, floor)
        # pointers: null, nothing asked for, misaligned, a short scratch
        for call in (ifreq, squeeze, fused):
            for kw in (dict(z=None), dict(scratch=None)):
                assert call(good, **kw) < 0 and b"null" in lib.qi_last_error(), (call.__name__, kw)
            assert call(good, out=None) < 0 and b"nothing" in lib.qi_last_error(), call.__name__
            low = query({**good, "nbin": 1}) if call is ifreq else need
            assert call(good, nbytes=low - 1) < 0 and b"scratch" in lib.qi_last_error(), call.__name__
            assert call(good, nbytes=0) < 0 and b"scratch" in lib.qi_last_error(), call.__name__
            for kw in (dict(z=at(e)), dict(out=at(e // 2) if call is ifreq else at(e)), dict(scratch=at(8))):
                assert call(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), (call.__name__, kw)
        assert squeeze(good, f=None) < 0 and b"null" in lib.qi_last_error()
        assert squeeze(good, f=at(e // 2)) < 0 and b"misaligned" in lib.qi_last_error()
    assert ifreq({**GOOD, "dtype": _lib.QI_F64}, out=at(4)) < 0 and b"misaligned" in lib.qi_last_error()


# ---- the host helper ------------------------------------------------------------------------------------------------------------------
def test_bin_edges_are_the_restatement():
    from quantum_inferno_amd import scales_dyadic as scales

    tables = [scales.log_frequency_hz_from_fft_points(sq.FS, 4096, order) for order in (1, 3, 12)]
    tables += [np.array([1.0, 2.0]), np.array([3.0, 5.0, 6.0, 40.0, 41.0])]  # two bands; slopes that differ
    for f in tables:
        for per in (1, 2, 3, 8):
            edges, centre = scales.squeeze_bin_edges(f, per)
            w_edges, w_centre = sq.bin_edges_restated(f, per)
            assert edges.dtype == centre.dtype == np.float64
            assert np.array_equal(edges, w_edges) and np.array_equal(centre, w_centre), (len(f), per)  # bit for bit
            assert len(edges) == len(f) * per + 1 and (np.diff(edges) > 0).all()
            assert ((edges[:-1] < centre) & (centre < edges[1:])).all()
            # every band centre lies in its own group of bins, and with one bin per band in the middle of its bin
            k = np.searchsorted(edges, f, side="right") - 1
            assert np.array_equal(k // per, np.arange(len(f)))
            if per == 1:
                # (exp2 of log2 f: the logarithm's rounding, half an ulp of |log2 f|, times ln 2, and an ulp of exp2 and of the quotient)
                assert np.abs(centre / f - 1).max() <= (np.abs(np.log2(f)).max() * np.log(2.0) + 2.0) * np.finfo(np.float64).eps
        inner_edges = scales.squeeze_bin_edges(f, 1)[0][1:-1]
        assert np.allclose(inner_edges, np.sqrt(f[:-1] * f[1:]), rtol=1e-14)  # the geometric means of neighbours
    for bad in (dict(frequency_hz=[1.0]), dict(frequency_hz=[2.0, 1.0]), dict(frequency_hz=[1.0, 1.0]), dict(frequency_hz=[0.0, 1.0]),
                dict(frequency_hz=[1.0, np.nan]), dict(frequency_hz=[[1.0, 2.0]]), dict(frequency_hz=[1.0, 2.0], bins_per_band=0),
                dict(frequency_hz=[1.0, 2.0], bins_per_band=1.5)):
        with pytest.raises(ValueError):
            scales.squeeze_bin_edges(**bad)


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sq.DTYPES)
def test_squeeze_restatement_against_a_dense_contraction(dtype):
    """Gaussian-integer panels: every sum is exact in either precision, whatever the order -- the restatement equals the
    contraction of the panel with the one-hot tensor of the bins, formed in float64."""
    for cid in ("c3_b5_n3_k7", "c3_b24_n256_k32", "c1_b71_n700_k568"):
        c = sq.by_id(cid)
        z = sq.panel(cid, dtype, whole=True)
        edges = sq.case_edges(sq.bins(c, dtype))
        for kind in sq.TABLE_KINDS:
            f = sq.given_frequencies(cid, dtype, kind)
            k = sq.bins_of(f, edges)
            hot = (k[:, :, None, :] == np.arange(len(edges) - 1)[None, None, :, None]).astype(np.float64)
            dense = np.einsum("cbt,cbkt->ckt", z.astype(np.complex128), hot)
            got = sq.squeeze_restated(z, f, edges)
            assert got.dtype == z.dtype and np.array_equal(got.astype(np.complex128), dense), (cid, kind)
            two = sq.squeeze_restated(z, f, edges, np.full(c.nb, 2.0))
            assert np.array_equal(two.astype(np.complex128), 2 * dense)


@pytest.mark.parametrize("dtype", sq.DTYPES)
def test_bin_rule_on_planted_values(dtype):
    r = np.dtype(dtype).type
    edges = np.array([-3.5, -1.0, 0.0, 0.1, 7.25]).astype(r)
    below, above = np.nextafter(edges, r(-np.inf)), np.nextafter(edges, r(np.inf))
    f = np.concatenate([edges, below, above, [np.nan, np.inf, -np.inf, -0.0]]).astype(r)
    want = [0, 1, 2, 3, -1] + [-1, 0, 1, 2, 3] + [0, 1, 2, 3, -1] + [-1, -1, -1, 2]
    assert sq.bins_of(f, edges).tolist() == want
    # one column per planted value, two bands: the moved coefficients arrive, the others enter nothing -- NaN and Inf included
    z = np.empty((1, 2, len(f)), dtype=sq.COMPLEX[dtype])
    z[0, 0], z[0, 1] = 1 + 2j, np.where(np.arange(len(f)) % 2 == 0, np.nan, np.inf) * (1 + 1j)
    table = np.stack([f, np.full(len(f), np.nan, dtype=r)])[None]
    out = sq.squeeze_restated(z, table, edges)
    for t, k in enumerate(want):
        column = out[0, :, t]
        assert np.isfinite(column).all() and np.count_nonzero(column) == (k >= 0)
        assert k < 0 or column[k] == 1 + 2j


def test_sum_over_bins_is_the_sum_of_the_moved(capsys):
    for dtype, bound in (("float64", 1e-15), ("float32", 1e-6)):
        for cid in ("c1_b71_n700_k568", "c3_b24_n700_k65"):
            c = sq.by_id(cid)
            z = sq.panel(cid, dtype)
            edges, w = sq.case_edges(sq.bins(c, dtype)), sq.weight_of(c.nb)
            f = sq.given_frequencies(cid, dtype, "random")
            out = sq.squeeze_restated(z, f, edges, w).astype(np.complex128)
            moved = sq.bins_of(f, edges) >= 0
            want = (np.where(moved, z.astype(np.complex128), 0) * w.astype(dtype).astype(np.float64)[None, :, None]).sum(axis=1)
            err = np.abs(out.sum(axis=1) - want).max() / np.abs(z).max()
            with capsys.disabled():
                print(f"squeeze sum over bins {cid} {dtype}: {err:.3g} of the largest modulus")
            # nb terms of modulus <= 2 max|z| each, added in some order in the panel's precision: nb eps at the very most
            assert err <= bound * c.nb


# ---- the method, through the restatement ---------------------------------------------------------------------------------------------------
def squeezed_power(kind, order, signal, per, carrier="snapped"):
    from quantum_inferno_amd import scales_dyadic as scales

    f, z, snapped = sq.cpu_panel(kind, order, signal)
    edges, centre = scales.squeeze_bin_edges(f, per)
    out, ifreq = sq.synchro_restated(z, sq.FS, edges, snapped if carrier == "snapped" else f)
    return f, np.abs(z[0]) ** 2, edges, centre, np.abs(out[0]) ** 2, ifreq[0]


@pytest.mark.parametrize("kind", ("cwt", "stx"))
@pytest.mark.parametrize("order", sq.ORDERS)
def test_a_tone_is_squeezed_into_its_bin(kind, order, capsys):
    f, raw, edges, _, power, _ = squeezed_power(kind, order, "tone", 1)
    k = int(np.searchsorted(edges, sq.TONE_HZ)) - 1
    cols = sq.inner(sq.METHOD_N)
    share, before = sq.bin_share(power, k, cols), sq.bin_share(raw, k, cols)
    with capsys.disabled():
        print(f"squeeze tone {kind} order {order}: {share:.4f} of the power in the tone's bin, {before:.4f} in the raw panel")
    assert share >= 0.95 and before < 0.9


@pytest.mark.parametrize("kind", ("cwt", "stx"))
@pytest.mark.parametrize("order", sq.ORDERS)
def test_a_chirp_ridge_is_sharpened(kind, order, capsys):
    f, raw, _, centre, power, _ = squeezed_power(kind, order, "chirp", 8)
    truth, cols = sq.chirp()[1], sq.inner(sq.METHOD_N)
    ridge, ridge_raw = sq.ridge_error_octaves(power, centre, truth, cols), sq.ridge_error_octaves(raw, f, truth, cols)
    near = sq.share_near_truth(power, centre, truth, cols, 1 / (4 * order))
    near_raw = sq.share_near_truth(raw, f, truth, cols, 1 / (4 * order))
    with capsys.disabled():
        print(f"squeeze chirp {kind} order {order}: median ridge error {ridge:.4f} octaves (raw {ridge_raw:.4f}, ratio {ridge / ridge_raw:.2f}); "
              f"share within 1 / {4 * order} octave {near:.3f} (raw {near_raw:.3f}, {near / near_raw:.2f} x)")
    assert ridge <= 0.5 * ridge_raw
    assert near >= 1.5 * near_raw


@pytest.mark.parametrize("order", sq.ORDERS)
def test_a_stockwell_panel_turns_at_the_snapped_bin(order, capsys):
    """The Stockwell bands are demodulated by the FFT bin their centres were snapped to.  With the nominal centres as the carrier
    every frequency is off by the snap, up to half a bin of the record's spectrum (0.098 Hz here): the power-weighted rms error
    of the tone's frequency grows from 0.0021 / 0.0049 Hz (orders 3 / 12) to 0.033 / 0.081 Hz, and at order 12 with eight bins
    per band the tone's bin keeps 0.158 of the power instead of all of it."""
    cols = sq.inner(sq.METHOD_N)
    rms = {}
    for carrier in ("snapped", "nominal"):
        _, raw, _, _, _, ifreq = squeezed_power("stx", order, "tone", 1, carrier)
        rms[carrier] = float(np.sqrt((raw[:, cols] * (ifreq[:, cols] - sq.TONE_HZ) ** 2).sum() / raw[:, cols].sum()))
    with capsys.disabled():
        print(f"squeeze stockwell carrier order {order}: rms error of the tone's frequency {rms['snapped']:.4f} Hz snapped, {rms['nominal']:.4f} Hz nominal")
    assert rms["snapped"] <= 0.01 and rms["nominal"] >= 10 * rms["snapped"]
    if order == 12:
        shares = {}
        for carrier in ("snapped", "nominal"):
            _, _, edges, _, power, _ = squeezed_power("stx", order, "tone", 8, carrier)
            shares[carrier] = sq.bin_share(power, int(np.searchsorted(edges, sq.TONE_HZ)) - 1, cols)
        with capsys.disabled():
            print(f"squeeze stockwell carrier order 12, eight bins per band: {shares['snapped']:.4f} in the tone's bin snapped, {shares['nominal']:.4f} nominal")
        assert shares["snapped"] >= 0.95 and shares["nominal"] <= 0.5
