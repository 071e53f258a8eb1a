"""The census of tests/stream_cases.py against include/qi_tfr.h (no GPU, no library): every entry point that takes a
`qi_stream` is named by a case, the table names nothing the header lacks, and the paths the table promises are all there
-- a new entry point cannot land without a stream case, and a case cannot leave unnoticed."""
import re

import stream_cases as sc
from stream_table import Case, header_functions, stream_functions

HEADER = "qi_tfr.h"
T = sc.TABLE


def test_header_is_parsed():
    fns = header_functions(HEADER)
    assert {"qi_abi_version", "qi_plan_create", "qi_cwt", "qi_stft_out_range", "qi_doppler"} <= set(fns)
    streams = stream_functions(HEADER)
    assert "qi_cwt_stx" in streams and "qi_plan_set_gabor_bank" in streams
    assert "qi_plan_set_stx_bands" not in streams and "qi_stft_segments" not in streams and "qi_peaks_select_distance" not in streams
    assert len(streams) >= 32, streams  # (the count when this test was written)


def test_every_stream_entry_point_has_a_case():
    missing = [f for f in stream_functions(HEADER) if f not in T.named_functions()]
    assert not missing, f"entry points that take a qi_stream and have no case in tests/stream_cases.py: {missing}"


def test_table_names_only_header_functions():
    unknown = [f for f in T.named_functions() if f not in stream_functions(HEADER)]
    assert not unknown, unknown


def test_flags_and_ids():
    ids = T.ids()
    assert len(set(ids)) == len(ids)
    for case in T.cases:
        assert case.functions and callable(case.build), case.id
        assert case.asynchronous or case.reason, case.id
    waits = sorted(c.id for c in T.cases if not c.asynchronous)
    assert waits == ["gabor_atoms", "gabor_atoms_at", "set_gabor_bank-then-cwt"], waits
    assert set(sc.SHARED_STATE) <= set(ids)


def test_every_promised_path_is_in_the_table():
    """The table's shape, pinned: each plan transform on each engine with every output and with the band form, alone and
    in a batch; each short-time entry point at a fused and at a hipFFT shape; both forms of the ops that have two."""
    ids = set(T.ids())
    for key in sc.ENGINES:
        for transform in ("cwt_styx", "cwt_atoms", "stx", "cwt_stx"):
            for outputs in ("all", "band"):
                for records in (1, 8):
                    assert f"{transform}-{key}-{outputs}-r{records}" in ids
    assert [sc.ENGINES[k][:2] for k in sc.ENGINES] == [("float32", 1 << 14), ("float64", 1 << 15), ("float32", 1 << 11),
                                                       ("float64", 1 << 11), ("float32", 3000)]
    assert sc.PASS2_ENGINE[1][:2] == ("float32", 1 << 20)  # the two-pass kernels: a one-band table at 2^20 samples
    for form in ("all-r1", "band-r1", "band-r8"):
        assert f"cwt_styx-{sc.PASS2_ENGINE[0]}-{form}" in ids
    for shape in ("fused", "hipfft"):
        for form in ("stft", "out_reduced", "out_panels", "out_range", "welch", "sliding_stft", "sliding_istft"):
            assert f"{form}-{shape}" in ids
    for name in ("pooled-average-f32_n2048", "pooled_strip-f32_n2048", "filtfilt_ba", "filtfilt_sos", "interp_shared", "interp_rows",
                 "cumtrapz_dx", "cumtrapz_rows", "gradient_h", "difference_rows", "pool_strip-with-stats"):
        assert name in ids
    assert len(ids) == 125, len(ids)  # a case that leaves the table fails here even where its function keeps another case


def test_every_case_is_in_one_thread_group():
    """tests/test_gpu_threads.py runs the plan-less cases from several host threads at once and the plan cases with one plan
    per thread.  Which group a case is in is told by the header: a case reaches a function that takes a `qi_plan*` exactly
    when it names the plan it runs on (`engine`), and the names are those of the plans stream_cases builds."""
    import array_stream_cases as asc

    plan_functions = {name for name, params in header_functions(HEADER).items() if re.search(r"\bqi_plan\s*\*", params)}
    assert {"qi_cwt", "qi_stx", "qi_cwt_stx", "qi_plan_set_gabor_bank"} <= plan_functions and "qi_stft_out_range" not in plan_functions
    keys = set(sc.ENGINES) | {sc.PASS2_ENGINE[0], "set_bank"}
    for case in T.cases:
        takes_plan = any(f in plan_functions for f in case.functions)
        assert (case.engine is not None) == takes_plan, case.id
        assert case.engine is None or case.engine in keys, case.id
        if case.engine in sc.ENGINES or case.engine == sc.PASS2_ENGINE[0]:
            assert case.engine in case.id, case.id
    plan_cases = [c.id for c in T.cases if c.engine is not None]
    assert len(plan_cases) + len(T.plan_less_ids()) == len(T.cases) == 125 and not set(plan_cases) & set(T.plan_less_ids())
    # each engine's transforms, the two-pass forms, the two pooled forms, the bank upload; the rest is plan-less
    assert len(plan_cases) == len(sc.ENGINES) * 16 + len(sc.PASS2_FORMS) + 2 + 1 and len(T.plan_less_ids()) == 39
    assert set(sc.SHARED_STATE) <= set(T.plan_less_ids())
    for key in ("f32_n16384", "f64_n32768", "f32_n2048", "f32_n3000"):  # test_threads_one_plan_each: a thread per key
        assert T.by_id(f"cwt_stx-{key}-all-r1").engine == key
    assert asc.TABLE.plan_less_ids() == asc.TABLE.ids() and len(asc.TABLE.ids()) == 4  # include/qi_array.h has no plans
    assert all(len(c) == len(Case._fields) for c in asc.TABLE.cases)


def test_tables_declare_what_the_harness_checks():
    """What tests/stream_order.py does with a table's cases is the table's own data: pinned here, so that a rule cannot
    weaken unnoticed.  (header, input through view_as_complex, power rule, finite, no fill value, outputs that are zero.)"""
    import stream_order as sot  # (imports torch, touches no device)

    declared = [(t.header, t.complex_input, t.power, t.finite, t.no_fill, t.zero_outputs) for t in sot.TABLES]
    assert declared == [("qi_tfr.h", False, "any", False, False, {}),
                        ("qi_array.h", False, "every", True, False, {}),
                        ("qi_beam.h", True, "every", True, False, {}),
                        ("qi_adaptive.h", True, "first", True, False, {"whiten-info": 1}),
                        ("qi_subspace.h", True, "first", True, False, {"eigh-info": 2}),
                        ("qi_steer.h", False, "every", True, True, {}),
                        ("qi_windows.h", False, "every", True, True, {}),
                        ("qi_lags.h", False, "every", True, True, {})]
    assert [len(t.cases) for t in sot.TABLES] == [125, 4, 2, 3, 3, 4, 6, 4]
    assert len({t.name for t in sot.TABLES}) == len(sot.TABLES)
    for t in sot.TABLES:
        assert set(t.zero_outputs) <= set(t.ids()), t.header


def test_strip_shapes_fold_partials():
    s = sc.STRIP
    assert sc.strip_segments(s["records"] * s["bands"], s["windows"], s["factor"]) == 5
    assert sc.strip_segments(6, 256, 2) == 1  # (what S = 1 looks like: no fold)
