"""The census of tests/stream_cases.py against include/qi_tfr.h (no GPU, no library): every entry point that takes a
`qi_stream` is named by a case, the table names nothing the header lacks, and the paths the table promises are all there
-- a new entry point cannot land without a stream case, and a case cannot leave unnoticed."""
import os
import re

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    """{name: parameter text} of every function include/qi_tfr.h declares (comments removed first)."""
    with open(os.path.join(ROOT, "include", "qi_tfr.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    return dict(re.findall(r"\b(qi_\w+)\s*\(([^;{}()]*)\)\s*;", text))


def stream_functions():
    return sorted(name for name, params in header_functions().items() if re.search(r"\bqi_stream\b", params))


def test_header_is_parsed():
    fns = header_functions()
    assert {"qi_abi_version", "qi_plan_create", "qi_cwt", "qi_stft_out_range", "qi_doppler"} <= set(fns)
    streams = stream_functions()
    assert "qi_cwt_stx" in streams and "qi_plan_set_gabor_bank" in streams
    assert "qi_plan_set_stx_bands" not in streams and "qi_stft_segments" not in streams and "qi_peaks_select_distance" not in streams
    assert len(streams) >= 32, streams  # (the count when this test was written)


def test_every_stream_entry_point_has_a_case():
    missing = [f for f in stream_functions() if f not in sc.named_functions()]
    assert not missing, f"entry points that take a qi_stream and have no case in tests/stream_cases.py: {missing}"


def test_table_names_only_header_functions():
    unknown = [f for f in sc.named_functions() if f not in stream_functions()]
    assert not unknown, unknown


def test_flags_and_ids():
    ids = sc.ids()
    assert len(set(ids)) == len(ids)
    for case in sc.CASES:
        assert case.functions and callable(case.build), case.id
        assert case.asynchronous or case.reason, case.id
    waits = sorted(c.id for c in sc.CASES if not c.asynchronous)
    assert waits == ["gabor_atoms", "gabor_atoms_at", "set_gabor_bank-then-cwt"], waits
    assert set(sc.SHARED_STATE) <= set(ids)


def test_every_promised_path_is_in_the_table():
    """The table's shape, pinned: each plan transform on each engine with every output and with the band form, alone and
    in a batch; each short-time entry point at a fused and at a hipFFT shape; both forms of the ops that have two."""
    ids = set(sc.ids())
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

    plan_functions = {name for name, params in header_functions().items() if re.search(r"\bqi_plan\s*\*", params)}
    assert {"qi_cwt", "qi_stx", "qi_cwt_stx", "qi_plan_set_gabor_bank"} <= plan_functions and "qi_stft_out_range" not in plan_functions
    keys = set(sc.ENGINES) | {sc.PASS2_ENGINE[0], "set_bank"}
    for case in sc.CASES:
        takes_plan = any(f in plan_functions for f in case.functions)
        assert (case.engine is not None) == takes_plan, case.id
        assert case.engine is None or case.engine in keys, case.id
        if case.engine in sc.ENGINES or case.engine == sc.PASS2_ENGINE[0]:
            assert case.engine in case.id, case.id
    plan_cases = [c.id for c in sc.CASES if c.engine is not None]
    assert len(plan_cases) + len(sc.plan_less_ids()) == len(sc.CASES) == 125 and not set(plan_cases) & set(sc.plan_less_ids())
    # each engine's transforms, the two-pass forms, the two pooled forms, the bank upload; the rest is plan-less
    assert len(plan_cases) == len(sc.ENGINES) * 16 + len(sc.PASS2_FORMS) + 2 + 1 and len(sc.plan_less_ids()) == 39
    assert set(sc.SHARED_STATE) <= set(sc.plan_less_ids())
    for key in ("f32_n16384", "f64_n32768", "f32_n2048", "f32_n3000"):  # test_threads_one_plan_each: a thread per key
        assert sc.by_id(f"cwt_stx-{key}-all-r1").engine == key
    assert asc.plan_less_ids() == asc.ids() and len(asc.ids()) == 4  # include/qi_array.h has no plans
    assert all(len(c) == len(sc.Case._fields) for c in asc.CASES)


def test_strip_shapes_fold_partials():
    s = sc.STRIP
    assert sc.strip_segments(s["records"] * s["bands"], s["windows"], s["factor"]) == 5
    assert sc.strip_segments(6, 256, 2) == 1  # (what S = 1 looks like: no fold)
