"""The small-record engine's public surface, without a GPU: the appended profiling stage, the stage names of the binding,
the unchanged ABI version and the exported symbols."""
import os
import re

from conftest import ROOT

from quantum_inferno_amd import _lib


def _header():
    return open(os.path.join(ROOT, "include", "qi_tfr.h")).read()


def test_header_appends_the_small_stage():
    stages = dict((k, int(v)) for k, v in re.findall(r"\b(QI_STAGE_[A-Z0-9_]+)\s*=\s*(\d+)", _header()))
    assert stages["QI_STAGE_SMALL"] == 9 and stages["QI_STAGE_COUNT"] == 10
    # no existing value moved
    assert [stages[f"QI_STAGE_{s}"] for s in ("FORWARD", "MULTIPLY", "INVERSE", "EPILOGUE", "PASS1", "PASS2", "BLOCK", "ZOOM",
                                              "ZOOM_COARSE")] == list(range(9))


def test_binding_names_the_small_stage():
    assert len(_lib.STAGES) == 10 and _lib.STAGES[9] == "small"
    assert _lib.STAGES[:9] == ("forward", "multiply", "inverse", "epilogue", "pass1", "pass2", "block", "zoom", "zoom_coarse")


def test_abi_version_and_exports():
    assert re.search(r"#define\s+QI_TFR_ABI_VERSION\s+1\b", _header())
    lib = _lib.load()
    assert lib.qi_abi_version() == 1
    declared = set(re.findall(r"\b(qi_[a-z0-9_]+)\s*\(", _header()))
    assert declared
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_tfr.h but not exported"
