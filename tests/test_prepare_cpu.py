"""CPU-side checks of the explicit layout build (bsmr_plan_prepare and its panel / query forms):
the C ABI's argument checks, the status code and the binding's surface. No device call: every
call below fails its argument check before the library touches a plan."""
import os
import re

import pytest

import bsmr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # BSMR_ERR_INVALID
NAMES = ["bsmr_plan_prepare", "bsmr_plan_prepare_panels", "bsmr_plan_prepared",
         "bsmr_plan_panels_prepared"]


def _last_error():
    return bsmr.lib().bsmr_last_error().decode()


def test_null_plan_is_invalid_and_names_the_function():
    L = bsmr.lib()
    assert L.bsmr_plan_prepare(None, 128, 0) == INVALID
    assert "bsmr_plan_prepare:" in _last_error()
    assert L.bsmr_plan_prepare_panels(None, 128, 0, 0, 1, 0) == INVALID
    assert "bsmr_plan_prepare_panels:" in _last_error()
    assert L.bsmr_plan_prepared(None, 128, 0) == 0
    assert "bsmr_plan_prepared:" in _last_error()
    assert L.bsmr_plan_panels_prepared(None, 128, 0, 0, 1, 1) == 0
    assert "bsmr_plan_panels_prepared:" in _last_error()


def test_not_prepared_status_value():
    assert bsmr.NOT_PREPARED == 8
    header = open(os.path.join(ROOT, "include", "bsmr.h")).read()
    assert re.search(r"\bBSMR_ERR_NOT_PREPARED\s*=\s*8\b", header)


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_declared(name):
    header = open(os.path.join(ROOT, "include", "bsmr.h")).read()
    assert name in bsmr.EXPORTS
    assert re.search(r"\bint\s+%s\s*\(\s*const bsmr_plan\*" % name, header)
    assert hasattr(bsmr.lib(), name)


def test_bsmr_error_carries_the_status():
    with pytest.raises(bsmr.BsmrError) as ei:
        bsmr._check(bsmr.lib().bsmr_plan_prepare(None, 128, 0), "bsmr_plan_prepare")
    assert ei.value.status == INVALID
    assert str(ei.value).startswith("bsmr_plan_prepare failed with status 1: bsmr_plan_prepare:")
    assert bsmr.BsmrError("binding-side error").status is None


def test_plan_has_prepare_and_prepared():
    for m in ("prepare", "prepared"):
        assert callable(getattr(bsmr.Plan, m))
