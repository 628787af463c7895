"""GPU: the row-block launch layouts of a fixed case table are bit-identical to the recorded ones.

tests/golden/mi355x_rb_layout_digests.json holds one SHA-256 per case of rb_layout_cases.CASES
(items, item ends and pieces of the whole-plan layout, through bsmr_debug_rb_items /
bsmr_debug_rb_pieces), recorded by tools/rb_layout_digest.py --record on the commit named in the
file. A change to the layout build that is meant to change no layout must reproduce all of them; one
that is meant to change layouts re-records the file and says so.
"""
import pytest

import rb_layout_cases as R
from gpu_util import torch_cuda

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    g = R.load_golden()
    cus = torch_cuda().cuda.get_device_properties(0).multi_processor_count
    assert cus == g["cus"], (f"this device has {cus} CUs, the digests were recorded on one with "
                             f"{g['cus']}: layouts depend on the CU count, re-record on this device")
    return g


def test_table_and_file_agree(golden):
    assert sorted(golden["digests"]) == sorted(R.CASES)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_layout_digest(name, golden):
    assert name in golden["digests"], f"{name} is not in the golden file"
    assert R.case_digest(name) == golden["digests"][name], \
        f"{name}: layout differs from commit {golden['commit']}"
