"""The circuit compiler against digests recorded before its working state moved from raw record slots to typed sites
(tools/circuit_digests.py -> tests/golden/compiled_circuit_digests.json): the blob, report(), pbs_counts(), margin_model() and the
simulation sigmas of eleven circuits -- all four look-up modes, both hand-overs of the one-bit steps, a max pool -- byte for byte
(the floats by repr: one ulp moves a digest).  No GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("circuit_digests", os.path.join(ROOT, "tools", "circuit_digests.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

with open(tool.FIXTURE) as _f:
    ROWS = json.load(_f)


def test_fixture_holds_the_tools_cases():
    assert [r["case"] for r in ROWS] == tool.CASES


@pytest.mark.parametrize("row", ROWS, ids=[r["case"]["id"] for r in ROWS])
def test_compiled_circuit_digests(row):
    got = tool.digests(tool.compile_case(row["case"]))
    assert got == {k: row[k] for k in tool.DIGESTS}
