"""Which kernel dcvc_conv2d launches for which call, pinned.

The split-family launchers (tconv, nconv, wconv, xconv, dconv, sconv / sgemm)
and the bf16 / fp32 dispatcher decline a call by returning "unsupported", and
the next kernel in line computes the same values, only slower: a launcher that
starts to refuse a view or a shape it used to take fails no numerical test.
So every case of tests/conv_cases.py (the table this test shares with the value
checks of test_gpu_conv_conformance.py) records dcvc_last_kernel() after the call (the whole
string, "@threads" suffix included, i.e. instantiation and grid) or the error
the call raised, and compares it with tests/golden/conv_routing.json.

DCVC_RECORD_ROUTING=1 rewrites the golden file from the library under test
instead of comparing (off by default).
"""
import json
import os

import pytest
import torch

from tests.conv_cases import CASES, GOLDEN, launch

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("DCVC_RECORD_ROUTING", "0") == "1"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_recorded = {}


def route(c):
    """The kernel the call launched, or "error: ..." for a call that raised."""
    return launch(c, "zeros")[0]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_conv_routing(c):
    from dcvc_amd._native import _ERRORS
    got = route(c)
    # a refusal (invalid / unsupported) is a route like any other, a failed launch
    # (DCVC_HIP_ELAUNCH = -2, in check()'s words) never is, on any library
    assert got and got != f"error: conv2d: {_ERRORS[-2]}", got
    if RECORD:
        _recorded[c["name"]] = got
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert got == golden[c["name"]]


def test_golden_has_one_entry_per_case():
    if RECORD:
        assert sorted(_recorded) == sorted(c["name"] for c in CASES)
        with open(GOLDEN, "w") as f:
            json.dump(_recorded, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(c["name"] for c in CASES)
