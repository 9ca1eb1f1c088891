"""The DPB bar of tests/parity.py has teeth, shown oracle against oracle on
the CPU: 8 frames of the DC-bench case at 128x128, free running.

A run whose ref_feature is wrong by 1e-4 of the tensor's maximum after every
frame passes everything the suite looked at before the DPB comparison (every
symbol equal, every differing index a rate-capped tie, bits, PSNR, the decoded
picture within REC_MAXABS), and misses the DPB bar.  That is why compare_dpb
exists.  The same run without the perturbation holds the bar at the parity
factor against the committed self-noise fixture.
"""
import json

import pytest
import torch

from tests.freerun import CASES, OraclePlayer, make_frames, make_pair, run_free
from tests.parity import DPB_FACTOR, REC_MAXABS, idx_allowed, selfnoise

CASE, N, H, W = "DC-bench", 8, 128, 128
EPS = 1e-4


@pytest.fixture(scope="module")
def setup():
    try:
        import os
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = 4
    old = torch.get_num_threads()
    torch.set_num_threads(1)            # the judging oracle; the player runs at `threads`
    yield make_pair(CASE), make_frames(CASE, N, H, W), max(1, min(16, n))
    torch.set_num_threads(old)


def _run(setup, perturb, record=None):
    pair, frames, threads = setup
    c = CASES[CASE]
    return run_free(pair, frames, c["q"], H, W, c["gop"], CASE, DPB_FACTOR["parity"], selfnoise(CASE),
                    player=OraclePlayer(pair, threads, perturb), record=record)


def test_unperturbed_oracle_holds_the_parity_bar(setup):
    r = _run(setup, None)
    assert r["sym_diff"] == 0
    print({k: (v["rel"], v["bar"]) for k, v in r["dpb"].items()})


def test_perturbed_ref_feature_passes_the_older_bars_and_misses_the_dpb_bar(setup, tmp_path):
    g = torch.Generator().manual_seed(7)

    def perturb(dpb):
        f = dpb["ref_feature"]
        if f is not None:
            f.add_((torch.rand(f.shape, generator=g) * 2 - 1) * (EPS * float(f.abs().max())))

    record = str(tmp_path / "perturbed.json")
    with pytest.raises(AssertionError, match="DPB over the bar") as err:
        _run(setup, perturb, record)
    assert "ref_feature" in str(err.value)
    # run_free asserts the replay's strict bar (compare_forced / check_forced)
    # and REC_MAXABS frame by frame before it records and before the DPB bars:
    # the record exists, so all 8 frames passed them
    with open(record) as f:
        r = json.load(f)[CASE]
    assert len(r["frames"]) == N and r["sym_diff"] == 0 and r["rec_maxabs"] <= REC_MAXABS
    assert all(not fr["unexplained"] for fr in r["frames"])
    assert r["idx_diff_max"] <= idx_allowed(0)
    print({k: (v["rel"], v["bar"]) for k, v in r["dpb"].items()}, r["idx_diff"], r["forced"], r["rec_maxabs"])
    # every P-frame's ref_feature misses, by about EPS / bar
    bar = DPB_FACTOR["parity"] * selfnoise(CASE)["ref_feature"]
    for fr in r["frames"][1:]:
        assert fr["dpb"]["ref_feature"]["rel"] > 10 * bar, fr["t"]
