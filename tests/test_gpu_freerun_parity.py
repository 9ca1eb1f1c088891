"""Free-running parity of the HIP codecs against the oracle over whole GOPs,
with the decoded picture buffer compared tensor by tensor.

The strict cases of tests/test_gpu_parity_strict.py are teacher-forced; here
each P-frame reads the DPB the product itself wrote for the previous frame, as
in the benchmark's 32-frame GOP, through real .bin files.  The oracle runs
beside it on its own DPB with the product's symbols replayed at its rounding
ties and never receives a float from the product (tests/freerun.py).  Every
frame holds the replay's strict bar and REC_MAXABS; ref_frame, ref_feature,
ref_mv_feature, ref_y and ref_mv_y lie within DPB_FACTOR[precision] times the
oracle's own recorded reordering noise (tests/golden/freerun_selfnoise.json);
and the differences do not grow over the run.  The per-frame figures go to
parity_freerun.json, beside the strict file's parity_strict.json.
"""
import os
import tempfile

import pytest
import torch

from tests.freerun import CASES, OUT, ProductPlayer, make_frames, make_pair, run_free
from tests.parity import DPB_FACTOR, compare_dpb, dpb_over, selfnoise

pytestmark = pytest.mark.gpu

RECORD = os.path.join(OUT, "parity_freerun.json")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, n)))
    yield
    torch.set_num_threads(old)


@pytest.mark.parametrize("case,prec", [("DC-bench", "split"), ("DC-bench", "parity"), ("DC-golden", "split"),
                                       ("HEM-bench", "split")])
def test_freerun_parity(case, prec):
    c = CASES[case]
    pair = make_pair(case, prec)
    r = run_free(pair, make_frames(case), c["q"] if c["codec"] == "dc" else None, c["h"], c["w"], c["gop"],
                 f"{case}_{prec}", DPB_FACTOR[prec], selfnoise(case), record=RECORD)
    print({k: f"{v['rel']:.3g} ({v['ratio']:.2f}x the bar, t={v['frame']})" for k, v in r["dpb"].items()},
          "forced", r["forced"], "idx_diff", r["idx_diff"], "rec_maxabs", r["rec_maxabs"], "growth",
          {k: round(v["ratio"], 2) for k, v in r["growth"].items()})


def test_bf16_misses_the_dpb_bar():
    """Negative control: DC-bench, I + 3 P, free running in Precision.fast()
    (bf16 features, about 4e-3) against the oracle on its own DPB: some
    tensor must miss the split bar on some frame."""
    case = "DC-bench"
    c = CASES[case]
    pair = make_pair(case, "fast")
    noise, over = selfnoise(case), {}
    with tempfile.TemporaryDirectory() as td:
        play, dpb_o = ProductPlayer(pair, c["h"], c["w"], td), None
        for t, (x, xp) in enumerate(make_frames(case, 4)):
            _, _, _, dpb_p = play(t, t == 0, xp, c["q"], t % 4)
            _, _, _, dpb_o = pair.oracle(t, xp, dpb_o, c["q"], t % 4)
            d = compare_dpb(dpb_p, dpb_o, c["h"], c["w"], noise, DPB_FACTOR["split"])
            over[t] = {k: round(v["ratio"], 1) for k, v in dpb_over(d).items()}
    print(over)
    ok = not any(over.values())
    assert not ok, "bf16 features passed the split DPB bar"
    assert over[1] and "ref_feature" in over[1], over
