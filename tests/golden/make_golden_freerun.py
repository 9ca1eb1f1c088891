"""The oracle's own reordering noise over a free-running GOP: the yardstick
of the DPB bars in tests/parity.py (CPU only, the project's oracle alone).

Per case of tests/freerun.py the oracle codes the sequence with 16 threads,
and again with 1 thread replaying the first run's symbols at its rounding ties
(Forcer, TIE_EPS); each run keeps its own decoded picture buffer.  Recorded
per DPB tensor: the largest max |a - b| and the largest rel = max |a - b| /
max |b| over all frames, the frame of that rel, and the ratio of the last
quarter of the run to the first quarter of its P-frames.  The runs must code
the same symbols and hold the replay's strict bar on every frame, and the
ratio may not exceed tests.parity.GROWTH (tests.freerun.run_free asserts
both): that is what makes these inputs usable for the product.  HEM-C1 is a
yardstick alone, for the teacher-forced hem_C1 cases: the three torch.rand
frames the golden config C1 codes in write mode, on which the oracle's picture
is three times as noisy as on HEM-bench's (the recon conv's output reaches 4.5
there before the clamp to 0..1, and rel is taken against the clamped maximum);
three frames have no quarters, so its ratio is recorded and not asserted.

    python tests/golden/make_golden_freerun.py
"""
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.freerun import CASES, OraclePlayer, make_frames, make_pair, run_free   # noqa: E402

OUT = os.path.join(HERE, "freerun_selfnoise.json")
THREADS = (16, 1)   # the run that plays the product, the run that replays it


def main():
    cases = {}
    for name, c in CASES.items():
        t0 = time.time()
        pair = make_pair(name)
        torch.set_num_threads(THREADS[1])
        r = run_free(pair, make_frames(name), c["q"] if c["codec"] == "dc" else None, c["h"], c["w"], c["gop"], name,
                     None, player=OraclePlayer(pair, THREADS[0]), grow=c.get("grow", True))
        assert r["sym_diff"] == 0, (name, r["sym_diff"])
        cases[name] = dict({k: c[k] for k in ("codec", "weights", "q", "frames", "h", "w", "gop")},
                           dpb={k: {"maxabs": v["maxabs"], "rel": v["rel"], "frame": v["frame"],
                                    "growth": r["growth"][k]["ratio"] if k in r["growth"] else None}
                                for k, v in r["dpb"].items()},
                           forced=r["forced"], sym_diff=r["sym_diff"], idx_diff=r["idx_diff"],
                           idx_diff_max_per_frame=r["idx_diff_max"], rec_maxabs=r["rec_maxabs"])
        print(name, f"{time.time() - t0:.0f} s", json.dumps(cases[name]["dpb"]), flush=True)
    with open(OUT, "w") as f:
        json.dump({"source": "oracle vs oracle, free running: %d threads against %d threads replaying its ties "
                             "(tests/golden/make_golden_freerun.py)" % THREADS, "threads": list(THREADS),
                   "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
