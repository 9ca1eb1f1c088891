"""Free-running parity over whole GOPs (tests/parity.py states the bars).

A "player" codes every frame from ITS OWN decoded picture buffer: the HIP
product through real .bin files (tests/test_gpu_freerun_parity.py), or, on the
CPU, a second oracle at another thread count (the self-noise fixture of
tests/golden/make_golden_freerun.py, tests/test_freerun_bar.py).  The judging
oracle codes the same frame once from its own previous DPB, with the player's
symbols replayed at its rounding ties (Forcer), and never receives a float
from the player.  Per frame the replay's strict bar holds (compare_forced /
check_forced), the decoded picture lies within REC_MAXABS, and every DPB
tensor is compared (compare_dpb); after the last frame the differences may
not have grown (growth).
"""
import json
import os
import tempfile

import numpy as np
import torch

from tests.parity import (DPB_KEYS, REC_MAXABS, REC_MAXABS_HEM, TIE_EPS, _np, check_dpb, check_forced, check_growth,
                          compare_dpb, compare_forced, growth, rec_maxabs)
from tests.test_gpu_parity_strict import OUT, HemPair, Pair, psnr   # OUT: where the records go

# codec, weights, rate, frames of moving_pattern (seed 1), size, padding, GOP:
# the smallest padded sizes that are no multiple of 64.  DC-bench is the
# bench's own GOP (I + 31 P); the other two cross two GOP boundaries.
CASES = {
    "DC-bench": dict(codec="dc", weights="bench", q=0, frames=32, h=120, w=136, pad=(16, "replicate"), gop=32),
    "DC-golden": dict(codec="dc", weights="golden", q=40, frames=17, h=100, w=130, pad=(16, "replicate"), gop=8),
    "HEM-bench": dict(codec="hem", weights="bench", q=0, frames=16, h=120, w=136, pad=(64, "constant"), gop=8),
    # yardstick only (no product case): the HEM golden config C1 in write mode (I, P1, P2 of its
    # torch.rand frames, IP=4), the frames the teacher-forced hem_C1 cases of
    # tests/test_gpu_parity_strict.py code.  Three frames have no quarters, so the growth bar is
    # not asserted on it (its ratio is recorded).
    "HEM-C1": dict(codec="hem", weights="golden", tag="C1", q=None, frames=3, h=256, w=256, pad=(64, "constant"),
                   gop=4, grow=False),
}


def make_pair(case, prec=None):
    """The case's Pair / HemPair; ``prec=None``: the oracle alone (CPU)."""
    import bench
    c = CASES[case]
    kw = dict(prec=prec) if prec else dict(product=False)
    if c["weights"] == "golden" and c["codec"] == "hem":
        from tests.hem_fixtures import HEMGolden
        g = HEMGolden()
        return HemPair(g.i_state_dict(), g.p_state_dict(), g.q(c["tag"]), **kw)
    if c["weights"] == "golden":
        from tests.dc_fixtures import DCGolden
        g = DCGolden()
        return Pair(g.i_state_dict(), g.p_state_dict(), **kw)
    isd, psd = bench.make_weights(None, 0, torch.device("cpu"), c["codec"])
    if c["codec"] == "hem":
        return HemPair(isd, psd, bench.hem_q(isd, psd, c["q"]), **kw)
    return Pair(isd, psd, **kw)


def make_frames(case, frames=None, h=None, w=None):
    """[(x (1, 3, h, w), x padded)] of a case (or of another count / size)."""
    from dcvc_amd.synth import moving_pattern, to_float
    c = CASES[case]
    if "tag" in c:   # the golden fixture's own frames
        from tests.hem_fixtures import HEMGolden
        g = HEMGolden()
        return [g.frame_tensor(c["tag"], t) for t in range(frames or c["frames"])]
    h, w, (m, mode) = h or c["h"], w or c["w"], c["pad"]
    out = []
    for t in range(frames or c["frames"]):
        x = torch.from_numpy(to_float(moving_pattern(h, w, t, seed=1))).unsqueeze(0)
        out.append((x, torch.nn.functional.pad(x, (0, -w % m, 0, -h % m), mode=mode)))
    return out


def as_player(calls):
    """An oracle's calls [(kind, symbols, indexes)] as a player's trace."""
    return [(np.clip(_np(s).astype(np.int64), -30000, 30000), _np(i).astype(np.int64)) for _, s, i in calls]


class ProductPlayer:
    """The HIP codecs of a Pair, each frame from the DPB they returned."""

    def __init__(self, pair, h, w, folder):
        self.pair, self.h, self.w, self.folder, self.dpb = pair, h, w, folder, None

    def __call__(self, t, intra, xp, q, fidx):
        enc, bits, rec, self.dpb = self.pair.product(0 if intra else 1, xp, self.dpb, q, fidx,
                                                     os.path.join(self.folder, f"{t}.bin"), self.h, self.w,
                                                     want_dpb=True)
        return enc, bits, rec, self.dpb


class OraclePlayer:
    """The oracle at ``threads`` CPU threads playing the product; ``perturb
    (dpb)`` may change the DPB it keeps (and shows) after every frame."""

    def __init__(self, pair, threads, perturb=None):
        self.pair, self.threads, self.perturb, self.dpb = pair, threads, perturb, None

    def __call__(self, t, intra, xp, q, fidx):
        n = torch.get_num_threads()
        torch.set_num_threads(self.threads)
        try:
            calls, _, bits, self.dpb = self.pair.oracle(0 if intra else 1, xp, self.dpb, q, fidx)
        finally:
            torch.set_num_threads(n)
        if self.perturb is not None:
            self.perturb(self.dpb)
        return as_player(calls), bits, self.dpb["ref_frame"].clamp(0, 1), self.dpb


def run_free(pair, frames, q, h, w, gop, name, factor, noise=None, player=None, record=None, grow=True):
    """frames: [(x, x padded)]; frame t is an I-frame when t % gop == 0 and
    carries frame_idx t % 4.  ``player`` defaults to the pair's HIP product.
    Returns {"frames": per-frame rows, "dpb": per-key maxima, "growth", ...};
    ``record``: a JSON file that receives it under ``name`` before the DPB
    and growth bars are asserted (``grow=False``: the growth ratio is only
    returned, for a run too short to have quarters)."""
    from oracle.dc_oracle import Forcer
    rec_bar = REC_MAXABS_HEM if isinstance(pair, HemPair) else REC_MAXABS
    rows, dpb_o = [], None
    with tempfile.TemporaryDirectory() as td:
        play = player or ProductPlayer(pair, h, w, td)
        for t, (x, xp) in enumerate(frames):
            intra, fidx = t % gop == 0, t % 4
            tt = 0 if intra else 1
            enc, bits, rec, dpb_p = play(t, intra, xp, q, fidx)
            fr = Forcer([s for s, _ in enc], TIE_EPS)
            calls_f, tap_f, bits_f, dpb_o = pair.oracle(tt, xp, dpb_o, q, fidx, force=fr)
            sf = compare_forced(enc, calls_f, tap_f, fr.forced)
            p, p_f = psnr(rec[:, :, :h, :w], x), psnr(dpb_o["ref_frame"][:, :, :h, :w], x)
            sf.update({"t": t, "type": "I" if intra else "P", "bits": int(bits), "bits_replay": int(bits_f),
                       "psnr": p, "psnr_replay": p_f,
                       "rec_maxabs": rec_maxabs(rec[:, :, :h, :w], dpb_o["ref_frame"][:, :, :h, :w].clamp(0, 1))})
            if sf["sym_diff"] == 0:
                sf["bits_replay_tied"] = pair.coded_bits(tt, [(c[0], ps, pi) for c, (ps, pi) in zip(calls_f, enc)])
            check_forced(sf, bits, bits_f, p, p_f, f"{name} t={t}", rec_bar)
            assert sf["rec_maxabs"] <= rec_bar, (name, t, sf["rec_maxabs"])
            sf["dpb"] = compare_dpb(dpb_p, dpb_o, h, w, noise, factor)
            rows.append(sf)
    rel = [{k: v["rel"] for k, v in r["dpb"].items()} for r in rows]
    top = {}
    for k in DPB_KEYS:
        ts = [t for t in range(len(rows)) if k in rows[t]["dpb"]]
        if ts:
            t = max(ts, key=lambda t: rows[t]["dpb"][k]["rel"])
            top[k] = dict(rows[t]["dpb"][k], frame=t, maxabs=max(rows[u]["dpb"][k]["maxabs"] for u in ts))
    out = {"frames": rows, "dpb": top, "growth": growth(rel, gop), "forced": sum(r["forced"] for r in rows),
           "sym_diff": sum(r["sym_diff"] for r in rows), "idx_diff": sum(r["idx_diff"] for r in rows),
           "idx_diff_max": max(r["idx_diff"] for r in rows), "rec_maxabs": max(r["rec_maxabs"] for r in rows)}
    if record is not None:
        os.makedirs(os.path.dirname(record), exist_ok=True)
        d = json.load(open(record)) if os.path.exists(record) else {}
        d[name] = out
        json.dump(d, open(record, "w"), indent=1)
    for r in rows:   # after the record is written
        check_dpb(r["dpb"], f"{name} t={r['t']}")
    if grow:
        check_growth(out["growth"], name)
    return out
