"""Strict per-frame parity between the HIP product and the CPU oracle.

The reference computes every symbol as round(y - means) and every CDF index
as int((log(scale) - log_min) / step) of fp32 network outputs.  Both are
discontinuous: a value within float rounding error of a half-integer (symbol)
or of an integer (index) lands on either side depending on the order in
which a convolution sums its products.  The reference itself is not stable
under that: the same model on the same input run with 1 and with 8 CPU threads
changes a CDF index and the estimated bits.  So "bit-exact" is
checked here as:

  * every coder call the product makes equals the oracle's, symbol for symbol
    and index for index, EXCEPT at elements whose oracle pre-rounding /
    pre-truncation value lies within TIE_EPS of the discontinuity (a tie);
  * the first symbol that differs, in the order the codec computes them
    (mv_z, mv_y quadtree steps, z, y quadtree steps), must be such a tie.  A
    changed symbol changes y_hat, which every later step and call of the frame
    reads, so differences after it are a consequence (a "cascade");
  * the cascade is then checked element by element, not excused: the oracle
    codes the frame again with the product's symbols replayed at its own
    rounding ties (oracle.dc_oracle.Forcer), so it runs every later step on the
    product's y_hat.  In that replay every symbol must equal the product's and
    every index must equal it or sit on a tie of the replay's own values
    (compare_forced), and the product's reconstruction must lie within PSNR_DB
    of the replay's, which is the oracle's decode of the product's stream;
  * a frame whose calls all agree has identical bits (the coder is
    deterministic) and its reconstruction within PSNR_DB of the oracle's;
  * the reconstruction itself, pixel by pixel: the product's decoded frame
    within REC_MAXABS of the oracle's (of the replay's after a flipped tie).
    With seeded random weights every picture sits at 6-7 dB, where the PSNR
    bar alone bounds only the mean squared error.

Two tie widths.  A symbol tie is a distance to a half-integer of y - means
(unit scale), and the first flips seen sit within 4.2e-7 of it: SYM_TIE_EPS.
An index is (log(scale) - log(scale_min)) / step with a table step near 0.1,
so fp32 reordering noise in a scale (~1e-5 relative after a deep network)
shows as ~1e-4 in index units; the widest index tie seen is 4.8e-4:
IDX_TIE_EPS.  That width alone would let a systematic kernel error of ~1e-4
relative in the scales pass as ties, one index in a thousand flipped; the
count does not: IDX_RATE caps the differing indexes of a frame (before its
first flipped symbol, or in the replay) at 1e-4 of the indexes compared (the
codec's frames show 1-25 per million).

The decoded picture buffer.  The symbols and pixels above do not see an error
of 1e-4 relative in ref_feature (tests/test_freerun_bar.py shows it on the
CPU), so the tensors a P-frame hands to the next one are compared directly
(compare_dpb / check_dpb): max |product - oracle| over max |oracle| per tensor,
against the oracle's own reordering noise.  That noise is measured, not chosen:
tests/golden/make_golden_freerun.py runs the oracle with 16 threads and again
with 1, each on its own DPB, and records per tensor the largest relative
difference of a whole GOP in tests/golden/freerun_selfnoise.json.  The bar is
DPB_FACTOR[precision] times that figure.
"""
import json
import os

import numpy as np

SYM_TIE_EPS = 1e-5    # symbol: distance of y - means to the half-integer (largest first flip seen: 4.2e-7)
IDX_TIE_EPS = 1e-3    # index: distance of the pre-truncation index to the integer (largest seen: 4.8e-4)
IDX_RATE = 1e-4       # differing indexes per index compared (codec frames: <= 2.5e-5)
IDX_FLOOR = 8         # ... but at least this many on small frames
TIE_EPS = SYM_TIE_EPS  # the symbols the replay forces (oracle.*.Forcer)
PSNR_DB = 1e-4        # BASELINE.json: PSNR delta < 1e-4 dB
REC_MAXABS = 1e-5     # decoded pixel values (0..1), product vs oracle / replay (DC: largest seen <= 1e-5)
REC_MAXABS_HEM = 1e-4  # ... DCVC-HEM (largest seen 4.4e-5, C2 1080p split; 1/39 of an 8-bit level)
# DPB tensors: allowed rel = factor x the oracle's recorded self-noise (freerun_selfnoise.json).
#   parity: the same fp32 products as the oracle in another summation order; 4 covers an MFMA
#           K-blocking that differs more from either CPU order than the two CPU orders from each other.
#   split:  each product carries 2^-21 instead of 2^-24 (8x), times 2 for the spread of a maximum
#           taken over one seed.
DPB_FACTOR = {"parity": 4, "split": 16}
GROWTH = 2.0          # last quarter of a free run vs the first quarter of its P-frames (oracle vs itself: ~1)
DPB_KEYS = ("ref_frame", "ref_feature", "ref_mv_feature", "ref_y", "ref_mv_y")
SELFNOISE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freerun_selfnoise.json")


def selfnoise(case, unmeasured=None):
    """{key: rel} of a case of the committed fixture.  ``unmeasured``: the case whose figure stands
    in for a tensor on which this case's two runs agreed to the bit (rel 0: at 256x256 the motion
    path is too small for the thread count to reorder its sums), which says nothing about noise."""
    with open(SELFNOISE) as f:
        cases = json.load(f)["cases"]
    out = {k: v["rel"] for k, v in cases[case]["dpb"].items()}
    if unmeasured is not None:
        out.update({k: cases[unmeasured]["dpb"][k]["rel"] for k, v in out.items() if v == 0})
    return out


def dpb_view(v):
    """torch view of a DPB entry (Act, tensor or None)."""
    return v.t() if hasattr(v, "buf") else v


def keep_dpb(dpb):
    """A copy of a DPB that later frames cannot touch."""
    return {k: (None if v is None else dpb_view(v).clone()) for k, v in dpb.items()}


def _chw(v):
    """A DPB entry as a float32 (C, H, W) array: an Act is (H, W, C), a tensor (1, C, H, W)."""
    t = dpb_view(v)
    t = t.permute(2, 0, 1) if hasattr(v, "buf") else t.reshape(t.shape[-3:])
    return t.detach().float().cpu().numpy()


def compare_dpb(prod_dpb, oracle_dpb, h, w, noise=None, factor=None):
    """Per DPB key {"maxabs", "rel", "bar", "ratio"}: rel = max |product - oracle| / max |oracle| in float64;
    ref_frame clamped to [0, 1] and cropped to h x w, the other tensors whole.  bar = factor *
    noise[key] (None where no noise is given), ratio = rel / bar.  A key that is None on one side
    must be None on both."""
    out = {}
    for k in DPB_KEYS:
        if k not in oracle_dpb and k not in prod_dpb:
            continue
        a, b = prod_dpb.get(k), oracle_dpb.get(k)
        if a is None or b is None:
            assert a is None and b is None, f"{k}: None on one side only"
            continue
        a, b = _chw(a), _chw(b)
        if k == "ref_frame":
            a, b = np.clip(a[:, :h, :w], 0, 1), np.clip(b[:, :h, :w], 0, 1)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        # the differences in float64, a channel at a time (a 4K ref_feature is 1.6 GB in fp32)
        maxabs = max(float(np.abs(a[c].astype(np.float64) - b[c]).max()) for c in range(a.shape[0]))
        bar = factor * noise[k] if noise is not None else None   # a tensor without a recorded noise is an error
        rel = maxabs / float(np.abs(b).max())
        out[k] = {"maxabs": maxabs, "rel": rel, "bar": bar, "ratio": rel / bar if bar else None}
    return out


def dpb_over(d):
    """The keys of compare_dpb's dict that miss their bar (NaN misses)."""
    return {k: v for k, v in d.items() if v["bar"] is not None and not v["rel"] <= v["bar"]}


def check_dpb(d, name=""):
    bad = dpb_over(d)
    assert not bad, f"{name} DPB over the bar: " + ", ".join(
        f"{k} rel={v['rel']:.3g} > {v['bar']:.3g} ({v['rel'] / v['bar']:.2f}x)" for k, v in bad.items())


def growth(rows, gop):
    """rows[t]: {key: rel} of frame t of a free run.  Per key {"first", "last", "ratio"}: the largest
    rel over the first quarter of the P-frames and over the last quarter of the frames."""
    n = len(rows)
    pf = [t for t in range(n) if t % gop]
    first, last = pf[:-(-len(pf) // 4)], range(n - max(1, n // 4), n)
    out = {}
    for k in DPB_KEYS:
        a = [rows[t][k] for t in first if k in rows[t]]
        b = [rows[t][k] for t in last if k in rows[t]]
        if a and b:
            out[k] = {"first": max(a), "last": max(b), "ratio": max(b) / max(a) if max(a) > 0 else float(max(b) > 0)}
    return out


def check_growth(g, name=""):
    bad = {k: v for k, v in g.items() if not v["last"] <= GROWTH * v["first"]}
    assert not bad, f"{name} DPB difference grows over the run: {bad}"


def idx_allowed(n):
    """Differing indexes allowed among n compared."""
    return max(IDX_FLOOR, int(IDX_RATE * n))


def rec_maxabs(a, b):
    """max |a - b| of two decoded frames (any shape, same size)."""
    a = np.asarray(a.detach().float().cpu() if hasattr(a, "detach") else a, dtype=np.float64)
    b = np.asarray(b.detach().float().cpu() if hasattr(b, "detach") else b, dtype=np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


def _np(t):
    return t.detach().reshape(-1).cpu().numpy() if hasattr(t, "detach") else np.asarray(t).reshape(-1)


def sym_tie_distance(pre):
    """|distance of pre to the nearest half-integer| (round() flips there)."""
    a = np.abs(pre.astype(np.float64))
    return np.abs(a - np.floor(a) - 0.5)


def idx_tie_distance(v):
    """distance of the pre-truncation index to the nearest integer."""
    v = v.astype(np.float64)
    return np.abs(v - np.round(v))


def compare_frame(prod_calls, oracle_calls, tap):
    """prod_calls: [(symbols, indexes)] in stream order (the product's encoder
    trace); oracle_calls: [(kind, symbols, indexes)] in stream order; tap: the
    oracle's compress(tap=...) dict.  Returns a stats dict."""
    assert len(prod_calls) == len(oracle_calls), (len(prod_calls), len(oracle_calls))
    out = {"calls": [], "symbols": 0, "sym_diff": 0, "idx_diff": 0, "first_flip": None,
           "unexplained": [], "cascade_sym": 0, "cascade_idx": 0, "max_tie_dist": 0.0,
           "max_sym_tie": 0.0, "max_idx_tie": 0.0, "idx_compared": 0, "idx_diff_compared": 0}
    flipped = False
    for c in tap["order"]:
        ps, pi = (np.asarray(a).reshape(-1) for a in prod_calls[c])
        kind, os_, oi = oracle_calls[c]
        os_ = np.clip(_np(os_), -30000, 30000).astype(np.int64)
        oi = _np(oi).astype(np.int64)
        ds = np.nonzero(ps.astype(np.int64) != os_)[0]
        di = np.nonzero(pi.astype(np.int64) != oi)[0]
        out["symbols"] += ps.size
        out["sym_diff"] += int(ds.size)
        out["idx_diff"] += int(di.size)
        rec = {"call": c, "kind": kind, "n": int(ps.size), "sym_diff": int(ds.size), "idx_diff": int(di.size)}
        if flipped:
            out["cascade_sym"] += int(ds.size)
            out["cascade_idx"] += int(di.size)
        else:
            out["idx_compared"] += int(pi.size)
            out["idx_diff_compared"] += int(di.size)
            if di.size:
                d = idx_tie_distance(_np(tap["idx_f"][c])[di]) if tap["idx_f"][c] is not None else np.full(di.size, 1.0)
                rec["idx_tie_max"] = float(d.max())
                out["max_tie_dist"] = max(out["max_tie_dist"], float(d.max()))
                out["max_idx_tie"] = max(out["max_idx_tie"], float(d.max()))
                bad = di[d >= IDX_TIE_EPS]
                if bad.size:
                    out["unexplained"].append({"call": c, "what": "index", "pos": bad[:8].tolist(),
                                               "dist": d[d >= IDX_TIE_EPS][:8].tolist()})
            if ds.size:
                d = sym_tie_distance(_np(tap["pre"][c])[ds])
                rec["sym_tie_max"] = float(d.max())
                out["max_tie_dist"] = max(out["max_tie_dist"], float(d.max()))
                out["max_sym_tie"] = max(out["max_sym_tie"], float(d.max()))
                bad = ds[d >= SYM_TIE_EPS]
                if bad.size:
                    out["unexplained"].append({"call": c, "what": "symbol", "pos": bad[:8].tolist(),
                                               "dist": d[d >= SYM_TIE_EPS][:8].tolist()})
                out["first_flip"] = {"call": c, "kind": kind, "count": int(ds.size), "tie_dist": d[:8].tolist()}
                flipped = True
        out["calls"].append(rec)
    out["identical"] = out["sym_diff"] == 0 and out["idx_diff"] == 0
    return out


def compare_forced(prod_calls, oracle_calls, tap, forced):
    """The replay (module docstring): oracle_calls / tap from the oracle coding
    the frame with the product's symbols forced at ties (``forced`` of them).
    Every symbol must now agree; every differing index must be a tie of the
    replay's own pre-truncation values."""
    out = {"forced": int(forced), "sym_diff": 0, "idx_diff": 0, "unexplained": [], "max_tie_dist": 0.0,
           "idx_compared": 0}
    for c in tap["order"]:
        ps, pi = (np.asarray(a).reshape(-1) for a in prod_calls[c])
        kind, os_, oi = oracle_calls[c]
        os_ = np.clip(_np(os_), -30000, 30000).astype(np.int64)
        oi = _np(oi).astype(np.int64)
        ds = np.nonzero(ps.astype(np.int64) != os_)[0]
        di = np.nonzero(pi.astype(np.int64) != oi)[0]
        out["sym_diff"] += int(ds.size)
        out["idx_diff"] += int(di.size)
        out["idx_compared"] += int(pi.size)
        if ds.size:
            d = sym_tie_distance(_np(tap["pre"][c])[ds])
            out["unexplained"].append({"call": c, "what": "symbol (replay)", "pos": ds[:8].tolist(),
                                       "dist": d[:8].tolist()})
        if di.size:
            d = idx_tie_distance(_np(tap["idx_f"][c])[di]) if tap["idx_f"][c] is not None else np.full(di.size, 1.0)
            out["max_tie_dist"] = max(out["max_tie_dist"], float(d.max()))
            bad = di[d >= IDX_TIE_EPS]
            if bad.size:
                out["unexplained"].append({"call": c, "what": "index (replay)", "pos": bad[:8].tolist(),
                                           "dist": d[d >= IDX_TIE_EPS][:8].tolist()})
    if out["idx_diff"] > idx_allowed(out["idx_compared"]):
        out["unexplained"].append({"what": "index ties (replay)", "count": out["idx_diff"],
                                   "allowed": idx_allowed(out["idx_compared"])})
    out["identical"] = out["sym_diff"] == 0 and out["idx_diff"] == 0
    return out


def check_forced(sf, bits, bits_replay, psnr, psnr_replay, name="", rec_bar=REC_MAXABS):
    """The replay's bar (compare_forced's dict; sf["rec_maxabs"]: the product's
    decoded frame against the replay's)."""
    msg = (f"{name} replay: forced={sf['forced']} dsym={sf['sym_diff']} didx={sf['idx_diff']}, "
           f"bits {bits} vs replay {bits_replay}, dPSNR={psnr - psnr_replay:.3g} dB, "
           f"rec maxabs={sf.get('rec_maxabs')}, unexplained={sf['unexplained']}")
    assert not sf["unexplained"], msg
    if sf["sym_diff"] == 0 and "rec_maxabs" in sf:
        assert sf["rec_maxabs"] <= rec_bar, msg
    if sf["identical"]:
        assert bits == bits_replay, msg
    if "bits_replay_tied" in sf:
        # symbols all agree: the replay coded with the product's decisions at
        # its index ties is the product's stream
        assert bits == sf["bits_replay_tied"], msg + f", replay with the product's tie indexes {sf['bits_replay_tied']}"
    assert abs(psnr - psnr_replay) < PSNR_DB, msg
    return msg


def check_frame(st, bits, bits_oracle, psnr, psnr_oracle, name="", rec_bar=REC_MAXABS):
    """The strict bar (module docstring).  st: compare_frame's dict
    (st["rec_maxabs"]: the product's decoded frame against the oracle's)."""
    msg = (f"{name}: dsym={st['sym_diff']} didx={st['idx_diff']} of {st['symbols']} symbols, "
           f"bits {bits} vs oracle {bits_oracle} (d={bits - bits_oracle}), "
           f"dPSNR={psnr - psnr_oracle:.3g} dB, rec maxabs={st.get('rec_maxabs')}, "
           f"first_flip={st['first_flip']}, unexplained={st['unexplained']}")
    assert not st["unexplained"], msg
    assert st["idx_diff_compared"] <= idx_allowed(st["idx_compared"]), msg + (
        f", {st['idx_diff_compared']} index ties of {st['idx_compared']} (allowed {idx_allowed(st['idx_compared'])})")
    if st["identical"]:
        assert bits == bits_oracle, msg
    if st["sym_diff"] == 0:
        assert abs(psnr - psnr_oracle) < PSNR_DB, msg
        if "rec_maxabs" in st:
            assert st["rec_maxabs"] <= rec_bar, msg
    return msg
