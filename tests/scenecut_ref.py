"""numpy restatement of the scene statistics (include/dcvc_hip.h
dcvc_scene_stats, INTEGRATION.md "Scene-cut keyframes"), and the synthetic
sequences the scene-cut tests share.

Everything is integer arithmetic over int64, so the kernel's two words must
equal these exactly, whatever its reduction order.
"""
import numpy as np

BINS = 64


def samples(plane, depth):
    """A plane as int64 samples: uint8 at depth 8, the unsigned reading of a
    2-byte integer array above (an int16 array holds the bits of uint16)."""
    a = np.ascontiguousarray(np.asarray(plane)).reshape(-1)
    if depth == 8:
        assert a.dtype == np.uint8, a.dtype
    else:
        assert a.dtype.itemsize == 2 and a.dtype.kind in "iu", a.dtype
        a = a.view(np.uint16)
    return a.astype(np.int64)


def hist(plane, depth):
    """64 bins; the bin of a sample is sample >> (depth - 6).  (A sample above
    (1 << depth) - 1, which no valid plane holds, counts in the last bin.)"""
    return np.bincount(np.minimum(samples(plane, depth) >> (depth - 6), BINS - 1), minlength=BINS).astype(np.int64)


def sad(cur, prev, depth):
    return int(np.abs(samples(cur, depth) - samples(prev, depth)).sum())


def hdiff(cur, prev, depth):
    return int(np.abs(hist(cur, depth) - hist(prev, depth)).sum())


def stats(cur, prev, depth):
    """(sad, hdiff): the two words dcvc_scene_stats writes."""
    return sad(cur, prev, depth), hdiff(cur, prev, depth)


def score(cur, prev, depth):
    """What SceneCutDetector.score returns for a pair of planes."""
    n, max_val = samples(cur, depth).size, (1 << depth) - 1
    s, hd = stats(cur, prev, depth)
    return {"sad": s, "hdiff": hd, "n": n, "max_val": max_val, "mad": s / (n * max_val), "hd": hd / (2 * n)}


def scores(planes, depth):
    """[None, score(planes[1], planes[0]), ...]: the detector over a sequence."""
    return [None] + [score(planes[t], planes[t - 1], depth) for t in range(1, len(planes))]


# ---- the sequences of the tests: 11 frames at 100 x 130 with a hard cut at frame 5
H, W, FRAMES, CUT = 100, 130, 11, 5


def cut_sequence(darken):
    """moving_pattern seed 1 for t < 5, seed 2 from frame 5 on (uint8 CHW RGB);
    ``darken`` halves the samples after the cut, which moves the histogram."""
    from dcvc_amd.synth import moving_pattern
    out = []
    for t in range(FRAMES):
        if t < CUT:
            out.append(moving_pattern(H, W, t, seed=1))
        else:
            f = moving_pattern(H, W, t, seed=2)
            out.append(f // 2 if darken else f)
    return out


def yuv420_sequence_10bit(n=4):
    """moving_pattern_yuv420 scaled to 10 bits: [(y, uv)] as uint16."""
    from dcvc_amd.synth import moving_pattern_yuv420
    out = []
    for t in range(n):
        y, uv = moving_pattern_yuv420(H, W, t, seed=1 if t < 2 else 2)
        out.append((y.astype(np.uint16) * 4 + (t & 3), uv.astype(np.uint16) * 4))
    return out
