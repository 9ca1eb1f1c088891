"""Scene-cut keyframes: the statistics the encoder reads per source frame,
the decision that turns them into a cut, and the keyframe schedule that turns
cuts into I frames (INTEGRATION.md "Scene-cut keyframes").

``SceneCutDetector`` is the device side: one ``hip.scene_stats`` call and one
16-byte read per frame, on source samples only, so it is the same for every
codec.  ``KeyframeSchedule`` and ``is_cut`` are plain Python.
"""
import numbers

import torch


def check_threshold(name, value):
    """A threshold of ``encode_video`` (None: off, or a number in (0, 1])."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0 < value <= 1:
        raise ValueError(f"{name} {value!r} is not None or a number in (0, 1]")
    return float(value)


def check_interval(value):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < 1:
        raise ValueError(f"min_keyframe_interval {value!r} is not an integer >= 1")
    return value


def is_cut(score, scene_cut=None, scene_cut_mad=None):
    """Whether ``score`` (a SceneCutDetector.score dict, None for the first
    frame) reaches any given threshold: hd >= scene_cut or mad >= scene_cut_mad."""
    if score is None:
        return False
    return (scene_cut is not None and score["hd"] >= scene_cut) or \
        (scene_cut_mad is not None and score["mad"] >= scene_cut_mad)


class KeyframeSchedule:
    """The frame types of one encode.  ``next(cut)`` returns "I" for the first
    frame, when ``gop_size`` frames have passed since the last keyframe, and
    when ``cut`` is true and at least ``min_keyframe_interval`` frames have
    passed since it; "P" otherwise.  A keyframe from either cause restarts the
    ``gop_size`` count, so with ``cut`` never true the types are those of
    ``frame_idx % gop_size == 0``."""

    def __init__(self, gop_size, min_keyframe_interval=1):
        if isinstance(gop_size, bool) or not isinstance(gop_size, numbers.Integral) or gop_size < 1:
            raise ValueError(f"gop_size {gop_size!r} is not an integer >= 1")
        self.gop_size = gop_size
        self.min_keyframe_interval = check_interval(min_keyframe_interval)
        self.since = None         # frames since the last keyframe; None before the first frame

    def peek(self, cut=False):
        """What ``next(cut)`` would return; the schedule does not advance."""
        if self.since is None or self.since >= self.gop_size or (cut and self.since >= self.min_keyframe_interval):
            return "I"
        return "P"

    def next(self, cut=False):
        ftype = self.peek(cut)
        self.since = 1 if ftype == "I" else self.since + 1
        return ftype


class SceneCutDetector:
    """``score(dframe)`` compares the frame ``FrameStage.upload`` just returned
    with the one before it: the Y plane of a YUV source (``dframe[0]``, any
    chroma layout), the G plane of an RGB source (``dframe[1]`` of the CHW
    frame).  It keeps a reference to the previous frame's device tensor
    (``upload`` returns a fresh one per frame), launches ``hip.scene_stats`` on
    the current stream and reads the two words back (which waits for them).
    None for the first frame, else {"sad", "hdiff", "n", "max_val",
    "mad": sad / (n max_val), "hd": hdiff / (2 n)}."""

    def __init__(self, h, w, src_format, bit_depth, device):
        from . import hip as K
        if src_format not in ("rgb", "420", "422", "444"):
            raise ValueError(f"unknown src_format {src_format!r}")
        self.depth = K.check_depth8(bit_depth)
        self.n, self.rgb = h * w, src_format == "rgb"
        if self.n < 1:
            raise ValueError(f"no samples in a {w} x {h} plane")
        self.max_val = (1 << self.depth) - 1
        self.ws = K.scene_stats_workspace(device)
        self.out = torch.empty(2, dtype=torch.int64, device=device)
        self.prev = None

    def plane(self, dframe):
        p = dframe[1] if self.rgb else dframe[0]
        if p.numel() != self.n:
            raise ValueError(f"the plane holds {p.numel()} samples, not {self.n}")
        return p

    def score(self, dframe):
        from . import hip as K
        cur = self.plane(dframe)
        prev, self.prev = self.prev, cur
        if prev is None:
            return None
        sad, hdiff = K.scene_stats(cur, prev, self.depth, self.ws, self.out).cpu().tolist()
        return {"sad": sad, "hdiff": hdiff, "n": self.n, "max_val": self.max_val,
                "mad": sad / (self.n * self.max_val), "hd": hdiff / (2 * self.n)}
