"""Golden vectors of the cross-format source conversions from the reference's
own functions (DCVC-DC/src/transforms/functional.py:16-72: ycbcr420_to_rgb,
rgb_to_ycbcr420, ycbcr420_to_444; numpy / scipy only), imported from
/root/reference by path.  Inputs are regenerated from the seeds stored in the
fixture.  crossfmt_golden.json holds seeds, shapes and the sha256 of each
output's float32 bytes; crossfmt_golden.npz the full arrays of the two small
cases.

    python tests/golden/make_golden_crossfmt.py
"""
import hashlib
import importlib.util
import json
import os

import numpy as np

REF = "/root/reference/DCVC-DC/src/transforms/functional.py"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT_JSON = os.path.join(HERE, "crossfmt_golden.json")
OUT_NPZ = os.path.join(HERE, "crossfmt_golden.npz")

# (seed, h, w): the degenerate 2-pixel zoom axes, odd half-planes (19 x 27),
# 100 x 130 of the end-to-end tests, and 1080p
CASES = [(11, 2, 2), (12, 38, 54), (13, 100, 130), (14, 1080, 1920)]
STORED = {(2, 2), (38, 54)}


def inputs(seed, h, w):
    """uint8 source planes of both formats: y (h, w), uv (2, h/2, w/2) and
    CHW RGB (3, h, w)."""
    g = np.random.Generator(np.random.PCG64(seed))
    y = g.integers(0, 256, size=(h, w), dtype=np.uint8)
    uv = g.integers(0, 256, size=(2, h // 2, w // 2), dtype=np.uint8)
    rgb = g.integers(0, 256, size=(3, h, w), dtype=np.uint8)
    return y, uv, rgb


def digest(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return hashlib.sha256(a.tobytes()).hexdigest()


def main():
    spec = importlib.util.spec_from_file_location("ref_functional", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    rows, arrays = [], {}
    for seed, h, w in CASES:
        y8, uv8, rgb8 = inputs(seed, h, w)
        # the readers' float conversion (video_reader.py:70-71, 155-156)
        rgb = m.ycbcr420_to_rgb(y8.astype(np.float32)[None] / 255, uv8.astype(np.float32) / 255, order=1)
        y, uv = m.rgb_to_ycbcr420(rgb8.astype("float32") / 255.)
        yuv444 = m.ycbcr420_to_444(y, uv, order=0)
        rows.append({"seed": seed, "h": h, "w": w, "rgb": digest(rgb), "y": digest(y), "uv": digest(uv),
                     "yuv444": digest(yuv444)})
        if (h, w) in STORED:
            for k, a in (("rgb", rgb), ("y", y), ("uv", uv), ("yuv444", yuv444)):
                arrays[f"{k}_{h}x{w}"] = a
    with open(OUT_JSON, "w") as f:
        json.dump({"source": "DCVC-DC/src/transforms/functional.py ycbcr420_to_rgb(order=1), rgb_to_ycbcr420, "
                             "ycbcr420_to_444(order=0) of uint8 / 255 inputs; sha256 of the float32 bytes",
                   "cases": rows}, f, indent=1)
    np.savez_compressed(OUT_NPZ, **arrays)
    print(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
