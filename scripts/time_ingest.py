"""Microseconds per 1080p frame of the source-ingest kernels: the matched
paths (frame_to_nhwc, yuv420_to_nhwc) and the two cross-format paths
(yuv420_to_rgb_nhwc; rgb_to_yuv420_planes + yuv420f_to_nhwc).

Method: 20 warm-up calls, then 7 repetitions of 50 back-to-back launches on
one stream between two HIP events; the per-launch time of each repetition is
the event interval / 50 (launch overhead of a saturated queue included, the
inputs stay in the GPU's caches).  Reports median, min and max over the 7.

    python scripts/time_ingest.py [out.json]    # profiles/crossfmt_ingest_us_1080p.json
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcvc_amd import hip as K  # noqa: E402

WARMUP, REPS, LAUNCHES = 20, 7, 50


def main():
    h, w, H, W = 1080, 1920, 1088, 1920
    dev = torch.device("cuda", 0)
    g = np.random.default_rng(0)
    y = torch.from_numpy(g.integers(0, 256, (h, w), dtype=np.uint8)).to(dev)
    uv = torch.from_numpy(g.integers(0, 256, (2, h // 2, w // 2), dtype=np.uint8)).to(dev)
    rgb = torch.from_numpy(g.integers(0, 256, (3, h, w), dtype=np.uint8)).to(dev)
    x = K.empty(H, W, 3, K.F32, dev)
    pl = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    yf = torch.empty((h, w), dtype=torch.float32, device=dev)
    uvf = torch.empty((2, h // 2, w // 2), dtype=torch.float32, device=dev)

    def rgb_path():
        K.rgb_to_yuv420_planes(rgb, h, w, yf, uvf)
        K.yuv420f_to_nhwc(yf, uvf, h, w, x)

    cases = {"yuv420_to_nhwc": lambda: K.yuv420_to_nhwc(y, uv, h, w, x),
             "frame_to_nhwc": lambda: K.frame_to_nhwc(rgb, h, w, x),
             "yuv420_to_rgb_nhwc": lambda: K.yuv420_to_rgb_nhwc(y, uv, h, w, x, pl),
             "rgb_to_yuv420_planes+yuv420f_to_nhwc": rgb_path}
    out = {"method": f"scripts/time_ingest.py: {h}x{w}, {WARMUP} warm-up calls, {REPS} x {LAUNCHES} back-to-back "
                     "launches between HIP events, us per launch; one box"}
    for name, f in cases.items():
        for _ in range(WARMUP):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                f()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1000 / LAUNCHES)
        out[name] = {"us_median": round(float(np.median(ts)), 2), "us_min": round(min(ts), 2),
                     "us_max": round(max(ts), 2)}
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
