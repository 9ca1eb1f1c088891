"""Golden vectors of the full-resolution colour arithmetic from the reference's
own code: rgb_to_ycbcr and ycbcr_to_rgb (DCVC-DC/src/transforms/functional.py:
95-126), imported from /root/reference by path, on 4:4:4 frames of 8, 10 and
16-bit samples and on writer frames that leave [0, 1] on both sides.

Inputs are regenerated from the seeds stored in the fixture (``inputs`` /
``writer_inputs`` below, which the tests import).  chroma_golden.json holds
seeds, shapes, depths and the sha256 of each output's bytes; chroma_golden.npz
the full arrays of the 2 x 2 cases and of 37 x 53 at 10 bits.

    python tests/golden/make_golden_chroma.py
"""
import hashlib
import json
import os
import sys

import numpy as np

REF = "/root/reference/DCVC-DC"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT_JSON = os.path.join(HERE, "chroma_golden.json")
OUT_NPZ = os.path.join(HERE, "chroma_golden.npz")

SHAPES = [(31, 2, 2), (32, 37, 53)]           # (seed, h, w)
DEPTHS = (8, 10, 16)
STORED = {(2, 2, 8), (2, 2, 10), (2, 2, 16), (37, 53, 10)}


def inputs(seed, h, w, d):
    """A 4:4:4 frame (3, h, w) of d-bit samples (uint8 at 8 bits, else uint16),
    uniform in [0, max_val], with 0 and max_val planted in every plane.  Its
    colours cover the whole YCbCr cube, so ycbcr_to_rgb clips on both sides."""
    mx = (1 << d) - 1
    g = np.random.Generator(np.random.PCG64(seed * 100 + d))
    a = g.integers(0, mx + 1, size=(3, h, w), dtype=np.uint16)
    for c in range(3):
        flat = a[c].reshape(-1)
        flat[c % flat.size] = 0
        flat[(c + 1) % flat.size] = mx
    return a.astype(np.uint8) if d == 8 else a


def writer_inputs(seed, h, w):
    """float32 RGB frame (3, h, w), uniform in [-0.1, 1.1), with the exact ends
    0 and 1 and values below 0 and above 1 planted."""
    g = np.random.Generator(np.random.PCG64(seed * 100 + 77))
    f = (g.random((3, h, w)) * 1.2 - 0.1).astype(np.float32)
    flat = f.reshape(-1)
    special = np.array([0, 1, -0.25, 1.5], dtype=np.float32)
    flat[:min(4, flat.size)] = special[:min(4, flat.size)]
    flat[-4:] = special[::-1]
    return f


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    sys.path.insert(0, REF)
    from src.transforms import functional as F
    rows, arrays = [], {}
    for seed, h, w in SHAPES:
        for d in DEPTHS:
            mx = (1 << d) - 1
            yuv = inputs(seed, h, w, d).astype(np.float32) / mx      # the readers' sample rule
            fr = writer_inputs(seed, h, w)
            vals = {"yuv_to_rgb": F.ycbcr_to_rgb(yuv), "rgb_to_yuv": F.rgb_to_ycbcr(fr)}
            for k, v in vals.items():
                assert v.dtype == np.float32 and v.shape == (3, h, w), (k, v.dtype, v.shape)
                assert v.min() == 0 and v.max() == 1, k               # clipped on both sides
            row = {"seed": seed, "h": h, "w": w, "depth": d}
            row.update({k: digest(v) for k, v in vals.items()})
            rows.append(row)
            if (h, w, d) in STORED:
                for k, v in vals.items():
                    arrays[f"{k}_{h}x{w}_{d}"] = v
    with open(OUT_JSON, "w") as f:
        json.dump({"source": "DCVC-DC/src/transforms/functional.py rgb_to_ycbcr / ycbcr_to_rgb; sha256 of the "
                             "float32 bytes", "cases": rows}, f, indent=1)
    np.savez_compressed(OUT_NPZ, **arrays)
    print(json.dumps(rows[:2], indent=1), len(rows), os.path.getsize(OUT_NPZ))


if __name__ == "__main__":
    main()
