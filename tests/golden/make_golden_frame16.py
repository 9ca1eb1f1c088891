"""Golden vectors of the high-bit-depth sample rule from the reference's own
code: RGBReader / RGBWriter(bit_depth) (DCVC-DC/src/utils/video_reader.py:
83-118, video_writer.py:50-80) reading and writing real .rgb files, and
functional.py (rgb_to_ycbcr420, ycbcr420_to_rgb, ycbcr420_to_444,
ycbcr444_to_420) on their values, imported from /root/reference by path.

Inputs are regenerated from the seeds stored in the fixture (``inputs`` /
``writer_inputs`` below, which the tests import).  frame16_golden.json holds
seeds, shapes, depths and the sha256 of each output's bytes;
frame16_golden.npz the full arrays of the two small shapes.

The reference has no 16-bit YUV420 file; those rows apply its sample rule
(astype(float32) / max_val in, clip(rint(x * max_val)) out, written here as
RGBReader / RGBWriter write it) to planes and call functional.py on the result.

    python tests/golden/make_golden_frame16.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

REF = "/root/reference/DCVC-DC"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT_JSON = os.path.join(HERE, "frame16_golden.json")
OUT_NPZ = os.path.join(HERE, "frame16_golden.npz")

# (seed, h, w): the degenerate 2-pixel zoom axes, odd half-planes (19 x 27),
# 100 x 130 of the end-to-end tests
SHAPES = [(21, 2, 2), (22, 38, 54), (23, 100, 130)]
DEPTHS = (10, 12, 16)
STORED = {(2, 2), (38, 54)}


def inputs(seed, h, w, d):
    """uint16 source planes of both formats at depth d: y (h, w), uv (2, h/2,
    w/2) and CHW RGB (3, h, w), uniform in [0, max_val], with 0, max_val and
    max_val - 1 planted in each and, below 16 bits, one sample above max_val
    (the reference does not clamp it)."""
    mx = (1 << d) - 1
    g = np.random.Generator(np.random.PCG64(seed * 100 + d))
    y = g.integers(0, mx + 1, size=(h, w), dtype=np.uint16)
    uv = g.integers(0, mx + 1, size=(2, h // 2, w // 2), dtype=np.uint16)
    rgb = g.integers(0, mx + 1, size=(3, h, w), dtype=np.uint16)
    special = [0, mx, mx - 1] + ([mx + 5] if d < 16 else [])
    for a in (y, rgb):
        flat = a.reshape(-1)
        for k, v in enumerate(special):
            flat[(k * 7919 + 1) % flat.size if flat.size > len(special) else k] = v
    uv.reshape(-1)[0] = mx
    uv.reshape(-1)[-1] = 0
    return y, uv, rgb


def writer_inputs(seed, h, w, d):
    """float32 frame (3, h, w) for the writers: uniform in [-0.1, 1.1) (values
    below 0 and above 1), with a run of values whose product with max_val lies
    within one fp32 ulp of a half-integer, on both sides and on it, and the
    exact ends 0 and 1."""
    mx = (1 << d) - 1
    g = np.random.Generator(np.random.PCG64(seed * 100 + d + 50))
    f = (g.random((3, h, w)) * 1.2 - 0.1).astype(np.float32)
    flat = f.reshape(-1)
    ks = g.integers(0, mx, size=max(1, min(flat.size // 4, 64)))
    ties = [np.float32(0), np.float32(1), np.float32(-0.25), np.float32(1.5)]
    for k in ks:
        v = np.float32((np.float64(k) + 0.5) / mx)
        ties += [v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2))]
    n = min(len(ties), flat.size)
    flat[:n] = np.array(ties[:n], dtype=np.float32)
    return f


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    sys.path.insert(0, REF)
    from src.transforms import functional as F
    from src.utils.video_reader import RGBReader
    from src.utils.video_writer import RGBWriter
    rows, arrays = [], {}
    with tempfile.TemporaryDirectory() as td:
        for seed, h, w in SHAPES:
            for d in DEPTHS:
                mx = (1 << d) - 1
                y16, uv16, rgb16 = inputs(seed, h, w, d)
                # ---- in: a real .rgb file through the reference's reader, both dst formats
                path = os.path.join(td, f"s{seed}_{d}")
                with open(path + ".rgb", "wb") as f:
                    f.write(rgb16.astype("<u2").tobytes() * 2)
                rd = RGBReader(path, w, h, bit_depth=d)
                rgb = rd.read_one_frame(dst_format="rgb")
                y_c, uv_c = rd.read_one_frame(dst_format="420")
                assert rd.read_one_frame(dst_format="rgb") is None
                rd.close()
                yuv444_c = F.ycbcr420_to_444(y_c, uv_c, order=0)
                # ---- in: 16-bit YUV420 planes under the same sample rule
                y = y16.astype(np.float32)[None] / mx
                uv = uv16.astype(np.float32) / mx
                yuv444 = F.ycbcr420_to_444(y, uv, order=0)
                rgb_c = F.ycbcr420_to_rgb(y, uv, order=1)
                # ---- out: the reference's writer, RGB frame and 4:2:0 frame
                fr = writer_inputs(seed, h, w, d)
                wr = RGBWriter(os.path.join(td, f"o{seed}_{d}.rgb"), w, h, bit_depth=d)
                wr.write_one_frame(rgb=fr, src_format="rgb")
                y_w, uv_w = F.ycbcr444_to_420(fr)
                wr.write_one_frame(y=y_w, uv=uv_w, src_format="420")
                wr.close()
                out = np.fromfile(os.path.join(td, f"o{seed}_{d}.rgb"), dtype="<u2").reshape(2, 3, h, w)
                # ---- out: a YUV420 file under the writer's rule (4:4:4 frame, RGB frame)
                q = lambda v: np.clip(np.rint(v * mx), 0, mx).astype(np.uint16)  # noqa: E731 (video_writer.py:75)
                yuv_same = np.concatenate((q(y_w).reshape(-1), q(uv_w).reshape(-1)))
                y_x, uv_x = F.rgb_to_ycbcr420(fr)
                yuv_cross = np.concatenate((q(y_x).reshape(-1), q(uv_x).reshape(-1)))
                vals = {"rgb": rgb, "rgb_to_y": y_c, "rgb_to_uv": uv_c, "rgb_to_yuv444": yuv444_c, "yuv444": yuv444,
                        "yuv_to_rgb": rgb_c, "w_rgb": out[0], "w_rgb_from_444": out[1], "w_yuv": yuv_same,
                        "w_yuv_from_rgb": yuv_cross}
                for k in ("rgb", "rgb_to_y", "rgb_to_uv", "rgb_to_yuv444", "yuv444", "yuv_to_rgb"):
                    assert vals[k].dtype == np.float32, (k, vals[k].dtype)
                row = {"seed": seed, "h": h, "w": w, "depth": d}
                row.update({k: digest(v) for k, v in vals.items()})
                rows.append(row)
                if (h, w) in STORED:
                    for k, v in vals.items():
                        arrays[f"{k}_{h}x{w}_{d}"] = v
    with open(OUT_JSON, "w") as f:
        json.dump({"source": "DCVC-DC/src/utils/video_reader.py RGBReader(bit_depth), video_writer.py "
                             "RGBWriter(bit_depth) on real files, and src/transforms/functional.py on their values; "
                             "sha256 of the float32 / uint16 bytes",
                   "cases": rows}, f, indent=1)
    np.savez_compressed(OUT_NPZ, **arrays)
    print(json.dumps(rows[:2], indent=1), len(rows), os.path.getsize(OUT_NPZ))


if __name__ == "__main__":
    main()
