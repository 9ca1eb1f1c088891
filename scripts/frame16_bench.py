#!/usr/bin/env python3
"""Timing of the high-bit-depth frame kernels (frame16.hip) against their
8-bit twins on one GPU.

At 1080 x 1920 padded to 1088 x 1920 (a 3-channel fp32 NHWC frame), each
same-format 16-bit kernel and its uint8 twin in one process, interleaved:
per repeat, device events around ``--iters`` back-to-back launches of the
16-bit kernel, then of the twin, after a warm-up of both.  Reports the median
and the range of the per-call time over the repeats, and the bytes a call has
to move (source samples read, fp32 frame read and / or written, samples
written), computed from the shapes.

Writes one JSON object to ``--out`` and prints it.

    python scripts/frame16_bench.py [--out profiles/frame16_bench.json --iters 50 --repeats 3]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "frame16_bench needs a GPU"
    from dcvc_amd import hip as K
    from dcvc_amd.stream_helper import get_padding_size

    dev = torch.device("cuda", 0)
    h, w, d = a.height, a.width, a.depth
    _, pr, _, pb = get_padding_size(h, w, 16)
    H, W = h + pb, w + pr
    g = torch.Generator().manual_seed(1)
    n_rgb, n_y, n_uv = 3 * h * w, h * w, 2 * (h // 2) * (w // 2)

    def u8(n):
        return torch.randint(0, 256, (n,), generator=g).to(torch.uint8).to(dev)

    def u16(n):
        return torch.randint(0, 1 << d, (n,), generator=g).to(torch.int16).to(dev)

    rgb8, y8, uv8, rgb16, y16, uv16 = u8(n_rgb), u8(n_y), u8(n_uv), u16(n_rgb), u16(n_y), u16(n_uv)
    x = K.Act((torch.rand(H, W, 3, generator=g) * 1.2 - 0.1).to(dev))
    out = K.empty(H, W, 3, K.F32, dev)
    ws = K.frame_sse_workspace(dev)
    sse = torch.zeros(3, dtype=torch.float64, device=dev)
    o8 = torch.empty(n_rgb, dtype=torch.uint8, device=dev)
    o16 = torch.empty(n_rgb, dtype=torch.int16, device=dev)
    n_yuv = n_y + n_uv
    frame = H * W * 3 * 4                     # the padded fp32 frame, bytes
    crop = h * w * 3 * 4                      # its crop (strided rows of the same frame)

    # name: (16-bit call, 8-bit twin, bytes moved by the 16-bit call, by the twin)
    cases = {
        "rgb_to_nhwc": (lambda: K.frame16_to_nhwc(rgb16, h, w, d, out), lambda: K.frame_to_nhwc(rgb8, h, w, out),
                        2 * n_rgb + frame, n_rgb + frame),
        "rgb_to_nhwc_zero_pad": (lambda: K.frame16_to_nhwc(rgb16, h, w, d, out, zero_pad=True),
                                 lambda: K.frame_to_nhwc(rgb8, h, w, out, zero_pad=True),
                                 2 * n_rgb + frame, n_rgb + frame),
        "yuv420_to_nhwc": (lambda: K.yuv420p16_to_nhwc(y16, uv16, h, w, d, out),
                           lambda: K.yuv420_to_nhwc(y8, uv8, h, w, out), 2 * n_yuv + frame, n_yuv + frame),
        "sse_rgb": (lambda: K.frame16_sse(x, rgb16, h, w, d, ws, sse), lambda: K.frame_sse(x, rgb8, h, w, ws, sse),
                    2 * n_rgb + 2 * frame, n_rgb + 2 * frame),
        "sse_yuv420": (lambda: K.frame16_sse(x, y16, h, w, d, ws, sse, uv_u16=uv16),
                       lambda: K.frame_sse(x, y8, h, w, ws, sse, uv_u8=uv8), 2 * n_yuv + 2 * frame, n_yuv + 2 * frame),
        "recon_rgb": (lambda: K.recon_to_u16(x, h, w, d, False, o16), lambda: K.recon_to_u8(x, h, w, False, o8),
                      crop + 2 * n_rgb, crop + n_rgb),
        "recon_yuv420": (lambda: K.recon_to_u16(x, h, w, d, True, o16[:n_yuv]),
                         lambda: K.recon_to_u8(x, h, w, True, o8), crop + 2 * n_yuv, crop + n_yuv),
        "recon_cross_to_rgb": (lambda: K.recon_to_u16_cross(x, h, w, d, True, o16),
                               lambda: K.recon_to_u8_cross(x, h, w, True, o8), crop + 2 * n_rgb, crop + n_rgb),
        "recon_cross_to_yuv420": (lambda: K.recon_to_u16_cross(x, h, w, d, False, o16[:n_yuv]),
                                  lambda: K.recon_to_u8_cross(x, h, w, False, o8), crop + 2 * n_yuv, crop + n_yuv),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters        # microseconds per call

    rows = {}
    for name, (f16, f8, b16, b8) in cases.items():
        for _ in range(5):                                # warm-up: code objects, caches
            f16()
            f8()
        torch.cuda.synchronize()
        t16, t8 = [], []
        for _ in range(a.repeats):                        # interleaved, same process
            t16.append(timed(f16))
            t8.append(timed(f8))
        m16, m8 = statistics.median(t16), statistics.median(t8)
        rows[name] = {"us_16bit": summary(t16), "us_8bit": summary(t8), "ratio": round(m16 / m8, 3),
                      "bytes_16bit": b16, "bytes_8bit": b8, "GBps_16bit": round(b16 / (m16 * 1e-6) / 1e9, 1),
                      "GBps_8bit": round(b8 / (m8 * 1e-6) / 1e9, 1)}
    res = {"what": "frame16_bench", "device": torch.cuda.get_device_name(dev), "height": h, "width": w,
           "padded": [H, W], "depth": d, "iters": a.iters, "repeats": a.repeats,
           "note": "us per call: device events around `iters` back-to-back launches; the sse rows include the "
                   "one-block final reduction launch; bytes: algorithmic, from the shapes",
           "kernels": rows}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
