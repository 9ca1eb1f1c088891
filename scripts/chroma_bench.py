#!/usr/bin/env python3
"""Timing of the chroma-layout frame kernels (chroma.hip) against their 4:2:0
twins on one GPU.

At 1080 x 1920 padded to 1088 x 1920 (a 3-channel fp32 NHWC frame), at 8 and
10 bits: each new kernel at 4:4:4, 4:2:2 and (test-only) 4:2:0, in one process
and interleaved with the 4:2:0 kernel the harness uses at that depth: per
repeat, device events around ``--iters`` back-to-back launches of the new
kernel, then of the twin, after a warm-up of both.  Reports the median and the
range of the per-call time over the repeats, the bytes a call has to move
(source samples read, fp32 frame read and / or written, samples written),
computed from the shapes, and the yardstick: the twin's time scaled by the
ratio of bytes moved.

Writes one JSON object to ``--out`` and prints it.

    python scripts/chroma_bench.py [--out profiles/chroma_bench.json --iters 50 --repeats 3]
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
    ap.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "chroma_bench needs a GPU"
    from dcvc_amd import hip as K
    from dcvc_amd.stream_helper import get_padding_size

    dev = torch.device("cuda", 0)
    h, w = a.height, a.width
    _, pr, _, pb = get_padding_size(h, w, 16)
    H, W = h + pb, w + pr
    g = torch.Generator().manual_seed(1)
    x = K.Act((torch.rand(H, W, 3, generator=g) * 1.2 - 0.1).to(dev))
    out = K.empty(H, W, 3, K.F32, dev)
    planes = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    ws = K.frame_sse_workspace(dev)
    sse = torch.zeros(3, dtype=torch.float64, device=dev)
    n_y = h * w
    frame = H * W * 3 * 4                     # the padded fp32 frame, bytes
    crop = h * w * 3 * 4                      # its crop / the planar fp32 RGB source

    def samples(n, d):
        t = torch.randint(0, 1 << d, (n,), generator=g)
        return (t.to(torch.uint8) if d == 8 else t.to(torch.int16)).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters        # microseconds per call

    rows = {}
    for d in a.depths:
        B = 1 if d == 8 else 2
        dt = torch.uint8 if d == 8 else torch.int16
        n420 = 2 * (h // 2) * (w // 2)
        y, uv420 = samples(n_y, d), samples(n420, d)
        o = torch.empty(3 * n_y, dtype=dt, device=dev)
        yf, uvf = torch.empty(n_y, device=dev), torch.empty(n420, device=dev)

        def rgb16_twin():
            K.u16_to_f32(y, d, yf)
            K.u16_to_f32(uv420, d, uvf)
            K.yuv420f_to_rgb_nhwc(yf, uvf, h, w, out, planes)

        s420 = B * (n_y + n420)
        # kernel: (the 4:2:0 twin at this depth, bytes it moves)
        twins = {
            "to_nhwc": ((lambda: K.yuv420_to_nhwc(y, uv420, h, w, out)) if d == 8 else
                        (lambda: K.yuv420p16_to_nhwc(y, uv420, h, w, d, out)), s420 + frame),
            "to_rgb_nhwc": ((lambda: K.yuv420_to_rgb_nhwc(y, uv420, h, w, out, planes)) if d == 8 else rgb16_twin,
                            s420 + frame + crop + (0 if d == 8 else 10 * (n_y + n420) - s420)),
            "sse": ((lambda: K.frame_sse(x, y, h, w, ws, sse, uv_u8=uv420)) if d == 8 else
                    (lambda: K.frame16_sse(x, y, h, w, d, ws, sse, uv_u16=uv420)), s420 + 2 * frame),
            "recon_from_yuv": ((lambda: K.recon_to_u8(x, h, w, True, o)) if d == 8 else
                               (lambda: K.recon_to_u16(x, h, w, d, True, o[:n_y + n420])), crop + s420),
            "recon_from_rgb": ((lambda: K.recon_to_u8_cross(x, h, w, False, o)) if d == 8 else
                               (lambda: K.recon_to_u16_cross(x, h, w, d, False, o[:n_y + n420])), crop + s420),
        }
        for chroma in ("444", "422", "420"):
            sx, sy = K.chroma_sub(chroma)
            n_uv = 2 * (h // sy) * (w // sx)
            uv = samples(n_uv, d)
            s = B * (n_y + n_uv)
            ob = o[:n_y + n_uv]
            new = {
                "to_nhwc": (lambda: K.yuvp_to_nhwc(y, uv, h, w, d, chroma, out), s + frame),
                "to_rgb_nhwc": (lambda: K.yuvp_to_rgb_nhwc(y, uv, h, w, d, chroma, out, planes), s + frame + crop),
                "sse": (lambda: K.yuvp_sse(x, y, uv, h, w, d, chroma, ws, sse), s + 2 * frame),
                "recon_from_yuv": (lambda: K.recon_to_yuvp(x, h, w, d, chroma, False, ob), crop + s),
                "recon_from_rgb": (lambda: K.recon_to_yuvp(x, h, w, d, chroma, True, ob), crop + s),
            }
            for name, (fn, b_new) in new.items():
                ft, b_twin = twins[name]
                for _ in range(5):                        # warm-up: code objects, caches
                    fn()
                    ft()
                torch.cuda.synchronize()
                t_new, t_twin = [], []
                for _ in range(a.repeats):                # interleaved, same process
                    t_new.append(timed(fn))
                    t_twin.append(timed(ft))
                m_new, m_twin = statistics.median(t_new), statistics.median(t_twin)
                yard = m_twin * b_new / b_twin
                rows[f"{name}_{chroma}_{d}bit"] = {
                    "us": summary(t_new), "us_twin_420": summary(t_twin), "ratio_to_twin": round(m_new / m_twin, 3),
                    "bytes": b_new, "bytes_twin_420": b_twin, "yardstick_us": round(yard, 3),
                    "over_yardstick_us": round(m_new - yard, 3), "twin_range_us": round(max(t_twin) - min(t_twin), 3),
                    "GBps": round(b_new / (m_new * 1e-6) / 1e9, 1), "GBps_twin_420": round(b_twin / (m_twin * 1e-6) / 1e9, 1)}
    res = {"what": "chroma_bench", "device": torch.cuda.get_device_name(dev), "height": h, "width": w,
           "padded": [H, W], "depths": a.depths, "iters": a.iters, "repeats": a.repeats,
           "note": "us per call: device events around `iters` back-to-back launches; the sse rows include the "
                   "one-block final reduction launch; the 10-bit to_rgb_nhwc twin is dcvc_u16_to_f32 twice plus "
                   "dcvc_yuv420f_to_rgb_nhwc (three launches, the fp32 planes written and read back); bytes: "
                   "algorithmic, from the shapes; yardstick_us: the twin's median scaled by bytes / bytes_twin_420",
           "kernels": rows}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
