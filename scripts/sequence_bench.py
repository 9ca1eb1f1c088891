#!/usr/bin/env python3
"""Timing of the stand-alone encoder and decoder against encode_decode, and
of the digest kernel against a copy of the same tensor, on one GPU.

DCVC-DC, RGB, split precision, intra period 32, synthetic weights and the
moving-pattern source (bench.py's), real bitstreams: a sequence file for the
stand-alone pair, N.bin files for encode_decode.  In one process, alternating
the three paths over the same GOP (``--repeats`` times each, after a warm-up
GOP prefix per path):

  encode_only    SequenceEncoder.encode per P frame (encoder + its own
                 reconstruction + DPB digest + record write)
  decode_only    SequenceDecoder per P frame (decoder + DPB digest + compare)
  encode_decode  the existing per-frame encode_decode through a file

and hip.digest / hip.copy of a 1088 x 1920 x 48 fp32 tensor (device events
around ``--kernel-iters`` back-to-back launches, after a warm-up).

Prints one JSON line.  Host threads: at most 16 (the rANS coder's pool).

    python scripts/sequence_bench.py [--height 1080 --width 1920 --gop 32 --repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def time_kernels(a, K, torch, dev, sync):
    """hip.digest against hip.copy of the same 1088 x 1920 x 48 fp32 tensor."""
    Hk, Wk, Ck = 1088, 1920, 48
    src = K.Act(torch.randn(Hk, Wk, Ck, device=dev))
    dst = K.empty(Hk, Wk, Ck, K.F32, dev)
    out = torch.zeros(2, dtype=torch.int64, device=dev)

    def timed(fn):
        for _ in range(5):
            fn()
        sync()
        runs = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.kernel_iters):
                fn()
            e1.record()
            e1.synchronize()
            runs.append(1e3 * e0.elapsed_time(e1) / a.kernel_iters)   # microseconds per call
        return runs

    dig = timed(lambda: K.digest(src, 1, out))
    cpy = timed(lambda: K.copy(src, dst))
    nbytes = Hk * Wk * Ck * 4
    return {"kernel_tensor": [Hk, Wk, Ck], "kernel_bytes": nbytes, "digest_us": summary(dig), "copy_us": summary(cpy),
            "digest_read_GBps": round(nbytes / (statistics.median(dig) * 1e-6) / 1e9, 1),
            "copy_read_plus_write_GBps": round(2 * nbytes / (statistics.median(cpy) * 1e-6) / 1e9, 1)}


def time_scene_cut(a, K, torch, dev, sync, nets):
    """What the scene-cut detector costs: whole-call encode_video time per
    frame over ``--scene-frames`` frames with scene_cut set to a value that
    never fires on this source (1.0: disjoint histograms) against the same call
    without it, alternating, ``--repeats`` pairs after one warm-up pair; and
    dcvc_scene_stats alone on one plane (device events)."""
    from dcvc_amd.harness import ArrayReader, encode_video
    from dcvc_amd.synth import moving_pattern
    h, w, n = a.height, a.width, a.scene_frames
    frames = [moving_pattern(h, w, t, seed=1) for t in range(n)]
    base = {"frame_num": n, "gop_size": a.gop, "src_height": h, "src_width": w, "q_in_ckpt": False,
            "i_frame_q_index": a.q_index}
    off, on, cuts = [], [], 0
    with tempfile.TemporaryDirectory() as td:
        def once(**more):
            sync()
            t0 = time.perf_counter()
            log = encode_video(*nets, dict(base, src_reader=ArrayReader(frames), seq_path=os.path.join(td, "s.seq"),
                                           **more))
            sync()
            return 1e3 * (time.perf_counter() - t0) / n, log
        once(frame_num=min(n, a.warmup_frames))
        once(frame_num=min(n, a.warmup_frames), scene_cut=1.0)
        for _ in range(a.repeats):
            off.append(once()[0])
            ms, log = once(scene_cut=1.0)
            on.append(ms)
            cuts += len(log["scene_cuts"])
    cur, prev = (torch.from_numpy(f).to(dev)[1] for f in frames[:2])
    ws, out = K.scene_stats_workspace(dev), torch.empty(2, dtype=torch.int64, device=dev)
    for _ in range(5):
        K.scene_stats(cur, prev, 8, ws, out)
    sync()
    runs = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_iters):
            K.scene_stats(cur, prev, 8, ws, out)
        e1.record()
        e1.synchronize()
        runs.append(1e3 * e0.elapsed_time(e1) / a.kernel_iters)
    return {"scene_cut": {"frames": n, "ms_per_frame_off": [round(v, 3) for v in off],
                          "ms_per_frame_on": [round(v, 3) for v in on], "cuts_fired": cuts,
                          "scene_stats_us": summary(runs), "plane_samples": h * w}}


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--gop", type=int, default=32)
    ap.add_argument("--q_index", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup-frames", type=int, default=3)
    ap.add_argument("--stream_part", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--paths", default="encode_only,decode_only,encode_decode,kernels",
                    help="comma list of what to time (encode_decode alone also runs on a tree without the "
                         "stand-alone pair, for a comparison with an earlier commit; scene_cut: encode_video "
                         "with and without the scene-cut detector)")
    ap.add_argument("--scene-frames", type=int, default=64, help="frames per encode_video call of the scene_cut path")
    a = ap.parse_args()
    paths = set(a.paths.split(","))
    pair = bool(paths & {"encode_only", "decode_only"})

    import torch
    assert torch.cuda.is_available(), "sequence_bench needs a GPU"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from dcvc_amd import hip as K
    from dcvc_amd.dc import DMC, IntraNoAR
    from dcvc_amd.harness import FrameStage
    from dcvc_amd.layers import Precision
    if pair:
        from dcvc_amd.sequence import SequenceEncoder, SequenceDecoder
    from dcvc_amd.synth import moving_pattern
    from dcvc_amd.weights import synthetic_state_dict

    with open(os.path.join(HERE, "dcvc_amd", "data", "dc_param_spec.json")) as f:
        d = json.load(f)
    isd = synthetic_state_dict([(n, tuple(s)) for n, s in d["intra"]], seed=0)
    psd = synthetic_state_dict([(n, tuple(s)) for n, s in d["inter"]], seed=1)

    def nets():
        i = IntraNoAR(precision=Precision.split(), stream_part=a.stream_part).load_state_dict(isd)
        p = DMC(precision=Precision.split(), stream_part=a.stream_part).load_state_dict(psd)
        i.update(force=True)
        p.update(force=True)
        return i, p

    enc_nets, dec_nets = nets(), nets()
    dev = enc_nets[0].dev
    h, w, n = a.height, a.width, a.gop
    stage = FrameStage(h, w, 16, False, zero_pad=False, frame_num=n, device=dev)
    coded = bool(paths & {"encode_only", "decode_only", "encode_decode"})
    xs = [stage.load(stage.upload(moving_pattern(h, w, t, seed=1))).nchw_view().clone()
          for t in range(n if coded else 0)]
    sync = torch.cuda.current_stream(dev).synchronize

    def run_encode(path, frames):
        """-> (seconds over the P frames, P frames, fallbacks)"""
        t_p, fb = 0.0, 0
        with SequenceEncoder(*enc_nets, path, w, h, a.gop, q_in_ckpt=False, q_index=a.q_index) as enc:
            for t in range(frames):
                sync()
                t0 = time.perf_counter()
                out = enc.encode(xs[t])
                sync()
                if t:
                    t_p += time.perf_counter() - t0
                fb += out["precision_fallback"] is not None
        return t_p, frames - 1, fb

    def run_decode(path):
        t_p, k = 0.0, 0
        with SequenceDecoder(*dec_nets, path) as dec:
            it = iter(dec)
            while True:
                sync()
                t0 = time.perf_counter()
                try:
                    next(it)
                except StopIteration:
                    break
                sync()
                if k:
                    t_p += time.perf_counter() - t0
                k += 1
        return t_p, k - 1

    def run_encode_decode(folder, frames):
        inet, pnet = enc_nets
        t_p, dpb = 0.0, None
        for t in range(frames):
            path = os.path.join(folder, f"{t}.bin")
            sync()
            t0 = time.perf_counter()
            if t == 0:
                r = inet.encode_decode(xs[t], False, a.q_index, path, pic_height=h, pic_width=w)
                dpb = {"ref_frame": r["x_hat"], "ref_feature": None, "ref_mv_feature": None, "ref_y": None,
                       "ref_mv_y": None}
            else:
                dpb = pnet.encode_decode(xs[t], dpb, False, a.q_index, path, pic_height=h, pic_width=w,
                                         frame_idx=t % 4)["dpb"]
            sync()
            if t:
                t_p += time.perf_counter() - t0
        return t_p, frames - 1

    res = {k: [] for k in (("encode_only", "decode_only") if pair else ())}
    if "encode_decode" in paths:
        res["encode_decode"] = []
    fallbacks = 0
    with torch.no_grad(), tempfile.TemporaryDirectory() as td:
        seq = os.path.join(td, "bench.seq")
        # warm-up: every path over a GOP prefix (code objects, pinned buffers, allocator)
        if pair:
            run_encode(seq, a.warmup_frames)
            run_decode(seq)
        if "encode_decode" in paths:
            run_encode_decode(td, a.warmup_frames)
        for _ in range(a.repeats):   # alternating, same process
            if pair:
                t_p, k, fb = run_encode(seq, n)
                fallbacks += fb
                res["encode_only"].append(1e3 * t_p / k)
                t_p, k = run_decode(seq)
                res["decode_only"].append(1e3 * t_p / k)
            if "encode_decode" in paths:
                t_p, k = run_encode_decode(td, n)
                res["encode_decode"].append(1e3 * t_p / k)
        seq_bytes = os.path.getsize(seq) if pair else None

    kernels = {}
    if "kernels" in paths:
        kernels = time_kernels(a, K, torch, dev, sync)
    if "scene_cut" in paths:
        kernels.update(time_scene_cut(a, K, torch, dev, sync, enc_nets))

    print(json.dumps({
        "what": "sequence_bench", "device": torch.cuda.get_device_name(dev), "height": h, "width": w, "gop": a.gop,
        "q_index": a.q_index, "precision": "split", "repeats": a.repeats, "p_frames_per_repeat": n - 1,
        "ms_per_p_frame": {k: summary(v) for k, v in res.items()},
        "encoder_fallbacks": fallbacks, "sequence_file_bytes": seq_bytes, **kernels,
    }))


if __name__ == "__main__":
    main()
