"""Scene-cut keyframes and keyframe seeking on the GPU: dcvc_scene_stats and
SceneCutDetector against the numpy restatement (tests/scenecut_ref.py) by
exact integer equality, encode_video with a threshold, the unchanged decoder
on the file it writes, and SequenceDecoder.frames / decode_video seeking into
it.  Codec comparisons are byte or torch.equal equality.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import scenecut_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT_TYPES = "I P P P I I P P P I P"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def kernel_constants():
    """(threads of a block, blocks of the capped grid) as scenecut.hip sets them."""
    text = open(os.path.join(ROOT, "dcvc_amd", "csrc", "hip", "scenecut.hip")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kBlock", "kMaxBlocks"))


def dev(a):
    """A sample array as the device tensor FrameStage.upload makes of it."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


class Runner:
    def __init__(self):
        from dcvc_amd import hip as K
        self.K = K
        self.ws = K.scene_stats_workspace(torch.device("cuda"))
        assert self.ws.numel() * 8 == int(K.lib().dcvc_scene_stats_workspace())

    def __call__(self, cur, prev, depth, fill=-1):
        out = torch.full((2,), fill, dtype=torch.int64, device="cuda")
        self.ws.fill_(fill)
        self.K.scene_stats(cur, prev, depth, self.ws, out)
        return tuple(out.cpu().tolist())


@pytest.fixture(scope="module")
def run():
    return Runner()


def rand(shape, depth, seed, lo=0):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(lo, 1 << depth, size=shape, dtype=np.uint8 if depth == 8 else np.uint16)


# ------------------------------------------------------------- the kernel
def check(run, cur, prev, depth):
    """cur / prev: device views; the result equals the restatement on what they hold."""
    got = run(cur, prev, depth)
    want = R.stats(host(cur), host(prev), depth)
    assert got == want, (got, want)
    return got


def test_less_than_one_wave(run):
    check(run, dev(rand((3, 5), 8, 1)), dev(rand((3, 5), 8, 2)), 8)
    check(run, dev(rand((3, 5), 12, 3)), dev(rand((3, 5), 12, 4)), 12)
    check(run, dev(rand((1,), 8, 5)), dev(rand((1,), 8, 6)), 8)


@pytest.mark.parametrize("depth,lo", [(8, 0), (10, 0), (16, 32768), (16, 0)])
def test_g_plane_of_a_37_by_53_frame(run, depth, lo):
    """The G plane of a 3 x 37 x 53 frame starts 1961 samples into its
    allocation: at an odd byte address at depth 8, 2 bytes past a 16-byte
    boundary above.  Depth 16 with every sample above 32767 catches a signed
    read."""
    a, b = dev(rand((3, 37, 53), depth, 10 + depth, lo)), dev(rand((3, 37, 53), depth, 40 + depth, lo))
    assert a[1].data_ptr() % 16 == (1961 * a.element_size()) % 16 and a[1].data_ptr() % 16 != 0
    sad, hdiff = check(run, a[1], b[1], depth)
    assert sad > 0 and hdiff > 0
    if lo:
        assert int(host(a[1]).min()) > 32767


@pytest.mark.parametrize("depth", [8, 10])
def test_planes_that_are_not_equally_aligned(run, depth):
    """cur and prev at different distances from a 16-byte boundary: the kernel
    reads single samples throughout.  Every pair of offsets 0..3 samples."""
    n = 37 * 53
    a, b = dev(rand((n + 8,), depth, 70 + depth)), dev(rand((n + 8,), depth, 80 + depth))
    for oa in range(4):
        for ob in range(4):
            check(run, a[oa:oa + n], b[ob:ob + n], depth)


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_all_samples_equal(run, depth):
    """Every histogram increment of a plane lands in one bin."""
    mx = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    a, b = dev(np.full((37, 53), mx, dtype=dt)), dev(np.full((37, 53), mx // 3, dtype=dt))
    assert check(run, a, a, depth) == (0, 0)
    assert check(run, a, b, depth) == (37 * 53 * (mx - mx // 3), 2 * 37 * 53)


def test_more_than_one_pass_of_the_capped_grid_at_16_bits(run):
    """cur all 0 against prev all 65535 on a plane longer than one pass of the
    capped grid (kMaxBlocks blocks of kBlock threads, 8 samples each), from an
    address that needs a head and a tail: sad = n * 65535 > 2^32 catches a
    32-bit partial anywhere."""
    block, blocks = kernel_constants()
    n = blocks * block * 8 + 8 * 1000 + 3
    a = torch.zeros(n + 1, dtype=torch.int16, device="cuda")[1:]
    b = torch.full((n + 1,), -1, dtype=torch.int16, device="cuda")[1:]
    got = run(a, b, 16)
    assert got == (n * 65535, 2 * n) and got[0] > 1 << 32


def test_more_than_one_pass_of_the_capped_grid_at_8_bits(run):
    block, blocks = kernel_constants()
    n = blocks * block * 16 + 16 * 777 + 5
    a, b = dev(rand((n + 3,), 8, 90)), dev(rand((n + 3,), 8, 91))
    check(run, a[3:], b[3:], 8)


def test_two_calls_give_one_result_whatever_the_outputs_held(run):
    a, b = dev(rand((3, 37, 53), 10, 20)), dev(rand((3, 37, 53), 10, 21))
    first = run(a[1], b[1], 10, fill=-1)
    assert first == run(a[1], b[1], 10, fill=0x5A5A5A5A5A5A5A5A) == run(a[1], b[1], 10, fill=0)
    assert first == R.stats(host(a[1]), host(b[1]), 10)


def test_the_entry_point_rejects_bad_arguments(run):
    K = run.K
    fn = K.lib().dcvc_scene_stats
    a, b = dev(rand((64,), 8, 30)), dev(rand((64,), 8, 31))
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    ok = [a.data_ptr(), b.data_ptr(), 64, 8, run.ws.data_ptr(), out.data_ptr(), K.stream()]
    assert fn(*ok) == 0
    for pos, bad in ((0, None), (1, None), (4, None), (5, None), (2, 0), (2, -5), (2, 1 << 31), (3, 7), (3, 17)):
        args = list(ok)
        args[pos] = bad
        assert fn(*args) == -1, (pos, bad)
    torch.cuda.synchronize()
    assert tuple(out.cpu().tolist()) == R.stats(host(a), host(b), 8)


# ----------------------------------------------------------- the detector
def test_detector_on_the_8_bit_rgb_sequence():
    from dcvc_amd.harness import FrameStage
    from dcvc_amd.scenecut import SceneCutDetector
    device = torch.device("cuda", torch.cuda.current_device())
    frames = R.cut_sequence(darken=True)
    stage = FrameStage(R.H, R.W, 16, False, zero_pad=False, frame_num=len(frames), device=device)
    det = SceneCutDetector(R.H, R.W, "rgb", 8, device)
    got = [det.score(stage.upload(f)) for f in frames]
    assert got[0] is None
    assert got == R.scores([f[1] for f in frames], 8)
    assert [t for t, s in enumerate(got) if s is not None and s["hd"] >= 0.5] == [R.CUT]


def test_detector_on_a_10_bit_yuv420_sequence():
    from dcvc_amd.harness import FrameStage
    from dcvc_amd.scenecut import SceneCutDetector
    device = torch.device("cuda", torch.cuda.current_device())
    frames = R.yuv420_sequence_10bit()
    stage = FrameStage(R.H, R.W, 16, True, zero_pad=False, frame_num=len(frames), device=device, bit_depth=10)
    det = SceneCutDetector(R.H, R.W, "420", 10, device)
    got = [det.score(stage.upload(f)) for f in frames]
    assert got[0] is None and got == R.scores([y for y, _ in frames], 10)
    assert all(s["max_val"] == 1023 and s["n"] == R.H * R.W for s in got[1:])


# ------------------------------------------------------------- DC, golden
Q = 40


def _nets(g):
    from tests.test_gpu_sequence import dc_nets
    return dc_nets(g)


def _args(frames, seq, **more):
    from dcvc_amd.harness import ArrayReader
    return dict({"frame_num": len(frames), "gop_size": 4, "src_height": R.H, "src_width": R.W, "q_in_ckpt": False,
                 "i_frame_q_index": Q, "src_reader": ArrayReader(frames), "seq_path": seq, "verbose": 1}, **more)


def _types(path):
    from dcvc_amd.sequence import SequenceReader
    with SequenceReader(path) as r:
        return " ".join(e.type for e in r.index())


@pytest.fixture(scope="module")
def coded(dc_golden, tmp_path_factory):
    """The darkened-cut sequence coded once with scene_cut=0.5 at gop_size 4:
    the file, the log, the encoder's reconstructions, and the full decode of it
    by separately built nets through the unchanged __iter__."""
    from dcvc_amd import harness, sequence
    td = tmp_path_factory.mktemp("scenecut")
    enc_nets, dec_nets = _nets(dc_golden), _nets(dc_golden)
    frames = R.cut_sequence(darken=True)
    seq = str(td / "cut.seq")
    recons, inner = [], sequence.SequenceEncoder.encode

    def spy(self, x, keyframe=False):
        out = inner(self, x, keyframe=keyframe)
        recons.append(out["recon"].clone())
        return out
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(sequence.SequenceEncoder, "encode", spy)
        log = harness.encode_video(*enc_nets, _args(frames, seq, scene_cut=0.5))
    with sequence.SequenceDecoder(*dec_nets, seq) as dec:
        full = [dict(type=o["type"], x_hat=o["x_hat"].clone(), bit=o["bit"]) for o in dec]   # every digest verifies
    return {"td": td, "seq": seq, "log": log, "recons": recons, "full": full, "frames": frames,
            "enc_nets": enc_nets, "dec_nets": dec_nets}


def test_scene_cut_places_a_keyframe(coded):
    log = coded["log"]
    assert _types(coded["seq"]) == WANT_TYPES
    assert log["scene_cuts"] == [R.CUT]
    assert log["frame_type"] == [0 if t == "I" else 1 for t in WANT_TYPES.split()]
    want = R.scores([f[1] for f in coded["frames"]], 8)
    assert log["scene_scores"] == [None] + [[s["hd"], s["mad"]] for s in want[1:]]
    json.dumps(log)


def test_the_unchanged_decoder_reproduces_the_encoder(coded):
    full, recons = coded["full"], coded["recons"]
    assert len(full) == len(recons) == R.FRAMES
    assert " ".join(o["type"] for o in full) == WANT_TYPES
    for t, (o, r) in enumerate(zip(full, recons)):
        assert torch.equal(o["x_hat"], r), t
    assert [o["bit"] for o in full] == coded["log"]["frame_bits"]


def test_without_a_threshold_the_file_is_the_plain_encoders(coded):
    from dcvc_amd import harness
    from dcvc_amd.sequence import SequenceEncoder
    td, frames, (inet, pnet) = coded["td"], coded["frames"], coded["enc_nets"]
    plain, video = str(td / "plain.seq"), str(td / "video.seq")
    log = harness.encode_video(inet, pnet, _args(frames, video))
    assert "scene_cuts" not in log and "scene_scores" not in log
    stage = harness.FrameStage(R.H, R.W, 16, False, zero_pad=False, frame_num=len(frames), device=inet.dev)
    with SequenceEncoder(inet, pnet, plain, R.W, R.H, 4, q_in_ckpt=False, q_index=Q) as enc:
        for f in frames:
            enc.encode(stage.load(stage.upload(f)))
    data = open(video, "rb").read()
    assert data == open(plain, "rb").read()
    assert _types(video) == "I P P P I P P P I P P"
    assert data != open(coded["seq"], "rb").read()


def test_frames_seeks_to_the_keyframe(coded):
    from dcvc_amd.sequence import SequenceDecoder
    full = coded["full"]
    with SequenceDecoder(*coded["dec_nets"], coded["seq"]) as dec:
        assert dec.frames == R.FRAMES
        got = list(dec.frames(start=7, count=2))
        assert [o["frame_idx"] for o in got] == [7, 8] and (dec.last_keyframe, dec.frames_decoded) == (5, 4)
        for o in got:
            assert set(o) == {"type", "x_hat", "dpb", "bit", "frame_idx"}
            assert torch.equal(o["x_hat"], full[o["frame_idx"]]["x_hat"]) and o["bit"] == full[o["frame_idx"]]["bit"]
        # a keyframe as the start: only what is emitted is decoded
        got = [(o["frame_idx"], o["type"]) for o in dec.frames(start=5, count=3)]
        assert got == [(5, "I"), (6, "P"), (7, "P")] and (dec.last_keyframe, dec.frames_decoded) == (5, 3)
        # a count past the end is clipped; none: to the end
        got = list(dec.frames(start=9, count=100))
        assert [o["frame_idx"] for o in got] == [9, 10] and (dec.last_keyframe, dec.frames_decoded) == (9, 2)
        assert torch.equal(got[1]["x_hat"], full[10]["x_hat"])
        assert [o["frame_idx"] for o in dec.frames(start=10)] == [10] and dec.frames_decoded == 2
        with pytest.raises(ValueError):
            dec.frames(start=R.FRAMES)
        # from frame 0 it is the whole decode
        got = list(dec.frames())
        assert len(got) == R.FRAMES and (dec.last_keyframe, dec.frames_decoded) == (0, R.FRAMES)
        assert all(torch.equal(o["x_hat"], f["x_hat"]) for o, f in zip(got, full))


def test_a_seek_never_reads_an_earlier_gop(coded):
    """One byte of frame 1's payload flipped on the host (the lowest bit of the
    q_index in its first byte, 40 -> 41: the decoder dequantises with other
    scales, so its frame differs): frames(start=6) still succeeds, __iter__
    fails at frame 1."""
    from dcvc_amd.sequence import DigestMismatch, SequenceDecoder, SequenceReader
    bad = str(coded["td"] / "bad.seq")
    shutil.copy(coded["seq"], bad)
    with SequenceReader(bad) as r:
        entry = r.index()[1]
    assert entry.type == "P"
    with open(bad, "r+b") as f:
        f.seek(entry.offset)
        b = f.read(1)[0]
        assert (b & 0x7F) >> 1 == Q          # stream_helper.pack_p: flag byte, frame_idx, length, stream
        f.seek(entry.offset)
        f.write(bytes([b ^ 2]))
    full = coded["full"]
    with SequenceDecoder(*coded["dec_nets"], bad) as dec:
        got = list(dec.frames(start=6))
        assert [o["frame_idx"] for o in got] == [6, 7, 8, 9, 10] and dec.last_keyframe == 5
        for o in got:
            assert torch.equal(o["x_hat"], full[o["frame_idx"]]["x_hat"])
    with SequenceDecoder(*coded["dec_nets"], bad) as dec:
        seen = []
        with pytest.raises((DigestMismatch, ValueError, RuntimeError)) as err:    # the coder may refuse the payload
            for _ in dec:
                seen.append(1)
        assert len(seen) == 1 and getattr(err.value, "frame_idx", 1) == 1


def test_decode_video_writes_the_frames_it_was_asked_for(coded):
    from dcvc_amd import harness
    td = coded["td"]
    base = {"seq_path": coded["seq"], "save_decoded_frame": True, "src_type": "rgb"}
    whole = harness.decode_video(*coded["dec_nets"], dict(base, recon_path=str(td / "whole")))
    part = harness.decode_video(*coded["dec_nets"], dict(base, recon_path=str(td / "part"), start_frame=7,
                                                         frame_num=2))
    fs = 3 * R.H * R.W
    a, b = (td / "whole" / "out.rgb").read_bytes(), (td / "part" / "out.rgb").read_bytes()
    assert len(a) == R.FRAMES * fs and len(b) == 2 * fs and b == a[7 * fs:9 * fs]
    gops = [[0, 4], [4, 5], [5, 9], [9, 11]]
    assert (part["start_frame"], part["keyframe"], part["frames_decoded"], part["frame_num"]) == (7, 5, 4, 2)
    assert part["gops"] == gops and part["frame_bits"] == whole["frame_bits"][7:9] and part["frame_type"] == [1, 1]
    assert (whole["start_frame"], whole["keyframe"], whole["frames_decoded"], whole["frame_num"]) == \
        (0, 0, R.FRAMES, R.FRAMES)
    assert whole["gops"] == gops and whole["frame_bits"] == coded["log"]["frame_bits"]
    json.dumps(part)
    # PNG output: numbered from the first emitted frame, as a fresh writer numbers them
    harness.decode_video(*coded["dec_nets"], {"seq_path": coded["seq"], "save_decoded_frame": True,
                                              "recon_path": str(td / "png"), "start_frame": 7, "frame_num": 2})
    assert sorted(os.listdir(td / "png")) == ["im00001.png", "im00002.png"]


def test_the_mad_threshold_cuts_the_plain_sequence(coded):
    from dcvc_amd import harness
    frames = R.cut_sequence(darken=False)
    seq = str(coded["td"] / "mad.seq")
    log = harness.encode_video(*coded["enc_nets"], _args(frames, seq, scene_cut_mad=0.15))
    assert log["scene_cuts"] == [R.CUT] and _types(seq) == WANT_TYPES
    # the histogram distance alone does not see this cut
    seq2 = str(coded["td"] / "hd.seq")
    log = harness.encode_video(*coded["enc_nets"], _args(frames, seq2, scene_cut=0.5, frame_num=7))
    assert log["scene_cuts"] == [] and _types(seq2) == "I P P P I P P"
    # and an interval of 2 keeps the cut one frame after the keyframe at 4 a P frame
    seq3 = str(coded["td"] / "interval.seq")
    log = harness.encode_video(*coded["enc_nets"], _args(frames, seq3, scene_cut_mad=0.15, min_keyframe_interval=2,
                                                         frame_num=7))
    assert log["scene_cuts"] == [] and _types(seq3) == "I P P P I P P"


# ------------------------------------------------------------ HEM, golden
def test_hem_keyframe_on_request(tmp_path):
    from dcvc_amd.sequence import SequenceDecoder, SequenceEncoder
    from tests.hem_fixtures import HEMGolden
    from tests.test_gpu_sequence import hem_nets, q_args
    g = HEMGolden()
    meta = g.meta["A"]
    xs = [g.frame_tensor("A", t)[1].cuda() for t in (0, 1, 2, 1)]
    path = str(tmp_path / "hem.seq")
    recons = []
    with SequenceEncoder(*hem_nets(g), path, meta["w"], meta["h"], 32, **q_args("hem", g.q("A"))) as enc:
        for t, x in enumerate(xs):
            out = enc.encode(x, keyframe=t == 2)
            recons.append((out["type"], out["recon"].clone()))
    assert _types(path) == "I P I P" == " ".join(t for t, _ in recons)
    with SequenceDecoder(*hem_nets(g), path) as dec:
        full = [o["x_hat"].clone() for o in dec]
        for x, (_, r) in zip(full, recons):
            assert torch.equal(x, r)
        got = list(dec.frames(start=3))
        assert [o["frame_idx"] for o in got] == [3] and (dec.last_keyframe, dec.frames_decoded) == (2, 2)
        assert torch.equal(got[0]["x_hat"], full[3])


# ----------------------------------------------------------- command line
def test_command_line_round_trip(dc_golden, tmp_path):
    """python -m dcvc_amd.sequence encode --scene_cut 0.5, then decode
    --start_frame 6 --frame_num 2, each in a fresh process."""
    frames = R.cut_sequence(darken=True)
    (tmp_path / "src.rgb").write_bytes(b"".join(f.tobytes() for f in frames))
    torch.save(dc_golden.i_state_dict(), tmp_path / "i.pth")
    torch.save(dc_golden.p_state_dict(), tmp_path / "p.pth")
    common = [sys.executable, "-m", "dcvc_amd.sequence", "MODE", "--i_frame_model_path", str(tmp_path / "i.pth"),
              "--p_frame_model_path", str(tmp_path / "p.pth"), "--seq_path", str(tmp_path / "a.seq"),
              "--src_type", "rgb"]

    def cli(mode, *more):
        cmd = [mode if c == "MODE" else c for c in common] + list(more)
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    elog = cli("encode", "--src_path", str(tmp_path / "src.rgb"), "--src_width", str(R.W), "--src_height", str(R.H),
               "--frame_num", str(R.FRAMES), "--gop_size", "4", "--q_index", str(Q), "--scene_cut", "0.5")
    assert elog["scene_cuts"] == [R.CUT] and elog["scene_scores"][0] is None and len(elog["scene_scores"]) == R.FRAMES
    assert _types(str(tmp_path / "a.seq")) == WANT_TYPES
    dlog = cli("decode", "--recon_path", str(tmp_path / "rec"), "--start_frame", "6", "--frame_num", "2")
    assert (dlog["start_frame"], dlog["keyframe"], dlog["frames_decoded"], dlog["frame_num"]) == (6, 5, 3, 2)
    assert dlog["frame_bits"] == elog["frame_bits"][6:8] and dlog["gops"] == [[0, 4], [4, 5], [5, 9], [9, 11]]
    assert os.path.getsize(tmp_path / "rec" / "out.rgb") == 2 * 3 * R.H * R.W
