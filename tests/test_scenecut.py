"""Scene-cut keyframes and keyframe seeking, the parts that need no GPU: the
keyframe schedule, ``lanes.keyframe_before``, the argument checks of
``encode_video`` / ``decode_video`` (which raise before any file or folder is
made), the ABI of the two new entry points, and the premise of the synthetic
sequences the GPU tests use (tests/scenecut_ref.py is the restatement).
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import scenecut_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dcvc_scene_stats_workspace", "dcvc_scene_stats")


def types_of(gop_size, n, cuts=(), interval=1):
    from dcvc_amd.scenecut import KeyframeSchedule
    s = KeyframeSchedule(gop_size, interval)
    return " ".join(s.next(cut=t in cuts) for t in range(n))


# ------------------------------------------------------------ the schedule
@pytest.mark.parametrize("gop_size", [1, 4, 7])
def test_schedule_without_cuts_is_the_fixed_gop(gop_size):
    want = " ".join("I" if t % gop_size == 0 else "P" for t in range(20))
    assert types_of(gop_size, 20) == want
    from dcvc_amd.scenecut import KeyframeSchedule
    s = KeyframeSchedule(gop_size)
    assert " ".join(s.next() for _ in range(20)) == want       # the default argument


def test_schedule_with_a_cut():
    assert types_of(4, 11, cuts={5}) == "I P P P I I P P P I P"
    # one frame has passed since the keyframe at 4: an interval of 2 suppresses the cut
    assert types_of(4, 11, cuts={5}, interval=2) == "I P P P I P P P I P P"
    assert types_of(4, 11, cuts={0}) == types_of(4, 11)
    assert types_of(4, 11, cuts={0}, interval=3) == types_of(4, 11)
    # a cut keyframe restarts the gop_size count
    assert types_of(4, 11, cuts={2}) == "I P I P P P I P P P I"
    # peek does not advance
    from dcvc_amd.scenecut import KeyframeSchedule
    s = KeyframeSchedule(4)
    assert [s.peek(), s.peek(True), s.next()] == ["I", "I", "I"]
    assert [s.peek(), s.peek(True), s.next(), s.peek(True)] == ["P", "I", "P", "I"]


def test_schedule_rejects_bad_arguments():
    from dcvc_amd.scenecut import KeyframeSchedule
    for gop, interval in ((0, 1), (4, 0), (4, -1), (4, 1.5), ("4", 1), (True, 1)):
        with pytest.raises(ValueError):
            KeyframeSchedule(gop, interval)


# ------------------------------------------------------------------ seeking
def _write(path, types, codec="DC"):
    from dcvc_amd.sequence import SequenceWriter
    with SequenceWriter(str(path), codec, "rgb", "split", 130, 100) as w:
        for t, ft in enumerate(types):
            w.write(ft, bytes([t]) * (3 + t), digest=(t, t))
    return str(path)


def test_keyframe_before(tmp_path):
    from dcvc_amd.lanes import gops_of, keyframe_before
    from dcvc_amd.sequence import SequenceFormatError, SequenceReader
    with SequenceReader(_write(tmp_path / "a.seq", "IPPIPI")) as r:
        index = r.index()
    assert [keyframe_before(index, t).frame_idx for t in range(6)] == [0, 0, 0, 3, 3, 5]
    assert all(keyframe_before(index, t) is index[k] for t, k in enumerate([0, 0, 0, 3, 3, 5]))
    assert gops_of(index) == [(0, 3), (3, 5), (5, 6)]
    for bad in (-1, 6, 100, 1.0, None, "2"):
        with pytest.raises(ValueError):
            keyframe_before(index, bad)
    with pytest.raises(ValueError):
        keyframe_before([], 0)
    with SequenceReader(_write(tmp_path / "p.seq", "PPI")) as r:
        index = r.index()
    for t in range(3):
        with pytest.raises(SequenceFormatError, match="frame 0 is a P frame"):
            keyframe_before(index, t)
    with pytest.raises(ValueError):                      # the range comes first
        keyframe_before(index, 3)


class Net:
    """What the drivers read of a net before they touch a device."""
    dev = torch.device("cpu")
    prec = types.SimpleNamespace(name="split")


def test_encode_video_checks_its_keys_before_the_file_exists(tmp_path):
    from dcvc_amd import harness
    seq = tmp_path / "a.seq"
    base = {"frame_num": 2, "gop_size": 4, "src_path": str(tmp_path / "nowhere"), "src_width": 130, "src_height": 100,
            "q_in_ckpt": False, "i_frame_q_index": 0, "seq_path": str(seq)}
    for key in ("scene_cut", "scene_cut_mad"):
        for bad in (0, 1.5, "0.5", -0.25, True, float("nan")):
            with pytest.raises(ValueError, match=key):
                harness.encode_video(Net(), Net(), dict(base, **{key: bad}))
    for bad in (0, -3, 1.5, "2"):
        with pytest.raises(ValueError, match="min_keyframe_interval"):
            harness.encode_video(Net(), Net(), dict(base, scene_cut=0.5, min_keyframe_interval=bad))
        with pytest.raises(ValueError, match="min_keyframe_interval"):     # also with the detector off
            harness.encode_video(Net(), Net(), dict(base, min_keyframe_interval=bad))
    assert not seq.exists() and os.listdir(tmp_path) == []


def test_decode_video_checks_its_range_before_any_folder_exists(tmp_path):
    from dcvc_amd import harness
    seq = _write(tmp_path / "a.seq", "IPPIPI")
    rec = tmp_path / "rec"
    base = {"seq_path": seq, "save_decoded_frame": True, "recon_path": str(rec), "decoded_frame_folder": str(rec)}
    for start in (-1, 6, 7, 1.5, "3"):
        with pytest.raises(ValueError):
            harness.decode_video(Net(), Net(), dict(base, start_frame=start))
    for num in (0, -2, 1.5, "3"):
        with pytest.raises(ValueError, match="count"):
            harness.decode_video(Net(), Net(), dict(base, start_frame=2, frame_num=num))
    assert not rec.exists()


def test_decoder_frames_is_still_the_frame_count(tmp_path):
    """``SequenceDecoder.frames`` has been the file's frame count since the
    class exists; it stays one and can also be called."""
    from dcvc_amd.sequence import SequenceDecoder
    with SequenceDecoder(Net(), Net(), _write(tmp_path / "a.seq", "IPPIPI")) as dec:
        assert dec.frames == 6 and isinstance(dec.frames, int) and callable(dec.frames)
        assert (dec.last_keyframe, dec.frames_decoded) == (None, None)
        key, stop = dec.seek(4, 5)
        assert (key.frame_idx, key.type, stop) == (3, "I", 6)
        assert dec.seek(2)[1] == 6 and dec.seek(2, 1) == (dec.reader.index()[0], 3)
        with pytest.raises(ValueError):
            dec.frames(start=6)                       # at the call, not at the first next()


# ---------------------------------------------------------------------- ABI
def test_the_entry_points_are_declared_exported_and_bound():
    from dcvc_amd import hip as K
    text = open(os.path.join(ROOT, "include", "dcvc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert re.search(r"int64_t\s+dcvc_scene_stats_workspace\s*\(\s*void\s*\)\s*;", text)
    assert re.search(r"int\s+dcvc_scene_stats\s*\(\s*const void \*cur,\s*const void \*prev,\s*int64_t n,\s*int depth,"
                     r"\s*void \*workspace,\s*int64_t \*out2,\s*void \*stream\s*\)\s*;", text)
    lib = ctypes.CDLL(os.path.join(ROOT, "dcvc_amd", "lib", "libdcvc_hip.so"))
    bound = {n: (res, args) for n, res, args in K.HIP_SYMBOLS}
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in bound and K.CTensor not in bound[name][1], name
        assert not any(isinstance(a, type) and issubclass(a, ctypes._Pointer) for a in bound[name][1]), name
    assert bound["dcvc_scene_stats_workspace"] == (ctypes.c_int64, [])
    assert len(bound["dcvc_scene_stats"][1]) == 7 and bound["dcvc_scene_stats"][1][2] is ctypes.c_int64
    # they are no chroma / frame16 entry points (existing tests count those sets)
    assert not set(SYMBOLS) & (set(K.CHROMA_SYMBOLS) | set(K.SCALAR_VIEW_SYMBOLS))
    chroma = open(os.path.join(ROOT, "dcvc_amd", "csrc", "hip", "chroma.hip")).read()
    assert "scene_stats" not in chroma
    # the workspace size is a host computation: it needs no device
    K.lib().dcvc_scene_stats_workspace.restype = ctypes.c_int64
    n = int(K.lib().dcvc_scene_stats_workspace())
    assert n > 0 and n % 8 == 0


def test_the_wrapper_rejects_bad_planes_before_the_device():
    """ValueError on mismatched sizes or dtypes or a bad depth; CPU tensors, so
    a call that got as far as the library would fail differently."""
    from dcvc_amd import hip as K
    ws = torch.empty(int(K.lib().dcvc_scene_stats_workspace()) // 8, dtype=torch.int64)
    out = torch.empty(2, dtype=torch.int64)
    u8 = torch.zeros(15, dtype=torch.uint8)
    s16 = torch.zeros(15, dtype=torch.int16)
    for cur, prev, depth in ((u8, u8[:14], 8), (u8, s16, 8), (s16, s16, 8), (u8, u8, 10), (s16, u8, 10),
                             (u8, u8, 7), (s16, s16, 17), (u8, u8, 8.0), (u8.float(), u8.float(), 8),
                             (u8[:0], u8[:0], 8), (u8[::2], u8[::2], 8)):
        with pytest.raises(ValueError):
            K.scene_stats(cur, prev, depth, ws, out)
    with pytest.raises(ValueError):
        K.scene_stats(u8, u8, 8, ws[:8], out)
    with pytest.raises(ValueError):
        K.scene_stats(u8, u8, 8, ws, out.int())


# ------------------------------------------- the premise of the sequences
def test_the_restatement_on_a_case_done_by_hand():
    cur = np.array([0, 3, 4, 255, 128], dtype=np.uint8)        # bins 0 0 1 63 32
    prev = np.array([4, 3, 0, 0, 130], dtype=np.uint8)         # bins 1 0 0 0 32
    # bin 0: 2 against 3, bins 1 and 32: 1 against 1, bin 63: 1 against 0
    assert R.stats(cur, prev, 8) == (4 + 0 + 4 + 255 + 2, 1 + 1)
    hc, hp = R.hist(cur, 8), R.hist(prev, 8)
    assert (hc[0], hc[1], hc[32], hc[63], hc.sum()) == (2, 1, 1, 1, 5)
    assert (hp[0], hp[1], hp[32], hp[63], hp.sum()) == (3, 1, 1, 0, 5)
    # 16-bit samples are read unsigned, from either view of the bits
    a = np.array([65535, 40000, 0], dtype=np.uint16)
    b = np.array([0, 40001, 65535], dtype=np.uint16)
    assert R.stats(a, b, 16) == R.stats(a.view(np.int16), b.view(np.int16), 16) == (65535 + 1 + 65535, 0)
    s = R.score(a, b, 16)
    assert s["mad"] == (2 * 65535 + 1) / (3 * 65535) and s["hd"] == 0.0 and s["n"] == 3 and s["max_val"] == 65535


def test_the_darkened_cut_moves_the_histogram_only_at_the_cut():
    """moving_pattern seed 1, then seed 2 halved: on the G plane hd >= 0.5 at
    frame 5 only (0.685 there, at most 0.035 elsewhere)."""
    sc = R.scores([f[1] for f in R.cut_sequence(darken=True)], 8)
    assert sc[0] is None and len(sc) == R.FRAMES
    hd = [s["hd"] for s in sc[1:]]
    print("hd", [round(v, 4) for v in hd])
    assert [t + 1 for t, v in enumerate(hd) if v >= 0.5] == [R.CUT]
    assert abs(hd[R.CUT - 1] - 0.685) < 0.01 and max(v for t, v in enumerate(hd) if t + 1 != R.CUT) <= 0.035 + 1e-3


def test_the_plain_cut_shows_in_mad_and_not_in_hd():
    """The same without the halving: mad >= 0.15 at frame 5 only (0.20 against
    at most 0.074) while hd stays below 0.05 everywhere: why both exist."""
    sc = R.scores([f[1] for f in R.cut_sequence(darken=False)], 8)
    mad, hd = [s["mad"] for s in sc[1:]], [s["hd"] for s in sc[1:]]
    print("mad", [round(v, 4) for v in mad], "hd", [round(v, 4) for v in hd])
    assert [t + 1 for t, v in enumerate(mad) if v >= 0.15] == [R.CUT]
    assert abs(mad[R.CUT - 1] - 0.20) < 0.01 and max(v for t, v in enumerate(mad) if t + 1 != R.CUT) <= 0.074 + 1e-3
    assert max(hd) < 0.05


def test_is_cut_takes_any_given_threshold():
    from dcvc_amd.scenecut import is_cut
    s = {"hd": 0.5, "mad": 0.1}
    assert not is_cut(None, 0.1, 0.1) and not is_cut(s) and not is_cut(s, None, None)
    assert is_cut(s, 0.5) and not is_cut(s, 0.51) and is_cut(s, None, 0.1) and not is_cut(s, None, 0.11)
    assert is_cut(s, 0.9, 0.1) and is_cut(s, 0.5, 0.9) and not is_cut(s, 0.9, 0.9)
