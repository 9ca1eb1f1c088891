"""The stand-alone encoder and decoder (dcvc_amd/sequence.py, the codecs'
encode_frame / decode_frame, harness.encode_video / decode_video) against the
existing encode_decode path, free-running in the bench's split precision.

Every comparison is byte, bit or torch.equal equality: the encoder's own
reconstruction IS the decoder's, and the stored DPB digests say so per frame.
Weights and frames are the committed synthetic fixtures; no oracle is needed.
"""
import os
import shutil
import struct

import pytest
import torch

from tests.parity import dpb_view as _t, keep_dpb as keep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _prec(name):
    from dcvc_amd.layers import Precision
    return getattr(Precision, name)()


def dc_nets(g, prec="split", i_sd=None, p_sd=None):
    from dcvc_amd.dc import DMC, IntraNoAR
    inet = IntraNoAR(precision=_prec(prec)).load_state_dict(i_sd if i_sd is not None else g.i_state_dict())
    pnet = DMC(precision=_prec(prec)).load_state_dict(p_sd if p_sd is not None else g.p_state_dict())
    inet.update(force=True)
    pnet.update(force=True)
    return inet, pnet


def hem_nets(g, prec="split", i_sd=None, p_sd=None):
    from dcvc_amd.hem import DMC, IntraNoAR
    inet = IntraNoAR(precision=_prec(prec)).load_state_dict(i_sd if i_sd is not None else g.i_state_dict())
    pnet = DMC(precision=_prec(prec)).load_state_dict(p_sd if p_sd is not None else g.p_state_dict())
    inet.update(force=True)
    pnet.update(force=True)
    return inet, pnet


@pytest.fixture(scope="module")
def hem_golden():
    from tests.hem_fixtures import HEMGolden
    return HEMGolden()


@pytest.fixture(scope="module")
def dc_enc_nets(dc_golden):
    return dc_nets(dc_golden)


@pytest.fixture(scope="module")
def dc_dec_nets(dc_golden):
    """Built apart from the encoder's, as another process would."""
    return dc_nets(dc_golden)


@pytest.fixture(scope="module")
def hem_enc_nets(hem_golden):
    return hem_nets(hem_golden)


def assert_dpb_equal(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        ta, tb = _t(a[k]), _t(b[k])
        if k == "ref_frame":
            assert ta.dim() == 4 and tb.dim() == 4
        assert ta.shape == tb.shape and torch.equal(ta, tb), (what, k)


def reference_loop(kind, inet, pnet, xs, h, w, q, gop, folder):
    """The existing path, as run_test / run_test_hem drive it: encode_decode
    per frame through a real N.bin file.  Per frame (file bytes, dpb, bit)."""
    out, dpb = [], None
    for t, x in enumerate(xs):
        path = os.path.join(folder, f"{t}.bin")
        if t % gop == 0:
            if kind == "dc":
                r = inet.encode_decode(x, False, q, path, pic_height=h, pic_width=w)
                dpb = {"ref_frame": r["x_hat"], "ref_feature": None, "ref_mv_feature": None, "ref_y": None,
                       "ref_mv_y": None}
            else:
                r = inet.encode_decode(x, q[0], path, pic_height=h, pic_width=w)
                dpb = {"ref_frame": r["x_hat"], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
        elif kind == "dc":
            r = pnet.encode_decode(x, dpb, False, q, path, pic_height=h, pic_width=w, frame_idx=t % 4)
            dpb = r["dpb"]
        else:
            r = pnet.encode_decode(x, dpb, path, pic_height=h, pic_width=w, mv_y_q_scale=q[1], y_q_scale=q[2])
            dpb = r["dpb"]
        with open(path, "rb") as f:
            out.append((f.read(), keep(dpb), r["bit"]))
    return out


def q_args(kind, q):
    if kind == "dc":
        return dict(q_in_ckpt=False, q_index=q)
    return dict(i_frame_q_scale=q[0], p_frame_mv_y_q_scale=q[1], p_frame_y_q_scale=q[2])


def encode_sequence(kind, inet, pnet, xs, h, w, q, gop, path):
    """Per frame: the SequenceEncoder's dict with the dpb copied."""
    from dcvc_amd.sequence import SequenceEncoder
    out = []
    with SequenceEncoder(inet, pnet, path, w, h, gop, **q_args(kind, q)) as enc:
        for x in xs:
            r = enc.encode(x)
            out.append(dict(r, dpb=keep(enc.dpb)))
    return out


def check_against_reference(kind, inet, pnet, xs, h, w, q, gop, tmp_path):
    """The three equalities of the golden tests: payload == .bin bytes, the
    encoder's DPB == the decoder's tensor by tensor, stored digests == the
    digests of the decoder's DPB."""
    from dcvc_amd.sequence import SequenceReader, FrameDigest
    ref = reference_loop(kind, inet, pnet, xs, h, w, q, gop, str(tmp_path))
    path = str(tmp_path / "a.seq")
    enc = encode_sequence(kind, inet, pnet, xs, h, w, q, gop, path)
    with SequenceReader(path) as r:
        records = list(r)
    assert len(records) == len(xs)
    digest = FrameDigest(inet.dev)
    for t, ((data, dpb, bit), e, rec) in enumerate(zip(ref, enc, records)):
        assert e["payload"] == data == rec["payload"], t
        assert e["bit"] == bit == len(data) * 8, t
        assert e["type"] == rec["type"] == ("I" if t % gop == 0 else "P")
        assert_dpb_equal(e["dpb"], dpb, (kind, t))
        assert rec["digest"] is not None and rec["digest"] == e["digest"] == digest(dpb), t
    return enc, records


# ------------------------------------------------------------------ 1 and 4
def test_dc_golden_encoder_is_the_decoder(dc_golden, dc_enc_nets, tmp_path):
    g = dc_golden
    meta = g.meta["A"]
    assert (meta["h"], meta["w"], meta["frames"]) == (176, 240, 4)
    xs = [g.frame_tensor("A", t)[1].cuda() for t in range(meta["frames"])]
    check_against_reference("dc", *dc_enc_nets, xs, meta["h"], meta["w"], meta["q_index"], 32, tmp_path)


def test_hem_golden_encoder_is_the_decoder(hem_golden, hem_enc_nets, tmp_path):
    g = hem_golden
    meta = g.meta["A"]
    assert meta["frames"] == 3
    # I + 3 P: the fixture holds three frames, the fourth is frame 1 again
    xs = [g.frame_tensor("A", t)[1].cuda() for t in (0, 1, 2, 1)]
    check_against_reference("hem", *hem_enc_nets, xs, meta["h"], meta["w"], g.q("A"), 32, tmp_path)


# ------------------------------------------------------------- 2, 6 and 7
H2, W2, N2, GOP2, Q2 = 100, 130, 9, 8, 40


def _stage_inputs(frames, h, w, yuv, dev):
    """The padded codec inputs FrameStage.load produces, one tensor each."""
    from dcvc_amd.harness import FrameStage
    stage = FrameStage(h, w, 16, yuv, zero_pad=False, frame_num=len(frames), device=dev)
    return [stage.load(stage.upload(f)).nchw_view().clone() for f in frames]


@pytest.fixture(scope="module")
def free_run(dc_golden, dc_enc_nets, tmp_path_factory):
    """More than one GOP, free running: 9 frames of moving_pattern at
    100 x 130 (pads to 112 x 144, no multiple of 64), gop_size 8, q 40, coded
    once to a sequence file and once by the encode_decode loop."""
    from dcvc_amd.synth import moving_pattern
    td = tmp_path_factory.mktemp("free_run")
    inet, pnet = dc_enc_nets
    xs = _stage_inputs([moving_pattern(H2, W2, t, seed=1) for t in range(N2)], H2, W2, False, inet.dev)
    assert xs[0].shape == (1, 3, 112, 144)
    path = str(td / "free.seq")
    enc = encode_sequence("dc", inet, pnet, xs, H2, W2, Q2, GOP2, path)
    ref = reference_loop("dc", inet, pnet, xs, H2, W2, Q2, GOP2, str(td))
    return path, enc, ref


def test_free_running_decoder(free_run, dc_dec_nets):
    from dcvc_amd.sequence import SequenceDecoder
    path, enc, ref = free_run
    assert [e["type"] for e in enc] == ["I"] + ["P"] * 7 + ["I"]
    with SequenceDecoder(*dc_dec_nets, path) as dec:
        assert (dec.width, dec.height, dec.frames) == (W2, H2, N2)
        n = 0
        for t, out in enumerate(dec):      # every digest verifies, or this raises
            assert out["type"] == enc[t]["type"]
            assert torch.equal(out["x_hat"], enc[t]["dpb"]["ref_frame"]), t
            assert_dpb_equal(keep(out["dpb"]), enc[t]["dpb"], t)
            assert out["bit"] == enc[t]["bit"] == ref[t][2], t
            assert enc[t]["payload"] == ref[t][0], t
            n += 1
    assert n == N2


def test_tampered_digest_is_caught(free_run, dc_dec_nets, tmp_path):
    """One bit of one stored digest flipped on the host: the decoder names
    that frame, and the frames before it decode as they should."""
    from dcvc_amd.sequence import SequenceDecoder, DigestMismatch
    path, enc, _ = free_run
    bad, victim = str(tmp_path / "bad.seq"), 5
    shutil.copy(path, bad)
    with open(bad, "r+b") as f:
        pos = 40
        for _ in range(victim):
            f.seek(pos + 4)
            pos += 24 + struct.unpack("<I", f.read(4))[0]
        f.seek(pos + 8 + 3)               # a byte of the first digest word
        b = f.read(1)[0]
        f.seek(pos + 8 + 3)
        f.write(bytes([b ^ 0x10]))
    good = []
    with SequenceDecoder(*dc_dec_nets, bad) as dec, pytest.raises(DigestMismatch) as err:
        for out in dec:
            good.append(out["x_hat"].clone())
    assert err.value.frame_idx == victim and f"frame {victim}:" in str(err.value)
    assert err.value.stored[0] == err.value.computed[0] ^ (0x10 << 24)
    assert err.value.stored[1] == err.value.computed[1] == enc[victim]["digest"][1]
    assert len(good) == victim
    for t, x in enumerate(good):
        assert torch.equal(x, enc[t]["dpb"]["ref_frame"]), t


def test_header_mismatch(free_run, dc_golden, hem_enc_nets, dc_dec_nets):
    """Nets that are not what wrote the file: refused before any frame."""
    from dcvc_amd.sequence import SequenceDecoder
    path = free_run[0]
    with pytest.raises(ValueError, match="HEM"):
        SequenceDecoder(*hem_enc_nets, path)
    with pytest.raises(ValueError, match="parity"):
        SequenceDecoder(*dc_nets(dc_golden, "parity"), path)
    inet, pnet = dc_dec_nets
    try:
        inet.codec_format = pnet.codec_format = "yuv420"
        with pytest.raises(ValueError, match="yuv420"):
            SequenceDecoder(inet, pnet, path)
    finally:
        del inet.codec_format, pnet.codec_format
    with pytest.raises(ValueError):   # an I and a P codec of two precisions
        SequenceDecoder(inet, dc_nets(dc_golden, "parity")[1], path)


# ------------------------------------------------------------------------ 3
def test_yuv420_encode_video_decode_video(dc_golden, dc_enc_nets, dc_dec_nets, tmp_path):
    """The YUV420 codec path through encode_video / decode_video: the decoded
    out.yuv is byte for byte what run_test(save_decoded_frame) writes."""
    from dcvc_amd.harness import run_test, encode_video, decode_video, ArrayReader
    from dcvc_amd.synth import moving_pattern_yuv420
    frames = [moving_pattern_yuv420(H2, W2, t, seed=1) for t in range(N2)]
    base = {"frame_num": N2, "gop_size": GOP2, "src_type": "yuv420", "src_height": H2, "src_width": W2,
            "dist_in_yuv420": True, "q_in_ckpt": False, "i_frame_q_index": Q2, "verbose": 1}
    inet, pnet = dc_enc_nets
    dnets = dc_dec_nets
    try:
        seq = str(tmp_path / "v.seq")
        elog = encode_video(inet, pnet, dict(base, src_reader=ArrayReader(frames), seq_path=seq))
        dlog = decode_video(*dnets, {"seq_path": seq, "dist_in_yuv420": True, "src_type": "yuv420",
                                     "save_decoded_frame": True, "recon_path": str(tmp_path / "dec")})
    finally:
        for net in (inet, pnet) + tuple(dnets):
            net.__dict__.pop("codec_format", None)
    bins = tmp_path / "bins"
    bins.mkdir()
    rec = tmp_path / "ref" / "seq" / "0"
    rlog = run_test(pnet, inet, dict(base, src_reader=ArrayReader(frames), write_stream=True, bin_folder=str(bins),
                                     save_decoded_frame=True, recon_path=str(rec), rate_idx=0))
    folders = os.listdir(tmp_path / "ref" / "seq")
    assert len(folders) == 1
    want = (tmp_path / "ref" / "seq" / folders[0] / "out.yuv").read_bytes()
    got = (tmp_path / "dec" / "out.yuv").read_bytes()
    assert len(want) == N2 * (H2 * W2 + 2 * (H2 // 2) * (W2 // 2)) and got == want
    bits = [os.path.getsize(bins / f"{t}.bin") * 8 for t in range(N2)]
    assert elog["frame_bits"] == dlog["frame_bits"] == bits
    assert dlog["frame_type"] == rlog["frame_type"] == elog["frame_type"]
    # the encoder's reconstruction is the decoder's, so its PSNR is run_test's
    assert elog["frame_psnr"] == rlog["frame_psnr"] and elog["frame_psnr_u"] == rlog["frame_psnr_u"]


# ------------------------------------------------------------------------ 5
@pytest.mark.parametrize("case", [("dc", "P", "compress"), ("dc", "P", "decompress"), ("hem", "I", "compress")])
def test_precision_fallback(case, dc_golden, hem_golden, tmp_path):
    """A frame the split cannot carry (the scaled weight pairs of
    tests/test_gpu_split_range.py): the stand-alone encoder codes it on the
    fp32 twin and says so in the file; a split decoder takes the twin for that
    frame, verifies the digest and returns the fp32 codec's reconstruction.
    The "decompress" pair trips in the ENCODER as well, whose reconstruction
    runs the decoder's kernels."""
    from tests.test_gpu_split_range import HOT_PAIRS, _hot
    from dcvc_amd.sequence import SequenceDecoder, SequenceReader
    model, kind, _ = case
    g = dc_golden if model == "dc" else hem_golden
    make = dc_nets if model == "dc" else hem_nets
    meta = g.meta["A"]
    h, w = meta["h"], meta["w"]
    q = meta["q_index"] if model == "dc" else g.q("A")
    isd, psd = g.i_state_dict(), g.p_state_dict()
    hot_i = _hot(isd, HOT_PAIRS[case]) if kind == "I" else isd
    hot_p = _hot(psd, HOT_PAIRS[case]) if kind == "P" else psd
    t_hot = 0 if kind == "I" else 1
    xs = [g.frame_tensor("A", t)[1].cuda() for t in range(t_hot + 1)]
    path = str(tmp_path / "hot.seq")
    inet, pnet = make(g, "split", hot_i, hot_p)
    enc = encode_sequence(model, inet, pnet, xs, h, w, q, 32, path)
    hot_net = inet if kind == "I" else pnet
    assert enc[t_hot]["precision_fallback"] == "parity" and hot_net.fallbacks == 1
    with SequenceReader(path) as r:
        records = list(r)
    assert [rec["twin"] for rec in records] == [t == t_hot and True for t in range(t_hot + 1)]
    if t_hot:
        assert enc[0]["precision_fallback"] is None
    # the fp32 codec on the unscaled weights, from the encoder's own DPB
    ri, rp = make(g, "parity", isd, psd)
    if kind == "I":
        ref = ri.encode_frame(xs[0], q[0], h, w) if model == "hem" else ri.encode_frame(xs[0], False, q, h, w)
        ref_frame = ref["x_hat"]
    else:
        ref = rp.encode_frame(xs[1], enc[0]["dpb"], False, q, 1)
        ref_frame = ref["dpb"]["ref_frame"]
    assert ref["precision_fallback"] is None
    assert enc[t_hot]["payload"] == ref["payload"] == records[t_hot]["payload"]
    assert torch.equal(enc[t_hot]["dpb"]["ref_frame"], ref_frame)
    # a split decoder with the scaled weights
    di, dp = make(g, "split", hot_i, hot_p)
    with SequenceDecoder(di, dp, path) as dec:
        frames = [dict(out, x_hat=out["x_hat"].clone()) for out in dec]   # digests verified
    assert len(frames) == t_hot + 1
    assert torch.equal(frames[t_hot]["x_hat"], ref_frame)
    hot_dec = di if kind == "I" else dp
    assert getattr(hot_dec, "_parity_twin", None) is not None, "the flagged frame was not decoded by the twin"
    assert getattr(hot_dec, "fallbacks", 0) == 0
