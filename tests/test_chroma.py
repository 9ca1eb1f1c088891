"""Planar YUV 4:4:4 and 4:2:2 sources and output, 8..16 bits per sample
(INTEGRATION.md "Chroma layouts", chroma.hip).

CPU tests pin the numpy restatement (tests/chroma_ref.py) to scipy and numpy on
this machine and to the reference's own rgb_to_ycbcr / ycbcr_to_rgb
(tests/golden/chroma_golden.*, written by make_golden_chroma.py), and check
the readers, the argument errors and the ABI.  GPU tests hold every entry
point bit-equal to the restatement at the three layouts, the (2, 2)
instantiation bit-equal to the 4:2:0 kernels it is defined by, and the harness
paths (run_test, encode_video / decode_video, the command line) to the 4:2:0
path on sources that give the codec the same input, to the oracle codec, and
to the restatement of what they write.
"""
import ctypes
import functools
import hashlib
import importlib.util
import json
import os
import re
import struct
import tempfile

import numpy as np
import pytest
import scipy.ndimage
import torch

from oracle import harness_oracle as HO
from tests import chroma_ref as C
from tests import crossfmt_ref as R
from tests import frame16_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ["dcvc_yuvp_to_nhwc", "dcvc_yuvp_to_rgb_nhwc", "dcvc_yuvp_sse", "dcvc_recon_to_yuvp"]
TOL_SSE = 1e-12       # tests/test_frame16.py (rtol of the three sums)
DEPTHS = (8, 10, 16)
# (h, w, H, W) -> the layouts that take it: one-column chroma; odd sizes; odd
# height with chroma width 27 and padding on both axes; all three; several blocks
SHAPES = {(2, 2, 16, 16): ("444", "422", "420"), (37, 53, 48, 64): ("444",), (37, 54, 48, 64): ("444", "422"),
          (38, 54, 48, 64): ("444", "422", "420"), (100, 130, 112, 144): ("444", "422", "420")}
CASES = [(s, c, d) for s, cs in SHAPES.items() for c in cs for d in DEPTHS]
TWIN_CASES = [(s, d) for s, cs in SHAPES.items() if "420" in cs for d in (8, 10)]
WIDTHS = (1, 2, 3, 27, 65)


@functools.lru_cache(maxsize=None)
def _fixture():
    spec = importlib.util.spec_from_file_location("make_golden_chroma", os.path.join(GOLDEN, "make_golden_chroma.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with open(os.path.join(GOLDEN, "chroma_golden.json")) as f:
        cases = {(c["h"], c["w"], c["depth"]): c for c in json.load(f)["cases"]}
    return m, cases, np.load(os.path.join(GOLDEN, "chroma_golden.npz"))


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _planes(seed, shape, d):
    """Sample planes of one shape at depth d: uniform in [0, max_val]."""
    g = np.random.default_rng(seed)
    a = g.integers(0, (1 << d), size=shape, dtype=np.uint16)
    return a.astype(np.uint8) if d == 8 else a


@functools.lru_cache(maxsize=None)
def _source(h, w, d, chroma):
    """y (h, w), uv (2, h/sy, w/sx) holding 0, max_val, max_val - 1 and, at 10
    bits, one sample above max_val (the rule does not clamp it).  Shared; no
    test writes to them."""
    sx, sy = C.sub(chroma)
    mx = C.max_val(d)
    y, uv = _planes(h * 1000 + w + d, (h, w), d).copy(), _planes(h * 1000 + w + d + 1, (2, h // sy, w // sx), d).copy()
    special = [0, mx, mx - 1] + ([mx + 5] if d == 10 else [])
    for a in (y, uv):
        flat = a.reshape(-1)
        for k, v in enumerate(special[:flat.size]):
            flat[(k * 7919 + 1) % flat.size if flat.size > len(special) else k] = v
    return y, uv


@functools.lru_cache(maxsize=None)
def _writer_frame(h, w, d):
    """float32 (3, h, w) in [-0.1, 1.1) with the run of values within one fp32
    ulp of a half-integer of max_val on both sides (the frame16 fixtures' rule)."""
    from tests.test_frame16 import _fixture as f16
    return f16()[0].writer_inputs(h * 7 + w, h, w, d)


# --------------------------------------------------------------------- CPU
@pytest.mark.parametrize("d", DEPTHS)
@pytest.mark.parametrize("m", WIDTHS)
def test_restatement_bit_equal_to_scipy_and_numpy(m, d):
    """The (1, 1, 2) zooms of both orders against scipy, the pair mean against
    numpy's mean over the pair, on planes m chroma columns wide."""
    a = C.to_float(_planes(m * 100 + d, (2, 5, m), d), d)
    np.testing.assert_array_equal(C.zoom0_x(a), scipy.ndimage.zoom(a, (1, 1, 2), order=0))
    np.testing.assert_array_equal(C.zoom1_x(a), scipy.ndimage.zoom(a, (1, 1, 2), order=1))
    assert C.zoom1_x(a).dtype == np.float32
    g = np.random.default_rng(m + d)
    wide = (g.random((2, 5, 2 * m)) * 1.2 - 0.1).astype(np.float32)
    for p in (wide, C.to_float(_planes(m + d, (2, 5, 2 * m), d), d)):
        ref = np.mean(np.reshape(p, (2, 5, m, 2)), axis=-1)
        assert ref.dtype == np.float32
        np.testing.assert_array_equal(C.pair_mean(p), ref)


@pytest.mark.parametrize("d", DEPTHS)
@pytest.mark.parametrize("m", WIDTHS)
def test_420_restatement_is_the_cross_format_one(m, d):
    """With (2, 2) every function is crossfmt_ref's / frame16_ref's."""
    h, w = 6, 2 * m
    y, uv = _planes(m + d, (h, w), d), _planes(m + d + 1, (2, h // 2, m), d)
    yf, uvf = C.to_float(y, d), C.to_float(uv, d)
    H, W = 16, 16 * ((w + 15) // 16)
    np.testing.assert_array_equal(C.ingest_yuv(y, uv, d, "420", H, W), R.pad_nhwc(R.yuv420_to_444(yf[None], uvf), H, W))
    x, rgb = C.ingest_rgb(y, uv, d, "420", H, W)
    np.testing.assert_array_equal(rgb, R.yuv420_to_rgb(yf[None], uvf))
    np.testing.assert_array_equal(x, R.pad_nhwc(rgb, H, W))
    g = np.random.default_rng(m)
    crop = (g.random((3, h, w)) * 1.2 - 0.1).astype(np.float32)
    ya, uva = C.yuv444_planes(crop, "420")
    yb, uvb = F.yuv444_to_420(crop)
    np.testing.assert_array_equal(ya, yb)
    np.testing.assert_array_equal(uva, uvb)
    ya, uva = C.rgb_planes(crop, "420")
    yb, uvb = R.rgb_to_yuv420(crop)
    np.testing.assert_array_equal(ya, yb)
    np.testing.assert_array_equal(uva, uvb)
    if d > 8:
        np.testing.assert_array_equal(C.file_frame(crop, d, "420"), F.yuv_file_frame(crop, d))
        np.testing.assert_array_equal(C.file_frame(crop, d, "420", True), F.yuv_file_frame_from_rgb(crop, d))
    else:
        assert C.file_frame(crop, d, "420", True).tobytes() == R.yuv_bytes_from_rgb(crop)
    cl = np.clip(crop, 0, 1)
    np.testing.assert_array_equal(C.sse_yuv(cl, y, uv, d, "420"), F.sse_yuv(cl, yf, uvf))


@pytest.mark.parametrize("h,w,d", [(2, 2, 8), (2, 2, 10), (2, 2, 16), (37, 53, 8), (37, 53, 10), (37, 53, 16)])
def test_restatement_reproduces_reference_fixture(h, w, d):
    """tests/chroma_ref.py against the reference's rgb_to_ycbcr / ycbcr_to_rgb:
    every digest, and the stored arrays."""
    m, cases, arrays = _fixture()
    c = cases[(h, w, d)]
    yuv = m.inputs(c["seed"], h, w, d)
    assert yuv.min() == 0 and yuv.max() == C.max_val(d)
    x, rgb = C.ingest_rgb(yuv[0], yuv[1:3], d, "444", h, w)
    fr = m.writer_inputs(c["seed"], h, w)
    assert fr.min() < 0 and fr.max() > 1 and (fr == 0).any() and (fr == 1).any()
    out = np.concatenate(C.rgb_planes(fr, "444"), axis=0)
    assert rgb.dtype == np.float32 and out.dtype == np.float32
    for got in (rgb, out):
        assert got.min() == 0 and got.max() == 1                         # clipped on both sides
    assert _digest(rgb) == c["yuv_to_rgb"] and _digest(out) == c["rgb_to_yuv"]
    np.testing.assert_array_equal(x, rgb.transpose(1, 2, 0))
    if f"yuv_to_rgb_{h}x{w}_{d}" in arrays:
        np.testing.assert_array_equal(rgb, arrays[f"yuv_to_rgb_{h}x{w}_{d}"])
        np.testing.assert_array_equal(out, arrays[f"rgb_to_yuv_{h}x{w}_{d}"])
    assert {f"{k}_{hh}x{ww}_{dd}" for k in ("yuv_to_rgb", "rgb_to_yuv") for hh, ww, dd in m.STORED} == set(arrays.files)


def test_rule_four_is_the_420_writer_with_a_1x2_block():
    """4:2:2 output from an RGB frame: y clipped, cb / cr unclipped into the
    pair mean, then clipped, on a frame whose chroma leaves [0, 1] before it."""
    g = np.random.default_rng(3)
    crop = (g.random((3, 5, 8)) * 1.6 - 0.3).astype(np.float32)
    y, cb, cr = R.rgb_to_ycc(crop)
    assert cb.min() < 0 or cr.min() < 0 or cb.max() > 1 or cr.max() > 1
    ya, uva = C.rgb_planes(crop, "422")
    np.testing.assert_array_equal(ya, np.clip(y, 0, 1))
    for k, p in enumerate((cb, cr)):
        ref = np.clip(np.mean(np.reshape(p, (1, 5, 4, 2)), axis=-1), 0, 1)
        np.testing.assert_array_equal(uva[k:k + 1], ref)
    yb, uvb = C.rgb_planes(crop, "444")
    np.testing.assert_array_equal(np.concatenate((yb, uvb)), np.clip(np.concatenate((y, cb, cr)), 0, 1))


@pytest.mark.parametrize("d", [8, 10])
@pytest.mark.parametrize("chroma", ["422", "444"])
def test_yuv_reader_reads_422_and_444_files(tmp_path, chroma, d):
    """Real files: plane shapes and types, frame and skip sizes, ".yuv"
    appended, a short last frame is the end and the end is sticky."""
    from dcvc_amd.harness import YUVReader
    h, w, n = 5, 6, 3
    sx, sy = C.sub(chroma)
    dt = np.dtype(np.uint8) if d == 8 else np.dtype("<u2")
    frames = [(_planes(t, (h, w), d), _planes(t + 50, (2, h // sy, w // sx), d)) for t in range(n)]
    raw = b"".join(y.astype(dt).tobytes() + uv.astype(dt).tobytes() for y, uv in frames)
    fs = (h * w + 2 * (h // sy) * (w // sx)) * dt.itemsize
    assert len(raw) == n * fs and sum(C.frame_sizes(h, w, chroma)) * dt.itemsize == fs
    open(tmp_path / "seq.yuv", "wb").write(raw + raw[:fs - 1])           # a fourth frame cut short
    r = YUVReader(str(tmp_path / "seq"), w, h, src_format=chroma, bit_depth=d)
    assert r.src_path.endswith("seq.yuv") and r.y_size + r.uv_size == fs and r.src_format == chroma
    for y, uv in frames:
        gy, guv = r.read_one_frame(dst_format="420")
        assert gy.dtype == dt and guv.dtype == dt and gy.shape == (h, w) and guv.shape == (2, h // sy, w // sx)
        np.testing.assert_array_equal(gy, y)
        np.testing.assert_array_equal(guv, uv)
    assert r.read_one_frame() == (None, None) and r.eof
    assert r.read_one_frame(dst_format="rgb") == (None, None)            # sticky
    with pytest.raises(ValueError):
        r.read_one_frame(dst_format="444")                               # the layout is never a dst_format
    r.close()
    r = YUVReader(str(tmp_path / "seq.yuv"), w, h, src_format=chroma, skip_frame=2, bit_depth=d)
    gy, guv = r.read_one_frame()
    np.testing.assert_array_equal(gy, frames[2][0])
    np.testing.assert_array_equal(guv, frames[2][1])
    r.close()


def test_yuv_reader_argument_errors(tmp_path):
    from dcvc_amd.harness import YUVReader
    open(tmp_path / "a.yuv", "wb").write(b"\0" * 64)
    with pytest.raises(ValueError, match="even width"):
        YUVReader(str(tmp_path / "a"), 5, 4, src_format="422")
    for fmt in ("411", "rgb", "yuv444", None):
        with pytest.raises(ValueError):
            YUVReader(str(tmp_path / "a"), 4, 4, src_format=fmt)
    YUVReader(str(tmp_path / "a"), 5, 3, src_format="444").close()       # 4:4:4 takes any size
    YUVReader(str(tmp_path / "a"), 4, 3, src_format="422").close()       # 4:2:2: odd height


def test_python_level_argument_errors(tmp_path):
    """Unknown src_type / chroma, calc_ssim on a YUV codec, PNG kinds and HEM
    with the new layouts: a ValueError before anything touches the device or a
    file is opened or created."""
    from dcvc_amd import hip as K
    from dcvc_amd import harness
    from dcvc_amd.harness import FrameStage, ReconWriter, _reader, _src_format, _writer_kind, psnr_yuv
    cpu = torch.device("cpu")
    for bad in ("yuv411", "444", "yuv", 444):
        with pytest.raises(ValueError, match="src_type"):
            _src_format(bad, "420")
    assert [_src_format(t, "rgb") for t in ("yuv420", "yuv422", "yuv444", "png", "rgb", None)] == \
        ["420", "422", "444", "rgb", "rgb", "rgb"]
    assert _writer_kind("yuv444", "444", 8) == "yuv" and _writer_kind("yuv422", "422", 10) == "yuv"
    with pytest.raises(ValueError, match="src_type"):
        _reader({"src_type": "yuv440", "src_path": str(tmp_path / "x"), "src_width": 4, "src_height": 4}, True)
    for bad in ("411", "rgb", (1, 2), None):
        with pytest.raises(ValueError, match="chroma"):
            K.chroma_sub(bad)
        with pytest.raises(ValueError):
            ReconWriter(str(tmp_path / "r"), 4, 6, "yuv", "420", cpu, chroma=bad)
        with pytest.raises(ValueError):
            psnr_yuv(np.ones(3), 4, 6, bad)
    assert [K.chroma_sub(c) for c in ("444", "422", "420", (2, 1))] == [(1, 1), (2, 1), (2, 2), (2, 1)]
    t8, t16 = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.int16)
    x = K.Act(torch.zeros((16, 16, 3)), 0, 3)
    for fn in (lambda c, d: K.yuvp_to_nhwc(t8, t8, 4, 4, d, c, x),
               lambda c, d: K.yuvp_to_rgb_nhwc(t8, t8, 4, 4, d, c, x, torch.zeros(48)),
               lambda c, d: K.yuvp_sse(x, t8, t8, 4, 4, d, c, torch.zeros(8, dtype=torch.float64),
                                       torch.zeros(3, dtype=torch.float64)),
               lambda c, d: K.recon_to_yuvp(x, 4, 4, d, c, False, t16)):
        for c, d in (("411", 8), ("rgb", 8), ("444", 7), ("444", 17), ("422", 10.0), ("444", None)):
            with pytest.raises(ValueError):
                fn(c, d)
    with pytest.raises(ValueError):
        K.yuvp_sizes(4, 5, "422")                                        # odd width
    with pytest.raises(ValueError):
        K.yuvp_sizes(5, 4, "420")
    assert K.yuvp_sizes(5, 4, "422") == (2, 1, 20, 20) and K.yuvp_sizes(5, 3, "444") == (1, 1, 15, 30)
    for kind in ("png", "hem_png", "rgb"):
        for chroma in ("422", "444"):
            with pytest.raises(ValueError, match="out.yuv"):
                ReconWriter(str(tmp_path / "r"), 4, 6, kind, "rgb", cpu, chroma=chroma)
    with pytest.raises(ValueError, match="even"):
        ReconWriter(str(tmp_path / "r"), 4, 7, "yuv", "420", cpu, chroma="422")
    with pytest.raises(ValueError, match="even"):
        FrameStage(4, 7, 16, True, False, 1, cpu, src_format="422")
    with pytest.raises(ValueError, match="even"):
        FrameStage(4, 7, 16, True, False, 1, cpu, bit_depth=10)          # 4:2:0 as before
    with pytest.raises(ValueError):
        FrameStage(4, 6, 64, False, True, 1, cpu, src_format="444")      # no zero padding
    with pytest.raises(ValueError, match="src_format"):
        FrameStage(4, 6, 16, True, False, 1, cpu, src_format="411")
    assert not os.path.exists(tmp_path / "r")

    class Net:
        dev = cpu
    missing = str(tmp_path / "nowhere" / "src")
    base = {"frame_num": 1, "gop_size": 8, "src_path": missing, "src_width": 6, "src_height": 4, "q_in_ckpt": False,
            "i_frame_q_index": 0, "save_decoded_frame": True, "recon_path": str(tmp_path / "rec"),
            "decoded_frame_folder": str(tmp_path / "rec"), "seq_path": str(tmp_path / "a.seq")}
    for st in ("yuv422", "yuv444"):
        with pytest.raises(ValueError, match="calc_ssim"):
            harness.run_test(Net(), Net(), dict(base, src_type=st, dist_in_yuv420=True, calc_ssim=True))
        with pytest.raises(ValueError, match="HEM harness reads RGB"):
            harness.run_test_hem(Net(), Net(), dict(base, src_type=st))
    with pytest.raises(ValueError, match="HEM harness reads RGB"):
        harness.run_test_hem(Net(), Net(), dict(base, src_type="yuv420"))
    assert not os.path.exists(tmp_path / "rec") and not os.path.exists(tmp_path / "a.seq")


def test_hem_encoder_rejects_the_new_sources(tmp_path):
    from dcvc_amd import harness
    from dcvc_amd.hem import IntraNoAR
    net = IntraNoAR.__new__(IntraNoAR)
    for st in ("yuv420", "yuv422", "yuv444"):
        with pytest.raises(ValueError, match="HEM harness reads RGB"):
            harness.encode_video(net, net, {"frame_num": 1, "gop_size": 8, "src_type": st,
                                            "seq_path": str(tmp_path / "a.seq")})
    assert not os.path.exists(tmp_path / "a.seq")


def test_psnr_yuv_takes_the_sources_plane_sizes():
    from dcvc_amd.harness import calc_psnr_from_sse, psnr_yuv
    sse, h, w = np.array([0.5, 0.25, 0.125]), 37, 54
    assert psnr_yuv(sse, 38, w) == psnr_yuv(sse, 38, w, "420")
    for chroma, n in (("444", h * w), ("422", h * (w // 2))):
        py, pu, pv, p = psnr_yuv(sse, h, w, chroma)
        assert (py, pu, pv) == (calc_psnr_from_sse(0.5, h * w), calc_psnr_from_sse(0.25, n),
                                calc_psnr_from_sse(0.125, n))
        assert p == (6 * py + pu + pv) / 8


def test_header_declares_and_library_exports_the_symbols():
    from dcvc_amd import hip as K
    header = open(os.path.join(ROOT, "include", "dcvc_hip.h")).read()
    lib = K.lib()
    bound = {n: args for n, _, args in K.HIP_SYMBOLS}
    assert tuple(K.CHROMA_SYMBOLS) == tuple(NEW_SYMBOLS)
    assert not set(NEW_SYMBOLS) & set(K.SCALAR_VIEW_SYMBOLS)
    text = open(os.path.join(ROOT, "dcvc_amd", "csrc", "hip", "chroma.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (dcvc_\w+)\(', text)) == set(NEW_SYMBOLS)
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\(", header), s
        assert hasattr(lib, s), s
        assert s in bound and K.CTensor not in bound[s], s
        assert all(a in (ctypes.c_void_p, ctypes.c_int) for a in bound[s]), s       # no tensor-struct parameter
        assert not re.search(r"16|yuv420f_to_rgb|rgbf_", s), s
        m = re.search(rf"int {s}\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == len(bound[s]), s
        assert "dcvc_tensor" not in m.group(1), s


def test_eight_bit_420_sequence_file_bytes_are_unchanged(tmp_path):
    """An 8-bit 4:2:0 SequenceWriter file is the documented layout: the chroma
    layouts add nothing to the header or the records."""
    from dcvc_amd.sequence import SequenceWriter
    payloads = [("I", b"\x01\x02\x03", False, (5, 6)), ("P", b"", True, None), ("P", b"\xff" * 7, False, (1, 2))]
    want = b"DCVCSEQ1" + bytes([0, 1]) + b"split" + b"\0" * 11 + struct.pack("<HIII", 0, 130, 100, 3)
    for t, payload, twin, digest in payloads:
        flags = (1 if twin else 0) | (2 if digest else 0)
        want += struct.pack("<BBHIQQ", "IP".index(t), flags, 0, len(payload), *(digest or (0, 0))) + payload
    p = str(tmp_path / "a.seq")
    with SequenceWriter(p, "DC", "yuv420", "split", 130, 100) as wr:
        for t, payload, twin, digest in payloads:
            wr.write(t, payload, twin=twin, digest=digest)
    assert open(p, "rb").read() == want


# --------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    """Sample planes on the device as FrameStage uploads them: uint8, or the
    bits of uint16 as int16."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).to(DEV)


def _view(H, W, fill=None):
    from tests.test_frame16 import _view as v
    return v(H, W, fill)


def _untouched(a):
    from tests.test_frame16 import _untouched as u
    return u(a)


def _bits(t):
    """A float32 tensor or numpy array as its int32 bit patterns (CPU)."""
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.cpu().contiguous()
    return t.view(torch.int32)


def _host(t, d):
    a = t.cpu().numpy()
    return a if d == 8 else a.view(np.uint16)


def _out_buf(n, d):
    return (torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV) if d == 8
            else torch.full((n,), -23131, dtype=torch.int16, device=DEV))


def _stage(h, w, yuv420, src_format, d, n=1):
    from dcvc_amd.harness import FrameStage
    return FrameStage(h, w, 16, yuv420, zero_pad=False, frame_num=n, device=DEV, src_format=src_format, bit_depth=d)


@gpu
@pytest.mark.parametrize("shape,chroma,d", CASES)
def test_ingest_bit_exact(shape, chroma, d):
    """dcvc_yuvp_to_nhwc and dcvc_yuvp_to_rgb_nhwc into a view with coff 2 of a
    cstride-8 buffer, and through FrameStage: the padded input and src_f32
    equal the restatement bit for bit."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    y, uv = _source(h, w, d, chroma)
    dy, duv = _dev(y), _dev(uv)
    ref = C.ingest_yuv(y, uv, d, chroma, H, W)
    out = _view(H, W)
    K.yuvp_to_nhwc(dy, duv, h, w, d, chroma, out)
    assert torch.equal(_bits(out.t()), _bits(ref))
    assert _untouched(out)
    xr, rgb = C.ingest_rgb(y, uv, d, chroma, H, W)
    out, planes = _view(H, W), torch.full((3, h, w), float("nan"), dtype=torch.float32, device=DEV)
    K.yuvp_to_rgb_nhwc(dy, duv, h, w, d, chroma, out, planes)
    assert torch.equal(_bits(out.t()), _bits(xr))
    assert torch.equal(_bits(planes), _bits(rgb))
    assert _untouched(out)
    if chroma == "420":
        return                                                            # the harness never routes 4:2:0 here
    st = _stage(h, w, True, chroma, d)
    assert (st.H, st.W) == (H, W) and not st.cross and st.src_f32 is None and st.chroma == chroma
    assert torch.equal(_bits(st.load(st.upload((y, uv))).t()), _bits(ref))
    st = _stage(h, w, False, chroma, d)
    assert st.cross
    dframe = st.upload((y, uv))
    assert torch.equal(_bits(st.load(dframe).t()), _bits(xr))
    assert torch.equal(_bits(st.src_f32[0]), _bits(rgb))
    assert st.source_f32(dframe) is st.src_f32


@gpu
@pytest.mark.parametrize("shape,chroma,d", CASES)
def test_yuvp_sse_and_inplace_clamp(shape, chroma, d):
    """dcvc_yuvp_sse: the three sums to rtol 1e-12, the frame clamped in place
    over the whole padded view (values below 0 and above 1) and nothing
    outside it; FrameStage.distortion gives the same sums."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    y, uv = _source(h, w, d, chroma)
    g = np.random.default_rng(w + d)
    xh = torch.from_numpy((g.random((H, W, 3)) * 1.4 - 0.2).astype(np.float32))
    assert xh.min() < 0 and xh.max() > 1
    x = _view(H, W, xh)
    clamped = xh.clamp(0, 1).numpy()
    crop = np.ascontiguousarray(clamped[:h, :w].transpose(2, 0, 1))
    ws = K.frame_sse_workspace(DEV)
    out = torch.zeros(3, dtype=torch.float64, device=DEV)
    K.yuvp_sse(x, _dev(y), _dev(uv), h, w, d, chroma, ws, out)
    ref = C.sse_yuv(crop, y, uv, d, chroma)
    print("sse", chroma, d, out.cpu().numpy(), ref)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=TOL_SSE)
    np.testing.assert_array_equal(x.t().cpu().numpy(), clamped)
    assert _untouched(x)
    if chroma != "420":
        st = _stage(h, w, True, chroma, d)
        a = K.Act(xh.to(DEV))
        st.distortion(a, st.upload((y, uv)), 0)
        assert torch.equal(st.sse[0].view(torch.int64), out.view(torch.int64))
        np.testing.assert_array_equal(a.t().cpu().numpy(), clamped)


@gpu
@pytest.mark.parametrize("from_rgb", [False, True])
@pytest.mark.parametrize("shape,chroma,d", CASES)
def test_recon_to_yuvp_bit_exact(shape, chroma, d, from_rgb):
    """dcvc_recon_to_yuvp from both codec formats: the writer frame (ties,
    values below 0 and above 1) inside a padded offset view, byte for byte."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    fr = _writer_frame(h, w, d)
    full = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(h)) * 1.2 - 0.1
    full[:h, :w] = torch.from_numpy(fr.copy()).permute(1, 2, 0)
    x = _view(H, W, full)
    n = sum(C.frame_sizes(h, w, chroma))
    out = _out_buf(n, d)
    K.recon_to_yuvp(x, h, w, d, chroma, from_rgb, out)
    got, ref = _host(out, d), C.file_frame(fr, d, chroma, from_rgb)
    assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes()
    assert got.max() <= C.max_val(d)
    np.testing.assert_array_equal(x.t().cpu().numpy(), full.numpy())     # the writer leaves the frame alone


@gpu
@pytest.mark.parametrize("shape,d", TWIN_CASES)
def test_420_instantiation_is_bit_equal_to_the_420_kernels(shape, d):
    """Every entry point with (2, 2) against its 4:2:0 twin on the same inputs:
    the definition of that instantiation, the one-column mean4 order included."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    y, uv = _source(h, w, d, "420")
    dy, duv = _dev(y), _dev(uv)
    bits = _bits
    # ---- rule 1
    a, b = _view(H, W), _view(H, W)
    K.yuvp_to_nhwc(dy, duv, h, w, d, "420", a)
    if d == 8:
        K.yuv420_to_nhwc(dy, duv, h, w, b)
    else:
        K.yuv420p16_to_nhwc(dy, duv, h, w, d, b)
    assert torch.equal(bits(a.t()), bits(b.t()))
    # ---- rule 2
    a, b = _view(H, W), _view(H, W)
    pa, pb = torch.empty((3, h, w), device=DEV), torch.empty((3, h, w), device=DEV)
    K.yuvp_to_rgb_nhwc(dy, duv, h, w, d, "420", a, pa)
    if d == 8:
        K.yuv420_to_rgb_nhwc(dy, duv, h, w, b, pb)
    else:
        yf, uvf = torch.empty(h * w, device=DEV), torch.empty(uv.size, device=DEV)
        K.u16_to_f32(dy, d, yf)
        K.u16_to_f32(duv, d, uvf)
        K.yuv420f_to_rgb_nhwc(yf, uvf, h, w, b, pb)
    assert torch.equal(bits(a.t()), bits(b.t())) and torch.equal(bits(pa), bits(pb))
    # ---- rule 3
    g = np.random.default_rng(h + d)
    xh = torch.from_numpy((g.random((H, W, 3)) * 1.4 - 0.2).astype(np.float32))
    a, b = _view(H, W, xh), _view(H, W, xh)
    ws = K.frame_sse_workspace(DEV)
    sa, sb = torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    K.yuvp_sse(a, dy, duv, h, w, d, "420", ws, sa)
    if d == 8:
        K.frame_sse(b, dy, h, w, ws, sb, uv_u8=duv)
    else:
        K.frame16_sse(b, dy, h, w, d, ws, sb, uv_u16=duv)
    print("sse twin", sa.cpu().numpy(), sb.cpu().numpy())
    assert torch.equal(sa.view(torch.int64), sb.view(torch.int64))
    assert torch.equal(bits(a.t()), bits(b.t()))
    # ---- rule 4, both codec formats
    fr = _writer_frame(h, w, d)
    full = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(w)) * 1.2 - 0.1
    full[:h, :w] = torch.from_numpy(fr.copy()).permute(1, 2, 0)
    x = _view(H, W, full)
    n = sum(C.frame_sizes(h, w, "420"))
    for from_rgb in (False, True):
        oa, ob = _out_buf(n, d), _out_buf(n, d)
        K.recon_to_yuvp(x, h, w, d, "420", from_rgb, oa)
        if d == 8 and from_rgb:
            K.recon_to_u8_cross(x, h, w, False, ob)
        elif d == 8:
            K.recon_to_u8(x, h, w, True, ob)
        elif from_rgb:
            K.recon_to_u16_cross(x, h, w, d, False, ob)
        else:
            K.recon_to_u16(x, h, w, d, True, ob)
        assert torch.equal(oa, ob), from_rgb


@gpu
def test_entry_points_reject_bad_arguments():
    """Every DCVC_HIP_EINVAL condition; every buffer is real and large enough
    for the call as made.  The wrappers raise."""
    _need_gpu()
    from dcvc_amd import hip as K
    from dcvc_amd._native import NativeError
    L, st = K.lib(), K.stream()
    h, w, H, W = 6, 8, 16, 16
    x = torch.zeros((H, W, 8), dtype=torch.float32, device=DEV)
    s = torch.zeros(4096, dtype=torch.int16, device=DEV)
    f32 = torch.zeros(3 * H * W, dtype=torch.float32, device=DEV)
    ws, out3 = K.frame_sse_workspace(DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    X, S, Fp, WS, O3 = x.data_ptr(), s.data_ptr(), f32.data_ptr(), ws.data_ptr(), out3.data_ptr()
    good = (X, H, W, 8, 2)
    bad_views = [(None, H, W, 8, 2), (X, H, W, 8, 6), (X, H, W, 8, -1), (X, 0, W, 8, 2), (X, H, 0, 8, 2),
                 (X, 4, W, 8, 2), (X, H, 6, 8, 2)]                         # the last two: smaller than the frame
    EINVAL = -1                                                           # DCVC_HIP_EINVAL (dcvc_hip.h)

    def calls(v, d, hh, ww, sx, sy, y=S, uv=S, dst=S, planes=Fp, wsp=WS, o3=O3):
        return {
            "to_nhwc": lambda: L.dcvc_yuvp_to_nhwc(y, uv, hh, ww, d, sx, sy, *v, st),
            "to_rgb": lambda: L.dcvc_yuvp_to_rgb_nhwc(y, uv, hh, ww, d, sx, sy, *v, planes, st),
            "sse": lambda: L.dcvc_yuvp_sse(*v, y, uv, hh, ww, d, sx, sy, wsp, o3, st),
            "recon": lambda: L.dcvc_recon_to_yuvp(*v, hh, ww, d, sx, sy, 0, dst, st),
            "recon rgb": lambda: L.dcvc_recon_to_yuvp(*v, hh, ww, d, sx, sy, 1, dst, st),
        }
    for sx, sy in ((1, 1), (2, 1), (2, 2)):
        for d in (8, 9, 16):
            for name, fn in calls(good, d, h, w, sx, sy).items():
                assert fn() == 0, (name, sx, sy, d)                       # the call as made is valid
        for v in bad_views:
            for name, fn in calls(v, 10, h, w, sx, sy).items():
                assert fn() == EINVAL, (name, v)
        for d in (7, 17, 0, -1):
            for name, fn in calls(good, d, h, w, sx, sy).items():
                assert fn() == EINVAL, (name, d)
        for kw in ({"y": None}, {"uv": None}, {"dst": None}, {"planes": None}, {"wsp": None}, {"o3": None}):
            used = {"y": ("to_nhwc", "to_rgb", "sse"), "uv": ("to_nhwc", "to_rgb", "sse"),
                    "dst": ("recon", "recon rgb"), "planes": ("to_rgb",), "wsp": ("sse",), "o3": ("sse",)}
            for name, fn in calls(good, 10, h, w, sx, sy, **kw).items():
                if name in used[next(iter(kw))]:
                    assert fn() == EINVAL, (name, kw)
        for hh, ww in ((5, 8), (6, 7), (0, 8), (6, 0), (-2, 8)):
            ok = hh > 0 and ww > 0 and hh % sy == 0 and ww % sx == 0
            for name, fn in calls(good, 10, hh, ww, sx, sy).items():
                assert fn() == (0 if ok else EINVAL), (name, hh, ww, sx, sy)
    for sx, sy in ((1, 2), (0, 1), (2, 0), (3, 1), (4, 2), (-1, 1)):
        for name, fn in calls(good, 10, h, w, sx, sy).items():
            assert fn() == EINVAL, (name, sx, sy)
    torch.cuda.synchronize()
    act = K.Act(x, 2, 3)
    with pytest.raises(NativeError):                                      # a view smaller than the frame
        K.yuvp_to_nhwc(s[:32 * 32], s[:2 * 32 * 32], 32, 32, 10, "444", act)
    with pytest.raises(ValueError):
        K.yuvp_to_nhwc(s[:48], s[:48], 6, 8, 10, "411", act)
    with pytest.raises(AssertionError):
        K.yuvp_to_nhwc(s[:48], s[:47], 6, 8, 10, "422", act)              # a plane of the wrong size
    with pytest.raises(AssertionError):
        K.yuvp_to_nhwc(s[:48], s[:48], 6, 8, 8, "422", act)               # 2-byte samples at 8 bits


# ------------------------------------------------------------ end to end
def _nets(dc_golden):
    from tests.test_frame16 import _nets as n
    return n(dc_golden)


@pytest.fixture(scope="module")
def nets(dc_golden):
    _need_gpu()
    return _nets(dc_golden)


def _capture_distortion(monkeypatch):
    """Every frame FrameStage.distortion has clamped, as (H, W, 3) float32
    numpy, with the three sums it wrote."""
    from dcvc_amd import harness
    from dcvc_amd.dc.video_model import as_act
    seen, orig = [], harness.FrameStage.distortion

    def distortion(self, recon, dframe, slot):
        orig(self, recon, dframe, slot)
        seen.append((as_act(recon).t().float().cpu().numpy().copy(), self.sse[slot].cpu().numpy().copy()))
    monkeypatch.setattr(harness.FrameStage, "distortion", distortion)
    return seen


def _tied_sources(h, w, n):
    """An 8-bit 4:2:0 source and the 4:4:4 and 4:2:2 sources that give the
    codec the same padded input: uv444 = zoom0(uv); the 4:2:2 chroma rows taken
    through zoom0's row index map only."""
    from dcvc_amd.synth import moving_pattern_yuv420
    f420 = [moving_pattern_yuv420(h, w, t, seed=5) for t in range(n)]
    f444 = [(y, np.ascontiguousarray(R.zoom0(uv))) for y, uv in f420]
    f422 = [(y, np.ascontiguousarray(uv[:, C.zoom_index(h // 2), :])) for y, uv in f420]
    assert f444[0][1].shape == (2, h, w) and f422[0][1].shape == (2, h, w // 2)
    return {"420": f420, "444": f444, "422": f422}


def _crop(r, h, w):
    return np.ascontiguousarray(r[:h, :w].transpose(2, 0, 1))


@gpu
def test_run_test_ties_444_and_422_sources_to_the_420_path(nets, monkeypatch):
    """DC YUV codec, split precision, 100 x 130, I + 2 P: the three tied
    sources give identical per-frame bits and luma PSNR; chroma PSNR is measured
    at each source's own resolution and equals the restatement's value on the
    product's own reconstruction."""
    from dcvc_amd.harness import run_test, ArrayReader, calc_psnr_from_sse
    inet, pnet = nets
    h, w, H, W, n = 100, 130, 112, 144, 3
    src = _tied_sources(h, w, n)
    x420 = HO.yuv_u8_to_input(*src["420"][0], H, W)
    logs = {}
    for chroma in ("420", "444", "422"):
        np.testing.assert_array_equal(C.ingest_yuv(*src[chroma][0], 8, chroma, H, W), x420)
        seen = _capture_distortion(monkeypatch)
        with tempfile.TemporaryDirectory() as td:
            logs[chroma] = run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True,
                                                 "bin_folder": td, "src_reader": ArrayReader(src[chroma]),
                                                 "src_type": "yuv" + chroma, "src_height": h, "src_width": w,
                                                 "dist_in_yuv420": True, "q_in_ckpt": False, "i_frame_q_index": 0,
                                                 "verbose": 1})
        monkeypatch.undo()
        assert len(seen) == n
        sx, sy = C.sub(chroma)
        for t, (r, sums) in enumerate(seen):
            ref = C.sse_yuv(_crop(r, h, w), *src[chroma][t], 8, chroma)
            print("tie", chroma, t, sums, ref, logs[chroma]["frame_bpp"][t])
            np.testing.assert_allclose(sums, ref, rtol=TOL_SSE)
            nc = (h // sy) * (w // sx)
            assert logs[chroma]["frame_psnr_u"][t] == calc_psnr_from_sse(sums[1], nc)
            assert logs[chroma]["frame_psnr_v"][t] == calc_psnr_from_sse(sums[2], nc)
            assert logs[chroma]["frame_psnr_y"][t] == calc_psnr_from_sse(sums[0], h * w)
    for chroma in ("444", "422"):
        assert logs[chroma]["frame_bpp"] == logs["420"]["frame_bpp"], chroma
        assert logs[chroma]["frame_psnr_y"] == logs["420"]["frame_psnr_y"], chroma
        assert logs[chroma]["frame_type"] == [0, 1, 1]
        assert set(logs[chroma]) == set(logs["420"])                     # the log's keys are unchanged


@gpu
def test_encode_video_ties_444_and_422_sources_to_the_420_path(nets, tmp_path):
    """encode_video of the three tied sources: identical payload bytes, twin
    flags and digests, record by record."""
    from dcvc_amd.harness import encode_video, ArrayReader
    from dcvc_amd.sequence import SequenceReader
    inet, pnet = nets
    h, w, n = 100, 130, 3
    src = _tied_sources(h, w, n)
    recs, raw, logs = {}, {}, {}
    for chroma in ("420", "444", "422"):
        p = str(tmp_path / f"s{chroma}.seq")
        logs[chroma] = encode_video(inet, pnet, {"frame_num": n, "gop_size": 32, "seq_path": p,
                                                 "src_reader": ArrayReader(src[chroma]), "src_type": "yuv" + chroma,
                                                 "src_height": h, "src_width": w, "dist_in_yuv420": True,
                                                 "q_in_ckpt": False, "i_frame_q_index": 0, "verbose": 1})
        with SequenceReader(p) as r:
            recs[chroma] = list(r)
        raw[chroma] = open(p, "rb").read()
    for chroma in ("444", "422"):
        assert recs[chroma] == recs["420"] and all(r["digest"] is not None for r in recs[chroma])
        assert raw[chroma] == raw["420"]                                  # the file does not record the layout
        assert logs[chroma]["frame_bits"] == logs["420"]["frame_bits"]
        assert logs[chroma]["frame_psnr_y"] == logs["420"]["frame_psnr_y"]


def _native_frames(h, w, n, d, chroma):
    """A source that is not derived from 4:2:0: the moving pattern's three
    channels as Y, U, V samples (U, V decimated along x for 4:2:2), with the low
    bits in use above 8 bits."""
    from dcvc_amd.synth import moving_pattern
    from tests.test_frame16 import _deepen
    sx, _ = C.sub(chroma)
    out = []
    for t in range(n):
        f = moving_pattern(h, w, t, seed=5)
        f = _deepen(f, d) if d > 8 else f
        out.append((np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1:3, :, ::sx])))
    return out


def _write_yuv(path, frames, d):
    dt = np.dtype(np.uint8) if d == 8 else np.dtype("<u2")
    with open(path, "wb") as f:
        f.write(b"".join(y.astype(dt).tobytes() + uv.astype(dt).tobytes() for y, uv in frames))
    return dt


@gpu
def test_run_test_10_bit_yuv444_source_matches_oracle(dc_golden, nets, tmp_path, monkeypatch):
    """A native 10-bit 4:4:4 .yuv file on the DC YUV codec: bits, PSNR_y / u /
    v and their 6:1:1 mean against the oracle codec fed the restatement's
    input, at the parity bars, and out.yuv bit-equal to the restatement's
    quantisation of the product's reconstruction."""
    from dcvc_amd.harness import run_test
    from tests.test_crossfmt import _oracle
    from tests.test_frame16 import _capture_recons
    from tests.test_gpu_model_dc import PARITY_TOL
    inet, pnet = nets
    h, w, H, W, n, q, d = 100, 130, 112, 144, 3, 0, 10
    frames = _native_frames(h, w, n, d, "444")
    _write_yuv(tmp_path / "src.yuv", frames, d)
    recons = _capture_recons(monkeypatch)
    os.makedirs(tmp_path / "bins")
    log = run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True,
                                "bin_folder": str(tmp_path / "bins"),
                                "src_type": "yuv444", "src_path": str(tmp_path / "src"), "src_bit_depth": d,
                                "src_height": h, "src_width": w, "dist_in_yuv420": True, "q_in_ckpt": False,
                                "i_frame_q_index": q, "verbose": 1, "save_decoded_frame": True,
                                "recon_path": str(tmp_path / "rec" / "cur"), "rate_idx": 0})
    xs = [C.ingest_yuv(y, uv, d, "444", H, W) for y, uv in frames]
    ref = _oracle(dc_golden, xs, h, w, q)
    for t, (bits, rec) in enumerate(ref):
        y, uv = C.to_float(frames[t][0], d), C.to_float(frames[t][1], d)
        rec = np.clip(rec, 0, 1)
        py = HO.calc_psnr(y, rec[0], data_range=1)
        pu = HO.calc_psnr(uv[0], rec[1], data_range=1)
        pv = HO.calc_psnr(uv[1], rec[2], data_range=1)
        print("yuv444", t, log["frame_bpp"][t] * h * w, bits, log["frame_psnr_y"][t], py, log["frame_psnr_u"][t], pu)
        assert abs(log["frame_bpp"][t] * h * w - bits) / bits <= PARITY_TOL["bits_rel"], (t, log["frame_bpp"][t], bits)
        assert abs(log["frame_psnr_y"][t] - py) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr_u"][t] - pu) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr_v"][t] - pv) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr"][t] - (6 * py + pu + pv) / 8) <= PARITY_TOL["psnr_db"], t
    (folder,) = [e for e in os.listdir(tmp_path / "rec")]
    data = np.fromfile(tmp_path / "rec" / folder / "out.yuv", dtype="<u2")
    fs = 3 * h * w
    assert data.size == n * fs and len(recons) == n
    for t, r in enumerate(recons):
        np.testing.assert_array_equal(data[t * fs:(t + 1) * fs], C.file_frame(_crop(r, h, w), d, "444"))


@gpu
@pytest.mark.parametrize("d", [8, 10])
@pytest.mark.parametrize("chroma", ["444", "422"])
def test_run_test_new_sources_on_the_rgb_codec(nets, tmp_path, monkeypatch, chroma, d):
    """4:4:4 and 4:2:2 files on the DC RGB codec: the sums equal the
    restatement's against the restatement's converted source (rtol 1e-12) and
    the PSNR is psnr_rgb of them; out.yuv, written back in the source's layout
    and depth, equals the restatement of rule 4."""
    from dcvc_amd.harness import run_test, psnr_rgb
    inet, pnet = nets
    h, w, H, W, n = 100, 130, 112, 144, 2
    frames = _native_frames(h, w, n, d, chroma)
    dt = _write_yuv(tmp_path / "src.yuv", frames, d)
    seen = _capture_distortion(monkeypatch)
    os.makedirs(tmp_path / "bins")
    log = run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True,
                                "bin_folder": str(tmp_path / "bins"),
                                "src_type": "yuv" + chroma, "src_path": str(tmp_path / "src"), "src_bit_depth": d,
                                "src_height": h, "src_width": w, "dist_in_yuv420": False, "q_in_ckpt": False,
                                "i_frame_q_index": 0, "verbose": 1, "save_decoded_frame": True,
                                "recon_path": str(tmp_path / "rec" / "cur"), "rate_idx": 0})
    assert "frame_psnr_y" not in log and len(seen) == n
    (folder,) = [e for e in os.listdir(tmp_path / "rec")]
    data = np.fromfile(tmp_path / "rec" / folder / "out.yuv", dtype=dt)
    fs = sum(C.frame_sizes(h, w, chroma))
    assert data.size == n * fs
    for t, (r, sums) in enumerate(seen):
        crop = _crop(r, h, w)
        ref = F.sse_rgb(crop, C.ingest_rgb(*frames[t], d, chroma, H, W)[1])
        print("rgb codec", chroma, d, t, sums, ref, log["frame_psnr"][t])
        np.testing.assert_allclose(sums, ref, rtol=TOL_SSE)
        assert log["frame_psnr"][t] == psnr_rgb(sums, h, w)
        np.testing.assert_array_equal(data[t * fs:(t + 1) * fs], C.file_frame(crop, d, chroma, from_rgb=True))


@gpu
def test_encode_video_decode_video_422_at_10_bits(dc_golden, nets, tmp_path, monkeypatch):
    """encode_video -> file -> decode_video with separately built codecs from
    a real 10-bit 4:2:2 file: every digest verifies, the decoder's out.yuv has
    the 4:2:2 frame size and equals the restatement's quantisation of the
    ENCODER's reconstruction."""
    from dcvc_amd import harness
    from dcvc_amd.sequence import SequenceReader
    inet, pnet = nets
    h, w, n, d = 100, 130, 3, 10
    frames = _native_frames(h, w, n, d, "422")
    _write_yuv(tmp_path / "src.yuv", frames, d)
    seen = _capture_distortion(monkeypatch)
    seq = str(tmp_path / "a.seq")
    base = {"dist_in_yuv420": True, "src_type": "yuv422", "seq_path": seq}
    elog = harness.encode_video(inet, pnet, dict(base, frame_num=n, gop_size=32, src_path=str(tmp_path / "src.yuv"),
                                                 src_bit_depth=d, src_height=h, src_width=w, q_in_ckpt=False,
                                                 i_frame_q_index=0))
    with SequenceReader(seq) as r:
        assert r.bit_depth == d and r.frames == n and all(rec["digest"] is not None for rec in r)
    dlog = harness.decode_video(*_nets(dc_golden), dict(base, save_decoded_frame=True,
                                                        recon_path=str(tmp_path / "rec")))
    assert dlog["bit_depth"] == d and dlog["frame_bits"] == elog["frame_bits"] and len(seen) == n
    data = np.fromfile(tmp_path / "rec" / "out.yuv", dtype="<u2")
    fs = h * w + 2 * h * (w // 2)
    assert data.size == n * fs
    for t, (r, _) in enumerate(seen):
        np.testing.assert_array_equal(data[t * fs:(t + 1) * fs], C.file_frame(_crop(r, h, w), d, "422"))


@gpu
def test_command_line_round_trips_a_10_bit_422_file(dc_golden, tmp_path):
    """python -m dcvc_amd.sequence encode --src_type yuv422 --bit-depth 10,
    then decode: the decoded file has the source's size and depth."""
    _need_gpu()
    from dcvc_amd import sequence
    h, w, n, d = 100, 130, 2, 10
    _write_yuv(tmp_path / "src.yuv", _native_frames(h, w, n, d, "422"), d)
    torch.save(dc_golden.i_state_dict(), tmp_path / "i.pth")
    torch.save(dc_golden.p_state_dict(), tmp_path / "p.pth")
    common = ["--i_frame_model_path", str(tmp_path / "i.pth"), "--p_frame_model_path", str(tmp_path / "p.pth"),
              "--seq_path", str(tmp_path / "a.seq"), "--src_type", "yuv422", "--yuv420"]
    sequence.main(["encode"] + common + ["--src_path", str(tmp_path / "src.yuv"), "--src_width", str(w),
                                         "--src_height", str(h), "--frame_num", str(n), "--q_index", "0",
                                         "--bit-depth", "10"])
    with sequence.SequenceReader(str(tmp_path / "a.seq")) as r:
        assert r.bit_depth == 10 and r.frames == n
    sequence.main(["decode"] + common + ["--recon_path", str(tmp_path / "rec")])
    out = tmp_path / "rec" / "out.yuv"
    assert os.path.getsize(out) == os.path.getsize(tmp_path / "src.yuv") == n * 2 * (h * w + 2 * h * (w // 2))
    assert np.fromfile(out, dtype="<u2").max() <= 1023
