"""High-bit-depth frames: 9..16-bit raw RGB and YUV420 sources and output
(INTEGRATION.md "High-bit-depth frames", frame16.hip).

CPU tests pin the numpy restatement (tests/frame16_ref.py) to what the
reference's own RGBReader / RGBWriter and functional.py produced
(tests/golden/frame16_golden.*, recorded by make_golden_frame16.py), and check
the readers, the sequence header's bit-depth field and the argument errors.
GPU tests hold every new kernel bit-equal to the restatement, the squared-error
sums and MS-SSIM to the bars of their 8-bit twins (tests/test_harness.py,
tests/test_crossfmt.py), a 16-bit source equal to v * 257 of an 8-bit one to the
8-bit path bit for bit, and 10-bit sources end to end against the oracle codec
on the restatement's converted input."""
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
import torch

from oracle import harness_oracle as HO
from tests import crossfmt_ref as R
from tests import frame16_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ["dcvc_frame16_to_nhwc", "dcvc_yuv420p16_to_nhwc", "dcvc_frame16_sse", "dcvc_recon_to_u16",
               "dcvc_recon_to_u16_cross", "dcvc_u16_to_f32", "dcvc_yuv420f_to_rgb_nhwc", "dcvc_rgbf_to_yuv420_planes"]
# (h, w, H, W) of tests/test_crossfmt.py: the degenerate 2-pixel zoom axes; odd
# half-planes (19 x 27) with padding on both axes; more than one block
SHAPES = [(2, 2, 16, 16), (38, 54, 48, 64), (100, 130, 112, 144)]
DEPTHS = (10, 12, 16)
TOL_SSE = 1e-12       # tests/test_harness.py test_frame_sse_and_inplace_clamp (rtol)
TOL_MSSSIM = 1e-10    # tests/test_harness.py test_run_test_yuv420_msssim (atol)
CASES = [(s, d) for s in SHAPES for d in DEPTHS]


@functools.lru_cache(maxsize=None)
def _fixture():
    spec = importlib.util.spec_from_file_location("make_golden_frame16", os.path.join(GOLDEN, "make_golden_frame16.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with open(os.path.join(GOLDEN, "frame16_golden.json")) as f:
        cases = {(c["h"], c["w"], c["depth"]): c for c in json.load(f)["cases"]}
    return m, cases, np.load(os.path.join(GOLDEN, "frame16_golden.npz"))


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _case(h, w, H, W, d):
    """The fixture's uint16 inputs of one shape and depth, the writers' float
    frame, and the restatement's conversions of them, computed once and
    shared; no test writes to them."""
    m, cases, _ = _fixture()
    seed = cases[(h, w, d)]["seed"]
    y16, uv16, rgb16 = m.inputs(seed, h, w, d)
    x_cross_rgb, rgb_c = F.ingest_yuv_source_rgb_codec(y16, uv16, d, H, W)
    x_cross_yuv, y_c, uv_c = F.ingest_rgb_source_yuv_codec(rgb16, d, H, W)
    return {"y16": y16, "uv16": uv16, "rgb16": rgb16, "fr": m.writer_inputs(seed, h, w, d),
            "x_rgb": F.ingest_rgb(rgb16, d, H, W), "x_rgb_zero": F.ingest_rgb(rgb16, d, H, W, zero_pad=True),
            "x_yuv": F.ingest_yuv(y16, uv16, d, H, W), "x_cross_rgb": x_cross_rgb, "rgb_c": rgb_c,
            "x_cross_yuv": x_cross_yuv, "y_c": y_c, "uv_c": uv_c}


# --------------------------------------------------------------------- CPU
@pytest.mark.parametrize("shape,d", CASES)
def test_restatement_reproduces_reference_fixture(shape, d):
    """tests/frame16_ref.py against the reference's RGBReader / RGBWriter and
    functional.py outputs: every digest, and the stored arrays of the two small
    shapes.  The same-format 4:4:4 -> 4:2:0 writer is defined with the pairwise
    block sum at every width; numpy sums a one-column chroma plane (w = 2)
    sequentially, so that row is pinned at the wider shapes."""
    h, w, H, W = shape
    _, cases, arrays = _fixture()
    c, k = cases[(h, w, d)], _case(*shape, d)
    mx = F.max_val(d)
    for a in (k["y16"], k["rgb16"]):
        assert 0 in a and mx in a and mx - 1 in a
    assert d == 16 or (k["rgb16"].max() > mx and k["y16"].max() > mx)      # unclamped on the way in
    fr = k["fr"]
    assert fr.min() < 0 and fr.max() > 1
    prod = fr.astype(np.float64) * mx                                      # ties: within an fp32 ulp of k + 0.5
    near = np.abs(prod - np.floor(prod) - 0.5) <= np.spacing(np.float32(prod)).astype(np.float64)
    assert near.sum() >= 6 and (prod[near] > np.floor(prod[near]) + 0.5).any() and \
        (prod[near] < np.floor(prod[near]) + 0.5).any()
    got = {"rgb": F.to_float(k["rgb16"], d), "rgb_to_y": k["y_c"][None], "rgb_to_uv": k["uv_c"],
           "rgb_to_yuv444": k["x_cross_yuv"][:h, :w].transpose(2, 0, 1),
           "yuv444": k["x_yuv"][:h, :w].transpose(2, 0, 1), "yuv_to_rgb": k["rgb_c"],
           "w_rgb": F.rgb_file_frame(fr, d), "w_rgb_from_444": F.rgb_file_frame_from_444(fr, d),
           "w_yuv_from_rgb": F.yuv_file_frame_from_rgb(fr, d)}
    if w > 2:
        got["w_yuv"] = F.yuv_file_frame(fr, d)
    for name, a in got.items():
        assert _digest(a) == c[name], name
        key = f"{name}_{h}x{w}_{d}"
        if key in arrays:
            np.testing.assert_array_equal(np.ascontiguousarray(a), arrays[key], err_msg=name)
    np.testing.assert_array_equal(k["x_rgb"][:h, :w].transpose(2, 0, 1), got["rgb"])


def test_eight_bit_values_scale_exactly():
    """float32(v * 257) / float32(65535) == float32(v) / float32(255) for all
    256 values: both are the correctly rounded quotient of the same real
    number.  The 16-bit-against-8-bit GPU tests lean on it."""
    v = np.arange(256, dtype=np.uint16)
    a = (v * 257).astype(np.float32) / np.float32(65535)
    b = v.astype(np.float32) / np.float32(255)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(F.to_float((v * 257).astype(np.uint16), 16), R.u8_to_float(v.astype(np.uint8)))


def test_header_declares_and_library_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "dcvc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dcvc_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared, sorted(set(NEW_SYMBOLS) - declared)
    lib = ctypes.CDLL(os.path.join(ROOT, "dcvc_amd", "lib", "libdcvc_hip.so"))
    assert not [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    from dcvc_amd import hip
    assert set(NEW_SYMBOLS) <= {s[0] for s in hip.HIP_SYMBOLS}
    assert set(hip.SCALAR_VIEW_SYMBOLS) <= set(NEW_SYMBOLS)


@pytest.mark.parametrize("d", [8, 10, 16])
def test_rgb_reader_reads_raw_planar_files(tmp_path, d):
    """RGBReader on a real file: '.rgb' appended to the name, frame size,
    little-endian uint16 above 8 bits, a short last frame is the end, and the
    end is sticky."""
    from dcvc_amd.harness import RGBReader
    h, w = 4, 6
    g = np.random.default_rng(d)
    dt = np.uint8 if d == 8 else np.uint16
    frames = [g.integers(0, 1 << d, (3, h, w)).astype(dt) for _ in range(2)]
    frames[0][0, 0, 0] = 0x12 if d == 8 else 0x0102
    raw = b"".join(f.astype("<u2" if d > 8 else np.uint8).tobytes() for f in frames)
    with open(tmp_path / "seq.rgb", "wb") as f:
        f.write(raw + raw[:7])                          # a third frame cut short
    size = 3 * h * w * (2 if d > 8 else 1)
    assert len(raw) == 2 * size
    if d > 8:
        assert raw[:2] == b"\x02\x01"                   # low byte first
    for name in ("seq", "seq.rgb"):
        r = RGBReader(str(tmp_path / name), w, h, bit_depth=d)
        assert r.src_path.endswith("seq.rgb") and r.rgb_size == size
        for f in frames:
            got = r.read_one_frame(dst_format="420")    # the native planes whatever the codec wants
            assert got.dtype == dt and got.shape == (3, h, w)
            np.testing.assert_array_equal(got, f)
        assert r.read_one_frame() is None and r.eof and r.read_one_frame() is None
        r.close()
    with pytest.raises(ValueError):
        RGBReader(str(tmp_path / "seq"), w, h, bit_depth=7)
    with pytest.raises(ValueError):
        RGBReader(str(tmp_path / "seq"), w, h, bit_depth=17)
    r = RGBReader(str(tmp_path / "seq"), w, h, bit_depth=d)
    with pytest.raises(ValueError):
        r.read_one_frame(dst_format="444")
    r.close()


def test_yuv_reader_reads_16_bit_planes(tmp_path):
    """YUVReader(bit_depth=10): uint16 planes, doubled frame and skip sizes,
    little-endian, a short last frame is the end."""
    from dcvc_amd.harness import YUVReader
    h, w = 4, 6
    g = np.random.default_rng(3)
    frames = [(g.integers(0, 1024, (h, w)).astype(np.uint16),
               g.integers(0, 1024, (2, h // 2, w // 2)).astype(np.uint16)) for _ in range(3)]
    frames[1][0][0, 0] = 0x0302
    raw = [y.astype("<u2").tobytes() + uv.astype("<u2").tobytes() for y, uv in frames]
    assert all(len(b) == h * w * 3 for b in raw)        # 2 bytes x 1.5 samples per pixel
    with open(tmp_path / "seq.yuv", "wb") as f:
        f.write(b"".join(raw) + raw[0][:h * w * 2 + 3])  # a fourth frame whose chroma is cut short
    r = YUVReader(str(tmp_path / "seq"), w, h, skip_frame=1, bit_depth=10)
    assert (r.y_size, r.uv_size) == (2 * h * w, h * w)
    y, uv = r.read_one_frame(dst_format="rgb")
    assert y.dtype == np.uint16 and uv.dtype == np.uint16 and y[0, 0] == 0x0302
    np.testing.assert_array_equal(y, frames[1][0])
    np.testing.assert_array_equal(uv, frames[1][1])
    y, uv = r.read_one_frame()
    np.testing.assert_array_equal(uv, frames[2][1])
    assert r.read_one_frame() == (None, None) and r.read_one_frame() == (None, None)
    r.close()
    r8 = YUVReader(str(tmp_path / "seq"), w, h)          # the 8-bit reader of the same bytes: half the frame size
    assert (r8.y_size, r8.uv_size) == (h * w, h * w // 2) and r8.read_one_frame()[0].dtype == np.uint8
    r8.close()
    with pytest.raises(ValueError):
        YUVReader(str(tmp_path / "seq"), 5, 4, bit_depth=10)
    with pytest.raises(ValueError):
        YUVReader(str(tmp_path / "seq"), w, h, bit_depth=17)


def test_array_reader_hands_over_uint16_frames():
    from dcvc_amd.harness import ArrayReader
    f = np.arange(24, dtype=np.uint16).reshape(3, 2, 4)
    r = ArrayReader([f])
    assert r.read_one_frame() is f and r.read_one_frame() is None


@pytest.mark.parametrize("d,field,shown", [(0, 0, 8), (8, 0, 8), (10, 10, 10), (16, 16, 16)])
def test_sequence_header_carries_the_bit_depth(tmp_path, d, field, shown):
    from dcvc_amd.sequence import SequenceReader, SequenceWriter
    p = str(tmp_path / "a.seq")
    with SequenceWriter(p, "DC", "yuv420", "split", 130, 100, bit_depth=d) as wr:
        wr.write("I", b"abc", digest=(1, 2))
    data = open(p, "rb").read()
    assert struct.unpack("<H", data[26:28]) == (field,)
    with SequenceReader(p) as r:
        assert r.bit_depth == shown and (r.width, r.height, r.frames) == (130, 100, 1)
        assert [x["payload"] for x in r] == [b"abc"]


@pytest.mark.parametrize("d", [7, 17])
def test_sequence_header_rejects_other_depths(tmp_path, d):
    from dcvc_amd.sequence import SequenceFormatError, SequenceReader, SequenceWriter
    p = str(tmp_path / "a.seq")
    with pytest.raises(ValueError):
        SequenceWriter(p, "DC", "rgb", "split", 130, 100, bit_depth=d)
    assert not os.path.exists(p)
    SequenceWriter(p, "DC", "rgb", "split", 130, 100).close()
    data = bytearray(open(p, "rb").read())
    data[26:28] = struct.pack("<H", d)
    open(p, "wb").write(bytes(data))
    with pytest.raises(SequenceFormatError):
        SequenceReader(p)


def test_eight_bit_sequence_file_bytes_are_unchanged(tmp_path):
    """An 8-bit SequenceWriter file, with and without the keyword, is the
    documented layout with a zero in the field: the bytes every earlier
    version wrote."""
    from dcvc_amd.sequence import SequenceWriter
    payloads = [("I", b"\x01\x02\x03", False, (5, 6)), ("P", b"", True, None)]
    want = b"DCVCSEQ1" + bytes([1, 0]) + b"split" + b"\0" * 11 + struct.pack("<HIII", 0, 1920, 1080, 2)
    for t, payload, twin, digest in payloads:
        flags = (1 if twin else 0) | (2 if digest else 0)
        want += struct.pack("<BBHIQQ", "IP".index(t), flags, 0, len(payload), *(digest or (0, 0))) + payload
    for kw in ({}, {"bit_depth": 8}, {"bit_depth": 0}):
        p = str(tmp_path / "a.seq")
        with SequenceWriter(p, "HEM", "rgb", "split", 1920, 1080, **kw) as wr:
            for t, payload, twin, digest in payloads:
                wr.write(t, payload, twin=twin, digest=digest)
        assert open(p, "rb").read() == want


def test_python_level_argument_errors(tmp_path):
    """PNG above 8 bits, depths out of range, odd sizes for 4:2:0: a
    ValueError before anything touches the device."""
    from dcvc_amd import hip as K
    from dcvc_amd.harness import FrameStage, ReconWriter, _bit_depths, _reader
    cpu = torch.device("cpu")
    for kind in ("png", "hem_png"):
        with pytest.raises(ValueError, match="8-bit"):
            ReconWriter(str(tmp_path / "r"), 4, 6, kind, "rgb", cpu, bit_depth=10)
    for d in (7, 17, 10.0, None):
        with pytest.raises(ValueError):
            ReconWriter(str(tmp_path / "r"), 4, 6, "rgb", "rgb", cpu, bit_depth=d)
        with pytest.raises(ValueError):
            FrameStage(4, 6, 16, False, False, 1, cpu, bit_depth=d)
        with pytest.raises(ValueError):
            _bit_depths({"src_bit_depth": d})
    for d in (8, 17, 0):
        with pytest.raises(ValueError):
            K.check_depth(d)
    with pytest.raises(ValueError, match="even"):
        ReconWriter(str(tmp_path / "r"), 5, 6, "yuv", "420", cpu, bit_depth=10)
    with pytest.raises(ValueError, match="even"):
        FrameStage(4, 7, 16, True, False, 1, cpu, bit_depth=10)
    with pytest.raises(ValueError, match="8-bit"):
        _reader({"src_type": "png", "src_path": str(tmp_path), "src_width": 6, "src_height": 4, "src_bit_depth": 10},
                False)
    with pytest.raises(ValueError):
        ReconWriter(str(tmp_path / "r"), 4, 6, "jpg", "rgb", cpu)
    assert not os.path.exists(tmp_path / "r")
    assert _bit_depths({}) == (8, 8) and _bit_depths({"src_bit_depth": 10}) == (10, 10)
    assert _bit_depths({"src_bit_depth": 10, "recon_bit_depth": 8}) == (10, 8)


# --------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev16(a):
    """A uint16 numpy array on the device, as FrameStage uploads it."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def _view(H, W, fill=None):
    """A 3-channel fp32 view with coff 2 inside an (H, W, 8) buffer of NaN."""
    from dcvc_amd import hip as K
    buf = torch.full((H, W, 8), float("nan"), dtype=torch.float32, device=DEV)
    a = K.Act(buf, 2, 3)
    if fill is not None:
        a.t().copy_(fill.to(DEV))
    return a


def _untouched(a):
    """No element outside the view's channels was written."""
    b = a.buf
    return bool(torch.isnan(b[:, :, :a.coff]).all()) and bool(torch.isnan(b[:, :, a.coff + 3:]).all())


def _stage(h, w, yuv420, src_format, d, align=16, zero_pad=False, n=1):
    from dcvc_amd.harness import FrameStage
    return FrameStage(h, w, align, yuv420, zero_pad=zero_pad, frame_num=n, device=DEV, src_format=src_format,
                      bit_depth=d)


@gpu
@pytest.mark.parametrize("shape,d", CASES)
def test_same_format_ingest_bit_exact(shape, d):
    """dcvc_frame16_to_nhwc (both paddings) and dcvc_yuv420p16_to_nhwc, into a
    view with coff 2 of a cstride-8 buffer and through FrameStage."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    k = _case(*shape, d)
    rgb, y, uv = _dev16(k["rgb16"]), _dev16(k["y16"]), _dev16(k["uv16"])
    for zero_pad, ref in ((False, k["x_rgb"]), (True, k["x_rgb_zero"])):
        out = _view(H, W)
        K.frame16_to_nhwc(rgb, h, w, d, out, zero_pad=zero_pad)
        np.testing.assert_array_equal(out.t().cpu().numpy(), ref)
        assert _untouched(out)
    out = _view(H, W)
    K.yuv420p16_to_nhwc(y, uv, h, w, d, out)
    np.testing.assert_array_equal(out.t().cpu().numpy(), k["x_yuv"])
    assert _untouched(out)
    st = _stage(h, w, False, None, d)
    assert (st.H, st.W) == (H, W) and not st.cross and st.src_f32 is None
    np.testing.assert_array_equal(st.load(st.upload(k["rgb16"])).t().cpu().numpy(), k["x_rgb"])
    st = _stage(h, w, True, "420", d)
    np.testing.assert_array_equal(st.load(st.upload((k["y16"], k["uv16"]))).t().cpu().numpy(), k["x_yuv"])


@gpu
@pytest.mark.parametrize("shape,d", CASES)
def test_cross_format_ingest_bit_exact(shape, d):
    """dcvc_u16_to_f32 and the fp32-source twins of the cross-ingest kernels:
    the fp32 planes and the padded input of both directions, directly (offset
    view) and through FrameStage; the fixture's digests."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    _, cases, _ = _fixture()
    c, k = cases[(h, w, d)], _case(*shape, d)
    f32 = torch.full((3 * h * w,), float("nan"), dtype=torch.float32, device=DEV)
    K.u16_to_f32(_dev16(k["rgb16"]), d, f32)
    np.testing.assert_array_equal(f32.cpu().numpy().reshape(3, h, w), F.to_float(k["rgb16"], d))
    yf, uvf = torch.empty(h * w, device=DEV), torch.empty(2 * (h // 2) * (w // 2), device=DEV)
    K.u16_to_f32(_dev16(k["y16"]), d, yf)
    K.u16_to_f32(_dev16(k["uv16"]), d, uvf)
    out, planes = _view(H, W), torch.full((3, h, w), float("nan"), dtype=torch.float32, device=DEV)
    K.yuv420f_to_rgb_nhwc(yf, uvf, h, w, out, planes)
    np.testing.assert_array_equal(out.t().cpu().numpy(), k["x_cross_rgb"])
    np.testing.assert_array_equal(planes.cpu().numpy(), k["rgb_c"])
    assert _untouched(out)
    st = _stage(h, w, False, "420", d)                   # a YUV420 source for an RGB codec
    assert st.cross
    x = st.load(st.upload((k["y16"], k["uv16"])))
    np.testing.assert_array_equal(x.t().cpu().numpy(), k["x_cross_rgb"])
    np.testing.assert_array_equal(st.src_f32[0].cpu().numpy(), k["rgb_c"])
    assert _digest(st.src_f32[0].cpu().numpy()) == c["yuv_to_rgb"]
    st = _stage(h, w, True, "rgb", d)                    # an RGB source for a YUV420 codec
    x = st.load(st.upload(k["rgb16"]))
    ys, uvs = st.src_f32[0].cpu().numpy(), st.src_f32[1].cpu().numpy()
    np.testing.assert_array_equal(x.t().cpu().numpy(), k["x_cross_yuv"])
    np.testing.assert_array_equal(ys, k["y_c"])
    np.testing.assert_array_equal(uvs, k["uv_c"])
    assert _digest(ys[None]) == c["rgb_to_y"] and _digest(uvs) == c["rgb_to_uv"]


@gpu
@pytest.mark.parametrize("shape,d", CASES)
def test_recon_to_u16_bit_exact(shape, d):
    """The four cases of ReconWriter: the fixture's writer frame (ties, values
    below 0 and above 1) inside a padded offset view, against the restatement
    and the reference's recorded files."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    _, cases, _ = _fixture()
    c, k = cases[(h, w, d)], _case(*shape, d)
    fr = torch.from_numpy(k["fr"])
    full = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(h)) * 1.2 - 0.1
    full[:h, :w] = fr.permute(1, 2, 0)
    x = _view(H, W, full)
    n_rgb, n_yuv = 3 * h * w, h * w + 2 * (h // 2) * (w // 2)
    for fn, flag, n, ref, name in ((K.recon_to_u16, False, n_rgb, F.rgb_file_frame(k["fr"], d), "w_rgb"),
                                   (K.recon_to_u16, True, n_yuv, F.yuv_file_frame(k["fr"], d), "w_yuv"),
                                   (K.recon_to_u16_cross, True, n_rgb, F.rgb_file_frame_from_444(k["fr"], d),
                                    "w_rgb_from_444"),
                                   (K.recon_to_u16_cross, False, n_yuv, F.yuv_file_frame_from_rgb(k["fr"], d),
                                    "w_yuv_from_rgb")):
        out = torch.full((n,), -23131, dtype=torch.int16, device=DEV)
        fn(x, h, w, d, flag, out)
        got = out.cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(got, ref.reshape(-1), err_msg=name)
        assert got.max() <= F.max_val(d)
        if name != "w_yuv" or w > 2:
            assert _digest(got) == c[name], name
    np.testing.assert_array_equal(x.t().cpu().numpy(), full.numpy())       # the writers leave the frame alone


@gpu
@pytest.mark.parametrize("yuv", [False, True])
@pytest.mark.parametrize("shape,d", CASES)
def test_frame16_sse_and_inplace_clamp(shape, d, yuv):
    """dcvc_frame16_sse at the bar of test_frame_sse_and_inplace_clamp: the
    three sums to rtol 1e-12, the frame clamped in place over the whole padded
    view and nothing outside it."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    k = _case(*shape, d)
    g = np.random.default_rng(w + d)
    xh = torch.from_numpy((g.random((H, W, 3)) * 1.4 - 0.2).astype(np.float32))
    x = _view(H, W, xh)
    clamped = xh.clamp(0, 1).numpy()
    crop = np.ascontiguousarray(clamped[:h, :w].transpose(2, 0, 1))
    ws = K.frame_sse_workspace(DEV)
    out = torch.zeros(3, dtype=torch.float64, device=DEV)
    if yuv:
        K.frame16_sse(x, _dev16(k["y16"]), h, w, d, ws, out, uv_u16=_dev16(k["uv16"]))
        ref = F.sse_yuv(crop, F.to_float(k["y16"], d), F.to_float(k["uv16"], d))
    else:
        K.frame16_sse(x, _dev16(k["rgb16"]), h, w, d, ws, out)
        ref = F.sse_rgb(crop, F.to_float(k["rgb16"], d))
    print("sse", out.cpu().numpy(), ref)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=TOL_SSE)
    np.testing.assert_array_equal(x.t().cpu().numpy(), clamped)
    assert _untouched(x)


@gpu
def test_msssim_of_16_bit_sources():
    """MS-SSIM is fed the converted source through run_f32.  YUV420 at 200 x
    256, 10 bits: the bar of test_run_test_yuv420_msssim against the oracle's
    calc_msssim.  RGB: on a 16-bit source equal to v * 257 the values are those
    of the uint8 run."""
    _need_gpu()
    from dcvc_amd import hip as K
    from dcvc_amd.harness import MsSsim, MsSsimRGB
    from dcvc_amd.synth import moving_pattern, moving_pattern_yuv420
    h, w, H, W, d = 200, 256, 208, 256, 10
    y8, uv8 = moving_pattern_yuv420(h, w, 0, seed=9)
    y16, uv16 = _deepen(y8, d), _deepen(uv8, d)
    st = _stage(h, w, True, "420", d)
    dframe = st.upload((y16, uv16))
    x_in = st.load(dframe).t().cpu().numpy()
    np.testing.assert_array_equal(x_in, F.ingest_yuv(y16, uv16, d, H, W))
    g = np.random.default_rng(9)
    xh = torch.from_numpy((x_in + g.normal(0, 0.04, (H, W, 3))).astype(np.float32)).to(DEV)
    src = st.source_f32(dframe)
    y, uv = F.to_float(y16, d), F.to_float(uv16, d)
    np.testing.assert_array_equal(src[0].cpu().numpy(), y)
    np.testing.assert_array_equal(src[1].cpu().numpy(), uv)
    ms = MsSsim(h, w, 1, DEV)
    ms.run_f32(K.Act(xh), *src, 0)
    got = ms.values(1)[0]
    crop = np.ascontiguousarray(np.clip(xh.cpu().numpy()[:h, :w].transpose(2, 0, 1), 0, 1))
    y_rec, uv_rec = F.yuv444_to_420(crop)
    ref = [HO.calc_msssim(y, y_rec[0]), HO.calc_msssim(uv[0], uv_rec[0]), HO.calc_msssim(uv[1], uv_rec[1])]
    print("msssim", got, ref)
    np.testing.assert_allclose(got[:3], ref, rtol=0, atol=TOL_MSSSIM)
    assert abs(got[3] - (6 * ref[0] + ref[1] + ref[2]) / 8) < TOL_MSSSIM
    rgb8 = moving_pattern(h, w, 0, seed=9)
    st = _stage(h, w, False, None, 16)
    dframe = st.upload(rgb8.astype(np.uint16) * 257)
    st.load(dframe)
    a, b = MsSsimRGB(h, w, 1, DEV), MsSsimRGB(h, w, 1, DEV)
    a.run(K.Act(xh), torch.from_numpy(rgb8).to(DEV), 0)
    b.run_f32(K.Act(xh), *st.source_f32(dframe), 0)
    assert a.values(1) == b.values(1)


def _deepen(a8, d):
    """A uint8 array as d-bit samples with the low bits in use (a pattern of
    the position), never above max_val."""
    low = (np.indices(a8.shape).sum(axis=0) * 5 + 1) & ((1 << (d - 8)) - 1)
    return ((a8.astype(np.uint16) << (d - 8)) | low.astype(np.uint16)).astype(np.uint16)


# ------------------------------------------------ 16-bit against 8-bit, same run
def _nets(dc_golden):
    from dcvc_amd.dc import DMC, IntraNoAR
    from dcvc_amd.layers import Precision
    inet = IntraNoAR(precision=Precision.split()).load_state_dict(dc_golden.i_state_dict())
    pnet = DMC(precision=Precision.split()).load_state_dict(dc_golden.p_state_dict())
    inet.update(force=True)
    pnet.update(force=True)
    return inet, pnet


@pytest.fixture(scope="module")
def nets(dc_golden):
    _need_gpu()
    return _nets(dc_golden)


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_16_bit_copy_of_an_8_bit_source_takes_the_same_values(shape):
    """Source = v * 257 at 16 bits: the padded input is torch.equal to the
    8-bit kernel's, in both formats and both paddings, and the squared-error
    sums are equal bit for bit."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    g = np.random.default_rng(h)
    rgb8 = g.integers(0, 256, (3, h, w), dtype=np.uint8)
    y8, uv8 = g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (2, h // 2, w // 2), dtype=np.uint8)
    up = lambda a: a.astype(np.uint16) * 257  # noqa: E731
    xh = torch.from_numpy((g.random((H, W, 3)) * 1.4 - 0.2).astype(np.float32)).to(DEV)
    ws = K.frame_sse_workspace(DEV)
    for yuv, zero_pad, f8, f16 in ((False, False, rgb8, up(rgb8)), (False, True, rgb8, up(rgb8)),
                                   (True, False, (y8, uv8), (up(y8), up(uv8)))):
        fmt = "420" if yuv else "rgb"
        s8, s16 = _stage(h, w, yuv, fmt, 8, zero_pad=zero_pad), _stage(h, w, yuv, fmt, 16, zero_pad=zero_pad)
        d8, d16 = s8.upload(f8), s16.upload(f16)
        assert torch.equal(s8.load(d8).t(), s16.load(d16).t())
        a, b = K.Act(xh.clone()), K.Act(xh.clone())
        s8.distortion(a, d8, 0)
        s16.distortion(b, d16, 0)
        assert torch.equal(s8.sse.view(torch.int64), s16.sse.view(torch.int64)), (s8.sse, s16.sse)
        assert torch.equal(a.t(), b.t())


@gpu
def test_run_test_on_a_16_bit_copy_equals_the_8_bit_run(nets):
    """run_test on the golden DC weights at 100 x 130, I + 2 P: the same bits
    and the same PSNR from the 8-bit frames and from v * 257 at 16 bits."""
    from dcvc_amd.harness import run_test, ArrayReader
    from dcvc_amd.synth import moving_pattern
    inet, pnet = nets
    h, w, n = 100, 130, 3
    frames = [moving_pattern(h, w, t, seed=5) for t in range(n)]
    logs = []
    for depth, fr in ((8, frames), (16, [f.astype(np.uint16) * 257 for f in frames])):
        with tempfile.TemporaryDirectory() as td:
            logs.append(run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True, "bin_folder": td,
                                              "src_reader": ArrayReader(fr), "src_type": "rgb", "src_bit_depth": depth,
                                              "src_height": h, "src_width": w, "dist_in_yuv420": False,
                                              "q_in_ckpt": False, "i_frame_q_index": 0, "verbose": 1}))
    assert logs[0]["frame_bpp"] == logs[1]["frame_bpp"]
    assert logs[0]["frame_psnr"] == logs[1]["frame_psnr"]
    assert logs[0]["i_frame_num"] == 1 and logs[0]["p_frame_num"] == 2


@gpu
def test_sequence_encoder_payloads_do_not_depend_on_the_depth(nets, tmp_path):
    """encode_video of the 8-bit frames and of v * 257 at 16 bits: the same
    payloads and digests record by record; only the header's field differs."""
    from dcvc_amd.harness import encode_video, ArrayReader
    from dcvc_amd.sequence import SequenceReader
    from dcvc_amd.synth import moving_pattern
    inet, pnet = nets
    h, w, n = 100, 130, 3
    frames = [moving_pattern(h, w, t, seed=5) for t in range(n)]
    recs, raw = [], []
    for depth, fr in ((8, frames), (16, [f.astype(np.uint16) * 257 for f in frames])):
        p = str(tmp_path / f"s{depth}.seq")
        encode_video(inet, pnet, {"frame_num": n, "gop_size": 32, "seq_path": p, "src_reader": ArrayReader(fr),
                                  "src_type": "rgb", "src_bit_depth": depth, "src_height": h, "src_width": w,
                                  "dist_in_yuv420": False, "q_in_ckpt": False, "i_frame_q_index": 0})
        with SequenceReader(p) as r:
            assert r.bit_depth == depth
            recs.append(list(r))
        raw.append(open(p, "rb").read())
    assert recs[0] == recs[1] and all(r["digest"] is not None for r in recs[0])
    assert raw[0][26:28] == b"\0\0" and raw[1][26:28] == struct.pack("<H", 16)
    assert raw[0][:26] == raw[1][:26] and raw[0][28:] == raw[1][28:]


# ------------------------------------------------------- end to end at 10 bits
def _oracle(dc_golden, xs, h, w, q):
    from tests.test_crossfmt import _oracle as crossfmt_oracle
    return crossfmt_oracle(dc_golden, xs, h, w, q)


def _capture_recons(monkeypatch):
    """Every frame ReconWriter.write receives, as (H, W, 3) float32 numpy."""
    from dcvc_amd import harness
    from dcvc_amd.dc.video_model import as_act
    seen, orig = [], harness.ReconWriter.write

    def write(self, recon, frame_idx):
        seen.append(as_act(recon).t().float().cpu().numpy().copy())
        return orig(self, recon, frame_idx)
    monkeypatch.setattr(harness.ReconWriter, "write", write)
    return seen


@gpu
def test_run_test_10_bit_rgb_source_matches_oracle(dc_golden, nets, tmp_path, monkeypatch):
    """A 10-bit raw .rgb file through run_test (src_type 'rgb'): bits and PSNR
    per frame against the oracle codec on the restatement's input, within
    PARITY_TOL, and out.rgb bit-equal to the restatement's quantisation of the
    product's reconstruction."""
    from dcvc_amd.harness import run_test
    from dcvc_amd.synth import moving_pattern
    from tests.test_gpu_model_dc import PARITY_TOL
    inet, pnet = nets
    h, w, H, W, n, q, d = 100, 130, 112, 144, 3, 0, 10
    frames = [_deepen(moving_pattern(h, w, t, seed=5), d) for t in range(n)]
    with open(tmp_path / "src.rgb", "wb") as f:
        f.write(b"".join(fr.astype("<u2").tobytes() for fr in frames))
    recons = _capture_recons(monkeypatch)
    os.makedirs(tmp_path / "bins")
    log = run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True,
                                "bin_folder": str(tmp_path / "bins"),
                                "src_type": "rgb", "src_path": str(tmp_path / "src"), "src_bit_depth": d,
                                "src_height": h, "src_width": w, "dist_in_yuv420": False, "q_in_ckpt": False,
                                "i_frame_q_index": q, "verbose": 1, "save_decoded_frame": True,
                                "recon_path": str(tmp_path / "rec" / "cur"), "rate_idx": 0})
    xs = [F.ingest_rgb(fr, d, H, W) for fr in frames]
    ref = _oracle(dc_golden, xs, h, w, q)
    assert "frame_psnr_y" not in log
    for t, (bits, rec) in enumerate(ref):
        p = HO.psnr_torch(torch.from_numpy(rec)[None], torch.from_numpy(F.to_float(frames[t], d))[None])
        print("rgb10", t, log["frame_bpp"][t] * h * w, bits, log["frame_psnr"][t], p)
        assert abs(log["frame_bpp"][t] * h * w - bits) / bits <= PARITY_TOL["bits_rel"], (t, log["frame_bpp"][t], bits)
        assert abs(log["frame_psnr"][t] - p) <= PARITY_TOL["psnr_db"], (t, log["frame_psnr"][t], p)
    (folder,) = [e for e in os.listdir(tmp_path / "rec")]
    data = np.fromfile(tmp_path / "rec" / folder / "out.rgb", dtype="<u2")
    assert data.size == n * 3 * h * w and len(recons) == n
    for t, r in enumerate(recons):
        assert r.min() >= 0 and r.max() <= 1                             # handed over clamped
        want = F.rgb_file_frame(np.ascontiguousarray(r[:h, :w].transpose(2, 0, 1)), d)
        np.testing.assert_array_equal(data[t * 3 * h * w:(t + 1) * 3 * h * w], want.reshape(-1))


@gpu
def test_run_test_10_bit_yuv420_source_matches_oracle(dc_golden, nets, tmp_path, monkeypatch):
    """A 10-bit .yuv file through run_test with dist_in_yuv420: bits, PSNR_y /
    u / v and their 6:1:1 mean against the oracle codec, and out.yuv bit-equal
    to the restatement's quantisation of the product's reconstruction."""
    from dcvc_amd.harness import run_test
    from dcvc_amd.synth import moving_pattern_yuv420
    from tests.test_gpu_model_dc import PARITY_TOL
    inet, pnet = nets
    h, w, H, W, n, q, d = 100, 130, 112, 144, 3, 0, 10
    frames = [tuple(_deepen(p, d) for p in moving_pattern_yuv420(h, w, t, seed=5)) for t in range(n)]
    with open(tmp_path / "src.yuv", "wb") as f:
        f.write(b"".join(y.astype("<u2").tobytes() + uv.astype("<u2").tobytes() for y, uv in frames))
    recons = _capture_recons(monkeypatch)
    os.makedirs(tmp_path / "bins")
    log = run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True,
                                "bin_folder": str(tmp_path / "bins"),
                                "src_type": "yuv420", "src_path": str(tmp_path / "src"), "src_bit_depth": d,
                                "src_height": h, "src_width": w, "dist_in_yuv420": True, "q_in_ckpt": False,
                                "i_frame_q_index": q, "verbose": 1, "save_decoded_frame": True,
                                "recon_path": str(tmp_path / "rec" / "cur"), "rate_idx": 0})
    xs = [F.ingest_yuv(y, uv, d, H, W) for y, uv in frames]
    ref = _oracle(dc_golden, xs, h, w, q)
    for t, (bits, rec) in enumerate(ref):
        y, uv = F.to_float(frames[t][0], d), F.to_float(frames[t][1], d)
        y_rec, uv_rec = HO.ycbcr444_to_420(rec)
        py = HO.calc_psnr(y, y_rec[0], data_range=1)
        pu = HO.calc_psnr(uv[0], uv_rec[0], data_range=1)
        pv = HO.calc_psnr(uv[1], uv_rec[1], data_range=1)
        print("yuv10", t, log["frame_bpp"][t] * h * w, bits, log["frame_psnr_y"][t], py)
        assert abs(log["frame_bpp"][t] * h * w - bits) / bits <= PARITY_TOL["bits_rel"], (t, log["frame_bpp"][t], bits)
        assert abs(log["frame_psnr_y"][t] - py) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr_u"][t] - pu) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr_v"][t] - pv) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr"][t] - (6 * py + pu + pv) / 8) <= PARITY_TOL["psnr_db"], t
    (folder,) = [e for e in os.listdir(tmp_path / "rec")]
    data = np.fromfile(tmp_path / "rec" / folder / "out.yuv", dtype="<u2")
    fs = h * w * 3 // 2
    assert data.size == n * fs and len(recons) == n
    for t, r in enumerate(recons):
        want = F.yuv_file_frame(np.ascontiguousarray(r[:h, :w].transpose(2, 0, 1)), d)
        np.testing.assert_array_equal(data[t * fs:(t + 1) * fs], want)


def _hem_oracle_sequence(g, xs, h, w, q):
    """DCVC-HEM's test loop with the oracle codec: per frame (stream bits with
    the product's coder on the oracle's symbols, decoded crop)."""
    from oracle import hem_oracle as O
    from oracle import rans_oracle as RO
    from tests.test_gpu_model_hem import _stream_bits
    from tests.test_oracle_hem import _indexes
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    io = O.IntraOracle(g.i_state_dict(), RO.pmf_to_quantized_cdf)
    po = O.DMCOracle(g.p_state_dict(), RO.pmf_to_quantized_cdf)
    tables = {n: g.table(n) for n in ("i_y", "i_z", "p_y", "p_z", "p_mvz")}
    qi, qmv, qy = (round(v * 100) / 100 for v in q)
    out, dpb = [], None
    with torch.no_grad():
        for t, x in enumerate(xs):
            xp = torch.from_numpy(x).permute(2, 0, 1)[None].contiguous()
            net = io if t == 0 else po
            calls = io.compress(xp, qi) if t == 0 else po.compress(xp, dpb, qmv, qy)
            coder = [(kind, sym.reshape(-1).int().numpy(), _indexes(net, kind, sym, sc).numpy().astype(np.int16))
                     for kind, sym, sc in calls]
            pos = [0]

            def decoder(kind, idx):
                s = coder[pos[0]][1]
                pos[0] += 1
                return torch.from_numpy(s.astype(np.int64))
            if t == 0:
                dpb = {"ref_frame": io.decompress(decoder, h, w, qi), "ref_feature": None, "ref_y": None,
                       "ref_mv_y": None}
            else:
                dpb = po.decompress(dpb, decoder, h, w, qmv, qy)
            dpb["ref_frame"].clamp_(0, 1)
            out.append((_stream_bits(coder, tables, 14 if t == 0 else 8), dpb["ref_frame"][0, :, :h, :w].numpy()))
    return out


@gpu
def test_run_test_hem_10_bit_rgb_source_matches_oracle(tmp_path, monkeypatch):
    """run_test_hem on a 10-bit source of golden sequence A's size (zero
    padding to 64): bits and PSNR per frame against the HEM oracle on the
    restatement's input, at the parity bars, in fp32 precision as
    tests/test_gpu_model_hem.py holds its free-running parity runs; out.rgb
    bit-equal to the restatement's quantisation."""
    _need_gpu()
    from dcvc_amd.harness import run_test_hem, ArrayReader
    from dcvc_amd.hem import DMC, IntraNoAR
    from dcvc_amd.layers import Precision
    from tests.hem_fixtures import HEMGolden
    from tests.test_gpu_model_dc import PARITY_TOL
    g = HEMGolden()
    meta = g.meta["A"]
    h, w, n, d = meta["h"], meta["w"], 3, 10
    assert (h, w) == (128, 192)
    H, W = 128, 192
    frames = [_deepen(np.ascontiguousarray(g.npz[f"A_frame{t}"]), d) for t in range(n)]
    assert frames[0].shape == (3, h, w)
    inet = IntraNoAR(precision=Precision.parity()).load_state_dict(g.i_state_dict())
    pnet = DMC(precision=Precision.parity()).load_state_dict(g.p_state_dict())
    inet.update(force=True)
    pnet.update(force=True)
    q = g.q("A")
    recons = _capture_recons(monkeypatch)
    os.makedirs(tmp_path / "bins")
    log = run_test_hem(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True,
                                    "bin_folder": str(tmp_path / "bins"), "src_reader": ArrayReader(frames),
                                    "src_type": "rgb", "src_bit_depth": d, "src_height": h, "src_width": w,
                                    "i_frame_q_scale": q[0], "p_frame_mv_y_q_scale": q[1], "p_frame_y_q_scale": q[2],
                                    "save_decoded_frame": True, "decoded_frame_folder": str(tmp_path / "rec")})
    xs = [F.ingest_rgb(fr, d, H, W, zero_pad=True) for fr in frames]
    ref = _hem_oracle_sequence(g, xs, h, w, q)
    for t, (bits, rec) in enumerate(ref):
        p = HO.psnr_torch(torch.from_numpy(rec)[None], torch.from_numpy(F.to_float(frames[t], d))[None])
        print("hem10", t, log["frame_bpp"][t] * h * w, bits, log["frame_psnr"][t], p)
        assert abs(log["frame_bpp"][t] * h * w - bits) / bits <= PARITY_TOL["bits_rel"], (t, log["frame_bpp"][t], bits)
        assert abs(log["frame_psnr"][t] - p) <= PARITY_TOL["psnr_db"], (t, log["frame_psnr"][t], p)
    data = np.fromfile(tmp_path / "rec" / "out.rgb", dtype="<u2")
    assert data.size == n * 3 * h * w and len(recons) == n
    for t, r in enumerate(recons):
        want = F.rgb_file_frame(np.ascontiguousarray(r[:h, :w].transpose(2, 0, 1)), d)
        np.testing.assert_array_equal(data[t * 3 * h * w:(t + 1) * 3 * h * w], want.reshape(-1))


@gpu
@pytest.mark.parametrize("src_type", ["yuv420", "rgb"])
def test_encode_video_decode_video_at_10_bits(dc_golden, nets, tmp_path, monkeypatch, src_type):
    """encode_video -> file -> decode_video with separately built codecs, from
    a real 10-bit file: the header records the depth, every digest verifies
    (decode_video raises otherwise), the decoder's output depth defaults to the
    header's, and its out.yuv / out.rgb equals the restatement's quantisation
    of the ENCODER's reconstruction, frame by frame."""
    from dcvc_amd import harness
    from dcvc_amd.dc.video_model import as_act
    from dcvc_amd.sequence import SequenceReader
    from dcvc_amd.synth import moving_pattern, moving_pattern_yuv420
    inet, pnet = nets
    h, w, n, d = 100, 130, 3, 10
    yuv = src_type == "yuv420"
    if yuv:
        frames = [tuple(_deepen(p, d) for p in moving_pattern_yuv420(h, w, t, seed=5)) for t in range(n)]
        raw = b"".join(y.astype("<u2").tobytes() + uv.astype("<u2").tobytes() for y, uv in frames)
    else:
        frames = [_deepen(moving_pattern(h, w, t, seed=5), d) for t in range(n)]
        raw = b"".join(fr.astype("<u2").tobytes() for fr in frames)
    src = str(tmp_path / ("src." + ("yuv" if yuv else "rgb")))
    open(src, "wb").write(raw)
    enc_recons, orig = [], harness.FrameStage.distortion

    def distortion(self, recon, dframe, slot):
        orig(self, recon, dframe, slot)                                   # clamps the frame in place
        enc_recons.append(as_act(recon).t().float().cpu().numpy().copy())
    monkeypatch.setattr(harness.FrameStage, "distortion", distortion)
    seq = str(tmp_path / "a.seq")
    base = {"dist_in_yuv420": yuv, "src_type": src_type, "seq_path": seq}
    elog = harness.encode_video(inet, pnet, dict(base, frame_num=n, gop_size=32, src_path=src, src_bit_depth=d,
                                                 src_height=h, src_width=w, q_in_ckpt=False, i_frame_q_index=0))
    with SequenceReader(seq) as r:
        assert r.bit_depth == d and r.frames == n and all(rec["digest"] is not None for rec in r)
    dnets = _nets(dc_golden)
    dlog = harness.decode_video(*dnets, dict(base, save_decoded_frame=True, recon_path=str(tmp_path / "rec")))
    assert dlog["bit_depth"] == d and dlog["frame_bits"] == elog["frame_bits"] and len(enc_recons) == n
    data = np.fromfile(tmp_path / "rec" / ("out.yuv" if yuv else "out.rgb"), dtype="<u2")
    fs = h * w * 3 // 2 if yuv else 3 * h * w
    assert data.size == n * fs
    for t, r in enumerate(enc_recons):
        crop = np.ascontiguousarray(r[:h, :w].transpose(2, 0, 1))
        want = F.yuv_file_frame(crop, d) if yuv else F.rgb_file_frame(crop, d).reshape(-1)
        np.testing.assert_array_equal(data[t * fs:(t + 1) * fs], want)
    # an explicit 8-bit request overrides the header: uint8 samples
    harness.decode_video(*dnets, dict(base, save_decoded_frame=True, recon_path=str(tmp_path / "rec8"),
                                      recon_bit_depth=8))
    assert os.path.getsize(tmp_path / "rec8" / ("out.yuv" if yuv else "out.rgb")) == n * fs


@gpu
@pytest.mark.parametrize("src_type", ["yuv420", "rgb"])
def test_command_line_round_trips_a_10_bit_file(dc_golden, tmp_path, src_type):
    """python -m dcvc_amd.sequence encode --bit-depth 10, then decode: the
    decoded 10-bit file has the source's size and the header's depth."""
    _need_gpu()
    from dcvc_amd import sequence
    from dcvc_amd.synth import moving_pattern, moving_pattern_yuv420
    h, w, n, d = 100, 130, 2, 10
    yuv = src_type == "yuv420"
    if yuv:
        raw = b"".join(_deepen(p, d).astype("<u2").tobytes() for t in range(n)
                       for p in moving_pattern_yuv420(h, w, t, seed=5))
    else:
        raw = b"".join(_deepen(moving_pattern(h, w, t, seed=5), d).astype("<u2").tobytes() for t in range(n))
    src = str(tmp_path / ("src." + ("yuv" if yuv else "rgb")))
    open(src, "wb").write(raw)
    torch.save(dc_golden.i_state_dict(), tmp_path / "i.pth")
    torch.save(dc_golden.p_state_dict(), tmp_path / "p.pth")
    common = ["--i_frame_model_path", str(tmp_path / "i.pth"), "--p_frame_model_path", str(tmp_path / "p.pth"),
              "--seq_path", str(tmp_path / "a.seq"), "--src_type", src_type] + (["--yuv420"] if yuv else [])
    sequence.main(["encode"] + common + ["--src_path", src, "--src_width", str(w), "--src_height", str(h),
                                         "--frame_num", str(n), "--q_index", "0", "--bit-depth", "10"])
    with sequence.SequenceReader(str(tmp_path / "a.seq")) as r:
        assert r.bit_depth == 10 and r.frames == n
    sequence.main(["decode"] + common + ["--recon_path", str(tmp_path / "rec")])
    out = tmp_path / "rec" / ("out.yuv" if yuv else "out.rgb")
    assert os.path.getsize(out) == len(raw)
    assert np.fromfile(out, dtype="<u2").max() <= 1023


# ---------------------------------------------------------- argument errors
@gpu
def test_entry_points_reject_bad_arguments():
    """Every DCVC_HIP_EINVAL condition: null pointers, coff + 3 > cstride,
    depth outside 9..16, a crop larger than the frame, odd sizes where 4:2:0 is
    involved.  Every buffer is real and large enough for the call as made."""
    _need_gpu()
    from dcvc_amd import hip as K
    from dcvc_amd._native import NativeError
    L, st = K.lib(), K.stream()
    h, w, H, W = 6, 8, 16, 16
    x = torch.zeros((H, W, 8), dtype=torch.float32, device=DEV)
    s16 = torch.zeros(4 * H * W, dtype=torch.int16, device=DEV)
    f32 = torch.zeros(4 * 1024, dtype=torch.float32, device=DEV)          # four regions of 1024 floats
    ws, out3 = K.frame_sse_workspace(DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    X, S, Fp, WS, O3 = x.data_ptr(), s16.data_ptr(), f32.data_ptr(), ws.data_ptr(), out3.data_ptr()
    F1, F2, F3 = Fp + 4096, Fp + 8192, Fp + 12288
    good = (H, W, 8, 2)
    views = [(X, *good)]
    bad_views = [(None, *good), (X, H, W, 8, 6), (X, H, W, 8, -1), (X, 0, W, 8, 2), (X, H, 0, 8, 2),
                 (X, 4, W, 8, 2), (X, H, 6, 8, 2)]                         # the last two: smaller than the crop
    EINVAL = -1                                                           # DCVC_HIP_EINVAL (dcvc_hip.h)
    rgb_only = {"frame16_to_nhwc", "frame16_sse rgb", "recon_to_u16 rgb"}

    def calls(v, d, hh, ww, src=S, src2=S, dst=S, f=F1, f2=F2):
        return {
            "frame16_to_nhwc": lambda: L.dcvc_frame16_to_nhwc(src, hh, ww, d, 0, *v, st),
            "yuv420p16_to_nhwc": lambda: L.dcvc_yuv420p16_to_nhwc(src, src2, hh, ww, d, *v, st),
            "frame16_sse rgb": lambda: L.dcvc_frame16_sse(*v, src, None, hh, ww, d, 0, WS, O3, st),
            "frame16_sse yuv": lambda: L.dcvc_frame16_sse(*v, src, src2, hh, ww, d, 1, WS, O3, st),
            "recon_to_u16 rgb": lambda: L.dcvc_recon_to_u16(*v, hh, ww, d, 0, dst, st),
            "recon_to_u16 yuv": lambda: L.dcvc_recon_to_u16(*v, hh, ww, d, 1, dst, st),
            "recon_to_u16_cross rgb": lambda: L.dcvc_recon_to_u16_cross(*v, hh, ww, d, 1, dst, st),
            "recon_to_u16_cross yuv": lambda: L.dcvc_recon_to_u16_cross(*v, hh, ww, d, 0, dst, st),
            "yuv420f_to_rgb_nhwc": lambda: L.dcvc_yuv420f_to_rgb_nhwc(f, f2, hh, ww, *v, Fp, st),
        }
    for name, fn in calls(views[0], 10, h, w).items():
        assert fn() == 0, name                                            # the call as made is valid
    assert L.dcvc_u16_to_f32(S, 64, 10, Fp, st) == 0 and L.dcvc_rgbf_to_yuv420_planes(F3, h, w, F1, F2, st) == 0
    for v in bad_views:
        for name, fn in calls(v, 10, h, w).items():
            assert fn() == EINVAL, (name, v)
    for d in (8, 17, 0, -1):
        for name, fn in calls(views[0], d, h, w).items():
            if name != "yuv420f_to_rgb_nhwc":                             # takes fp32 planes, no depth
                assert fn() == EINVAL, (name, d)
        assert L.dcvc_u16_to_f32(S, 64, d, Fp, st) == EINVAL
    for hh, ww in ((5, 8), (6, 7), (0, 8), (6, 0)):
        for name, fn in calls(views[0], 10, hh, ww).items():
            if name in rgb_only and hh > 0 and ww > 0:
                assert fn() == 0, (name, hh, ww)                          # RGB to RGB has no parity rule
            else:
                assert fn() == EINVAL, (name, hh, ww)
    assert L.dcvc_frame16_sse(X, 15, W, 8, 2, S, S, h, w, 10, 1, WS, O3, st) == EINVAL     # odd padded frame, 4:2:0
    assert L.dcvc_frame16_to_nhwc(S, 5, 7, 10, 1, *views[0], st) == 0
    null = {k: {k: None} for k in ("src", "src2", "dst", "f", "f2")}
    uses = {"frame16_to_nhwc": ["src"], "yuv420p16_to_nhwc": ["src", "src2"], "frame16_sse rgb": ["src"],
            "frame16_sse yuv": ["src", "src2"], "recon_to_u16 rgb": ["dst"], "recon_to_u16 yuv": ["dst"],
            "recon_to_u16_cross rgb": ["dst"], "recon_to_u16_cross yuv": ["dst"], "yuv420f_to_rgb_nhwc": ["f", "f2"]}
    for name, args in uses.items():
        for a in args:
            assert calls(views[0], 10, h, w, **null[a])[name]() == EINVAL, (name, a)
    assert L.dcvc_frame16_sse(*views[0], S, None, h, w, 10, 0, None, O3, st) == EINVAL
    assert L.dcvc_frame16_sse(*views[0], S, None, h, w, 10, 0, WS, None, st) == EINVAL
    assert L.dcvc_yuv420f_to_rgb_nhwc(Fp, Fp, h, w, *views[0], None, st) == EINVAL
    assert L.dcvc_u16_to_f32(S, 0, 10, Fp, st) == EINVAL and L.dcvc_u16_to_f32(S, 64, 10, None, st) == EINVAL
    for bad in ((None, Fp, Fp), (Fp, None, Fp), (Fp, Fp, None)):
        assert L.dcvc_rgbf_to_yuv420_planes(bad[0], h, w, bad[1], bad[2], st) == EINVAL
    assert L.dcvc_rgbf_to_yuv420_planes(F3, 5, w, F1, F2, st) == EINVAL
    torch.cuda.synchronize()
    with pytest.raises(NativeError):                                      # the wrappers turn the status into an error
        K.recon_to_u16(K.Act(x, 2, 3), 5, w, 10, True, s16[:5 * w + 2 * 2 * (w // 2)])
    with pytest.raises(ValueError):
        K.frame16_to_nhwc(s16[:3 * h * w], h, w, 8, K.Act(x, 2, 3))
