"""Cross-format sources of run_test (DCVC-DC/test_video.py:79-119): a YUV420
source coded by an RGB model, an RGB source coded by a YUV420 model, and the
decoded-frame writers' two cross cases.

CPU tests pin the numpy restatement (tests/crossfmt_ref.py) to the reference's
own outputs (tests/golden/crossfmt_golden.*, written by make_golden_crossfmt.py
from functional.py) and to scipy, and check the ABI and the readers.  GPU tests
hold the HIP kernels (crossfmt.hip) bit-equal to the restatement and to the
fixture, the fp32-source distortion and MS-SSIM to the bars of their uint8
twins in tests/test_harness.py, and both cross directions of ``run_test`` to
the oracle codec on the restatement's converted input."""
import ctypes
import functools
import hashlib
import importlib.util
import json
import os
import re
import tempfile

import numpy as np
import pytest
import scipy.ndimage
import torch

from oracle import harness_oracle as HO
from tests import crossfmt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ["dcvc_yuv420_to_rgb_nhwc", "dcvc_rgb_to_yuv420_planes", "dcvc_yuv420f_to_nhwc", "dcvc_frame_sse_f32",
               "dcvc_yuv_planes_f64_f32", "dcvc_rgb_planes_f64_f32", "dcvc_recon_to_u8_cross"]
# (h, w, H, W): the degenerate 2-pixel zoom axes; odd half-planes (19 x 27)
# with padding on both axes; more than one block; 1080 rows padded to 1088
SHAPES = [(2, 2, 16, 16), (38, 54, 48, 64), (100, 130, 112, 144), (1080, 1920, 1088, 1920)]


@functools.lru_cache(maxsize=None)
def _fixture():
    spec = importlib.util.spec_from_file_location("make_golden_crossfmt",
                                                  os.path.join(GOLDEN, "make_golden_crossfmt.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with open(os.path.join(GOLDEN, "crossfmt_golden.json")) as f:
        cases = {(c["h"], c["w"]): c for c in json.load(f)["cases"]}
    return m.inputs, cases, np.load(os.path.join(GOLDEN, "crossfmt_golden.npz"))


def _digest(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _case(h, w, H, W):
    """The fixture's uint8 inputs of one shape and the restatement's
    conversions of them, computed once and shared; no test writes to them."""
    inputs, cases, _ = _fixture()
    y8, uv8, rgb8 = inputs(cases[(h, w)]["seed"], h, w)
    x_rgb, rgb = R.ingest_yuv_source_rgb_codec(y8, uv8, H, W)
    x_yuv, y, uv = R.ingest_rgb_source_yuv_codec(rgb8, H, W)
    return {"y8": y8, "uv8": uv8, "rgb8": rgb8, "x_rgb": x_rgb, "rgb": rgb, "x_yuv": x_yuv, "y": y, "uv": uv}


# --------------------------------------------------------------------- CPU
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_reproduces_reference_fixture(shape):
    """tests/crossfmt_ref.py against the reference's functional.py outputs:
    every digest, and the stored arrays of the two small cases."""
    h, w, H, W = shape
    _, cases, arrays = _fixture()
    c, d = cases[(h, w)], _case(*shape)
    assert _digest(d["rgb"]) == c["rgb"]
    assert _digest(d["y"][None]) == c["y"]
    assert _digest(d["uv"]) == c["uv"]
    assert _digest(R.yuv420_to_444(d["y"][None], d["uv"])) == c["yuv444"]
    if f"rgb_{h}x{w}" in arrays:
        np.testing.assert_array_equal(d["rgb"], arrays[f"rgb_{h}x{w}"])
        np.testing.assert_array_equal(d["y"][None], arrays[f"y_{h}x{w}"])
        np.testing.assert_array_equal(d["uv"], arrays[f"uv_{h}x{w}"])
        np.testing.assert_array_equal(d["x_yuv"][:h, :w].transpose(2, 0, 1), arrays[f"yuv444_{h}x{w}"])


@pytest.mark.parametrize("n,m", [(1, 1), (1, 3), (2, 2), (3, 5), (19, 27), (50, 65), (135, 240), (540, 960)])
def test_zoom1_restatement_bit_equal_to_scipy(n, m):
    g = np.random.default_rng(n * 1000 + m)
    a = (g.integers(0, 256, (2, n, m)).astype(np.float32) / np.float32(255))
    np.testing.assert_array_equal(R.zoom1(a), scipy.ndimage.zoom(a, (1, 2, 2), order=1))
    np.testing.assert_array_equal(R.zoom0(a), scipy.ndimage.zoom(a, (1, 2, 2), order=0))


# half-plane heights at which this sweep's n x 2 planes hold an exact fp32 tie
# (for example (2a + b) / 3 with a = 14/255, b = 146/255): the last bit of the
# double sum decides the float32, and scipy's second tap weight 1 - (1 - f)
# gives another last bit than f does
TIE_N = (233, 234, 662, 769, 880, 920, 956, 1213, 1251)


@functools.lru_cache(maxsize=None)
def _sweep_planes():
    """uint8 chroma planes (1, n, 2) for n = 1..1299 from one seeded stream."""
    g = np.random.default_rng(0)
    return [g.integers(0, 256, (1, n, 2)).astype(np.uint8) for n in range(1, 1300)]


def _zoom1_with_weights_1mf_and_f(planes):
    """zoom1 with the second weight taken as f itself: the arithmetic that is
    off by one ulp at an fp32 tie; it marks which inputs are tie inputs."""
    keep = R._taps

    def taps(n):
        i0, i1, w0, _ = keep(n)
        return i0, i1, w0, np.arange(2 * n, dtype=np.float64) * ((n - 1) / (2 * n - 1) if n > 1 else 0.0) % 1.0
    R._taps = taps
    try:
        return R.zoom1(planes)
    finally:
        R._taps = keep


def test_zoom1_restatement_bit_equal_to_scipy_at_fp32_ties():
    """A sweep over n x 2 planes, 6.75 M values, nine of them exact fp32 ties:
    zoom1 equals scipy on all, and the ties are real (weights 1 - f, f miss)."""
    missed = []
    for p in _sweep_planes():
        a = R.u8_to_float(p)
        ref = scipy.ndimage.zoom(a, (1, 2, 2), order=1)
        np.testing.assert_array_equal(R.zoom1(a), ref)
        if p.shape[1] in TIE_N and not np.array_equal(_zoom1_with_weights_1mf_and_f(a), ref):
            missed.append(p.shape[1])
    assert tuple(missed) == TIE_N


@pytest.mark.parametrize("h,w", [(2, 2), (6, 2), (2, 6), (38, 54)])
def test_block_mean_order_matches_numpy(h, w):
    """mean2x2 against numpy's own mean over axes (-1, -3), the one-column
    chroma plane (w = 2) included."""
    g = np.random.default_rng(h * 100 + w)
    for _ in range(8):
        p = g.random((1, h, w)).astype(np.float32)
        ref = np.mean(np.reshape(p, (1, h // 2, 2, w // 2, 2)), axis=(-1, -3))
        np.testing.assert_array_equal(R.mean2x2(p), ref)


def test_writer_restatements_match_reference_formulas():
    """png_bytes_from_444 / yuv_bytes_from_rgb against the reference's
    formulas written with scipy and the oracle's writers (as
    test_recon_writers_match_reference_formulas states them)."""
    g = np.random.default_rng(5)
    crop = (g.random((3, 38, 54)) * 1.2 - 0.1).astype(np.float32)
    y, uv = HO.ycbcr444_to_420(crop)
    uvz = scipy.ndimage.zoom(uv, (1, 2, 2), order=1)
    r = y + (2 - 2 * 0.2126) * (uvz[1:2] - 0.5)
    b = y + (2 - 2 * 0.0722) * (uvz[0:1] - 0.5)
    gg = (y - 0.2126 * r - 0.0722 * b) / 0.7152
    np.testing.assert_array_equal(R.png_bytes_from_444(crop), HO.png_writer_u8(np.clip(np.concatenate((r, gg, b)), 0, 1)))
    kr, kg, kb = 0.2126, 0.7152, 0.0722
    r, gg, b = crop[0:1], crop[1:2], crop[2:3]
    y = kr * r + kg * gg + kb * b
    cb = 0.5 * (b - y) / (1 - kb) + 0.5
    cr = 0.5 * (r - y) / (1 - kr) + 0.5
    uv = np.concatenate(HO.ycbcr444_to_420(np.concatenate((y, cb, cr)))[1:], 0)
    assert R.yuv_bytes_from_rgb(crop) == HO.yuv_writer_bytes(np.clip(y, 0, 1), uv)


def test_header_declares_and_library_exports_cross_format_symbols():
    text = open(os.path.join(ROOT, "include", "dcvc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dcvc_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared, sorted(set(NEW_SYMBOLS) - declared)
    lib = ctypes.CDLL(os.path.join(ROOT, "dcvc_amd", "lib", "libdcvc_hip.so"))
    assert not [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    from dcvc_amd import hip
    assert set(NEW_SYMBOLS) <= {s[0] for s in hip.HIP_SYMBOLS}


def test_readers_hand_over_native_planes_for_either_codec_format(tmp_path):
    """YUVReader.read_one_frame("rgb") and PNGReader.read_one_frame("420")
    return the native uint8 planes; the conversion is FrameStage's."""
    from PIL import Image
    from dcvc_amd.harness import PNGReader, YUVReader
    g = np.random.default_rng(6)
    h, w = 4, 6
    y = g.integers(0, 256, (h, w), dtype=np.uint8)
    uv = g.integers(0, 256, (2, h // 2, w // 2), dtype=np.uint8)
    with open(tmp_path / "seq.yuv", "wb") as f:
        f.write(y.tobytes() + uv.tobytes())
    r = YUVReader(str(tmp_path / "seq"), w, h)
    ry, ruv = r.read_one_frame(dst_format="rgb")
    assert ry.dtype == np.uint8 and ruv.dtype == np.uint8
    np.testing.assert_array_equal(ry, y)
    np.testing.assert_array_equal(ruv, uv)
    assert r.read_one_frame(dst_format="rgb") == (None, None)
    r.close()
    rgb = g.integers(0, 256, (3, h, w), dtype=np.uint8)
    os.makedirs(tmp_path / "png")
    Image.fromarray(np.ascontiguousarray(rgb.transpose(1, 2, 0))).save(tmp_path / "png" / "im1.png")
    p = PNGReader(str(tmp_path / "png"), w, h)
    got = p.read_one_frame(dst_format="420")
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, rgb)
    assert p.read_one_frame(dst_format="420") is None
    r = YUVReader(str(tmp_path / "seq"), w, h)
    with pytest.raises(ValueError):
        r.read_one_frame(dst_format="444")
    r.close()


# --------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stage(h, w, yuv420, src_format):
    from dcvc_amd.harness import FrameStage
    return FrameStage(h, w, 16, yuv420, zero_pad=False, frame_num=1, device=torch.device("cuda", 0),
                      src_format=src_format)


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_ingest_yuv420_source_for_rgb_codec_bit_exact(shape):
    """dcvc_yuv420_to_rgb_nhwc through FrameStage: the padded NHWC input and
    the fp32 RGB source planes equal the restatement and the fixture."""
    _need_gpu()
    h, w, H, W = shape
    _, cases, arrays = _fixture()
    d = _case(*shape)
    st = _stage(h, w, False, "420")
    assert (st.H, st.W) == (H, W) and st.cross
    x = st.load(st.upload((d["y8"], d["uv8"])))
    planes = st.src_f32[0].cpu().numpy()
    np.testing.assert_array_equal(x.t().cpu().numpy(), d["x_rgb"])
    np.testing.assert_array_equal(planes, d["rgb"])
    assert _digest(planes) == cases[(h, w)]["rgb"]
    if f"rgb_{h}x{w}" in arrays:
        np.testing.assert_array_equal(planes, arrays[f"rgb_{h}x{w}"])


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_ingest_rgb_source_for_yuv420_codec_bit_exact(shape):
    """dcvc_rgb_to_yuv420_planes + dcvc_yuv420f_to_nhwc through FrameStage."""
    _need_gpu()
    h, w, H, W = shape
    _, cases, arrays = _fixture()
    d = _case(*shape)
    st = _stage(h, w, True, "rgb")
    assert (st.H, st.W) == (H, W) and st.cross
    x = st.load(st.upload(d["rgb8"]))
    y, uv = st.src_f32[0].cpu().numpy(), st.src_f32[1].cpu().numpy()
    np.testing.assert_array_equal(x.t().cpu().numpy(), d["x_yuv"])
    np.testing.assert_array_equal(y, d["y"])
    np.testing.assert_array_equal(uv, d["uv"])
    assert _digest(y[None]) == cases[(h, w)]["y"] and _digest(uv) == cases[(h, w)]["uv"]
    assert _digest(x.t().cpu().numpy()[:h, :w].transpose(2, 0, 1)) == cases[(h, w)]["yuv444"]
    if f"y_{h}x{w}" in arrays:
        np.testing.assert_array_equal(y[None], arrays[f"y_{h}x{w}"])
        np.testing.assert_array_equal(uv, arrays[f"uv_{h}x{w}"])


@gpu
def test_ingest_yuv420_source_at_fp32_ties_bit_exact():
    """dcvc_yuv420_to_rgb_nhwc on chroma planes whose order-1 zoom holds exact
    fp32 ties (TIE_N, 4-pixel-wide frames): equal to the reference's formula
    with scipy's own zoom, so the kernel's tap weights are scipy's to the last
    double bit."""
    _need_gpu()
    planes = _sweep_planes()
    g = np.random.default_rng(7)
    for n in TIE_N[:3]:
        h, w = 2 * n, 4
        uv8 = np.concatenate((planes[n - 1], planes[n - 1][:, ::-1]), axis=0)
        y8 = g.integers(0, 256, (h, w), dtype=np.uint8)
        uvz = scipy.ndimage.zoom(R.u8_to_float(uv8), (1, 2, 2), order=1)
        assert not np.array_equal(_zoom1_with_weights_1mf_and_f(R.u8_to_float(uv8)), uvz)   # a tie input
        ref = R.ycc_to_rgb(R.u8_to_float(y8)[None], uvz)
        st = _stage(h, w, False, "420")
        x = st.load(st.upload((y8, uv8))).t().cpu().numpy()
        np.testing.assert_array_equal(st.src_f32[0].cpu().numpy(), ref)
        np.testing.assert_array_equal(x, R.pad_nhwc(ref, st.H, st.W))


@gpu
def test_matched_formats_keep_the_uint8_path():
    """src_format equal to the codec's format (the default) is not a cross
    stage: no fp32 source planes, the uint8 kernels as before."""
    _need_gpu()
    d = _case(*SHAPES[1])
    h, w, H, W = SHAPES[1]
    for yuv, fmt, frame in ((False, None, d["rgb8"]), (False, "rgb", d["rgb8"]), (True, "420", (d["y8"], d["uv8"]))):
        st = _stage(h, w, yuv, fmt)
        assert not st.cross and st.src_f32 is None
        x = st.load(st.upload(frame)).t().cpu().numpy()
        ref = HO.yuv_u8_to_input(d["y8"], d["uv8"], H, W) if yuv else R.pad_nhwc(R.u8_to_float(d["rgb8"]), H, W)
        np.testing.assert_array_equal(x, ref)


@gpu
@pytest.mark.parametrize("yuv", [False, True])
def test_frame_sse_f32_and_inplace_clamp(yuv):
    """dcvc_frame_sse_f32 at the bar of test_frame_sse_and_inplace_clamp."""
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = SHAPES[1]
    d = _case(*SHAPES[1])
    g = np.random.default_rng(w)
    xh = torch.from_numpy((g.random((H, W, 3)) * 1.4 - 0.2).astype(np.float32)).cuda()
    x_act = K.Act(xh.clone())
    clamped = xh.clamp(0, 1).cpu().numpy()
    crop = np.ascontiguousarray(clamped[:h, :w].transpose(2, 0, 1))
    ws = K.frame_sse_workspace(xh.device)
    out = torch.zeros(3, dtype=torch.float64, device=xh.device)
    if yuv:
        K.frame_sse_f32(x_act, torch.from_numpy(d["y"]).cuda(), h, w, ws, out,
                        uv_f32=torch.from_numpy(d["uv"]).cuda())
        y_rec, uv_rec = HO.ycbcr444_to_420(crop)
        e = [y_rec[0].astype(np.float64) - d["y"], uv_rec[0].astype(np.float64) - d["uv"][0],
             uv_rec[1].astype(np.float64) - d["uv"][1]]
        ref = np.array([np.sum(np.square(v)) for v in e])
    else:
        K.frame_sse_f32(x_act, torch.from_numpy(d["rgb"]).cuda(), h, w, ws, out)
        e = crop - d["rgb"]
        ref = np.array([np.sum((e[c] * e[c]).astype(np.float64)) for c in range(3)])
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-12)
    np.testing.assert_array_equal(x_act.t().cpu().numpy(), clamped)


@gpu
def test_msssim_against_fp32_source_planes():
    """MsSsim.run_f32 at 200 x 256 on the fp32 planes of a converted RGB
    source, at the bar of test_run_test_yuv420_msssim; MsSsimRGB.run_f32 on
    uint8 / 255 planes equals run on the uint8 frame."""
    _need_gpu()
    from dcvc_amd import hip as K
    from dcvc_amd.harness import MsSsim, MsSsimRGB
    from dcvc_amd.synth import moving_pattern
    h, w, H, W = 200, 256, 208, 256
    rgb8 = moving_pattern(h, w, 0, seed=9)
    x_in, y, uv = R.ingest_rgb_source_yuv_codec(rgb8, H, W)
    g = np.random.default_rng(9)
    xh = torch.from_numpy((x_in + g.normal(0, 0.04, (H, W, 3))).astype(np.float32)).cuda()
    ms = MsSsim(h, w, 1, xh.device)
    ms.run_f32(K.Act(xh), torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), 0)
    got = ms.values(1)[0]
    crop = np.clip(xh.cpu().numpy()[:h, :w].transpose(2, 0, 1), 0, 1)
    y_rec, uv_rec = HO.ycbcr444_to_420(np.ascontiguousarray(crop))
    ref = [HO.calc_msssim(y, y_rec[0]), HO.calc_msssim(uv[0], uv_rec[0]), HO.calc_msssim(uv[1], uv_rec[1])]
    np.testing.assert_allclose(got[:3], ref, rtol=0, atol=1e-10)
    assert abs(got[3] - (6 * ref[0] + ref[1] + ref[2]) / 8) < 1e-10
    a, b = MsSsimRGB(h, w, 1, xh.device), MsSsimRGB(h, w, 1, xh.device)
    a.run(K.Act(xh), torch.from_numpy(rgb8).cuda(), 0)
    b.run_f32(K.Act(xh), torch.from_numpy(R.u8_to_float(rgb8)).cuda(), 0)
    assert a.values(1) == b.values(1)


@gpu
@pytest.mark.parametrize("shape", SHAPES[:2])
@pytest.mark.parametrize("to_rgb", [True, False])
def test_recon_to_u8_cross_matches_restatement(shape, to_rgb):
    _need_gpu()
    from dcvc_amd import hip as K
    h, w, H, W = shape
    g = torch.Generator().manual_seed(h)
    f = torch.rand(H, W, 3, generator=g) * 1.2 - 0.1
    crop = f[:h, :w].permute(2, 0, 1).contiguous().numpy()
    n = 3 * h * w if to_rgb else h * w * 3 // 2
    out = torch.zeros(n + 64, dtype=torch.uint8).cuda()
    K.recon_to_u8_cross(K.Act(f.cuda().contiguous()), h, w, to_rgb, out)
    got = out.cpu().numpy()
    assert not got[n:].any()
    if to_rgb:
        np.testing.assert_array_equal(got[:n].reshape(h, w, 3), R.png_bytes_from_444(crop))
    else:
        assert got[:n].tobytes() == R.yuv_bytes_from_rgb(crop)


@gpu
@pytest.mark.parametrize("kind,fmt", [("yuv", "rgb"), ("png", "420")])
def test_cross_recon_writers_match_restatement(tmp_path, kind, fmt):
    """ReconWriter's cross cases (GPU quantisation, pinned copy, writer
    thread) store the restatement's bytes."""
    _need_gpu()
    from PIL import Image
    from dcvc_amd import hip as K
    from dcvc_amd.harness import ReconWriter
    h, w, H, W = SHAPES[1]
    g = torch.Generator().manual_seed(4)
    frames = [torch.rand(H, W, 3, generator=g) * 1.2 - 0.1 for _ in range(2)]
    with ReconWriter(str(tmp_path / "rec"), h, w, kind, fmt, torch.device("cuda", 0)) as wr:
        for t, f in enumerate(frames):
            wr.write(K.Act(f.cuda().contiguous()), t)
    for t, f in enumerate(frames):
        crop = f[:h, :w].permute(2, 0, 1).contiguous().numpy()
        if kind == "png":
            got = np.asarray(Image.open(tmp_path / "rec" / f"im{t + 1:05d}.png"))
            np.testing.assert_array_equal(got, R.png_bytes_from_444(crop))
        else:
            n = h * w * 3 // 2
            assert (tmp_path / "rec" / "out.yuv").read_bytes()[t * n:(t + 1) * n] == R.yuv_bytes_from_rgb(crop)


def _nets(dc_golden):
    from dcvc_amd.dc import DMC, IntraNoAR
    from dcvc_amd.layers import Precision
    inet = IntraNoAR(precision=Precision.split()).load_state_dict(dc_golden.i_state_dict())
    pnet = DMC(precision=Precision.split()).load_state_dict(dc_golden.p_state_dict())
    inet.update(force=True)
    pnet.update(force=True)
    return inet, pnet


def _oracle(dc_golden, xs, h, w, q):
    from oracle import dc_oracle as O
    from oracle import rans_oracle as RO
    from tests.test_harness import _oracle_sequence
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    io = O.IntraOracle(dc_golden.i_state_dict(), RO.pmf_to_quantized_cdf)
    po = O.DMCOracle(dc_golden.p_state_dict(), RO.pmf_to_quantized_cdf)
    xps = [torch.from_numpy(x).permute(2, 0, 1)[None].contiguous() for x in xs]
    return _oracle_sequence(io, po, xps, h, w, q)


@gpu
def test_run_test_yuv420_source_rgb_codec_matches_oracle(dc_golden):
    """src_type yuv420 with dist_in_yuv420 off (an RGB model fed from a .yuv
    source): bits and PSNR per frame against the oracle codec on the
    restatement's converted input, within PARITY_TOL."""
    _need_gpu()
    from dcvc_amd.harness import run_test, ArrayReader
    from dcvc_amd.synth import moving_pattern_yuv420
    from tests.test_gpu_model_dc import PARITY_TOL
    h, w, H, W, n, q = 100, 130, 112, 144, 3, 0
    frames = [moving_pattern_yuv420(h, w, t, seed=5) for t in range(n)]
    inet, pnet = _nets(dc_golden)
    with tempfile.TemporaryDirectory() as td:
        log = run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True, "bin_folder": td,
                                    "src_reader": ArrayReader(frames), "src_type": "yuv420",
                                    "src_height": h, "src_width": w, "dist_in_yuv420": False,
                                    "q_in_ckpt": False, "i_frame_q_index": q, "verbose": 1})
    conv = [R.ingest_yuv_source_rgb_codec(y, uv, H, W) for y, uv in frames]
    ref = _oracle(dc_golden, [c[0] for c in conv], h, w, q)
    assert "frame_psnr_y" not in log
    for t, (bits, rec) in enumerate(ref):
        p = HO.psnr_torch(torch.from_numpy(rec)[None], torch.from_numpy(conv[t][1])[None])
        assert abs(log["frame_bpp"][t] * h * w - bits) / bits <= PARITY_TOL["bits_rel"], (t, log["frame_bpp"][t], bits)
        assert abs(log["frame_psnr"][t] - p) <= PARITY_TOL["psnr_db"], (t, log["frame_psnr"][t], p)
    assert log["i_frame_num"] == 1 and log["p_frame_num"] == n - 1


@gpu
def test_run_test_rgb_source_yuv420_codec_matches_oracle(dc_golden):
    """src_type png with dist_in_yuv420 on (a YUV420 model fed from RGB
    frames): bits, PSNR_y/u/v and their 6:1:1 mean against the oracle codec on
    the restatement's converted input, within PARITY_TOL."""
    _need_gpu()
    from dcvc_amd.harness import run_test, ArrayReader
    from dcvc_amd.synth import moving_pattern
    from tests.test_gpu_model_dc import PARITY_TOL
    h, w, H, W, n, q = 100, 130, 112, 144, 3, 0
    frames = [moving_pattern(h, w, t, seed=5) for t in range(n)]
    inet, pnet = _nets(dc_golden)
    with tempfile.TemporaryDirectory() as td:
        log = run_test(pnet, inet, {"frame_num": n, "gop_size": 32, "write_stream": True, "bin_folder": td,
                                    "src_reader": ArrayReader(frames), "src_type": "png",
                                    "src_height": h, "src_width": w, "dist_in_yuv420": True,
                                    "q_in_ckpt": False, "i_frame_q_index": q, "verbose": 1})
    conv = [R.ingest_rgb_source_yuv_codec(f, H, W) for f in frames]
    ref = _oracle(dc_golden, [c[0] for c in conv], h, w, q)
    for t, (bits, rec) in enumerate(ref):
        _, y, uv = conv[t]
        y_rec, uv_rec = HO.ycbcr444_to_420(rec)
        py = HO.calc_psnr(y, y_rec[0], data_range=1)
        pu = HO.calc_psnr(uv[0], uv_rec[0], data_range=1)
        pv = HO.calc_psnr(uv[1], uv_rec[1], data_range=1)
        assert abs(log["frame_bpp"][t] * h * w - bits) / bits <= PARITY_TOL["bits_rel"], (t, log["frame_bpp"][t], bits)
        assert abs(log["frame_psnr_y"][t] - py) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr_u"][t] - pu) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr_v"][t] - pv) <= PARITY_TOL["psnr_db"], t
        assert abs(log["frame_psnr"][t] - (6 * py + pu + pv) / 8) <= PARITY_TOL["psnr_db"], t
    assert log["i_frame_num"] == 1 and log["p_frame_num"] == n - 1


@gpu
@pytest.mark.parametrize("yuv", [True, False])
def test_run_test_calc_ssim_reads_the_converted_source(dc_golden, yuv):
    """run_test(calc_ssim=True) with a source of the other format, one I frame
    at 176 x 192: the logged MS-SSIM is that of the frame's recon against the
    converted fp32 source.  YUV420 codec: calc_msssim per plane at the bar of
    test_run_test_yuv420_msssim; RGB codec: the unpinned RGB restatement at the
    bar of test_gpu_rgb_msssim_matches_restatement."""
    _need_gpu()
    from dcvc_amd.dc.video_model import as_act
    from dcvc_amd.harness import run_test, ArrayReader
    from dcvc_amd.synth import moving_pattern, moving_pattern_yuv420
    h, w, q = 176, 192, 0
    inet, pnet = _nets(dc_golden)
    frame = moving_pattern(h, w, 0, seed=5) if yuv else moving_pattern_yuv420(h, w, 0, seed=5)
    log = run_test(pnet, inet, {"frame_num": 1, "gop_size": 32, "write_stream": False,
                                "src_reader": ArrayReader([frame]), "src_type": "png" if yuv else "yuv420",
                                "src_height": h, "src_width": w, "dist_in_yuv420": yuv, "q_in_ckpt": False,
                                "i_frame_q_index": q, "verbose": 1, "calc_ssim": True})
    # the same I frame again (the codec is deterministic), for its recon
    st = _stage(h, w, yuv, "rgb" if yuv else "420")
    with torch.no_grad():
        res = inet.encode_decode(st.load(st.upload(frame)), False, q, None, pic_height=h, pic_width=w)
    rec = np.clip(as_act(res["x_hat"]).t().float().cpu().numpy()[:h, :w].transpose(2, 0, 1), 0, 1)
    rec = np.ascontiguousarray(rec)
    if yuv:
        _, y, uv = R.ingest_rgb_source_yuv_codec(frame, st.H, st.W)
        y_rec, uv_rec = HO.ycbcr444_to_420(rec)
        ref = [HO.calc_msssim(y, y_rec[0]), HO.calc_msssim(uv[0], uv_rec[0]), HO.calc_msssim(uv[1], uv_rec[1])]
        got = [log["frame_msssim_y"][0], log["frame_msssim_u"][0], log["frame_msssim_v"][0]]
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10)
        assert abs(log["frame_msssim"][0] - (6 * ref[0] + ref[1] + ref[2]) / 8) < 1e-10
    else:
        _, rgb = R.ingest_yuv_source_rgb_codec(frame[0], frame[1], st.H, st.W)
        ref = HO.ms_ssim_torch(torch.from_numpy(rec)[None], torch.from_numpy(rgb)[None])
        assert abs(log["frame_msssim"][0] - ref) < 1e-5, (log["frame_msssim"][0], ref)
        assert log["msssim_unpinned"] is True
