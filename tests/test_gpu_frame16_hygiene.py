"""Kernel hygiene of the high-bit-depth frame entry points (frame16.hip and
the fp32-source twins in crossfmt.hip), with the helpers and the five steps of
tests/hygiene.py (tests/test_gpu_kernel_hygiene.py explains them).

These launchers take the NHWC frame as scalars (base, H, W, cstride, coff), so
the walk of test_gpu_kernel_hygiene.py, which looks for tensor-struct
parameters, does not see them; the table below covers them instead and a CPU
test walks hip.HIP_SYMBOLS and frame16.hip for entry points it misses.

Per entry: the frame view sits inside a larger buffer (32 guard rows above and
below, 8 lead and 8 tail channels), raw buffers have 64 guard elements on both
sides; the surroundings hold zero, all-ones NaN bits and 1e30 (integer
buffers: the type's minimum and maximum); outputs are pre-filled with NaN
inside and a canary around.  The results equal the restatement
(tests/frame16_ref.py), are bit-identical across the three fills, across two
runs and after dcvc_debug_poison_lds / dcvc_debug_poison_vgpr, no byte outside
a view is written and no output element is left unwritten (an integer output
starts as the canary pattern and must equal its reference everywhere)."""
import os
import re

import numpy as np
import pytest
import torch

from dcvc_amd import hip as K
from tests import frame16_ref as F
from tests import hygiene as HY
from tests.hygiene import seeded

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = (38, 54, 48, 64)      # h, w, H, W: odd half-planes, padding on both axes, more than one block
TOL_SSE = 1e-12               # tests/test_harness.py test_frame_sse_and_inplace_clamp (rtol)
TABLE = {}


def entry(name, *symbols):
    def deco(fn):
        assert name not in TABLE
        TABLE[name] = (fn, symbols)
        return fn
    return deco


def u16(E, key, d, *shape):
    """uint16 samples in [0, max_val] as the int16 bits the device tensors hold."""
    return E.const(f"{key}{d}", lambda: torch.from_numpy(
        torch.randint(0, 1 << d, shape, generator=seeded(f"{key}{d}")).numpy().astype(np.uint16).view(np.int16)))


def np16(t):
    return t.numpy().view(np.uint16)


def bits16(a):
    """A uint16 numpy array as the flat int16 tensor an output buffer holds."""
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int16))


def hwc(a):
    """(H, W, C) numpy -> (1, C, H, W) fp64 tensor."""
    return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).unsqueeze(0).double()


def frame_case(E, d, zero_pad):
    h, w, H, W = FRAME
    src = u16(E, "src", d, 3, h, w)
    y = E.y("y", 3, H, W)
    E.launch(K.frame16_to_nhwc, E.raw(src), h, w, d, y, zero_pad=zero_pad)
    E.ref("y", lambda: hwc(F.ingest_rgb(np16(src), d, H, W, zero_pad=zero_pad)), None)


entry("frame16_to_nhwc replicate, 10 bit", "dcvc_frame16_to_nhwc")(lambda E: frame_case(E, 10, False))
entry("frame16_to_nhwc zero pad, 16 bit", "dcvc_frame16_to_nhwc")(lambda E: frame_case(E, 16, True))


@entry("yuv420p16_to_nhwc, 12 bit", "dcvc_yuv420p16_to_nhwc")
def _yuv_in(E, d=12):
    h, w, H, W = FRAME
    yp, uv = u16(E, "y", d, h, w), u16(E, "uv", d, 2, h // 2, w // 2)
    out = E.y("y", 3, H, W)
    E.launch(K.yuv420p16_to_nhwc, E.raw(yp), E.raw(uv), h, w, d, out)
    E.ref("y", lambda: hwc(F.ingest_yuv(np16(yp), np16(uv), d, H, W)), None)


@entry("u16_to_f32, 10 bit", "dcvc_u16_to_f32")
def _to_f32(E, d=10):
    src = u16(E, "src", d, 5003)
    out = E.yraw("f32", 5003, torch.float32)
    E.launch(K.u16_to_f32, E.raw(src), d, out)
    E.ref("f32", lambda: torch.from_numpy(F.to_float(np16(src), d)), None)


@entry("yuv420f_to_rgb_nhwc", "dcvc_yuv420f_to_rgb_nhwc")
def _yuv_rgb(E, d=10):
    h, w, H, W = FRAME
    yp, uv = u16(E, "y", d, h, w), u16(E, "uv", d, 2, h // 2, w // 2)
    yf = E.const("yf", lambda: torch.from_numpy(F.to_float(np16(yp), d)))
    uvf = E.const("uvf", lambda: torch.from_numpy(F.to_float(np16(uv), d)))
    out = E.y("y", 3, H, W)
    planes = E.yraw("planes", 3 * h * w, torch.float32)
    E.launch(K.yuv420f_to_rgb_nhwc, E.raw(yf), E.raw(uvf), h, w, out, planes)
    ref = lambda: F.ingest_yuv_source_rgb_codec(np16(yp), np16(uv), d, H, W)  # noqa: E731
    E.ref("y", lambda: hwc(ref()[0]), None)
    E.ref("planes", lambda: torch.from_numpy(ref()[1]).reshape(-1), None)


@entry("rgbf_to_yuv420_planes", "dcvc_rgbf_to_yuv420_planes")
def _rgb_yuv(E, d=12):
    h, w, H, W = FRAME
    rgb = u16(E, "rgb", d, 3, h, w)
    rgbf = E.const("rgbf", lambda: torch.from_numpy(F.to_float(np16(rgb), d)))
    yf, uvf = E.yraw("yf", h * w, torch.float32), E.yraw("uvf", 2 * (h // 2) * (w // 2), torch.float32)
    E.launch(K.rgbf_to_yuv420_planes, E.raw(rgbf), h, w, yf, uvf)
    ref = lambda: F.ingest_rgb_source_yuv_codec(np16(rgb), d, H, W)  # noqa: E731
    E.ref("yf", lambda: torch.from_numpy(ref()[1]).reshape(-1), None)
    E.ref("uvf", lambda: torch.from_numpy(ref()[2]).reshape(-1), None)


def recon_case(E, d, yuv420, cross):
    """yuv420: what x_hat holds (YCbCr 4:4:4); cross: the writer is of the
    other format."""
    h, w, H, W = FRAME
    xh = E.const("xh", lambda: torch.rand(1, 3, H, W, generator=seeded("xh")) * 1.2 - 0.1)
    yuv_out = yuv420 != cross
    out = E.yraw("u16", h * w + 2 * (h // 2) * (w // 2) if yuv_out else 3 * h * w, torch.int16)
    xa = E.x(xh)
    if cross:
        E.launch(K.recon_to_u16_cross, xa, h, w, d, yuv420, out)      # to_rgb when x_hat holds YCbCr
    else:
        E.launch(K.recon_to_u16, xa, h, w, d, yuv420, out)
    crop = np.ascontiguousarray(xh[0, :, :h, :w].numpy())
    fn = {(False, False): F.rgb_file_frame, (True, False): F.yuv_file_frame,
          (True, True): F.rgb_file_frame_from_444, (False, True): F.yuv_file_frame_from_rgb}[(yuv420, cross)]
    E.ref("u16", lambda: bits16(fn(crop, d)), None)


entry("recon_to_u16 rgb, 10 bit", "dcvc_recon_to_u16")(lambda E: recon_case(E, 10, False, False))
entry("recon_to_u16 yuv420, 16 bit", "dcvc_recon_to_u16")(lambda E: recon_case(E, 16, True, False))
entry("recon_to_u16_cross to rgb, 12 bit", "dcvc_recon_to_u16_cross")(lambda E: recon_case(E, 12, True, True))
entry("recon_to_u16_cross to yuv420, 10 bit", "dcvc_recon_to_u16_cross")(lambda E: recon_case(E, 10, False, True))


def sse_case(E, d, yuv):
    """The three sums to rtol 1e-12, x_hat clamped in place over the whole view."""
    h, w, H, W = FRAME
    xh = E.const("xh", lambda: torch.rand(1, 3, H, W, generator=seeded("xh")) * 1.4 - 0.2)
    xa = E.inout("x_hat", xh)
    ws = E.scratch(int(K.lib().dcvc_frame_sse_workspace()) // 8, torch.float64) if not E.dry else None
    out = E.yraw("sse", 3, torch.float64)
    crop = np.ascontiguousarray(xh.clamp(0, 1)[0, :, :h, :w].numpy())
    if yuv:
        yp, uv = u16(E, "y", d, h, w), u16(E, "uv", d, 2, h // 2, w // 2)
        E.launch(K.frame16_sse, xa, E.raw(yp), h, w, d, ws, out, uv_u16=E.raw(uv))
        ref = lambda: torch.from_numpy(F.sse_yuv(crop, F.to_float(np16(yp), d), F.to_float(np16(uv), d)))  # noqa: E731
    else:
        src = u16(E, "src", d, 3, h, w)
        E.launch(K.frame16_sse, xa, E.raw(src), h, w, d, ws, out)
        ref = lambda: torch.from_numpy(F.sse_rgb(crop, F.to_float(np16(src), d)))  # noqa: E731
    E.ref("sse", ref, TOL_SSE, "rtol")
    E.ref("x_hat", lambda: xh.clamp(0, 1).double(), None)


entry("frame16_sse rgb, 12 bit", "dcvc_frame16_sse")(lambda E: sse_case(E, 12, False))
entry("frame16_sse yuv420, 10 bit", "dcvc_frame16_sse")(lambda E: sse_case(E, 10, True))


# ---------------------------------------------------------------- the tests
def entry_points():
    """The launchers this table answers for: the extern "C" functions of
    frame16.hip, hip.SCALAR_VIEW_SYMBOLS, and every bound symbol that names a
    16-bit or fp32-source frame path."""
    text = open(os.path.join(ROOT, "dcvc_amd", "csrc", "hip", "frame16.hip")).read()
    names = set(re.findall(r'extern "C" \w+ (dcvc_\w+)\(', text)) | set(K.SCALAR_VIEW_SYMBOLS)
    names |= {n for n, _, _ in K.HIP_SYMBOLS if re.search(r"16|yuv420f_to_rgb|rgbf_", n)}
    return names


def test_every_high_bit_depth_launcher_has_a_hygiene_case():
    covered = {s for _, syms in TABLE.values() for s in syms}
    known = {n for n, _, _ in K.HIP_SYMBOLS}
    names = entry_points()
    assert len(names) >= 8 and names <= known, sorted(names - known)
    assert {"dcvc_frame16_to_nhwc", "dcvc_frame16_sse", "dcvc_recon_to_u16_cross", "dcvc_u16_to_f32",
            "dcvc_yuv420f_to_rgb_nhwc", "dcvc_rgbf_to_yuv420_planes"} <= names
    missing = sorted(names - covered)
    assert not missing, f"high-bit-depth launchers without a hygiene case: {missing}"
    assert covered <= known
    # none of them is visible to the tensor-struct walk of test_gpu_kernel_hygiene.py
    for n, _, args in K.HIP_SYMBOLS:
        if n in names:
            assert K.CTensor not in args, n


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_entry_builds_on_the_cpu(name):
    """Every entry builds its call and its references without a device (the
    launches skipped): each reference has the shape of the output it is for."""
    fn, _ = TABLE[name]
    env = HY.Env("zero", {}, device=torch.device("cpu"), dry=True)
    fn(env)
    assert env.refs and set(env.refs) <= set(env.outs)
    for out, (ref, _, _) in env.refs.items():
        r = ref()
        assert tuple(r.shape) == tuple(env.values(out).shape), (out, tuple(r.shape))


@gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_kernel_hygiene(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fn, syms = TABLE[name]
    try:
        routes = HY.run_entry(fn, name)
    finally:
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:     # a GPU error poisons the process: launch nothing more
            pytest.exit(f"GPU error, stopping: {e}", returncode=3)
    assert set(routes) == set(syms), (routes, syms)
