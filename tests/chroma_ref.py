"""numpy restatement of the chroma-layout rule (INTEGRATION.md "Chroma
layouts") -- TEST INFRASTRUCTURE ONLY (the product path never imports it).

A chroma format is (sx, sy): 4:4:4 = (1, 1), 4:2:2 = (2, 1), 4:2:0 = (2, 2).  A
frame is planar Y (h, w) | U | V (h/sy, w/sx each), uint8 at 8 bits and uint16
at 9..16; a sample is float32(s) / float32(max_val) in and clip(rint(v *
max_val), 0, max_val) out (tests/frame16_ref.py; at 8 bits the uint8 rule).

* into a YUV codec: the order-0 zoom of ycbcr420_to_444 along the subsampled
  axes (``zoom0_x`` for 4:2:2), nothing for 4:4:4;
* into an RGB codec: the order-1 zoom of ycbcr420_to_rgb along the subsampled
  axes (``zoom1_x``: the 1-D form of crossfmt_ref._taps), then ycbcr_to_rgb
  (DCVC-DC/src/transforms/functional.py:114-126);
* distortion and output on a YUV codec: chroma = the clipped float32 mean of
  each footprint (``pair_mean`` for 4:2:2, the value itself for 4:4:4);
* output from an RGB codec: rgb_to_ycbcr (functional.py:95-111) per pixel, y
  clipped, cb / cr averaged unclipped over the footprint, then clipped.

With (2, 2) every function is crossfmt_ref's / frame16_ref's 4:2:0 function.
tests/test_chroma.py pins the pieces to scipy and numpy on this machine and to
the reference's rgb_to_ycbcr / ycbcr_to_rgb (tests/golden/chroma_golden.*).
"""
import numpy as np

from tests import crossfmt_ref as R
from tests import frame16_ref as F

F32 = np.float32
FORMATS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}


def sub(chroma):
    return FORMATS[chroma] if isinstance(chroma, str) else chroma


def max_val(d):
    if not 8 <= d <= 16:
        raise ValueError(d)
    return (1 << d) - 1


def to_float(a, d):
    a = np.asarray(a)
    assert a.dtype == (np.uint8 if d == 8 else np.uint16), (a.dtype, d)
    return a.astype(F32) / F32(max_val(d))


def quant(v, d):
    mx = max_val(d)
    return np.clip(np.rint(np.asarray(v, dtype=F32) * F32(mx)), 0, mx).astype(np.uint8 if d == 8 else np.uint16)


def zoom_index(k):
    """zoom0's index map of an axis k -> 2k: round(i (k - 1) / (2k - 1))."""
    if k <= 1:
        return np.zeros(2 * k, dtype=np.int64)
    return np.floor(np.arange(2 * k, dtype=np.float64) * ((k - 1) / (2 * k - 1)) + 0.5).astype(np.int64)


def zoom0_x(planes):
    """scipy.ndimage.zoom(planes, (1, 1, 2), order=0): (c, n, m) -> (c, n, 2m)."""
    return planes[:, :, zoom_index(planes.shape[2])]


def zoom1_x(planes):
    """scipy.ndimage.zoom(planes, (1, 1, 2), order=1): float32(v[i0] * w0 +
    v[i1] * w1) summed in double, taps and weights of crossfmt_ref._taps."""
    planes = np.asarray(planes, dtype=F32)
    c0, c1, w0, w1 = R._taps(planes.shape[2])
    v = planes.astype(np.float64)
    return (v[:, :, c0] * w0[None, None, :] + v[:, :, c1] * w1[None, None, :]).astype(F32)


def pair_mean(p):
    """float32 mean of each horizontal pair of (c, h, w): (x0 + x1) / 2."""
    p = np.asarray(p, dtype=F32)
    return (p[:, :, 0::2] + p[:, :, 1::2]) / F32(2)


def up0(uv, chroma):
    sx, sy = sub(chroma)
    return uv if sx == 1 else zoom0_x(uv) if sy == 1 else R.zoom0(uv)


def up1(uv, chroma):
    sx, sy = sub(chroma)
    return np.asarray(uv, dtype=F32) if sx == 1 else zoom1_x(uv) if sy == 1 else R.zoom1(uv)


# ------------------------------------------------------------------ ingest
def ingest_yuv(y, uv, d, chroma, H, W):
    """Rule 1: samples y (h, w), uv (2, h/sy, w/sx) -> padded NHWC 4:4:4 float32."""
    return R.pad_nhwc(np.concatenate((to_float(y, d)[None], up0(to_float(uv, d), chroma)), axis=0), H, W)


def ingest_rgb(y, uv, d, chroma, H, W):
    """Rule 2: (padded NHWC RGB input, planar float32 RGB source (3, h, w))."""
    rgb = R.ycc_to_rgb(to_float(y, d)[None], up1(to_float(uv, d), chroma))
    return R.pad_nhwc(rgb, H, W), rgb


# -------------------------------------------------- distortion and output
def down(planes, chroma, seq_ok=False):
    """The float32 footprint mean of (c, h, w) planes, unclipped.  4:2:0: the
    pairwise (x00 + x01) + (x10 + x11) order of the same-format kernels, or
    with ``seq_ok`` crossfmt_ref.mean2x2's (one-column planes run in sequence)."""
    sx, sy = sub(chroma)
    planes = np.asarray(planes, dtype=F32)
    if sx == 1:
        return planes
    if sy == 1:
        return pair_mean(planes)
    fn = R.mean2x2 if seq_ok else F.mean2x2_pairwise
    return np.concatenate([fn(planes[c:c + 1]) for c in range(planes.shape[0])], axis=0)


def yuv444_planes(crop, chroma):
    """A 4:4:4 frame (3, h, w) as the same-colour-space distortion and writer
    see it: (y (1, h, w) clipped, uv (2, h/sy, w/sx) clipped footprint means)."""
    crop = np.asarray(crop, dtype=F32)
    return np.clip(crop[0:1], F32(0), F32(1)), np.clip(down(crop[1:3], chroma), F32(0), F32(1))


def rgb_planes(crop, chroma):
    """An RGB frame (3, h, w) into YUV planes of ``chroma`` (rule 4)."""
    y, cb, cr = R.rgb_to_ycc(crop)
    uv = down(np.concatenate((cb, cr), axis=0), chroma, seq_ok=True)
    return np.clip(y, F32(0), F32(1)), np.clip(uv, F32(0), F32(1))


def file_frame(crop, d, chroma, from_rgb=False):
    """Rule 4: the decoded crop (3, h, w) as the flat Y | U | V samples of a file."""
    y, uv = rgb_planes(crop, chroma) if from_rgb else yuv444_planes(crop, chroma)
    return np.concatenate((quant(y, d).reshape(-1), quant(uv, d).reshape(-1)))


def sse_yuv(clamped_crop, y, uv, d, chroma):
    """Rule 3: calc_psnr's fp64 sums per plane against the source's samples."""
    y_rec, uv_rec = yuv444_planes(clamped_crop, chroma)
    yf, uvf = to_float(y, d), to_float(uv, d)
    e = [y_rec[0].astype(np.float64) - yf, uv_rec[0].astype(np.float64) - uvf[0],
         uv_rec[1].astype(np.float64) - uvf[1]]
    return np.array([np.sum(np.square(v)) for v in e])


def frame_sizes(h, w, chroma):
    """(luma samples, samples of U and V together) of one frame."""
    sx, sy = sub(chroma)
    return h * w, 2 * (h // sy) * (w // sx)
