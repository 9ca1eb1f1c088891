"""numpy restatement of the high-bit-depth sample rule (INTEGRATION.md
"High-bit-depth frames") and of the frame paths built on it -- TEST
INFRASTRUCTURE ONLY (the product path never imports it).

For a bit depth d in 9..16 and max_val = (1 << d) - 1:

* in:  ``x = float32(sample) / float32(max_val)`` (``to_float``), the
  reference's ``rgb.astype(np.float32) / self.max_val``
  (DCVC-DC/src/utils/video_reader.py:112-113), samples above max_val unclamped;
* out: ``uint16(clip(rint(float32(x) * float32(max_val)), 0, max_val))``
  (``quant``), the reference's RGBWriter (video_writer.py:75).

Everything else is tests/crossfmt_ref.py: the order-0 / order-1 chroma zooms,
BT.709, the 2x2 means, padding.  tests/test_frame16.py pins these functions to
what the reference's own RGBReader / RGBWriter and functional.py produced
(tests/golden/frame16_golden.*, recorded by make_golden_frame16.py).
"""
import numpy as np

from tests import crossfmt_ref as R

F32 = np.float32


def max_val(d):
    if not 9 <= d <= 16:
        raise ValueError(d)
    return (1 << d) - 1


def to_float(a, d):
    a = np.asarray(a)
    assert a.dtype == np.uint16, a.dtype
    return a.astype(F32) / F32(max_val(d))


def quant(v, d):
    mx = max_val(d)
    return np.clip(np.rint(np.asarray(v, dtype=F32) * F32(mx)), 0, mx).astype(np.uint16)


def pad_zero_nhwc(chw, H, W):
    """(3, h, w) -> (H, W, 3) zero-padded at the bottom and right (HEM)."""
    _, h, w = chw.shape
    return np.ascontiguousarray(np.pad(chw, ((0, 0), (0, H - h), (0, W - w))).transpose(1, 2, 0))


# ------------------------------------------------------------------ ingest
def ingest_rgb(rgb16, d, H, W, zero_pad=False):
    """A (3, h, w) uint16 frame for an RGB codec: padded NHWC float32."""
    x = to_float(rgb16, d)
    return pad_zero_nhwc(x, H, W) if zero_pad else R.pad_nhwc(x, H, W)


def ingest_yuv(y16, uv16, d, H, W):
    """uint16 planes y (h, w), uv (2, h/2, w/2) for a YUV420 codec: padded
    NHWC 4:4:4 float32 (ycbcr420_to_444(order=0))."""
    return R.pad_nhwc(R.yuv420_to_444(to_float(y16, d)[None], to_float(uv16, d)), H, W)


def ingest_yuv_source_rgb_codec(y16, uv16, d, H, W):
    """(padded NHWC input, planar float32 RGB source)."""
    rgb = R.yuv420_to_rgb(to_float(y16, d)[None], to_float(uv16, d))
    return R.pad_nhwc(rgb, H, W), rgb


def ingest_rgb_source_yuv_codec(rgb16, d, H, W):
    """(padded NHWC 4:4:4 input, float32 y (h, w), float32 uv (2, h/2, w/2))."""
    y, uv = R.rgb_to_yuv420(to_float(rgb16, d))
    return R.pad_nhwc(R.yuv420_to_444(y, uv), H, W), y[0], uv


# ------------------------------------------------------------------ output
def mean2x2_pairwise(p):
    """float32 2x2 block mean of (1, h, w), always (x00 + x01) + (x10 + x11):
    the summation order of sse_yuvp_kernel / recon_yuvp_kernel (YCbCr frame)."""
    x00, x01, x10, x11 = p[:, 0::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 0::2], p[:, 1::2, 1::2]
    return ((x00 + x01) + (x10 + x11)) / F32(4)


def yuv444_to_420(crop):
    """A 4:4:4 frame (3, h, w) as the same-format YUV writer and distortion
    see it: y clipped, u / v the clipped pairwise 2x2 means."""
    crop = np.asarray(crop, dtype=F32)
    uv = np.concatenate((mean2x2_pairwise(crop[1:2]), mean2x2_pairwise(crop[2:3])), axis=0)
    return np.clip(crop[0:1], F32(0), F32(1)), np.clip(uv, F32(0), F32(1))


def rgb_file_frame(crop, d):
    """An RGB frame (3, h, w) into RGBWriter: planar uint16 (3, h, w)."""
    return quant(crop, d)


def yuv_file_frame(crop, d):
    """A 4:4:4 frame (3, h, w) into a d-bit YUV420 file: Y | U | V uint16, flat."""
    y, uv = yuv444_to_420(crop)
    return np.concatenate((quant(y, d).reshape(-1), quant(uv, d).reshape(-1)))


def rgb_file_frame_from_444(crop, d):
    """A YCbCr 4:4:4 frame into RGBWriter (src_format '420'): ycbcr444_to_420,
    ycbcr420_to_rgb(order=1), quantised; planar uint16 (3, h, w)."""
    y, uv = R.yuv444_to_420(crop)
    return quant(R.yuv420_to_rgb(y, uv), d)


def yuv_file_frame_from_rgb(crop, d):
    """An RGB frame into a d-bit YUV420 file: rgb_to_ycbcr420, quantised."""
    y, uv = R.rgb_to_yuv420(crop)
    return np.concatenate((quant(y, d).reshape(-1), quant(uv, d).reshape(-1)))


# -------------------------------------------------------------- distortion
def sse_rgb(clamped_crop, rgb_f32):
    """PSNR()'s sums (test_video.py:65-68): fp32 difference and square, fp64 sum."""
    e = np.asarray(clamped_crop, dtype=F32) - rgb_f32
    return np.array([np.sum((e[c] * e[c]).astype(np.float64)) for c in range(3)])


def sse_yuv(clamped_crop, y_f32, uv_f32):
    """calc_psnr's sums (metrics.py:81-92) of ycbcr444_to_420 of the crop, fp64."""
    y_rec, uv_rec = yuv444_to_420(clamped_crop)
    e = [y_rec[0].astype(np.float64) - y_f32, uv_rec[0].astype(np.float64) - uv_f32[0],
         uv_rec[1].astype(np.float64) - uv_f32[1]]
    return np.array([np.sum(np.square(v)) for v in e])
