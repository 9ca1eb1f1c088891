"""numpy restatement of the cross-format conversions of run_test — TEST
INFRASTRUCTURE ONLY (the product path never imports it).

The reference's readers convert a source of the other format with
DCVC-DC/src/transforms/functional.py:16-72; crossfmt.hip does the same on the
GPU.  This module restates those conversions without scipy, for any shape:

* ``zoom1``: ``scipy.ndimage.zoom(uv, (1, 2, 2), order=1)`` as explicit
  arithmetic.  Output index i of an axis of length 2n samples the input at
  ``cc = i * ((n - 1) / (2n - 1))`` (ratio first, in double); the taps are
  floor(cc) and floor(cc) + 1 (clamped), the weights w0 = 1 - f and
  w1 = 1 - w0 (scipy's 1 - |k - cc| per tap; not always f in the last double
  bit, which decides fp32 ties); the four
  products ``(v * w_row) * w_col`` are summed in double in the order (r0, c0),
  (r0, c1), (r1, c0), (r1, c1) and rounded to float32.
* ``yuv420_to_rgb``: ycbcr420_to_rgb(order=1); ``rgb_to_yuv420``:
  rgb_to_ycbcr420; ``yuv420_to_444``: ycbcr420_to_444(order=0).
* ``pad_nhwc``: np_image_to_tensor + F.pad(replicate) (test_video.py:128-135).

tests/test_crossfmt.py pins every function to the reference's own outputs
(tests/golden/crossfmt_golden.*) and to scipy.
"""
import numpy as np

KR, KG, KB = 0.2126, 0.7152, 0.0722     # ITU-R BT.709
F32 = np.float32


def _taps(n):
    """Taps and double weights of the order-1 zoom of an axis n -> 2n."""
    i = np.arange(2 * n, dtype=np.float64)
    z = (n - 1) / (2 * n - 1) if n > 1 else 0.0
    cc = i * z
    fl = np.floor(cc)
    f = cc - fl
    i0 = np.minimum(fl.astype(np.int64), n - 1)
    i1 = np.minimum(fl.astype(np.int64) + 1, n - 1)
    w0 = 1.0 - f
    return i0, i1, w0, 1.0 - w0


def zoom1(planes):
    """(c, n, m) float32 -> (c, 2n, 2m) float32, bilinear as scipy's zoom."""
    planes = np.asarray(planes, dtype=F32)
    _, n, m = planes.shape
    r0, r1, wr0, wr1 = _taps(n)
    c0, c1, wc0, wc1 = _taps(m)
    v = planes.astype(np.float64)
    wr0, wr1 = wr0[None, :, None], wr1[None, :, None]
    wc0, wc1 = wc0[None, None, :], wc1[None, None, :]
    t = (v[:, r0][:, :, c0] * wr0) * wc0
    t = t + (v[:, r0][:, :, c1] * wr0) * wc1
    t = t + (v[:, r1][:, :, c0] * wr1) * wc0
    t = t + (v[:, r1][:, :, c1] * wr1) * wc1
    return t.astype(F32)


def zoom0(planes):
    """Nearest-neighbour zoom (order=0): index round(i (n - 1) / (2n - 1))."""
    _, n, m = planes.shape

    def idx(k):
        if k <= 1:
            return np.zeros(2 * k, dtype=np.int64)
        return np.floor(np.arange(2 * k, dtype=np.float64) * ((k - 1) / (2 * k - 1)) + 0.5).astype(np.int64)
    return planes[:, idx(n)][:, :, idx(m)]


def ycc_to_rgb(y, uv444):
    """BT.709 YCbCr (1, h, w) + (2, h, w) float32 -> RGB (3, h, w), clipped."""
    y = np.asarray(y, dtype=F32)
    cb, cr = uv444[0:1], uv444[1:2]
    r = y + F32(2 - 2 * KR) * (cr - F32(0.5))
    b = y + F32(2 - 2 * KB) * (cb - F32(0.5))
    g = (y - F32(KR) * r - F32(KB) * b) / F32(KG)
    return np.clip(np.concatenate((r, g, b), axis=0), F32(0), F32(1))


def yuv420_to_rgb(y, uv):
    """float32 y (1, h, w), uv (2, h/2, w/2) -> float32 RGB (3, h, w)."""
    return ycc_to_rgb(y, zoom1(uv))


def mean2x2(p):
    """float32 mean of each 2x2 block of (1, h, w), summed (x00 + x01) +
    (x10 + x11) as numpy's mean over axes (-1, -3) does; a plane two pixels
    wide is one contiguous run of four to numpy: ((x00 + x01) + x10) + x11."""
    x00, x01, x10, x11 = p[:, 0::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 0::2], p[:, 1::2, 1::2]
    if p.shape[2] == 2:
        return (((x00 + x01) + x10) + x11) / F32(4)
    return ((x00 + x01) + (x10 + x11)) / F32(4)


def rgb_to_ycc(rgb):
    """float32 RGB (3, h, w) -> unclipped y, cb, cr (1, h, w) each."""
    rgb = np.asarray(rgb, dtype=F32)
    r, g, b = rgb[0:1], rgb[1:2], rgb[2:3]
    y = F32(KR) * r + F32(KG) * g + F32(KB) * b
    cb = F32(0.5) * (b - y) / F32(1 - KB) + F32(0.5)
    cr = F32(0.5) * (r - y) / F32(1 - KR) + F32(0.5)
    return y, cb, cr


def rgb_to_yuv420(rgb):
    """float32 RGB (3, h, w) -> y (1, h, w), uv (2, h/2, w/2), clipped."""
    y, cb, cr = rgb_to_ycc(rgb)
    uv = np.concatenate((mean2x2(cb), mean2x2(cr)), axis=0)
    return np.clip(y, F32(0), F32(1)), np.clip(uv, F32(0), F32(1))


def yuv444_to_420(yuv):
    """ycbcr444_to_420: y clipped, uv the clipped 2x2 means."""
    yuv = np.asarray(yuv, dtype=F32)
    uv = np.concatenate((mean2x2(yuv[1:2]), mean2x2(yuv[2:3])), axis=0)
    return np.clip(yuv[0:1], F32(0), F32(1)), np.clip(uv, F32(0), F32(1))


def yuv420_to_444(y, uv):
    return np.concatenate((y, zoom0(uv)), axis=0)


def pad_nhwc(chw, H, W):
    """(3, h, w) -> (H, W, 3) replicate-padded at the bottom and right."""
    _, h, w = chw.shape
    return np.ascontiguousarray(np.pad(chw, ((0, 0), (0, H - h), (0, W - w)), mode="edge").transpose(1, 2, 0))


def u8_to_float(a):
    return a.astype(F32) / F32(255)


def ingest_yuv_source_rgb_codec(y_u8, uv_u8, H, W):
    """What a YUV420 source becomes for an RGB codec: (padded NHWC input,
    planar float32 RGB source)."""
    rgb = yuv420_to_rgb(u8_to_float(y_u8)[None], u8_to_float(uv_u8))
    return pad_nhwc(rgb, H, W), rgb


def ingest_rgb_source_yuv_codec(rgb_u8, H, W):
    """What an RGB source becomes for a YUV420 codec: (padded NHWC 4:4:4
    input, float32 y (h, w), float32 uv (2, h/2, w/2))."""
    y, uv = rgb_to_yuv420(u8_to_float(rgb_u8))
    return pad_nhwc(yuv420_to_444(y, uv), H, W), y[0], uv


def quant_u8(v):
    return np.clip(np.rint(v * F32(255)), 0, 255).astype(np.uint8)


def png_bytes_from_444(crop):
    """A YCbCr 4:4:4 frame (3, h, w) into PNGWriter: (h, w, 3) uint8."""
    y, uv = yuv444_to_420(crop)
    return quant_u8(yuv420_to_rgb(y, uv).transpose(1, 2, 0))


def yuv_bytes_from_rgb(crop):
    """An RGB frame (3, h, w) into YUVWriter: Y | U | V uint8 bytes."""
    y, uv = rgb_to_yuv420(crop)
    return quant_u8(y).tobytes() + quant_u8(uv).tobytes()
