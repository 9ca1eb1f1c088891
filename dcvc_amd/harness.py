"""The test harness around the codecs: ``run_test`` of DCVC-DC/test_video.py:
71-237 (RGB and YUV420 sources, I/P schedule, DPB aliasing, in-place clamp,
crop, PSNR, the JSON log of src/utils/common.py:44-140) and of
DCVC-HEM/test_video.py:80-172, with the per-frame tensor work on the GPU.

Source frames cross to the GPU as uint8 (a quarter of the reference's fp32
upload).  ``FrameStage`` turns them into the padded NHWC codec input
(``dcvc_frame_to_nhwc`` / ``dcvc_yuv420_to_nhwc``) and computes each frame's
distortion with ``dcvc_frame_sse``, which also performs
``recon_frame.clamp_(0, 1)`` on the DPB frame in place.  The squared-error
sums stay on the device until the end of the sequence (one transfer), and the
PSNR formulas are evaluated on the host exactly as the reference writes them.

The source format and the codec format are independent (test_video.py:79-119,
video_reader.py:33-42): a YUV420 file can feed an RGB model and a PNG folder a
YUV420 model.  The readers always hand over their native uint8 planes;
``FrameStage(src_format=...)`` converts on the GPU (crossfmt.hip:
``ycbcr420_to_rgb(order=1)`` or ``rgb_to_ycbcr420`` + ``ycbcr420_to_444``,
bit-equal to the reference's numpy / scipy values), keeps the converted fp32
source planes on the device, and the distortion and MS-SSIM compare against
those (``dcvc_frame_sse_f32``, ``dcvc_*_planes_f64_f32``).  The decoded-frame
writers' cross cases are quantised on the GPU too (``dcvc_recon_to_u8_cross``).

MS-SSIM: for YUV420 sources ``calc_ssim`` runs the reference's per-plane
``calc_msssim`` (src/utils/metrics.py:39-62) on the GPU in fp64 (``MsSsim``,
msssim.hip), pinned to the reference's outputs.  RGB MS-SSIM is
``pytorch_msssim.ms_ssim`` in the reference (DC and HEM), a package absent
from this image: ``MsSsimRGB`` follows its published algorithm on the GPU and
the log carries ``msssim_unpinned``.

High bit depth: raw planar .rgb (``RGBReader``, the reference's) and YUV420
files of 9..16 bits per sample hand over uint16 frames, which cross to the GPU
as they are; a sample is x / ((1 << d) - 1).  A source of the codec's format is
read by the 16-bit kernels directly (frame16.hip), the cross-format ingest and
MS-SSIM go through fp32 planes, and ``ReconWriter`` stores uint16 out.yuv /
out.rgb.  8 bits is the uint8 code, unchanged.

Chroma layouts: planar YUV 4:2:2 and 4:4:4 files (``src_type`` "yuv422" /
"yuv444", 8..16 bits) go through chroma.hip.  The YUV codecs code a 4:4:4
tensor, so a 4:4:4 source is taken as it is and a 4:2:2 source is resampled
along x only; distortion and out.yuv are at the source's own chroma
resolution.  4:2:0 stays on the kernels above.
"""
import contextlib
import os
import time

import numpy as np
import torch

from . import hip as K
from .stream_helper import get_padding_size


# ----------------------------------------------------------------- readers
def _check_bit_depth(bit_depth):
    if not isinstance(bit_depth, int) or isinstance(bit_depth, bool) or not 8 <= bit_depth <= 16:
        raise ValueError(f"bit depth {bit_depth!r} is outside 8..16")
    return bit_depth


def _sample_dtype(bit_depth):
    """uint8 at 8 bits, little-endian uint16 at 9..16 (video_reader.py:93-98)."""
    return np.dtype(np.uint8) if _check_bit_depth(bit_depth) == 8 else np.dtype("<u2")


def _frame_index(index):
    if not isinstance(index, (int, np.integer)) or isinstance(index, bool) or index < 0:
        raise ValueError(f"frame index {index!r} is not a non-negative int")
    return int(index)


def _pread(file, n, offset):
    """Up to ``n`` bytes of ``file`` at ``offset``, without moving its cursor
    (and so safe beside sequential reads of the same object)."""
    chunks = []
    while n > 0:
        b = os.pread(file.fileno(), n, offset)
        if not b:
            break
        chunks.append(b)
        n -= len(b)
        offset += len(b)
    return chunks[0] if len(chunks) == 1 else b"".join(chunks)


class YUVReader:
    """Raw YUV420 file reader (DCVC-DC/src/utils/video_reader.py:121-161).
    ``read_one_frame`` returns uint8 ``(y (h, w), uv (2, h/2, w/2))``, or
    ``(None, None)`` at the end of the file, whatever ``dst_format`` the codec
    wants; the reference's float conversion (x / 255) and, for an RGB codec,
    its ycbcr420_to_rgb happen on the GPU (FrameStage).  ``bit_depth`` 9..16
    (beyond the reference, whose YUVReader is 8-bit): little-endian uint16
    samples, full range like the 8-bit rule, returned as uint16 planes; frame
    and skip sizes double.  ``src_format`` "422" | "444" (beyond the reference,
    which stops at "420"): the same planar layout with chroma planes of
    h x w/2 or h x w samples; ``uv`` is then (2, h, w/2) or (2, h, w).  The
    layout belongs to the file, so it is this constructor's argument and never
    a ``dst_format``."""

    def __init__(self, src_path, width, height, src_format="420", skip_frame=0, bit_depth=8):
        if src_format not in K.CHROMA_FORMATS:
            raise ValueError(f"unknown src_format {src_format!r}: a YUV file is '420', '422' or '444'")
        self.src_format = src_format
        self.sub_x, self.sub_y = K.CHROMA_FORMATS[src_format]
        if src_format == "420" and _check_bit_depth(bit_depth) > 8 and (width % 2 or height % 2):
            raise ValueError(f"a 4:2:0 file needs even sizes, not {width} x {height}")
        if src_format == "422" and width % 2:
            raise ValueError(f"a 4:2:2 file needs an even width, not {width} x {height}")
        if not src_path.endswith(".yuv"):
            src_path = src_path + ".yuv"
        self.src_path, self.width, self.height = src_path, width, height
        self.bit_depth, self.dtype = bit_depth, _sample_dtype(bit_depth)
        self.y_size = width * height * self.dtype.itemsize
        if src_format == "420":
            self.uv_size = width * height // 2 * self.dtype.itemsize
        else:
            self.uv_size = 2 * (height // self.sub_y) * (width // self.sub_x) * self.dtype.itemsize
        self.eof = False
        self.skip_frame = skip_frame
        self.file = open(src_path, "rb")  # noqa: SIM115 (closed in close())
        for _ in range(skip_frame):
            if not self._read():
                break

    def _read(self):
        y = self.file.read(self.y_size)
        uv = self.file.read(self.uv_size)
        if len(y) < self.y_size or len(uv) < self.uv_size:
            self.eof = True
            return None
        return y, uv

    def read_one_frame(self, dst_format="420"):
        if dst_format not in ("420", "rgb"):
            raise ValueError(f"unknown dst_format {dst_format!r}")
        if self.eof:
            return None, None
        r = self._read()
        if r is None:
            return None, None
        return self._planes(*r)

    def _planes(self, y, uv):
        return (np.frombuffer(y, dtype=self.dtype).reshape(self.height, self.width),
                np.frombuffer(uv, dtype=self.dtype).reshape(2, self.height // self.sub_y, self.width // self.sub_x))

    def read_frame(self, index, dst_format="420"):
        """What the ``index``-th ``read_one_frame`` of a fresh reader returns
        (frames skipped by ``skip_frame`` not counted), by one positional read
        that leaves the sequential cursor alone."""
        if dst_format not in ("420", "rgb"):
            raise ValueError(f"unknown dst_format {dst_format!r}")
        size = self.y_size + self.uv_size
        data = _pread(self.file, size, (self.skip_frame + _frame_index(index)) * size)
        if len(data) < size:
            return None, None
        return self._planes(data[:self.y_size], data[self.y_size:])

    def close(self):
        self.file.close()


class RGBReader:
    """Raw planar RGB file reader (video_reader.py:83-118): 3 x h x w samples
    per frame, uint8 or, at ``bit_depth`` 9..16, little-endian uint16; ".rgb"
    is appended to a path that lacks it.  ``read_one_frame`` returns the CHW
    frame in its native type, or None at the end of the file (a last frame
    that is cut short counts as the end); the reference's float conversion
    (x / max_val) and, for a YUV420 codec, its rgb_to_ycbcr420 happen on the
    GPU (FrameStage)."""

    def __init__(self, src_path, width, height, bit_depth=8):
        if not src_path.endswith(".rgb"):
            src_path = src_path + ".rgb"
        self.src_path, self.width, self.height = src_path, width, height
        self.bit_depth, self.dtype = bit_depth, _sample_dtype(bit_depth)
        self.max_val = (1 << bit_depth) - 1
        self.rgb_size = width * height * 3 * self.dtype.itemsize
        self.eof = False
        self.file = open(src_path, "rb")  # noqa: SIM115 (closed in close())

    def read_one_frame(self, dst_format="rgb"):
        if dst_format not in ("rgb", "420"):
            raise ValueError(f"unknown dst_format {dst_format!r}")
        if self.eof:
            return None
        rgb = self.file.read(self.rgb_size)
        if len(rgb) < self.rgb_size:
            self.eof = True
            return None
        return np.frombuffer(rgb, dtype=self.dtype).reshape(3, self.height, self.width)

    def read_frame(self, index, dst_format="rgb"):
        """What the ``index``-th ``read_one_frame`` of a fresh reader returns,
        by one positional read that leaves the sequential cursor alone."""
        if dst_format not in ("rgb", "420"):
            raise ValueError(f"unknown dst_format {dst_format!r}")
        rgb = _pread(self.file, self.rgb_size, _frame_index(index) * self.rgb_size)
        if len(rgb) < self.rgb_size:
            return None
        return np.frombuffer(rgb, dtype=self.dtype).reshape(3, self.height, self.width)

    def close(self):
        self.file.close()


class PNGReader:
    """Folder of im1.png / im00001.png frames (video_reader.py:44-80);
    returns uint8 CHW RGB, or None at the end, whatever ``dst_format`` the
    codec wants (FrameStage converts for a YUV420 codec)."""

    def __init__(self, src_path, width, height, start_num=1):
        pngs = os.listdir(src_path)
        if "im1.png" in pngs:
            self.padding = 1
        elif "im00001.png" in pngs:
            self.padding = 5
        else:
            raise ValueError("unknown image naming convention; please specify")
        self.src_path, self.width, self.height = src_path, width, height
        self.start_num = self.current_frame_index = start_num
        self.eof = False

    def _load(self, number):
        """im<number>.png as uint8 CHW RGB, or None when there is no such file."""
        from PIL import Image
        p = os.path.join(self.src_path, f"im{str(number).zfill(self.padding)}.png")
        if not os.path.exists(p):
            return None
        rgb = np.asarray(Image.open(p).convert("RGB")).transpose(2, 0, 1)
        if rgb.shape[1:] != (self.height, self.width):
            raise ValueError(f"{p}: {rgb.shape[1:]} != {(self.height, self.width)}")
        return np.ascontiguousarray(rgb)

    def read_one_frame(self, dst_format="rgb"):
        if dst_format not in ("rgb", "420"):
            raise ValueError(f"unknown dst_format {dst_format!r}")
        if self.eof:
            return None
        rgb = self._load(self.current_frame_index)
        if rgb is None:
            self.eof = True
            return None
        self.current_frame_index += 1
        return rgb

    def read_frame(self, index, dst_format="rgb"):
        """What the ``index``-th ``read_one_frame`` of a fresh reader returns
        of a folder numbered without gaps: the file ``start_num + index``, or
        None when there is none.  The sequential cursor stays where it is."""
        if dst_format not in ("rgb", "420"):
            raise ValueError(f"unknown dst_format {dst_format!r}")
        return self._load(self.start_num + _frame_index(index))

    def close(self):
        self.current_frame_index = 1


class ArrayReader:
    """In-memory frames (synthetic sequences, tests): uint8 CHW RGB arrays,
    or (y, uv) uint8 plane pairs for YUV420; uint16 arrays for a 9..16-bit
    source (FrameStage's ``bit_depth`` says how many bits they hold)."""

    def __init__(self, frames):
        self.frames = list(frames)
        self.i = 0

    def read_one_frame(self, dst_format="rgb"):
        if self.i >= len(self.frames):
            return (None, None) if dst_format == "420" else None
        f = self.frames[self.i]
        self.i += 1
        return f

    def read_frame(self, index, dst_format="rgb"):
        """Frame ``index`` (what the ``index``-th ``read_one_frame`` returns);
        no state, so one reader can serve several threads."""
        if _frame_index(index) >= len(self.frames):
            return (None, None) if dst_format == "420" else None
        return self.frames[index]

    def close(self):
        pass


# ----------------------------------------------------------- device staging
class FrameStage:
    """Device side of one sequence: uint8 source upload, padded NHWC codec
    input, and the per-frame squared-error sums (frame_num x 3, fp64).

    ``src_format`` ("rgb" | "420") is what the reader hands over; it defaults
    to the codec's own format (``yuv420``).  When it differs, ``load`` converts
    the frame on the GPU and keeps the converted fp32 source planes
    (``src_f32``: (rgb 3 x h x w,) or (y, uv)) for ``distortion`` and MS-SSIM:
    the frame the reference's reader would have returned.

    ``bit_depth`` 9..16: the frames are uint16 (x / ((1 << bit_depth) - 1)),
    uploaded as they are.  A source of the codec's format is read directly by
    the 16-bit kernels (frame16.hip); one of the other format is first turned
    into fp32 planes (``dcvc_u16_to_f32``) and then converted as above.  8 is
    the uint8 code, untouched.

    ``src_format`` "422" | "444": (y, uv) planes of a planar YUV source in that
    chroma layout, at any depth (chroma.hip).  For a YUV codec the planes are
    taken as they are (4:2:2: zoomed along x) and the distortion is measured at
    the source's chroma resolution; for an RGB codec they are converted
    (``src_f32``: the planar fp32 RGB source) as a 4:2:0 source is."""

    def __init__(self, h, w, align, yuv420, zero_pad, frame_num, device, src_format=None, bit_depth=8):
        self.h, self.w, self.yuv, self.zero_pad = h, w, yuv420, zero_pad
        codec_format = "420" if yuv420 else "rgb"
        src_format = codec_format if src_format is None else src_format
        if src_format not in ("rgb", "420", "422", "444"):
            raise ValueError(f"unknown src_format {src_format!r}")
        self.bit_depth = _check_bit_depth(bit_depth)
        self.deep = bit_depth > 8
        self.src_yuv = src_format != "rgb"
        # a 4:2:2 / 4:4:4 source (chroma.hip): its layout; None for the older paths
        self.chroma = src_format if src_format in ("422", "444") else None
        if self.chroma is None and self.deep and (self.src_yuv or yuv420) and (h % 2 or w % 2):
            raise ValueError(f"4:2:0 needs even sizes, not {w} x {h}")
        if self.chroma == "422" and w % 2:
            raise ValueError(f"4:2:2 needs an even width, not {w} x {h}")
        if self.chroma is not None and zero_pad:
            raise ValueError("a 4:2:2 / 4:4:4 source is padded by replication")
        self.cross = self.src_yuv != bool(yuv420)
        self.src_f32 = None
        self.raw_f32 = None       # bit_depth > 8: the uint16 source as fp32 planes (cross ingest, MS-SSIM)
        if self.cross:
            if zero_pad or (self.chroma is None and (h % 2 or w % 2)):
                raise ValueError("a converted source needs even sizes and replicate padding")
            if yuv420:
                self.src_f32 = (torch.empty((h, w), dtype=torch.float32, device=device),
                                torch.empty((2, h // 2, w // 2), dtype=torch.float32, device=device))
            else:
                self.src_f32 = (torch.empty((3, h, w), dtype=torch.float32, device=device),)
        _, pr, _, pb = get_padding_size(h, w, align)
        self.H, self.W = h + pb, w + pr
        self.dev = device
        self.x = K.empty(self.H, self.W, 3, K.F32, device)
        self.ws = K.frame_sse_workspace(device)
        self.sse = torch.zeros((max(frame_num, 1), 3), dtype=torch.float64, device=device)

    def _up(self, a, key):
        if self.deep:
            a = np.asarray(a)
            if a.dtype != np.uint16:
                raise ValueError(f"a {self.bit_depth}-bit source hands over uint16 frames, not {a.dtype}")
            a = a.view(np.int16)          # the same bits: torch moves int16 on every build
        return K.upload(a, self.dev, key)

    def upload(self, frame):
        """Host frame (CHW RGB, or (y, uv); uint8, or uint16 above 8 bits) ->
        device tensors."""
        if self.src_yuv:
            y, uv = frame
            return self._up(y, "frame_y"), self._up(uv, "frame_uv")
        return self._up(frame, "frame")

    def _raw_f32(self, dframe):
        """The 16-bit source as fp32 planes x / max_val in its own layout."""
        h, w = self.h, self.w
        if self.raw_f32 is None:
            shapes = ((h, w), (2, h // 2, w // 2)) if self.src_yuv else ((3, h, w),)
            self.raw_f32 = tuple(torch.empty(s, dtype=torch.float32, device=self.dev) for s in shapes)
        for src, dst in zip(dframe if self.src_yuv else (dframe,), self.raw_f32):
            K.u16_to_f32(src, self.bit_depth, dst)
        return self.raw_f32

    def source_f32(self, dframe):
        """The fp32 source planes MS-SSIM compares against ((rgb,) or (y, uv)
        in the codec's format), or None for an 8-bit source of the codec's own
        format (whose uint8 planes the metrics read directly).  After ``load``
        of the same frame."""
        if self.cross:
            return self.src_f32
        if self.chroma is not None:
            raise ValueError("MS-SSIM of a 4:2:2 / 4:4:4 source on a YUV codec is not supported")
        return self._raw_f32(dframe) if self.deep else None

    def load(self, dframe):
        """Device source frame -> padded NHWC fp32 codec input (test_video.py:
        108-132: ycbcr420_to_444(order=0) for YUV, x / 255, F.pad; for a source
        of the other format, the reader's conversion first)."""
        if self.chroma is not None:     # 4:2:2 / 4:4:4 planes, any depth (chroma.hip)
            if self.cross:
                K.yuvp_to_rgb_nhwc(dframe[0], dframe[1], self.h, self.w, self.bit_depth, self.chroma, self.x,
                                   self.src_f32[0])
            else:
                K.yuvp_to_nhwc(dframe[0], dframe[1], self.h, self.w, self.bit_depth, self.chroma, self.x)
            return self.x
        if self.deep:
            return self._load16(dframe)
        if self.cross and self.yuv:
            K.rgb_to_yuv420_planes(dframe, self.h, self.w, *self.src_f32)
            K.yuv420f_to_nhwc(self.src_f32[0], self.src_f32[1], self.h, self.w, self.x)
        elif self.cross:
            K.yuv420_to_rgb_nhwc(dframe[0], dframe[1], self.h, self.w, self.x, self.src_f32[0])
        elif self.yuv:
            K.yuv420_to_nhwc(dframe[0], dframe[1], self.h, self.w, self.x)
        else:
            K.frame_to_nhwc(dframe, self.h, self.w, self.x, zero_pad=self.zero_pad)
        return self.x

    def _load16(self, dframe):
        h, w, d = self.h, self.w, self.bit_depth
        if self.cross and self.yuv:
            K.rgbf_to_yuv420_planes(self._raw_f32(dframe)[0], h, w, *self.src_f32)
            K.yuv420f_to_nhwc(self.src_f32[0], self.src_f32[1], h, w, self.x)
        elif self.cross:
            yf, uvf = self._raw_f32(dframe)
            K.yuv420f_to_rgb_nhwc(yf, uvf, h, w, self.x, self.src_f32[0])
        elif self.yuv:
            K.yuv420p16_to_nhwc(dframe[0], dframe[1], h, w, d, self.x)
        else:
            K.frame16_to_nhwc(dframe, h, w, d, self.x, zero_pad=self.zero_pad)
        return self.x

    def distortion(self, recon, dframe, slot):
        """recon_frame.clamp_(0, 1), crop, and the squared-error sums of the
        frame into row ``slot`` (test_video.py:169-195)."""
        from .dc.video_model import as_act
        r = as_act(recon)
        if self.cross and self.yuv:
            K.frame_sse_f32(r, self.src_f32[0], self.h, self.w, self.ws, self.sse[slot], uv_f32=self.src_f32[1])
        elif self.cross:
            K.frame_sse_f32(r, self.src_f32[0], self.h, self.w, self.ws, self.sse[slot])
        elif self.chroma is not None:
            K.yuvp_sse(r, dframe[0], dframe[1], self.h, self.w, self.bit_depth, self.chroma, self.ws, self.sse[slot])
        elif self.deep and self.yuv:
            K.frame16_sse(r, dframe[0], self.h, self.w, self.bit_depth, self.ws, self.sse[slot], uv_u16=dframe[1])
        elif self.deep:
            K.frame16_sse(r, dframe, self.h, self.w, self.bit_depth, self.ws, self.sse[slot])
        elif self.yuv:
            K.frame_sse(r, dframe[0], self.h, self.w, self.ws, self.sse[slot], uv_u8=dframe[1])
        else:
            K.frame_sse(r, dframe, self.h, self.w, self.ws, self.sse[slot])

    def sums(self):
        return self.sse.cpu().numpy()


class MsSsim:
    """calc_msssim (DCVC-DC/src/utils/metrics.py:39-62) of the three planes of
    a YUV420 frame, test_video.py:182-185: per level, the means of the ssim
    and cs maps on the GPU (dcvc_ssim_level), the 2x2 reflect downsample
    (dcvc_down2_f64); the weighted product on the host."""

    W5 = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
    W4 = np.array([0.0517, 0.3295, 0.3462, 0.2726])

    def __init__(self, h, w, frame_num, device):
        if min(h // 2, w // 2) < 88:
            raise ValueError("calc_msssim needs planes of at least 88 x 88 (metrics.py:49-50)")
        self.h, self.w, self.dev = h, w, device
        n = h * w + 2 * (h // 2) * (w // 2)
        self.src = torch.empty(n, dtype=torch.float64, device=device)
        self.rec = torch.empty(n, dtype=torch.float64, device=device)
        x, y = np.mgrid[-5:6, -5:6]                         # fspecial_gauss(11, 1.5), metrics.py:9-12
        g = np.exp(-((x ** 2 + y ** 2) / (2.0 * 1.5 ** 2)))
        self.win = torch.from_numpy(g / g.sum()).to(device)
        self.ws = torch.empty(int(K.lib().dcvc_ssim_workspace()) // 8, dtype=torch.float64, device=device)
        self.out = torch.zeros((max(frame_num, 1), 3, 5, 2), dtype=torch.float64, device=device)
        self.planes = []                                    # (offset, ph, pw, levels, level buffers)
        off = 0
        for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
            L = 5 if ph >= 176 and pw >= 176 else 4
            bufs, sh, sw = [], ph, pw
            for _ in range(L - 1):
                sh, sw = (sh + 1) // 2, (sw + 1) // 2
                bufs.append((torch.empty(sh * sw, dtype=torch.float64, device=device),
                             torch.empty(sh * sw, dtype=torch.float64, device=device), sh, sw))
            self.planes.append((off, ph, pw, L, bufs))
            off += ph * pw

    def run(self, x_hat, y_u8, uv_u8, slot):
        K.yuv_planes_f64(x_hat, y_u8, uv_u8, self.h, self.w, self.src, self.rec)
        self._levels(slot)

    def run_f32(self, x_hat, y_f32, uv_f32, slot):
        """``run`` against fp32 source planes (FrameStage.src_f32 of an RGB source)."""
        K.yuv_planes_f64_f32(x_hat, y_f32, uv_f32, self.h, self.w, self.src, self.rec)
        self._levels(slot)

    def _levels(self, slot):
        for p, (off, ph, pw, L, bufs) in enumerate(self.planes):
            a, b, sh, sw = self.src[off:off + ph * pw], self.rec[off:off + ph * pw], ph, pw
            for k in range(L):
                K.ssim_level(a, b, sh, sw, self.win, self.ws, self.out[slot, p, k])
                if k < L - 1:
                    na, nb, nh, nw = bufs[k]
                    K.down2_f64(a, sh, sw, na)
                    K.down2_f64(b, sh, sw, nb)
                    a, b, sh, sw = na, nb, nh, nw

    def values(self, n):
        """(msssim_y, msssim_u, msssim_v, (6 y + u + v) / 8) per frame."""
        o = self.out[:n].cpu().numpy()
        res = []
        for f in range(n):
            v = []
            for p, (_, _, _, L, _) in enumerate(self.planes):
                wgt = self.W5 if L == 5 else self.W4
                mssim, mcs = o[f, p, :L, 0], o[f, p, :L, 1]
                v.append(float(np.prod(mcs[0:L - 1] ** wgt[0:L - 1]) * (mssim[L - 1] ** wgt[L - 1])))
            res.append((v[0], v[1], v[2], (6 * v[0] + v[1] + v[2]) / 8))
        return res


class MsSsimRGB:
    """pytorch_msssim.ms_ssim(x_hat, x, data_range=1) as DCVC-DC/test_video.py:188
    and DCVC-HEM/test_video.py:153 call it, on the GPU in fp64.  The package is
    not installed here, so this follows its published algorithm (5 levels,
    weights W5, Gaussian 11 / 1.5 'valid' statistics (dcvc_ssim_level), relu on
    cs and ssim, F.avg_pool2d(2, padding=size % 2) between levels
    (dcvc_avgpool2_f64), mean over the 3 channels); parity unpinned."""

    def __init__(self, h, w, frame_num, device):
        if min(h, w) <= 160:
            raise ValueError("ms_ssim needs the smaller side > (11 - 1) * 2**4")
        self.h, self.w = h, w
        n = 3 * h * w
        self.src = torch.empty(n, dtype=torch.float64, device=device)
        self.rec = torch.empty(n, dtype=torch.float64, device=device)
        x = np.arange(11, dtype=np.float64) - 5
        g = np.exp(-(x ** 2) / (2 * 1.5 ** 2))
        g /= g.sum()
        self.win = torch.from_numpy(np.outer(g, g)).to(device)
        self.ws = torch.empty(int(K.lib().dcvc_ssim_workspace()) // 8, dtype=torch.float64, device=device)
        self.out = torch.zeros((max(frame_num, 1), 3, 5, 2), dtype=torch.float64, device=device)
        self.bufs, sh, sw = [], h, w
        for _ in range(4):
            sh, sw = (sh + 2 * (sh % 2) - 2) // 2 + 1, (sw + 2 * (sw % 2) - 2) // 2 + 1
            self.bufs.append([torch.empty(sh * sw, dtype=torch.float64, device=device) for _ in range(6)] + [sh, sw])

    def run(self, x_hat, src_u8, slot):
        K.rgb_planes_f64(x_hat, src_u8, self.h, self.w, self.src, self.rec)
        self._levels(slot)

    def run_f32(self, x_hat, src_f32, slot):
        """``run`` against a planar fp32 source (FrameStage.src_f32 of a YUV420 source)."""
        K.rgb_planes_f64_f32(x_hat, src_f32, self.h, self.w, self.src, self.rec)
        self._levels(slot)

    def _levels(self, slot):
        n = self.h * self.w
        for c in range(3):
            a, b, sh, sw = self.src[c * n:(c + 1) * n], self.rec[c * n:(c + 1) * n], self.h, self.w
            for k in range(5):
                K.ssim_level(a, b, sh, sw, self.win, self.ws, self.out[slot, c, k])
                if k < 4:
                    bufs = self.bufs[k]
                    na, nb, nh, nw = bufs[2 * c], bufs[2 * c + 1], bufs[6], bufs[7]
                    K.avgpool2_f64(a, sh, sw, na)
                    K.avgpool2_f64(b, sh, sw, nb)
                    a, b, sh, sw = na, nb, nh, nw

    def values(self, n):
        o = self.out[:n].cpu().numpy()
        res = []
        for f in range(n):
            per = []
            for c in range(3):
                mcs = np.maximum(o[f, c, :4, 1], 0.0)
                ssim = max(o[f, c, 4, 0], 0.0)
                per.append(float(np.prod(np.append(mcs, ssim) ** MsSsim.W5)))
            res.append(float(np.mean(per)))
        return res


class ReconWriter:
    """--save_decoded_frame: PNGWriter (im00001.png, ...) and YUVWriter
    (out.yuv) of DCVC-DC/src/utils/video_writer.py:26-111 as test_video.py:
    84-88, 210-221 drives them, and DCVC-HEM's save_torch_image
    ({frame_idx}.png, DCVC-HEM/test_video.py:68-71, 161-163).

    The decoded frame is quantised on the GPU (dcvc_recon_to_u8: the crop,
    clip(rint(v * 255)), and for YUV the ycbcr444_to_420 chroma means), copied
    once to pinned memory, and written by one background thread in frame order
    so file encoding overlaps the next frame.  kind: "png" | "yuv" | "hem_png" |
    "rgb" (RGBWriter's raw planar out.rgb, video_writer.py:50-80);
    src_format "rgb" | "420" (what the codec's frames hold, dist_in_yuv420).
    ``bit_depth`` 9..16: "yuv" and "rgb" store little-endian uint16 samples,
    clip(rint(v * max_val)) on the GPU (dcvc_recon_to_u16 / _cross); PNG output
    stays 8-bit.
    The reference's cross cases (a 4:2:0 frame into PNGWriter, an RGB frame into
    YUVWriter, functional.py:16-58) are converted and quantised on the GPU as
    well (dcvc_recon_to_u8_cross) and take the same pinned-copy path.
    ``chroma`` "422" | "444" (kind "yuv" only): out.yuv in that planar layout,
    from either codec format and at any depth (dcvc_recon_to_yuvp)."""

    def __init__(self, path, h, w, kind, src_format, device, bit_depth=8, chroma="420"):
        from concurrent.futures import ThreadPoolExecutor
        if kind not in ("png", "yuv", "hem_png", "rgb"):
            raise ValueError(f"unknown writer kind {kind!r}")
        if chroma not in K.CHROMA_FORMATS:
            raise ValueError(f"unknown chroma format {chroma!r}")
        if chroma != "420" and kind != "yuv":
            raise ValueError(f"chroma {chroma!r} is the layout of an out.yuv file, not of {kind!r} output")
        self.bit_depth = _check_bit_depth(bit_depth)
        self.deep = bit_depth > 8
        # out.yuv at 4:2:2 / 4:4:4 (dcvc_recon_to_yuvp, either codec format); None: the older paths
        self.chroma = chroma if chroma != "420" else None
        if self.deep and kind in ("png", "hem_png"):
            raise ValueError(f"PNG output is 8-bit; write {bit_depth}-bit frames as 'rgb' or 'yuv'")
        if self.chroma is None and self.deep and (kind == "yuv" or src_format == "420") and (h % 2 or w % 2):
            raise ValueError(f"4:2:0 needs even sizes, not {w} x {h}")
        if self.chroma == "422" and w % 2:
            raise ValueError(f"4:2:2 needs an even width, not {w} x {h}")
        os.makedirs(path, exist_ok=True)
        self.path, self.h, self.w, self.kind, self.fmt = path, h, w, kind, src_format
        self.yuv_out = kind == "yuv"
        self.quant_yuv = src_format == "420"
        self.cross = self.quant_yuv != self.yuv_out
        if self.chroma is not None:
            self.n = sum(K.yuvp_sizes(h, w, chroma)[2:])
        else:
            self.n = h * w + 2 * (h // 2) * (w // 2) if self.yuv_out else 3 * h * w
        self.dtype = torch.int16 if self.deep else torch.uint8      # uint16 bits travel as int16
        self.dev_buf = torch.empty(self.n, dtype=self.dtype, device=device)
        self.pool = ThreadPoolExecutor(1)
        self.jobs = []
        self.index = 1                              # PNGWriter.current_frame_index starts at 1
        self.file = None
        if kind in ("yuv", "rgb"):                  # YUVWriter / RGBWriter: out.yuv / out.rgb in the folder
            self.file = open(os.path.join(path, "out." + kind), "wb")  # noqa: SIM115 (closed in close())

    def write(self, recon, frame_idx):
        from .dc.video_model import as_act
        x = as_act(recon)
        if self.chroma is not None:
            K.recon_to_yuvp(x, self.h, self.w, self.bit_depth, self.chroma, not self.quant_yuv, self.dev_buf)
        elif self.deep and self.cross:
            K.recon_to_u16_cross(x, self.h, self.w, self.bit_depth, not self.yuv_out, self.dev_buf)
        elif self.deep:
            K.recon_to_u16(x, self.h, self.w, self.bit_depth, self.quant_yuv, self.dev_buf)
        elif self.cross:
            K.recon_to_u8_cross(x, self.h, self.w, not self.yuv_out, self.dev_buf)
        else:
            K.recon_to_u8(x, self.h, self.w, self.quant_yuv, self.dev_buf)
        host = torch.empty(self.n, dtype=self.dtype, pin_memory=True)
        host.copy_(self.dev_buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        name = (f"im{str(self.index).zfill(5)}.png" if self.kind == "png" else f"{frame_idx}.png")
        self.index += 1
        self.jobs.append(self.pool.submit(self._emit, host, ev, name))

    def _emit(self, host, ev, name):
        ev.synchronize()
        a = host.numpy()
        h, w = self.h, self.w
        if self.yuv_out:
            self.file.write(a.tobytes())            # Y plane then U, V planes (YUVWriter)
            return
        if self.kind == "rgb":                      # RGBWriter: planar 3 x h x w
            if not self.deep:                       # the uint8 kernels quantise into h x w x 3
                a = np.ascontiguousarray(a.reshape(h, w, 3).transpose(2, 0, 1))
            self.file.write(a.tobytes())
            return
        from PIL import Image
        Image.fromarray(a.reshape(h, w, 3)).save(os.path.join(self.path, name))

    def close(self):
        """Drain the writer thread and close out.yuv (idempotent)."""
        try:
            for j in self.jobs:
                j.result()
        finally:
            self.jobs = []
            self.pool.shutdown()
            if self.file is not None:
                self.file.close()
                self.file = None

    # run_test holds the writer in a `with`: on an exception mid-sequence the
    # queued frames are still written and the file closed
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def psnr_rgb(sse3, h, w):
    """PSNR() of test_video.py:65-68: mse = mean((x_hat - x)^2) as an fp32
    tensor, psnr = 20 * log10(1 / sqrt(mse)) in fp32."""
    mse = torch.tensor(float(np.sum(sse3)) / (3.0 * h * w), dtype=torch.float32)
    return (20 * torch.log10(1 / torch.sqrt(mse))).item()


def calc_psnr_from_sse(sse, n, data_range=1.0):
    """calc_psnr (src/utils/metrics.py:81-92) from an fp64 squared-error sum."""
    mse = sse / n
    if mse > 1e-10:
        return 10 * np.log10(data_range * data_range / mse)
    return 999.9


def psnr_yuv(sse3, h, w, chroma="420"):
    """(psnr_y, psnr_u, psnr_v, (6 y + u + v) / 8), test_video.py:177-181;
    the chroma planes have the size of the source's ``chroma`` format."""
    sx, sy = K.chroma_sub(chroma)
    py = calc_psnr_from_sse(sse3[0], h * w)
    pu = calc_psnr_from_sse(sse3[1], (h // sy) * (w // sx))
    pv = calc_psnr_from_sse(sse3[2], (h // sy) * (w // sx))
    return py, pu, pv, (6 * py + pu + pv) / 8


# ---------------------------------------------------------------- run_test
def generate_log_json(frame_num, frame_pixel_num, test_time, frame_types, bits, psnrs, ssims,
                      psnrs_y=None, psnrs_u=None, psnrs_v=None, ssims_y=None, ssims_u=None, ssims_v=None,
                      verbose=False):
    """DCVC-DC/src/utils/common.py:44-140 (same keys and averages)."""
    yuv = psnrs_y is not None
    acc = {k: {"bits": 0, "psnr": 0, "ssim": 0, "y": 0, "u": 0, "v": 0, "sy": 0, "su": 0, "sv": 0, "n": 0}
           for k in (0, 1)}
    for i in range(frame_num):
        a = acc[0 if frame_types[i] == 0 else 1]
        a["bits"] += bits[i]
        a["psnr"] += psnrs[i]
        a["ssim"] += ssims[i]
        a["n"] += 1
        if yuv:
            for key, src in (("y", psnrs_y), ("u", psnrs_u), ("v", psnrs_v),
                             ("sy", ssims_y), ("su", ssims_u), ("sv", ssims_v)):
                a[key] += src[i]
    ai, ap = acc[0], acc[1]
    log = {"frame_pixel_num": frame_pixel_num, "i_frame_num": ai["n"], "p_frame_num": ap["n"],
           "ave_i_frame_bpp": ai["bits"] / ai["n"] / frame_pixel_num,
           "ave_i_frame_psnr": ai["psnr"] / ai["n"], "ave_i_frame_msssim": ai["ssim"] / ai["n"]}
    if yuv:
        for c in "yuv":
            log[f"ave_i_frame_psnr_{c}"] = ai[c] / ai["n"]
        for c in "yuv":
            log[f"ave_i_frame_msssim_{c}"] = ai["s" + c] / ai["n"]
    if verbose:
        log["frame_bpp"] = list(np.array(bits) / frame_pixel_num)
        log["frame_psnr"] = psnrs
        log["frame_msssim"] = ssims
        log["frame_type"] = frame_types
        if yuv:
            log.update(frame_psnr_y=psnrs_y, frame_psnr_u=psnrs_u, frame_psnr_v=psnrs_v,
                       frame_msssim_y=ssims_y, frame_msssim_u=ssims_u, frame_msssim_v=ssims_v)
    log["test_time"] = test_time
    if ap["n"] > 0:
        log["ave_p_frame_bpp"] = ap["bits"] / (ap["n"] * frame_pixel_num)
        log["ave_p_frame_psnr"] = ap["psnr"] / ap["n"]
        log["ave_p_frame_msssim"] = ap["ssim"] / ap["n"]
        if yuv:
            for c in "yuv":
                log[f"ave_p_frame_psnr_{c}"] = ap[c] / ap["n"]
            for c in "yuv":
                log[f"ave_p_frame_msssim_{c}"] = ap["s" + c] / ap["n"]
    else:
        log["ave_p_frame_bpp"] = 0
        log["ave_p_frame_psnr"] = 0
        log["ave_p_frame_msssim"] = 0
        if yuv:
            for c in "yuv":
                log[f"ave_p_frame_psnr_{c}"] = 0
            for c in "yuv":
                log[f"ave_p_frame_msssim_{c}"] = 0
    log["ave_all_frame_bpp"] = (ai["bits"] + ap["bits"]) / (frame_num * frame_pixel_num)
    log["ave_all_frame_psnr"] = (ai["psnr"] + ap["psnr"]) / frame_num
    log["ave_all_frame_msssim"] = (ai["ssim"] + ap["ssim"]) / frame_num
    if yuv:
        for c in "yuv":
            log[f"ave_all_frame_psnr_{c}"] = (ai[c] + ap[c]) / frame_num
        for c in "yuv":
            log[f"ave_all_frame_msssim_{c}"] = (ai["s" + c] + ap["s" + c]) / frame_num
    return log


YUV_SRC_TYPES = {"yuv420": "420", "yuv422": "422", "yuv444": "444"}   # src_type -> YUVReader's src_format


def _reader(args, yuv):
    if "src_reader" in args:
        return args["src_reader"]
    depth = args.get("src_bit_depth", 8)
    if args["src_type"] in YUV_SRC_TYPES:
        return YUVReader(args["src_path"], args["src_width"], args["src_height"],
                         src_format=YUV_SRC_TYPES[args["src_type"]], bit_depth=depth)
    if args["src_type"] == "rgb":
        return RGBReader(args["src_path"], args["src_width"], args["src_height"], bit_depth=depth)
    if args["src_type"] == "png":
        if depth != 8:
            raise ValueError(f"PNG sources are 8-bit (src_bit_depth {depth})")
        return PNGReader(args.get("src_path", args.get("img_path")), args["src_width"], args["src_height"])
    raise ValueError(f"unknown src_type {args['src_type']!r}")


def _src_format(src_type, codec_fmt):
    """"rgb" | "420" | "422" | "444": what a source of ``src_type`` ('png' |
    'rgb' | 'yuv420' | 'yuv422' | 'yuv444', None: the codec's own format)
    hands over."""
    if src_type not in (None, "png", "rgb", *YUV_SRC_TYPES):
        raise ValueError(f"unknown src_type {src_type!r}")
    return codec_fmt if src_type is None else YUV_SRC_TYPES.get(src_type, "rgb")


def _dst_format(src_fmt):
    """What the drivers ask a reader for: "rgb", or "420" for every YUV source
    (the chroma layout is the reader's own, never a ``dst_format``)."""
    return "rgb" if src_fmt == "rgb" else "420"


def _chroma(src_fmt):
    """The chroma layout of the decoded-frame file that goes with a source."""
    return src_fmt if src_fmt in ("422", "444") else "420"


def _bit_depths(args, default=8):
    """(src_bit_depth, recon_bit_depth) of ``args``: the source's depth
    (``default`` when not given) and the decoded-frame files' (the source's
    when not given)."""
    src = _check_bit_depth(args.get("src_bit_depth", default))
    return src, _check_bit_depth(args.get("recon_bit_depth", src))


def _writer_kind(src_type, src_fmt, bit_depth):
    """The decoded-frame writer that goes with a source: out.yuv for a YUV420
    source, out.rgb for a raw RGB one (and for any RGB source above 8 bits,
    which a PNG cannot hold), PNG files otherwise."""
    if src_fmt != "rgb":
        return "yuv"
    return "rgb" if src_type == "rgb" or (src_type is None and bit_depth > 8) else "png"


def run_test(p_frame_net, i_frame_net, args):
    """DCVC-DC/test_video.py:71-237 on the GPU codecs.  ``args`` takes the
    reference's keys (frame_num, gop_size, write_stream, bin_folder,
    src_type 'png' | 'yuv420' | 'yuv422' | 'yuv444' | 'rgb' (a raw planar .rgb file), src_bit_depth
    (8; 9..16 for uint16 .rgb / .yuv files), recon_bit_depth (the decoded-frame
    files' depth, the source's by default), src_path, src_width, src_height,
    dist_in_yuv420, q_in_ckpt, i_frame_q_index, verbose, calc_ssim) plus an
    optional ``src_reader`` (an ArrayReader) in place of a file source.
    ``dist_in_yuv420`` selects the codec's format (YCbCr 4:4:4 input, as the
    reference's yuv420 checkpoints expect, against RGB) and ``src_type`` the
    source's, independently; a source of the other format is converted on the
    GPU as the reference's readers convert it (FrameStage)."""
    frame_num, gop_size = args["frame_num"], args["gop_size"]
    write_stream = bool(args.get("write_stream", False))
    verbose = args.get("verbose", 0)
    yuv = bool(args.get("dist_in_yuv420", False))
    codec_fmt = "420" if yuv else "rgb"
    src_type = args.get("src_type")
    src_fmt = _src_format(src_type, codec_fmt)
    src_depth, recon_depth = _bit_depths(args)
    if args.get("calc_ssim") and yuv and _chroma(src_fmt) != "420":
        raise ValueError(f"calc_ssim on a YUV codec needs a 4:2:0 or RGB source, not {src_type!r}: "
                         "per-plane MS-SSIM at other chroma plane sizes is not supported")
    device = i_frame_net.dev
    reader = _reader(args, yuv)
    h, w = args["src_height"], args["src_width"]
    stage = FrameStage(h, w, 16, yuv, zero_pad=False, frame_num=frame_num, device=device, src_format=src_fmt,
                       bit_depth=src_depth)
    writer = None
    if args.get("save_decoded_frame"):   # test_video.py:84-88
        writer = ReconWriter(args["recon_path"], h, w, _writer_kind(src_type, src_fmt, recon_depth), codec_fmt,
                             device, bit_depth=recon_depth, chroma=_chroma(src_fmt))
    ms = None
    if args.get("calc_ssim"):
        ms = MsSsim(h, w, frame_num, device) if yuv else MsSsimRGB(h, w, frame_num, device)
    frame_types, bits = [], []
    start_time = time.time()
    p_frame_number = 0
    enc_t = dec_t = 0.0
    dpb = None
    with torch.no_grad(), (writer if writer is not None else contextlib.nullcontext()):
        for frame_idx in range(frame_num):
            frame = reader.read_one_frame(dst_format=_dst_format(src_fmt))
            if frame is None or (src_fmt != "rgb" and frame[0] is None):
                raise ValueError(f"source ended at frame {frame_idx} of {frame_num}")
            dframe = stage.upload(frame)
            x = stage.load(dframe)
            bin_path = os.path.join(args["bin_folder"], f"{frame_idx}.bin") if write_stream else None
            if frame_idx % gop_size == 0:
                result = i_frame_net.encode_decode(x, args["q_in_ckpt"], args["i_frame_q_index"], bin_path,
                                                   pic_height=h, pic_width=w)
                dpb = {"ref_frame": result["x_hat"], "ref_feature": None, "ref_mv_feature": None,
                       "ref_y": None, "ref_mv_y": None}
                recon = result["x_hat"]
                frame_types.append(0)
            else:
                # test_video.py:152-155 passes i_frame_q_index to the P codec too
                result = p_frame_net.encode_decode(x, dpb, args["q_in_ckpt"], args["i_frame_q_index"], bin_path,
                                                   pic_height=h, pic_width=w, frame_idx=frame_idx % 4)
                dpb = result["dpb"]
                recon = dpb["ref_frame"]
                frame_types.append(1)
                p_frame_number += 1
                enc_t += result["encoding_time"]
                dec_t += result["decoding_time"]
            bits.append(result["bit"])
            stage.distortion(recon, dframe, frame_idx)
            if ms is not None:
                from .dc.video_model import as_act
                src_f32 = stage.source_f32(dframe)
                if src_f32 is not None:
                    ms.run_f32(as_act(recon), *src_f32, frame_idx)
                elif yuv:
                    ms.run(as_act(recon), dframe[0], dframe[1], frame_idx)
                else:
                    ms.run(as_act(recon), dframe, frame_idx)
            if writer is not None:
                writer.write(recon, frame_idx)
            if verbose >= 2:
                print(f"frame {frame_idx}, bits: {bits[-1]:.3f}", flush=True)
    sse = stage.sums()
    test_time = time.time() - start_time
    if verbose >= 1 and p_frame_number > 0:
        print(f"encoding/decoding {p_frame_number} P frames, "
              f"average encoding time {enc_t / p_frame_number * 1000:.0f} ms, "
              f"average decoding time {dec_t / p_frame_number * 1000:.0f} ms.")
    zeros = [0.0] * frame_num
    if yuv:
        per = [psnr_yuv(sse[i], h, w, _chroma(src_fmt)) for i in range(frame_num)]
        mv = ms.values(frame_num) if ms is not None else [(0.0, 0.0, 0.0, 0.0)] * frame_num
        log = generate_log_json(frame_num, h * w, test_time, frame_types, bits, [p[3] for p in per],
                                [m[3] for m in mv], [p[0] for p in per], [p[1] for p in per], [p[2] for p in per],
                                [m[0] for m in mv], [m[1] for m in mv], [m[2] for m in mv], verbose=verbose >= 1)
    else:
        psnrs = [psnr_rgb(sse[i], h, w) for i in range(frame_num)]
        mv = ms.values(frame_num) if ms is not None else zeros
        log = generate_log_json(frame_num, h * w, test_time, frame_types, bits, psnrs, mv,
                                verbose=verbose >= 1)
    if args.get("calc_ssim") and not yuv:
        log["msssim_unpinned"] = True   # pytorch_msssim's algorithm, package absent (MsSsimRGB)
    if writer is not None:
        # test_video.py:217-221: the recon folder is renamed after the rate point's averages
        avg_bpp = sum(bits) / len(bits) / w / h
        avg_psnr = log["ave_all_frame_psnr"]
        folder = f"{args.get('rate_idx', 0)}_{avg_bpp:.4f}_{avg_psnr:.4f}"
        os.rename(args["recon_path"], args["recon_path"] + f"/../{folder}")
    return log


def generate_log_json_hem(frame_num, frame_types, bits, psnrs, ssims, frame_pixel_num, test_time):
    """DCVC-HEM/src/utils/common.py:63-104."""
    log = generate_log_json(frame_num, frame_pixel_num, test_time, frame_types, bits, psnrs, ssims, verbose=True)
    keep = ("frame_pixel_num", "i_frame_num", "p_frame_num", "ave_i_frame_bpp", "ave_i_frame_psnr",
            "ave_i_frame_msssim", "frame_bpp", "frame_psnr", "frame_msssim", "frame_type", "test_time",
            "ave_p_frame_bpp", "ave_p_frame_psnr", "ave_p_frame_msssim", "ave_all_frame_bpp",
            "ave_all_frame_psnr", "ave_all_frame_msssim")
    return {k: log[k] for k in keep if k in log}


def run_test_hem(video_net, i_frame_net, args, device=None):
    """DCVC-HEM/test_video.py:80-172: PNG (or in-memory) RGB source, zero
    padding to a multiple of 64, q scales from ``args`` (i_frame_q_scale,
    p_frame_mv_y_q_scale, p_frame_y_q_scale).  ``src_type`` 'rgb' reads a raw
    planar .rgb file, ``src_bit_depth`` / ``recon_bit_depth`` as in
    ``run_test``."""
    frame_num, gop_size = args["frame_num"], args["gop_size"]
    write_stream = bool(args.get("write_stream", False))
    device = device if device is not None else i_frame_net.dev
    src_type = args.get("src_type", "png")
    if _src_format(src_type, "rgb") != "rgb":
        raise ValueError("the HEM harness reads RGB sources")
    src_depth, recon_depth = _bit_depths(args)
    reader = _reader({**args, "src_type": src_type}, False)
    h, w = args["src_height"], args["src_width"]
    stage = FrameStage(h, w, 64, False, zero_pad=True, frame_num=frame_num, device=device, bit_depth=src_depth)
    ms = MsSsimRGB(h, w, frame_num, device) if min(h, w) > 160 else None  # HEM always reports ms_ssim (:150)
    writer = None
    if args.get("save_decoded_frame"):   # DCVC-HEM/test_video.py:161-163, 204-209
        # a raw RGB source (or any depth above 8 bits) gets RGBWriter's out.rgb in place of the PNG files
        kind = "rgb" if src_type == "rgb" or recon_depth > 8 else "hem_png"
        writer = ReconWriter(args["decoded_frame_folder"], h, w, kind, "rgb", device, bit_depth=recon_depth)
    frame_types, bits = [], []
    start_time = time.time()
    dpb = None
    with torch.no_grad(), (writer if writer is not None else contextlib.nullcontext()):
        for frame_idx in range(frame_num):
            frame = reader.read_one_frame(dst_format="rgb")
            if frame is None:
                raise ValueError(f"source ended at frame {frame_idx} of {frame_num}")
            dframe = stage.upload(frame)
            x = stage.load(dframe)
            bin_path = os.path.join(args["bin_folder"], f"{frame_idx}.bin") if write_stream else None
            if frame_idx % gop_size == 0:
                result = i_frame_net.encode_decode(x, args["i_frame_q_scale"], bin_path, pic_height=h, pic_width=w)
                dpb = {"ref_frame": result["x_hat"], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
                recon = result["x_hat"]
                frame_types.append(0)
            else:
                result = video_net.encode_decode(x, dpb, bin_path, pic_height=h, pic_width=w,
                                                 mv_y_q_scale=args["p_frame_mv_y_q_scale"],
                                                 y_q_scale=args["p_frame_y_q_scale"])
                dpb = result["dpb"]
                recon = dpb["ref_frame"]
                frame_types.append(1)
            bits.append(result["bit"])
            stage.distortion(recon, dframe, frame_idx)
            if ms is not None:
                from .dc.video_model import as_act
                src_f32 = stage.source_f32(dframe)
                if src_f32 is not None:
                    ms.run_f32(as_act(recon), *src_f32, frame_idx)
                else:
                    ms.run(as_act(recon), dframe, frame_idx)
            if writer is not None:
                writer.write(recon, frame_idx)
    sse = stage.sums()
    psnrs = [psnr_rgb(sse[i], h, w) for i in range(frame_num)]
    mv = ms.values(frame_num) if ms is not None else [0.0] * frame_num
    log = generate_log_json_hem(frame_num, frame_types, bits, psnrs, mv, h * w, time.time() - start_time)
    log["msssim_unpinned"] = True   # pytorch_msssim's algorithm, package absent (MsSsimRGB)
    return log


# ------------------------------------------- stand-alone encoder / decoder
def _tag_format(nets, args):
    """``dist_in_yuv420`` in args is the caller's statement of which
    checkpoints the nets hold; the sequence drivers check it against the file."""
    if "dist_in_yuv420" in args:
        for net in nets:
            net.codec_format = "yuv420" if args["dist_in_yuv420"] else "rgb"


def encode_video(i_frame_net, p_frame_net, args):
    """Encoder only: ``run_test`` / ``run_test_hem`` (their keys, readers,
    FrameStage, both source formats) with the frames coded by a
    ``sequence.SequenceEncoder`` into the one file ``args["seq_path"]``
    instead of ``encode_decode`` and a bin folder; ``args["digest"]`` (default
    True) stores the DPB digests.  Nothing is decoded: the log's bits are the
    frames' payload bits and its PSNR is that of the ENCODER's reconstruction
    (which a decoder of the file reproduces bit for bit).  ``src_bit_depth``
    above 8 is recorded in the file's header; the payloads do not depend on it.

    Scene-cut keyframes (off by default; there is no default threshold):
    ``scene_cut`` / ``scene_cut_mad`` are thresholds in (0, 1] on the
    detector's ``hd`` / ``mad`` (``scenecut.SceneCutDetector``); a frame that
    reaches any given one (>=) is coded as an I frame once
    ``min_keyframe_interval`` (default 1) frames have passed since the last
    keyframe.  The log then gains "scene_cuts" (the frames coded as I because
    of a cut) and "scene_scores" ([hd, mad] per frame, None for frame 0).  With
    neither threshold no detector is built and the file is what it always was."""
    from . import scenecut
    from .sequence import SequenceEncoder, codec_of
    hem = codec_of(i_frame_net) == "HEM"
    cut_hd = scenecut.check_threshold("scene_cut", args.get("scene_cut"))
    cut_mad = scenecut.check_threshold("scene_cut_mad", args.get("scene_cut_mad"))
    min_interval = scenecut.check_interval(args.get("min_keyframe_interval", 1))
    detect = cut_hd is not None or cut_mad is not None
    _tag_format((i_frame_net, p_frame_net), args)
    frame_num, gop_size = args["frame_num"], args["gop_size"]
    verbose = args.get("verbose", 0)
    yuv = bool(args.get("dist_in_yuv420", False)) and not hem
    codec_fmt = "420" if yuv else "rgb"
    src_type = args.get("src_type")
    src_fmt = _src_format(src_type, codec_fmt)
    if hem and src_fmt != "rgb":
        raise ValueError("the HEM harness reads RGB sources")
    src_depth, _ = _bit_depths(args)
    device = i_frame_net.dev
    reader = _reader({**args, "src_type": src_type or "png"} if hem else args, yuv)
    h, w = args["src_height"], args["src_width"]
    if hem:
        stage = FrameStage(h, w, 64, False, zero_pad=True, frame_num=frame_num, device=device, bit_depth=src_depth)
        q = dict(i_frame_q_scale=args["i_frame_q_scale"], p_frame_mv_y_q_scale=args["p_frame_mv_y_q_scale"],
                 p_frame_y_q_scale=args["p_frame_y_q_scale"])
    else:
        stage = FrameStage(h, w, 16, yuv, zero_pad=False, frame_num=frame_num, device=device, src_format=src_fmt,
                           bit_depth=src_depth)
        q = dict(q_in_ckpt=args["q_in_ckpt"], q_index=args["i_frame_q_index"])
    frame_types, bits, fallbacks = [], [], []
    # the detector reads source samples only: one object for every codec, source type and depth
    detector = scenecut.SceneCutDetector(h, w, src_fmt, src_depth, device) if detect else None
    scene_cuts, scene_scores = [], []
    start_time = time.time()
    with SequenceEncoder(i_frame_net, p_frame_net, args["seq_path"], w, h, gop_size, yuv420=yuv,
                         digest=bool(args.get("digest", True)), bit_depth=src_depth,
                         min_keyframe_interval=min_interval, **q) as enc:
        for frame_idx in range(frame_num):
            frame = reader.read_one_frame(dst_format=_dst_format(src_fmt))
            if frame is None or (src_fmt != "rgb" and frame[0] is None):
                raise ValueError(f"source ended at frame {frame_idx} of {frame_num}")
            dframe = stage.upload(frame)
            cut = False
            if detector is not None:
                score = detector.score(dframe)
                scene_scores.append(None if score is None else [score["hd"], score["mad"]])
                cut = scenecut.is_cut(score, cut_hd, cut_mad)
            # with no cut this is the type of frame_idx % gop_size == 0 (the schedule is not advanced here)
            regular = enc.schedule.peek() == "I"
            out = enc.encode(stage.load(dframe), keyframe=cut)
            if cut and out["type"] == "I" and not regular:
                scene_cuts.append(frame_idx)
            frame_types.append(0 if out["type"] == "I" else 1)
            bits.append(out["bit"])
            fallbacks.append(out["precision_fallback"])
            stage.distortion(out["recon"], dframe, frame_idx)
            if verbose >= 2:
                print(f"frame {frame_idx}, bits: {bits[-1]:.3f}", flush=True)
    sse = stage.sums()
    test_time = time.time() - start_time
    zeros = [0.0] * frame_num
    if hem:
        log = generate_log_json_hem(frame_num, frame_types, bits, [psnr_rgb(sse[i], h, w) for i in range(frame_num)],
                                    zeros, h * w, test_time)
    elif yuv:
        per = [psnr_yuv(sse[i], h, w, _chroma(src_fmt)) for i in range(frame_num)]
        log = generate_log_json(frame_num, h * w, test_time, frame_types, bits, [p[3] for p in per], zeros,
                                [p[0] for p in per], [p[1] for p in per], [p[2] for p in per], zeros, zeros, zeros,
                                verbose=verbose >= 1)
    else:
        log = generate_log_json(frame_num, h * w, test_time, frame_types, bits,
                                [psnr_rgb(sse[i], h, w) for i in range(frame_num)], zeros, verbose=verbose >= 1)
    log["frame_bits"] = bits
    log["precision_fallbacks"] = fallbacks
    if detect:
        log["scene_cuts"] = scene_cuts
        log["scene_scores"] = scene_scores
    return log


def decode_video(i_frame_net, p_frame_net, args):
    """Decoder only: decodes ``args["seq_path"]`` with a
    ``sequence.SequenceDecoder`` (which verifies the stored DPB digests) and,
    with ``save_decoded_frame``, writes the frames as ``run_test`` /
    ``run_test_hem`` write them (``recon_path`` / ``decoded_frame_folder``;
    ``src_type`` selects PNG, out.rgb or out.yuv as there, the codec's own
    format by default; ``recon_bit_depth``, by default the source depth the
    file's header records).  Returns the per-frame bits and types.

    ``start_frame`` (default 0) and ``frame_num`` (default: to the end; clipped
    there) select the frames: decoding starts at the last keyframe at or before
    ``start_frame`` (``SequenceDecoder.frames``) and only the selected frames
    are returned and written, the files numbered from the first of them.  The
    result says where: "start_frame", "keyframe", "frames_decoded", and "gops"
    ((start, stop) of every GOP of the file, ``lanes.gops_of``)."""
    from .lanes import gops_of
    from .sequence import SequenceDecoder, codec_of
    hem = codec_of(i_frame_net) == "HEM"
    _tag_format((i_frame_net, p_frame_net), args)
    frame_types, bits = [], []
    start_time = time.time()
    with SequenceDecoder(i_frame_net, p_frame_net, args["seq_path"]) as dec:
        h, w = dec.height, dec.width
        start = args.get("start_frame", 0)
        frames = dec.frames(start, args.get("frame_num"))       # a bad range raises before any folder is made
        gops = [list(g) for g in gops_of(dec.reader.index(), dec.reader.path)]
        codec_fmt = "420" if dec.reader.format == "yuv420" else "rgb"
        src_type = args.get("src_type")
        src_fmt = _src_format(src_type, codec_fmt)
        _, depth = _bit_depths(args, default=dec.reader.bit_depth)   # the source's depth, from the header
        writer = None
        if args.get("save_decoded_frame"):
            if hem:
                kind = "rgb" if src_type == "rgb" or depth > 8 else "hem_png"
                writer = ReconWriter(args["decoded_frame_folder"], h, w, kind, "rgb", i_frame_net.dev,
                                     bit_depth=depth)
            else:
                writer = ReconWriter(args["recon_path"], h, w, _writer_kind(src_type, src_fmt, depth), codec_fmt,
                                     i_frame_net.dev, bit_depth=depth, chroma=_chroma(src_fmt))
        with (writer if writer is not None else contextlib.nullcontext()):
            for emitted, out in enumerate(frames):
                frame_types.append(0 if out["type"] == "I" else 1)
                bits.append(out["bit"])
                if writer is not None:
                    writer.write(out["x_hat"], emitted)
        keyframe, decoded = dec.last_keyframe, dec.frames_decoded
    return {"frame_num": len(bits), "frame_pixel_num": h * w, "frame_type": frame_types, "frame_bits": bits,
            "bit_depth": depth, "test_time": time.time() - start_time, "start_frame": start, "keyframe": keyframe,
            "frames_decoded": decoded, "gops": gops}
