// High-bit-depth frames: raw planar RGB and YUV420 sources of 9..16 bits per
// sample (little-endian uint16, as the reference's RGBReader / RGBWriter read
// and write them, DCVC-DC/src/utils/video_reader.py:83-118, video_writer.py:
// 50-80) into the codec's padded NHWC input, the per-frame distortion against
// them, and the decoded frame back into uint16 samples.
//
// With max_val = (1 << depth) - 1 a sample enters as float32(s) / float32(
// max_val), one IEEE division (u16f; samples above max_val are not clamped),
// and leaves as clip(rint(v * max_val), 0, max_val) in fp32 (q16).  Everything
// else (order-0 chroma zoom, 2x2 means, BT.709, padding, the in-place clamp,
// the fixed reduction order) is the arithmetic of the uint8 paths, and the
// same kernels: apart from the RGB ingest and the plane conversion below,
// every entry point here checks its arguments and runs the uint16
// instantiation of a kernel template of chroma.hip, frame.hip or crossfmt.hip
// through frame.h's launchers.  The same-format paths read the uint16 samples
// directly; the cross-format ingest goes through fp32 planes (dcvc_u16_to_f32,
// then crossfmt.hip's fp32-source entry points).
//
// The NHWC frame arrives as scalars (base, H, W, cstride, coff: the FView of
// frame.h), not as a dcvc_tensor.
#include "crossfmt.h"

namespace {

// frame_kernel (misc.hip) on uint16 CHW samples: one thread per output element
__global__ void frame16_kernel(const uint16_t *__restrict__ src, int h, int w, float mx, int zero_pad, FView y) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)y.H * y.W * 3) return;
  const int c = (int)(idx % 3);
  const int64_t pix = idx / 3;
  const int py = (int)(pix / y.W), px = (int)(pix - (int64_t)py * y.W);
  const int sy = min(py, h - 1), sx = min(px, w - 1);
  float v = u16f(src[((int64_t)c * h + sy) * w + sx], mx);
  if (zero_pad && (py >= h || px >= w)) v = 0.f;
  y.p[pix * y.cs + y.co + c] = v;
}

// dcvc_u16_to_f32: one thread per sample
__global__ void u16_f32_kernel(const uint16_t *__restrict__ src, int64_t n, float mx, float *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = u16f(src[i], mx);
}

}  // namespace

extern "C" int dcvc_frame16_to_nhwc(const uint16_t *src, int h, int w, int depth, int zero_pad, float *out, int H,
                                    int W, int cstride, int coff, void *stream) {
  if (!src || !view_ok(out, H, W, cstride, coff) || !depth_ok(depth, 9) || h <= 0 || w <= 0 || H < h || W < w)
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)H * W * 3;
  if ((n + 255) / 256 > 0x7fffffff) return DCVC_HIP_EINVAL;
  hipLaunchKernelGGL(frame16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, h, w, max_val(depth),
                     zero_pad ? 1 : 0, fvs(out, H, W, cstride, coff));
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_yuv420p16_to_nhwc(const uint16_t *y, const uint16_t *uv, int h, int w, int depth, float *out,
                                      int H, int W, int cstride, int coff, void *stream) {
  if (!y || !uv || !view_ok(out, H, W, cstride, coff) || !depth_ok(depth, 9) || !even_frame(h, w) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_ingest(FS_U16, max_val(depth), 2, 2, y, uv, h, w, fvs(out, H, W, cstride, coff),
                                  reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_frame16_sse(float *x_hat, int H, int W, int cstride, int coff, const uint16_t *src,
                                const uint16_t *uv, int h, int w, int depth, int yuv420, double *workspace,
                                double *out3, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !src || !workspace || !out3 || !depth_ok(depth, 9) || h <= 0 ||
      w <= 0 || H < h || W < w)
    return DCVC_HIP_EINVAL;
  if (yuv420 && (!uv || !even_frame(h, w) || !even_frame(H, W))) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const FView xh = fvs(x_hat, H, W, cstride, coff);
  if (yuv420) return dcvc_internal_yuv_sse(FS_U16, max_val(depth), 2, 2, xh, src, uv, h, w, workspace, out3, st);
  return dcvc_internal_rgb_sse(FS_U16, max_val(depth), xh, src, h, w, workspace, out3, st);
}

extern "C" int dcvc_recon_to_u16(const float *x_hat, int H, int W, int cstride, int coff, int h, int w, int depth,
                                 int yuv420, uint16_t *out, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !out || !depth_ok(depth, 9) || h <= 0 || w <= 0 || H < h || W < w)
    return DCVC_HIP_EINVAL;
  if (yuv420 && !even_frame(h, w)) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const FView xh = fvs(x_hat, H, W, cstride, coff);
  if (yuv420) return dcvc_internal_yuv_write(FS_U16, max_val(depth), 2, 2, false, xh, h, w, out, st);
  return dcvc_internal_rgb_write(FS_U16, max_val(depth), false, xh, h, w, out, st);
}

extern "C" int dcvc_recon_to_u16_cross(const float *x_hat, int H, int W, int cstride, int coff, int h, int w,
                                       int depth, int to_rgb, uint16_t *out, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !out || !depth_ok(depth, 9) || !even_frame(h, w) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const FView xh = fvs(x_hat, H, W, cstride, coff);
  if (to_rgb) return dcvc_internal_rgb_write(FS_U16, max_val(depth), true, xh, h, w, out, st);
  return dcvc_internal_yuv_write(FS_U16, max_val(depth), 2, 2, true, xh, h, w, out, st);
}

extern "C" int dcvc_u16_to_f32(const uint16_t *src, int64_t n, int depth, float *out, void *stream) {
  if (!src || !out || n <= 0 || !depth_ok(depth, 9)) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(u16_f32_kernel, dim3(cf_blocks(n)), dim3(CF_BLOCK), 0, st, src, n, max_val(depth), out);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}
