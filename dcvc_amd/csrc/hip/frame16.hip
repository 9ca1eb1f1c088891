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
// the fixed reduction order) is the arithmetic of the uint8 kernels in
// frame.hip, misc.hip and crossfmt.hip, whose helpers these kernels share.
// The same-format paths read the uint16 samples directly; the cross-format
// ingest goes through fp32 planes (dcvc_u16_to_f32, then crossfmt.hip's
// fp32-source entry points).
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

// yuv420_kernel (frame.hip) on uint16 planes
__global__ void yuv420p16_kernel(const uint16_t *__restrict__ ysrc, const uint16_t *__restrict__ uvsrc, int h, int w,
                                 float mx, FView out) {
  const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= (int64_t)out.H * out.W) return;
  const int py = (int)(pix / out.W), px = (int)(pix - (int64_t)py * out.W);
  const int sy = min(py, h - 1), sx = min(px, w - 1);
  const int hh = h / 2, hw = w / 2;
  const int uy = zoom_src(sy, hh), ux = zoom_src(sx, hw);
  float *o = out.p + pix * out.cs + out.co;
  o[0] = u16f(ysrc[(int64_t)sy * w + sx], mx);
  o[1] = u16f(uvsrc[(int64_t)uy * hw + ux], mx);
  o[2] = u16f(uvsrc[(int64_t)hh * hw + (int64_t)uy * hw + ux], mx);
}

// sse_rgb_kernel (frame.hip) against a uint16 CHW source
__global__ void __launch_bounds__(SSE_BLOCK) sse_rgb16_kernel(FView xh, const uint16_t *__restrict__ src, int h,
                                                              int w, float mx, double *part) {
  double a[3] = {0.0, 0.0, 0.0};
  const int64_t n = (int64_t)xh.H * xh.W;
  for (int64_t pix = (int64_t)blockIdx.x * SSE_BLOCK + threadIdx.x; pix < n; pix += (int64_t)gridDim.x * SSE_BLOCK) {
    const int py = (int)(pix / xh.W), px = (int)(pix - (int64_t)py * xh.W);
    float *p = xh.p + pix * xh.cs + xh.co;
    const float v0 = clamp01(p[0]), v1 = clamp01(p[1]), v2 = clamp01(p[2]);
    p[0] = v0;
    p[1] = v1;
    p[2] = v2;
    if (py < h && px < w) {
      const int64_t o = (int64_t)py * w + px, plane = (int64_t)h * w;
      const float d0 = v0 - u16f(src[o], mx), d1 = v1 - u16f(src[plane + o], mx),
                  d2 = v2 - u16f(src[2 * plane + o], mx);
      a[0] += (double)(d0 * d0);
      a[1] += (double)(d1 * d1);
      a[2] += (double)(d2 * d2);
    }
  }
  block_sum3(a[0], a[1], a[2], part);
}

// sse_yuv420_kernel (frame.hip) against uint16 Y and U|V planes
__global__ void __launch_bounds__(SSE_BLOCK) sse_yuv420p16_kernel(FView xh, const uint16_t *__restrict__ ysrc,
                                                                  const uint16_t *__restrict__ uvsrc, int h, int w,
                                                                  float mx, double *part) {
  double a[3] = {0.0, 0.0, 0.0};
  const int bh = xh.H / 2, bw = xh.W / 2, hw = w / 2, hh = h / 2;
  const int64_t n = (int64_t)bh * bw;
  for (int64_t b = (int64_t)blockIdx.x * SSE_BLOCK + threadIdx.x; b < n; b += (int64_t)gridDim.x * SSE_BLOCK) {
    const int by = (int)(b / bw), bx = (int)(b - (int64_t)by * bw);
    float v[2][2][3];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        float *p = xh.p + ((int64_t)(2 * by + dy) * xh.W + 2 * bx + dx) * xh.cs + xh.co;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[dy][dx][c] = clamp01(p[c]);
          p[c] = v[dy][dx][c];
        }
      }
    if (by < hh && bx < hw) {
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const double d =
              (double)v[dy][dx][0] - (double)u16f(ysrc[(int64_t)(2 * by + dy) * w + 2 * bx + dx], mx);
          a[0] += d * d;
        }
#pragma unroll
      for (int c = 1; c < 3; ++c) {
        const float s = (v[0][0][c] + v[0][1][c]) + (v[1][0][c] + v[1][1][c]);
        const float m = clamp01(s / 4.f);
        const double d = (double)m - (double)u16f(uvsrc[(int64_t)(c - 1) * hh * hw + (int64_t)by * hw + bx], mx);
        a[c] += d * d;
      }
    }
  }
  block_sum3(a[0], a[1], a[2], part);
}

// dcvc_recon_to_u16, RGB: one thread per crop pixel, planar 3 x h x w as
// RGBWriter stores it (video_writer.py:72-77)
__global__ void recon_rgb_u16_kernel(FView xh, int h, int w, float mx, uint16_t *__restrict__ out) {
  const int64_t n = (int64_t)h * w;
  const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= n) return;
  const int py = (int)(pix / w), px = (int)(pix - (int64_t)py * w);
  const float *p = xh.p + ((int64_t)py * xh.W + px) * xh.cs + xh.co;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c * n + pix] = q16(p[c], mx);
}

// dcvc_recon_to_u16, YUV420: recon_yuv_u8_kernel (frame.hip) with q16
__global__ void recon_yuv_u16_kernel(FView xh, int h, int w, float mx, uint16_t *__restrict__ out) {
  const int hh = h / 2, hw = w / 2;
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (int64_t)hh * hw) return;
  const int by = (int)(b / hw), bx = (int)(b - (int64_t)by * hw);
  float v[2][2][3];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const float *p = xh.p + ((int64_t)(2 * by + dy) * xh.W + 2 * bx + dx) * xh.cs + xh.co;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[dy][dx][c] = p[c];
      out[(int64_t)(2 * by + dy) * w + 2 * bx + dx] = q16(clamp01(v[dy][dx][0]), mx);
    }
#pragma unroll
  for (int c = 1; c < 3; ++c) {
    const float s = (v[0][0][c] + v[0][1][c]) + (v[1][0][c] + v[1][1][c]);
    out[(int64_t)h * w + (int64_t)(c - 1) * hh * hw + b] = q16(clamp01(s / 4.f), mx);
  }
}

// dcvc_recon_to_u16_cross, a YUV 4:4:4 frame into RGBWriter:
// recon_yuv_rgb_u8_kernel (crossfmt.hip) with q16 and planar output
__global__ void recon_yuv_rgb_u16_kernel(FView xh, int h, int w, double zy, double zx, float mx,
                                         uint16_t *__restrict__ out) {
  const int64_t n = (int64_t)h * w;
  const int hh = h / 2, hw = w / 2;
  for (int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < n; pix += (int64_t)gridDim.x * blockDim.x) {
    const int py = (int)(pix / w), px = (int)(pix - (int64_t)py * w);
    const bool seq = hw == 1;
    const Tap tr = zoom1_tap(py, hh, zy), tc = zoom1_tap(px, hw, zx);
    const float yv = clamp01(xh.p[((int64_t)py * xh.W + px) * xh.cs + xh.co]);
    const float cb = bilerp(block_mean(xh, tr.i0, tc.i0, 1, seq), block_mean(xh, tr.i0, tc.i1, 1, seq),
                            block_mean(xh, tr.i1, tc.i0, 1, seq), block_mean(xh, tr.i1, tc.i1, 1, seq), tr, tc);
    const float cr = bilerp(block_mean(xh, tr.i0, tc.i0, 2, seq), block_mean(xh, tr.i0, tc.i1, 2, seq),
                            block_mean(xh, tr.i1, tc.i0, 2, seq), block_mean(xh, tr.i1, tc.i1, 2, seq), tr, tc);
    float r, g, b;
    ycc_to_rgb(yv, cb, cr, r, g, b);
    out[pix] = q16(r, mx);
    out[n + pix] = q16(g, mx);
    out[2 * n + pix] = q16(b, mx);
  }
}

// dcvc_recon_to_u16_cross, an RGB frame into a YUV420 file:
// recon_rgb_yuv_u8_kernel (crossfmt.hip) with q16
__global__ void recon_rgb_yuv_u16_kernel(FView xh, int h, int w, float mx, uint16_t *__restrict__ out) {
  const int hh = h / 2, hw = w / 2;
  const int64_t n = (int64_t)hh * hw, plane = (int64_t)h * w;
  for (int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; blk < n; blk += (int64_t)gridDim.x * blockDim.x) {
    const int by = (int)(blk / hw), bx = (int)(blk - (int64_t)by * hw);
    float cb[2][2], cr[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float *p = xh.p + ((int64_t)(2 * by + dy) * xh.W + 2 * bx + dx) * xh.cs + xh.co;
        float y;
        rgb_to_ycc(p[0], p[1], p[2], y, cb[dy][dx], cr[dy][dx]);
        out[(int64_t)(2 * by + dy) * w + 2 * bx + dx] = q16(clamp01(y), mx);
      }
    out[plane + blk] = q16(clamp01(mean4(cb[0][0], cb[0][1], cb[1][0], cb[1][1], hw == 1)), mx);
    out[plane + n + blk] = q16(clamp01(mean4(cr[0][0], cr[0][1], cr[1][0], cr[1][1], hw == 1)), mx);
  }
}

// dcvc_u16_to_f32: one thread per sample
__global__ void u16_f32_kernel(const uint16_t *__restrict__ src, int64_t n, float mx, float *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = u16f(src[i], mx);
}

bool depth_ok(int depth) { return depth >= 9 && depth <= 16; }

float max_val(int depth) { return (float)((1 << depth) - 1); }

}  // namespace

extern "C" int dcvc_frame16_to_nhwc(const uint16_t *src, int h, int w, int depth, int zero_pad, float *out, int H,
                                    int W, int cstride, int coff, void *stream) {
  if (!src || !view_ok(out, H, W, cstride, coff) || !depth_ok(depth) || h <= 0 || w <= 0 || H < h || W < w)
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
  if (!y || !uv || !view_ok(out, H, W, cstride, coff) || !depth_ok(depth) || !even_frame(h, w) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(yuv420p16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, y, uv, h, w,
                     max_val(depth), fvs(out, H, W, cstride, coff));
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_frame16_sse(float *x_hat, int H, int W, int cstride, int coff, const uint16_t *src,
                                const uint16_t *uv, int h, int w, int depth, int yuv420, double *workspace,
                                double *out3, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !src || !workspace || !out3 || !depth_ok(depth) || h <= 0 || w <= 0 ||
      H < h || W < w)
    return DCVC_HIP_EINVAL;
  if (yuv420 && (!uv || (h & 1) || (w & 1) || (H & 1) || (W & 1))) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const FView xh = fvs(x_hat, H, W, cstride, coff);
  unsigned g;
  if (yuv420) {
    g = sse_blocks((int64_t)(H / 2) * (W / 2));
    hipLaunchKernelGGL(sse_yuv420p16_kernel, dim3(g), dim3(SSE_BLOCK), 0, st, xh, src, uv, h, w, max_val(depth),
                       workspace);
  } else {
    g = sse_blocks((int64_t)H * W);
    hipLaunchKernelGGL(sse_rgb16_kernel, dim3(g), dim3(SSE_BLOCK), 0, st, xh, src, h, w, max_val(depth), workspace);
  }
  DCVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sse_final_kernel, dim3(1), dim3(256), 0, st, workspace, (int)g, out3);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_recon_to_u16(const float *x_hat, int H, int W, int cstride, int coff, int h, int w, int depth,
                                 int yuv420, uint16_t *out, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !out || !depth_ok(depth) || h <= 0 || w <= 0 || H < h || W < w)
    return DCVC_HIP_EINVAL;
  if (yuv420 && ((h & 1) || (w & 1))) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const FView xh = fvs(x_hat, H, W, cstride, coff);
  const int64_t n = yuv420 ? (int64_t)(h / 2) * (w / 2) : (int64_t)h * w;
  if (yuv420)
    hipLaunchKernelGGL(recon_yuv_u16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xh, h, w,
                       max_val(depth), out);
  else
    hipLaunchKernelGGL(recon_rgb_u16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xh, h, w,
                       max_val(depth), out);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_recon_to_u16_cross(const float *x_hat, int H, int W, int cstride, int coff, int h, int w,
                                       int depth, int to_rgb, uint16_t *out, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !out || !depth_ok(depth) || !even_frame(h, w) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const FView xh = fvs(x_hat, H, W, cstride, coff);
  if (to_rgb)
    hipLaunchKernelGGL(recon_yuv_rgb_u16_kernel, dim3(cf_blocks((int64_t)h * w)), dim3(CF_BLOCK), 0, st, xh, h, w,
                       zoom_ratio(h / 2), zoom_ratio(w / 2), max_val(depth), out);
  else
    hipLaunchKernelGGL(recon_rgb_yuv_u16_kernel, dim3(cf_blocks((int64_t)(h / 2) * (w / 2))), dim3(CF_BLOCK), 0, st,
                       xh, h, w, max_val(depth), out);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_u16_to_f32(const uint16_t *src, int64_t n, int depth, float *out, void *stream) {
  if (!src || !out || n <= 0 || !depth_ok(depth)) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(u16_f32_kernel, dim3(cf_blocks(n)), dim3(CF_BLOCK), 0, st, src, n, max_val(depth), out);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}
