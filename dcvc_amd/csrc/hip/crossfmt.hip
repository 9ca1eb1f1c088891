// Cross-format frame kernels of run_test (DCVC-DC/test_video.py:79-119): a
// YUV420 source coded by an RGB model and an RGB source coded by a YUV420
// model, as the reference's readers convert them (video_reader.py:33-42,
// src/transforms/functional.py:16-58), and the two cross cases of the
// decoded-frame writers (video_writer.py:26-111).
//
//   * dcvc_yuv420_to_rgb_nhwc: ycbcr420_to_rgb(y / 255, uv / 255, order=1),
//     padded NHWC codec input plus the planar fp32 RGB source.
//   * dcvc_rgb_to_yuv420_planes + dcvc_yuv420f_to_nhwc: rgb_to_ycbcr420(rgb /
//     255) as fp32 planes, then ycbcr420_to_444(order=0) + replicate padding.
//   * dcvc_frame_sse_f32, dcvc_yuv_planes_f64_f32, dcvc_rgb_planes_f64_f32:
//     the distortion / MS-SSIM inputs against those fp32 source planes.
//   * dcvc_recon_to_u8_cross: a YUV 4:4:4 frame as PNGWriter stores it, an RGB
//     frame as YUVWriter stores it.
//
// Every value is bit-equal to the reference's numpy / scipy result, so the
// colour arithmetic (crossfmt.h, shared with frame16.hip) is written operation
// by operation in numpy's order with contraction into FMAs switched off (numpy
// rounds after every ufunc).
#include "crossfmt.h"

namespace {

// dcvc_yuv420_to_rgb_nhwc: one thread per pixel of the padded output; a
// padding pixel recomputes its edge pixel (F.pad replicate, test_video.py:
// 130-135).  rgb_planes (3 x h x w) receives the crop.  S: uint8 samples
// (x / 255) or fp32 planes already in [0, 1] (smp, crossfmt.h).
template <typename S>
__global__ void yuv420_rgb_kernel(const S *__restrict__ ysrc, const S *__restrict__ uvsrc, int h, int w, double zy,
                                  double zx, FView out, float *__restrict__ rgb_planes) {
  const int64_t n = (int64_t)out.H * out.W;
  const int hh = h / 2, hw = w / 2;
  const int64_t cplane = (int64_t)hh * hw, plane = (int64_t)h * w;
  for (int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < n; pix += (int64_t)gridDim.x * blockDim.x) {
    const int py = (int)(pix / out.W), px = (int)(pix - (int64_t)py * out.W);
    const int sy = min(py, h - 1), sx = min(px, w - 1);
    const Tap tr = zoom1_tap(sy, hh, zy), tc = zoom1_tap(sx, hw, zx);
    const int64_t o00 = (int64_t)tr.i0 * hw + tc.i0, o01 = (int64_t)tr.i0 * hw + tc.i1;
    const int64_t o10 = (int64_t)tr.i1 * hw + tc.i0, o11 = (int64_t)tr.i1 * hw + tc.i1;
    const float yv = smp(ysrc[(int64_t)sy * w + sx]);
    const float cb = bilerp(smp(uvsrc[o00]), smp(uvsrc[o01]), smp(uvsrc[o10]), smp(uvsrc[o11]), tr, tc);
    const float cr = bilerp(smp(uvsrc[cplane + o00]), smp(uvsrc[cplane + o01]), smp(uvsrc[cplane + o10]),
                            smp(uvsrc[cplane + o11]), tr, tc);
    float r, g, b;
    ycc_to_rgb(yv, cb, cr, r, g, b);
    float *o = out.p + pix * out.cs + out.co;
    o[0] = r;
    o[1] = g;
    o[2] = b;
    if (py < h && px < w) {
      const int64_t q = (int64_t)py * w + px;
      rgb_planes[q] = r;
      rgb_planes[plane + q] = g;
      rgb_planes[2 * plane + q] = b;
    }
  }
}

// dcvc_rgb_to_yuv420_planes: one thread per 2x2 block of the CHW frame
// (uint8, or fp32 for dcvc_rgbf_to_yuv420_planes);
// rgb_to_ycbcr420 (functional.py:16-39): Y of the four pixels and the block's
// Cb, Cr means, clipped after the mean
template <typename S>
__global__ void rgb_yuv420_planes_kernel(const S *__restrict__ src, int h, int w, float *__restrict__ yp,
                                         float *__restrict__ uvp) {
  const int hh = h / 2, hw = w / 2;
  const int64_t n = (int64_t)hh * hw, plane = (int64_t)h * w;
  for (int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; blk < n; blk += (int64_t)gridDim.x * blockDim.x) {
    const int by = (int)(blk / hw), bx = (int)(blk - (int64_t)by * hw);
    float cb[2][2], cr[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int64_t q = (int64_t)(2 * by + dy) * w + 2 * bx + dx;
        float y;
        rgb_to_ycc(smp(src[q]), smp(src[plane + q]), smp(src[2 * plane + q]), y, cb[dy][dx], cr[dy][dx]);
        yp[q] = clamp01(y);
      }
    uvp[blk] = clamp01(mean4(cb[0][0], cb[0][1], cb[1][0], cb[1][1], hw == 1));
    uvp[n + blk] = clamp01(mean4(cr[0][0], cr[0][1], cr[1][0], cr[1][1], hw == 1));
  }
}

// yuv420_kernel (frame.hip) on fp32 planes: ycbcr420_to_444(order=0) + pad
__global__ void yuv420f_kernel(const float *__restrict__ ysrc, const float *__restrict__ uvsrc, int h, int w,
                               FView out) {
  const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= (int64_t)out.H * out.W) return;
  const int py = (int)(pix / out.W), px = (int)(pix - (int64_t)py * out.W);
  const int sy = min(py, h - 1), sx = min(px, w - 1);
  const int hh = h / 2, hw = w / 2;
  const int uy = zoom_src(sy, hh), ux = zoom_src(sx, hw);
  float *o = out.p + pix * out.cs + out.co;
  o[0] = ysrc[(int64_t)sy * w + sx];
  o[1] = uvsrc[(int64_t)uy * hw + ux];
  o[2] = uvsrc[(int64_t)hh * hw + (int64_t)uy * hw + ux];
}

// sse_rgb_kernel (frame.hip) against a planar fp32 source
__global__ void __launch_bounds__(SSE_BLOCK) sse_rgb_f32_kernel(FView xh, const float *__restrict__ src, int h,
                                                                int w, double *part) {
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
      const float d0 = v0 - src[o], d1 = v1 - src[plane + o], d2 = v2 - src[2 * plane + o];
      a[0] += (double)(d0 * d0);
      a[1] += (double)(d1 * d1);
      a[2] += (double)(d2 * d2);
    }
  }
  block_sum3(a[0], a[1], a[2], part);
}

// sse_yuv420_kernel (frame.hip) against fp32 Y and U|V source planes.  Like
// its uint8 twin it sums a chroma block as (x00 + x01) + (x10 + x11) at every
// width: the one-column order of mean4 (w = 2) is followed by the conversion
// kernels only, the distortion twins keep the uint8 kernels' arithmetic.
__global__ void __launch_bounds__(SSE_BLOCK) sse_yuv420_f32_kernel(FView xh, const float *__restrict__ ysrc,
                                                                   const float *__restrict__ uvsrc, int h, int w,
                                                                   double *part) {
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
          const double d = (double)v[dy][dx][0] - (double)ysrc[(int64_t)(2 * by + dy) * w + 2 * bx + dx];
          a[0] += d * d;
        }
#pragma unroll
      for (int c = 1; c < 3; ++c) {
        const float s = (v[0][0][c] + v[0][1][c]) + (v[1][0][c] + v[1][1][c]);
        const float m = clamp01(s / 4.f);
        const double d = (double)m - (double)uvsrc[(int64_t)(c - 1) * hh * hw + (int64_t)by * hw + bx];
        a[c] += d * d;
      }
    }
  }
  block_sum3(a[0], a[1], a[2], part);
}

// planes_kernel (msssim.hip) with fp32 source planes: one thread per 2x2 block
// (chroma sum order as the uint8 twin at every width, see sse_yuv420_f32_kernel)
__global__ void planes_f32_kernel(FView xh, const float *__restrict__ ysrc, const float *__restrict__ uvsrc, int h,
                                  int w, double *__restrict__ sp, double *__restrict__ rp) {
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
      for (int c = 0; c < 3; ++c) v[dy][dx][c] = clamp01(p[c]);
    }
  const int64_t plane = (int64_t)h * w, cplane = (int64_t)hh * hw;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int64_t o = (int64_t)(2 * by + dy) * w + 2 * bx + dx;
      sp[o] = (double)ysrc[o];
      rp[o] = (double)v[dy][dx][0];
    }
#pragma unroll
  for (int c = 1; c < 3; ++c) {
    const float s = (v[0][0][c] + v[0][1][c]) + (v[1][0][c] + v[1][1][c]);
    const int64_t o = plane + (int64_t)(c - 1) * cplane + b;
    sp[o] = (double)uvsrc[(int64_t)(c - 1) * cplane + b];
    rp[o] = (double)clamp01(s / 4.f);
  }
}

// rgb_planes_kernel (msssim.hip) with a planar fp32 source
__global__ void rgb_planes_f32_kernel(FView xh, const float *__restrict__ src, int h, int w, double *__restrict__ sp,
                                      double *__restrict__ rp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)h * w;
  if (i >= n) return;
  const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
  const float *p = xh.p + ((int64_t)y * xh.W + x) * xh.cs + xh.co;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sp[c * n + i] = (double)src[c * n + i];
    rp[c * n + i] = (double)clamp01(p[c]);
  }
}

// dcvc_recon_to_u8_cross, a YUV 4:4:4 frame into PNGWriter: ycbcr444_to_420 of
// the crop (Y clipped; U, V = clipped 2x2 means of the values as given, as
// recon_yuv_u8_kernel), ycbcr420_to_rgb(order=1), clip(rint(v * 255)) as HWC
// uint8.  One thread per crop pixel, recomputing the four block means per
// chroma plane its taps need (block_mean, crossfmt.h).
__global__ void recon_yuv_rgb_u8_kernel(FView xh, int h, int w, double zy, double zx, uint8_t *__restrict__ out) {
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
    out[pix * 3 + 0] = q255(r);
    out[pix * 3 + 1] = q255(g);
    out[pix * 3 + 2] = q255(b);
  }
}

// dcvc_recon_to_u8_cross, an RGB frame into YUVWriter: rgb_to_ycbcr420 of the
// crop, clip(rint(v * 255)) into Y | U | V planes; one thread per 2x2 block
__global__ void recon_rgb_yuv_u8_kernel(FView xh, int h, int w, uint8_t *__restrict__ out) {
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
        out[(int64_t)(2 * by + dy) * w + 2 * bx + dx] = q255(clamp01(y));
      }
    out[plane + blk] = q255(clamp01(mean4(cb[0][0], cb[0][1], cb[1][0], cb[1][1], hw == 1)));
    out[plane + n + blk] = q255(clamp01(mean4(cr[0][0], cr[0][1], cr[1][0], cr[1][1], hw == 1)));
  }
}

}  // namespace

extern "C" int dcvc_yuv420_to_rgb_nhwc(const uint8_t *y, const uint8_t *uv, int h, int w, dcvc_tensor out,
                                       float *rgb_planes, void *stream) {
  if (!y || !uv || !rgb_planes || !frame_ok(out) || !even_frame(h, w) || out.H < h || out.W < w)
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)out.H * out.W;
  hipLaunchKernelGGL(yuv420_rgb_kernel<uint8_t>, dim3(cf_blocks(n)), dim3(CF_BLOCK), 0, st, y, uv, h, w,
                     zoom_ratio(h / 2), zoom_ratio(w / 2), fv(out), rgb_planes);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_yuv420f_to_rgb_nhwc(const float *y, const float *uv, int h, int w, float *out, int H, int W,
                                        int cstride, int coff, float *rgb_planes, void *stream) {
  if (!y || !uv || !rgb_planes || !view_ok(out, H, W, cstride, coff) || !even_frame(h, w) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(yuv420_rgb_kernel<float>, dim3(cf_blocks(n)), dim3(CF_BLOCK), 0, st, y, uv, h, w,
                     zoom_ratio(h / 2), zoom_ratio(w / 2), fvs(out, H, W, cstride, coff), rgb_planes);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_rgbf_to_yuv420_planes(const float *rgb, int h, int w, float *y_plane, float *uv_planes,
                                          void *stream) {
  if (!rgb || !y_plane || !uv_planes || !even_frame(h, w)) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)(h / 2) * (w / 2);
  hipLaunchKernelGGL(rgb_yuv420_planes_kernel<float>, dim3(cf_blocks(n)), dim3(CF_BLOCK), 0, st, rgb, h, w, y_plane,
                     uv_planes);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_rgb_to_yuv420_planes(const uint8_t *rgb, int h, int w, float *y_plane, float *uv_planes,
                                         void *stream) {
  if (!rgb || !y_plane || !uv_planes || !even_frame(h, w)) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)(h / 2) * (w / 2);
  hipLaunchKernelGGL(rgb_yuv420_planes_kernel<uint8_t>, dim3(cf_blocks(n)), dim3(CF_BLOCK), 0, st, rgb, h, w, y_plane,
                     uv_planes);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_yuv420f_to_nhwc(const float *y, const float *uv, int h, int w, dcvc_tensor out, void *stream) {
  if (!y || !uv || !frame_ok(out) || !even_frame(h, w) || out.H < h || out.W < w) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)out.H * out.W;
  hipLaunchKernelGGL(yuv420f_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, y, uv, h, w, fv(out));
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_frame_sse_f32(dcvc_tensor x_hat, const float *src, const float *uv, int h, int w, int yuv420,
                                  double *workspace, double *out3, void *stream) {
  if (!frame_ok(x_hat) || !src || !workspace || !out3 || h <= 0 || w <= 0 || x_hat.H < h || x_hat.W < w)
    return DCVC_HIP_EINVAL;
  if (yuv420 && (!uv || (h & 1) || (w & 1) || (x_hat.H & 1) || (x_hat.W & 1))) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned g;
  if (yuv420) {
    g = sse_blocks((int64_t)(x_hat.H / 2) * (x_hat.W / 2));
    hipLaunchKernelGGL(sse_yuv420_f32_kernel, dim3(g), dim3(SSE_BLOCK), 0, st, fv(x_hat), src, uv, h, w, workspace);
  } else {
    g = sse_blocks((int64_t)x_hat.H * x_hat.W);
    hipLaunchKernelGGL(sse_rgb_f32_kernel, dim3(g), dim3(SSE_BLOCK), 0, st, fv(x_hat), src, h, w, workspace);
  }
  DCVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sse_final_kernel, dim3(1), dim3(256), 0, st, workspace, (int)g, out3);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_yuv_planes_f64_f32(dcvc_tensor x_hat, const float *y, const float *uv, int h, int w,
                                       double *src_planes, double *rec_planes, void *stream) {
  if (!frame_ok(x_hat) || x_hat.H < h || x_hat.W < w || !y || !uv || !src_planes || !rec_planes ||
      !even_frame(h, w))
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)(h / 2) * (w / 2);
  hipLaunchKernelGGL(planes_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fv(x_hat), y, uv, h, w,
                     src_planes, rec_planes);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_rgb_planes_f64_f32(dcvc_tensor x_hat, const float *src, int h, int w, double *src_planes,
                                       double *rec_planes, void *stream) {
  if (!frame_ok(x_hat) || x_hat.H < h || x_hat.W < w || !src || !src_planes || !rec_planes || h < 1 || w < 1)
    return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(rgb_planes_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fv(x_hat), src, h,
                     w, src_planes, rec_planes);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_recon_to_u8_cross(dcvc_tensor x_hat, int h, int w, int to_rgb, uint8_t *out, void *stream) {
  if (!frame_ok(x_hat) || !out || !even_frame(h, w) || x_hat.H < h || x_hat.W < w) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (to_rgb)
    hipLaunchKernelGGL(recon_yuv_rgb_u8_kernel, dim3(cf_blocks((int64_t)h * w)), dim3(CF_BLOCK), 0, st, fv(x_hat), h,
                       w, zoom_ratio(h / 2), zoom_ratio(w / 2), out);
  else
    hipLaunchKernelGGL(recon_rgb_yuv_u8_kernel, dim3(cf_blocks((int64_t)(h / 2) * (w / 2))), dim3(CF_BLOCK), 0, st,
                       fv(x_hat), h, w, out);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}
