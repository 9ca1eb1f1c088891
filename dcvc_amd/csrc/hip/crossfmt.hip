// Cross-format frame entry points of run_test (DCVC-DC/test_video.py:79-119):
// a YUV420 source coded by an RGB model and an RGB source coded by a YUV420
// model, as the reference's readers convert them (video_reader.py:33-42,
// src/transforms/functional.py:16-58), the RGB decoded-frame writers
// (video_writer.py:26-111), and the float64 planes MS-SSIM is computed on.
//
//   * dcvc_yuv420_to_rgb_nhwc, dcvc_yuv420f_to_rgb_nhwc: ycbcr420_to_rgb(y, uv,
//     order=1) of uint8 / 255 or fp32 planes, padded NHWC codec input plus the
//     planar fp32 RGB source (chroma.hip's ingest-to-RGB at 4:2:0).
//   * dcvc_rgb_to_yuv420_planes + dcvc_yuv420f_to_nhwc: rgb_to_ycbcr420(rgb /
//     255) as fp32 planes, then ycbcr420_to_444(order=0) + replicate padding
//     (chroma.hip's ingest at 4:2:0 on fp32 planes).
//   * dcvc_frame_sse_f32: the distortion against those fp32 source planes
//     (chroma.hip's and frame.hip's distortion kernels on fp32 samples).
//   * dcvc_yuv_planes_f64, dcvc_rgb_planes_f64 and their _f32 twins: the
//     MS-SSIM inputs (msssim.hip computes on them) from uint8 or fp32 sources.
//   * dcvc_recon_to_u8_cross: a YUV 4:4:4 frame as PNGWriter stores it, an RGB
//     frame as YUVWriter stores it (chroma.hip's writer at 4:2:0).
//
// Every value is bit-equal to the reference's numpy / scipy result, so the
// colour arithmetic (crossfmt.h, shared with chroma.hip) is written operation
// by operation in numpy's order with contraction into FMAs switched off (numpy
// rounds after every ufunc).
#include "crossfmt.h"

namespace {

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

// channel c of RGB pixel pix of n as the writers lay a frame out: HWC
// (PNGWriter, the uint8 output) or planar 3 x h x w (RGBWriter, video_writer.py:
// 72-77, the uint16 output)
template <bool PLANAR, typename T>
__device__ __forceinline__ void rgb_store(T *out, int64_t pix, int64_t n, int c, float v, float mx) {
  qst(out + (PLANAR ? c * n + pix : pix * 3 + c), v, mx);
}

// an RGB frame's crop as file samples: one thread per crop pixel
template <typename T, bool PLANAR>
__global__ void recon_rgb_kernel(FView xh, int h, int w, float mx, T *__restrict__ out) {
  const int64_t n = (int64_t)h * w;
  const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= n) return;
  const int py = (int)(pix / w), px = (int)(pix - (int64_t)py * w);
  const float *p = xh.p + ((int64_t)py * xh.W + px) * xh.cs + xh.co;
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb_store<PLANAR>(out, pix, n, c, p[c], mx);
}

// a YUV 4:4:4 frame's crop as RGB file samples: ycbcr444_to_420 of the crop (Y
// clipped; U, V = clipped 2x2 means of the values as given), ycbcr420_to_rgb(
// order=1), then the quantiser.  One thread per crop pixel, recomputing the
// four block means per chroma plane its taps need (block_mean, crossfmt.h).
template <typename T, bool PLANAR>
__global__ void recon_yuv_rgb_kernel(FView xh, int h, int w, double zy, double zx, float mx, T *__restrict__ out) {
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
    rgb_store<PLANAR>(out, pix, n, 0, r, mx);
    rgb_store<PLANAR>(out, pix, n, 1, g, mx);
    rgb_store<PLANAR>(out, pix, n, 2, b, mx);
  }
}

// The float64 planes calc_msssim receives for a YUV420 source: the source
// planes and the clamped recon's ycbcr444_to_420 planes (functional.py:75-95),
// cropped, each [Y h*w | U hh*hw | V hh*hw].  One thread per 2x2 block of the
// crop; the chroma sum is (x00 + x01) + (x10 + x11) at every width, as the
// distortion forms it (sse_yuvp_kernel, chroma.hip).  S: uint8 or fp32 planes.
template <typename S>
__global__ void planes_kernel(FView xh, const S *__restrict__ ysrc, const S *__restrict__ uvsrc, int h, int w,
                              double *__restrict__ sp, double *__restrict__ rp) {
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
      sp[o] = (double)smp(ysrc[o]);
      rp[o] = (double)v[dy][dx][0];
    }
#pragma unroll
  for (int c = 1; c < 3; ++c) {
    const float s = (v[0][0][c] + v[0][1][c]) + (v[1][0][c] + v[1][1][c]);
    const int64_t o = plane + (int64_t)(c - 1) * cplane + b;
    sp[o] = (double)smp(uvsrc[(int64_t)(c - 1) * cplane + b]);
    rp[o] = (double)clamp01(s / 4.f);
  }
}

// The float64 planes of RGB MS-SSIM (msssim.hip): the planar source and the
// clamped recon's crop, 3 x h x w each.  One thread per crop pixel.
template <typename S>
__global__ void rgb_planes_kernel(FView xh, const S *__restrict__ src, int h, int w, double *__restrict__ sp,
                                  double *__restrict__ rp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)h * w;
  if (i >= n) return;
  const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
  const float *p = xh.p + ((int64_t)y * xh.W + x) * xh.cs + xh.co;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sp[c * n + i] = (double)smp(src[c * n + i]);
    rp[c * n + i] = (double)clamp01(p[c]);
  }
}

}  // namespace

int dcvc_internal_rgb_write(FSample s, float mx, bool from_yuv, FView xh, int h, int w, void *out, hipStream_t st) {
  if (s != FS_U8 && s != FS_U16) return DCVC_HIP_EINVAL;
  const int64_t n = (int64_t)h * w;
  const unsigned g = item_blocks(n);
  if (!g) return DCVC_HIP_EINVAL;
#define LAUNCH(T, PLANAR)                                                                                        \
  do {                                                                                                           \
    if (from_yuv)                                                                                                \
      hipLaunchKernelGGL((recon_yuv_rgb_kernel<T, PLANAR>), dim3(cf_blocks(n)), dim3(CF_BLOCK), 0, st, xh, h, w, \
                         zoom_ratio(h / 2), zoom_ratio(w / 2), mx, static_cast<T *>(out));                       \
    else                                                                                                         \
      hipLaunchKernelGGL((recon_rgb_kernel<T, PLANAR>), dim3(g), dim3(ITEM_BLOCK), 0, st, xh, h, w, mx,          \
                         static_cast<T *>(out));                                                                 \
  } while (0)
  if (s == FS_U8)
    LAUNCH(uint8_t, false);
  else
    LAUNCH(uint16_t, true);
#undef LAUNCH
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

int dcvc_internal_msssim_planes(FSample s, FView xh, const void *src, const void *uv, int h, int w, double *sp,
                                double *rp, hipStream_t st) {
  if (s != FS_U8 && s != FS_F32) return DCVC_HIP_EINVAL;
  const int64_t n = uv ? (int64_t)(h / 2) * (w / 2) : (int64_t)h * w;
  const unsigned g = item_blocks(n);
  if (!g) return DCVC_HIP_EINVAL;
#define LAUNCH(S)                                                                                            \
  do {                                                                                                       \
    if (uv)                                                                                                  \
      hipLaunchKernelGGL(planes_kernel<S>, dim3(g), dim3(ITEM_BLOCK), 0, st, xh, static_cast<const S *>(src), \
                         static_cast<const S *>(uv), h, w, sp, rp);                                          \
    else                                                                                                     \
      hipLaunchKernelGGL(rgb_planes_kernel<S>, dim3(g), dim3(ITEM_BLOCK), 0, st, xh,                         \
                         static_cast<const S *>(src), h, w, sp, rp);                                         \
  } while (0)
  if (s == FS_U8)
    LAUNCH(uint8_t);
  else
    LAUNCH(float);
#undef LAUNCH
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_yuv420_to_rgb_nhwc(const uint8_t *y, const uint8_t *uv, int h, int w, dcvc_tensor out,
                                       float *rgb_planes, void *stream) {
  if (!y || !uv || !rgb_planes || !frame_ok(out) || !even_frame(h, w) || out.H < h || out.W < w)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_ingest_rgb(FS_U8, max_val(8), 2, 2, y, uv, h, w, fv(out), rgb_planes,
                                      reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_yuv420f_to_rgb_nhwc(const float *y, const float *uv, int h, int w, float *out, int H, int W,
                                        int cstride, int coff, float *rgb_planes, void *stream) {
  if (!y || !uv || !rgb_planes || !view_ok(out, H, W, cstride, coff) || !even_frame(h, w) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_ingest_rgb(FS_F32, 1.f, 2, 2, y, uv, h, w, fvs(out, H, W, cstride, coff), rgb_planes,
                                      reinterpret_cast<hipStream_t>(stream));
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
  return dcvc_internal_yuv_ingest(FS_F32, 1.f, 2, 2, y, uv, h, w, fv(out), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_frame_sse_f32(dcvc_tensor x_hat, const float *src, const float *uv, int h, int w, int yuv420,
                                  double *workspace, double *out3, void *stream) {
  if (!frame_ok(x_hat) || !src || !workspace || !out3 || h <= 0 || w <= 0 || x_hat.H < h || x_hat.W < w)
    return DCVC_HIP_EINVAL;
  if (yuv420 && (!uv || !even_frame(h, w) || !even_frame(x_hat.H, x_hat.W))) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (yuv420) return dcvc_internal_yuv_sse(FS_F32, 1.f, 2, 2, fv(x_hat), src, uv, h, w, workspace, out3, st);
  return dcvc_internal_rgb_sse(FS_F32, 1.f, fv(x_hat), src, h, w, workspace, out3, st);
}

extern "C" int dcvc_yuv_planes_f64(dcvc_tensor x_hat, const uint8_t *y, const uint8_t *uv, int h, int w,
                                   double *src_planes, double *rec_planes, void *stream) {
  if (!frame_ok(x_hat) || x_hat.H < h || x_hat.W < w || !y || !uv || !src_planes || !rec_planes ||
      !even_frame(h, w))
    return DCVC_HIP_EINVAL;
  return dcvc_internal_msssim_planes(FS_U8, fv(x_hat), y, uv, h, w, src_planes, rec_planes,
                                     reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_yuv_planes_f64_f32(dcvc_tensor x_hat, const float *y, const float *uv, int h, int w,
                                       double *src_planes, double *rec_planes, void *stream) {
  if (!frame_ok(x_hat) || x_hat.H < h || x_hat.W < w || !y || !uv || !src_planes || !rec_planes ||
      !even_frame(h, w))
    return DCVC_HIP_EINVAL;
  return dcvc_internal_msssim_planes(FS_F32, fv(x_hat), y, uv, h, w, src_planes, rec_planes,
                                     reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_rgb_planes_f64(dcvc_tensor x_hat, const uint8_t *src, int h, int w, double *src_planes,
                                   double *rec_planes, void *stream) {
  if (!frame_ok(x_hat) || x_hat.H < h || x_hat.W < w || !src || !src_planes || !rec_planes || h < 1 || w < 1)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_msssim_planes(FS_U8, fv(x_hat), src, nullptr, h, w, src_planes, rec_planes,
                                     reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_rgb_planes_f64_f32(dcvc_tensor x_hat, const float *src, int h, int w, double *src_planes,
                                       double *rec_planes, void *stream) {
  if (!frame_ok(x_hat) || x_hat.H < h || x_hat.W < w || !src || !src_planes || !rec_planes || h < 1 || w < 1)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_msssim_planes(FS_F32, fv(x_hat), src, nullptr, h, w, src_planes, rec_planes,
                                     reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_recon_to_u8_cross(dcvc_tensor x_hat, int h, int w, int to_rgb, uint8_t *out, void *stream) {
  if (!frame_ok(x_hat) || !out || !even_frame(h, w) || x_hat.H < h || x_hat.W < w) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (to_rgb) return dcvc_internal_rgb_write(FS_U8, max_val(8), true, fv(x_hat), h, w, out, st);
  return dcvc_internal_yuv_write(FS_U8, max_val(8), 2, 2, true, fv(x_hat), h, w, out, st);
}
