// Planar YUV sources and output at any of the three chroma layouts, 8..16 bits
// per sample.  A chroma format is (SX, SY): 4:4:4 = (1, 1), 4:2:2 = (2, 1),
// 4:2:0 = (2, 2); a frame is Y (h x w) | U | V (h/SY x w/SX each), uint8 at 8
// bits and little-endian uint16 above.  The DC YUV checkpoints code a YCbCr
// 4:4:4 tensor, so a 4:4:4 source needs no resampling and a 4:2:2 source the
// horizontal half of what a 4:2:0 source needs:
//
//   * dcvc_yuvp_to_nhwc: the order-0 zoom of ycbcr420_to_444 along the
//     subsampled axes (zoom_src) + replicate padding.
//   * dcvc_yuvp_to_rgb_nhwc: the order-1 zoom of ycbcr420_to_rgb along the
//     subsampled axes (zoom1_tap), ycbcr_to_rgb (DCVC-DC/src/transforms/
//     functional.py:114-126), padding, and the planar fp32 RGB source.
//   * dcvc_yuvp_sse: the in-place clamp of the padded frame and the per-plane
//     squared-error sums at the source's own chroma resolution.
//   * dcvc_recon_to_yuvp: the decoded frame (YCbCr 4:4:4 or RGB) into the
//     samples of a planar file of that layout and depth.
//
// These four kernel templates are the only ones for their operations.  The
// 4:2:0 entry points of frame.hip, frame16.hip and crossfmt.hip (uint8,
// uint16 and fp32-plane sources), which the harness still calls for 4:2:0,
// check their own arguments and run the (2, 2) instantiation through the same
// launchers (frame.h), so a rounding rule is stated here once.  Bandwidth
// kernels without reuse: ingest runs one thread per padded output pixel, the
// distortion and the writer one thread per chroma sample's SX x SY footprint,
// consecutive lanes on consecutive samples of a plane row.  Arithmetic is
// written operation by operation in numpy's order (crossfmt.h), contraction
// off wherever numpy rounds in between.
//
// The NHWC frame arrives as scalars (base, H, W, cstride, coff: the FView of
// frame.h), not as a dcvc_tensor.
#include "crossfmt.h"

namespace {

// order-1 zoom along one axis only: float32(v0 * w0 + v1 * w1) summed in
// double (bilerp with an identity tap on the other axis)
__device__ __forceinline__ float lerp1(float v0, float v1, const Tap &t) {
#pragma clang fp contract(off)
  const double p0 = (double)v0 * t.w0;
  const double p1 = (double)v1 * t.w1;
  return (float)(p0 + p1);
}

// float32 mean of a chroma sample's SX x SY footprint as numpy forms it:
// the value itself, (x0 + x1) / 2, or mean4
template <int SX, int SY>
__device__ __forceinline__ float foot_mean(const float (&v)[SY][SX], bool seq) {
  if constexpr (SX == 1) {
    return v[0][0];
  } else if constexpr (SY == 1) {
    return (v[0][0] + v[0][1]) / 2.f;
  } else {
    return mean4(v[0][0], v[0][1], v[1][0], v[1][1], seq);
  }
}

// rule 1: one thread per pixel of the padded output
template <typename T, int SX, int SY>
__global__ void yuvp_kernel(const T *__restrict__ ysrc, const T *__restrict__ uvsrc, int h, int w, float mx,
                            FView out) {
  const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= (int64_t)out.H * out.W) return;
  const int ch = h / SY, cw = w / SX;
  const int64_t cplane = (int64_t)ch * cw;
  const int py = (int)(pix / out.W), px = (int)(pix - (int64_t)py * out.W);
  const int sy = min(py, h - 1), sx = min(px, w - 1);
  const int uy = SY == 2 ? zoom_src(sy, ch) : sy, ux = SX == 2 ? zoom_src(sx, cw) : sx;
  const int64_t c = (int64_t)uy * cw + ux;
  float *o = out.p + pix * out.cs + out.co;
  o[0] = smp(ysrc[(int64_t)sy * w + sx], mx);
  o[1] = smp(uvsrc[c], mx);
  o[2] = smp(uvsrc[cplane + c], mx);
}

// rule 2: one thread per pixel of the padded output; a padding pixel
// recomputes its edge pixel; rgb_planes (3 x h x w) receives the crop
template <typename T, int SX, int SY>
__global__ void yuvp_rgb_kernel(const T *__restrict__ ysrc, const T *__restrict__ uvsrc, int h, int w, float mx,
                                double zy, double zx, FView out, float *__restrict__ rgb_planes) {
  const int64_t n = (int64_t)out.H * out.W;
  const int ch = h / SY, cw = w / SX;
  const int64_t cplane = (int64_t)ch * cw, plane = (int64_t)h * w;
  for (int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < n; pix += (int64_t)gridDim.x * blockDim.x) {
    const int py = (int)(pix / out.W), px = (int)(pix - (int64_t)py * out.W);
    const int sy = min(py, h - 1), sx = min(px, w - 1);
    const float yv = smp(ysrc[(int64_t)sy * w + sx], mx);
    float cb, cr;
    if constexpr (SX == 1) {
      const int64_t c = (int64_t)sy * cw + sx;
      cb = smp(uvsrc[c], mx);
      cr = smp(uvsrc[cplane + c], mx);
    } else if constexpr (SY == 1) {
      const Tap tc = zoom1_tap(sx, cw, zx);
      const int64_t c0 = (int64_t)sy * cw + tc.i0, c1 = (int64_t)sy * cw + tc.i1;
      cb = lerp1(smp(uvsrc[c0], mx), smp(uvsrc[c1], mx), tc);
      cr = lerp1(smp(uvsrc[cplane + c0], mx), smp(uvsrc[cplane + c1], mx), tc);
    } else {
      const Tap tr = zoom1_tap(sy, ch, zy), tc = zoom1_tap(sx, cw, zx);
      const int64_t o00 = (int64_t)tr.i0 * cw + tc.i0, o01 = (int64_t)tr.i0 * cw + tc.i1;
      const int64_t o10 = (int64_t)tr.i1 * cw + tc.i0, o11 = (int64_t)tr.i1 * cw + tc.i1;
      cb = bilerp(smp(uvsrc[o00], mx), smp(uvsrc[o01], mx), smp(uvsrc[o10], mx), smp(uvsrc[o11], mx), tr, tc);
      cr = bilerp(smp(uvsrc[cplane + o00], mx), smp(uvsrc[cplane + o01], mx), smp(uvsrc[cplane + o10], mx),
                  smp(uvsrc[cplane + o11], mx), tr, tc);
    }
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

// rule 3: clamp_ in place over the padded frame, then per plane the fp64
// squared error of the crop against the samples (dist_in_yuv420,
// DCVC-DC/test_video.py:171-181, calc_psnr, metrics.py:81-92): Y pixel by
// pixel, U / V the clipped fp32 footprint mean of the clamped values, a 2x2
// footprint summed (x00 + x01) + (x10 + x11) at every width; differences and
// squares in double.  One thread per footprint of the padded frame (bh x bw
// of them).  A footprint cut by an odd view edge clamps the pixels it has: its
// first row and column always lie inside, bh and bw being rounded up, and the
// coordinates beyond the edge fall back on them, so every load is
// unconditional and the clamp, being idempotent, is merely applied twice there;
// no crop footprint is cut, the view being at least the frame.  The block size,
// sse_blocks and the order of a thread's sums fix the fp64 result.
template <typename T, int SX, int SY>
__global__ void __launch_bounds__(SSE_BLOCK) sse_yuvp_kernel(FView xh, const T *__restrict__ ysrc,
                                                             const T *__restrict__ uvsrc, int h, int w, float mx,
                                                             int bh, int bw, double *part) {
  double a[3] = {0.0, 0.0, 0.0};
  const int ch = h / SY, cw = w / SX;
  const int64_t n = (int64_t)bh * bw;
  for (int64_t b = (int64_t)blockIdx.x * SSE_BLOCK + threadIdx.x; b < n; b += (int64_t)gridDim.x * SSE_BLOCK) {
    const int by = (int)(b / bw), bx = (int)(b - (int64_t)by * bw);
    float v[3][SY][SX];
#pragma unroll
    for (int dy = 0; dy < SY; ++dy)
#pragma unroll
      for (int dx = 0; dx < SX; ++dx) {
        const int py = min(SY * by + dy, xh.H - 1), px = min(SX * bx + dx, xh.W - 1);
        float *p = xh.p + ((int64_t)py * xh.W + px) * xh.cs + xh.co;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c][dy][dx] = clamp01(p[c]);
          p[c] = v[c][dy][dx];
        }
      }
    if (by < ch && bx < cw) {
#pragma unroll
      for (int dy = 0; dy < SY; ++dy)
#pragma unroll
        for (int dx = 0; dx < SX; ++dx) {
          const double d =
              (double)v[0][dy][dx] - (double)smp(ysrc[(int64_t)(SY * by + dy) * w + SX * bx + dx], mx);
          a[0] += d * d;
        }
#pragma unroll
      for (int c = 1; c < 3; ++c) {
        const float m = clamp01(foot_mean<SX, SY>(v[c], false));
        const double d = (double)m - (double)smp(uvsrc[(int64_t)(c - 1) * ch * cw + (int64_t)by * cw + bx], mx);
        a[c] += d * d;
      }
    }
  }
  block_sum3(a[0], a[1], a[2], part);
}

// rule 4: one thread per chroma sample of the crop: the Y samples of its
// footprint and its U, V samples.  FROM_RGB = false: a YCbCr 4:4:4 frame, Y
// clipped, U / V the clipped footprint mean of the values as given
// (ycbcr444_to_420; run_test hands over the frame already clamped).  FROM_RGB
// = true: rgb_to_ycbcr per pixel, Y clipped, Cb / Cr unclipped into the
// footprint mean (mean4's one-column order included), then clipped
// (rgb_to_ycbcr420, as YUVWriter stores an RGB frame).
template <typename T, int SX, int SY, bool FROM_RGB>
__global__ void recon_yuvp_kernel(FView xh, int h, int w, float mx, T *__restrict__ out) {
  const int ch = h / SY, cw = w / SX;
  const int64_t n = (int64_t)ch * cw, plane = (int64_t)h * w;
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const int by = (int)(b / cw), bx = (int)(b - (int64_t)by * cw);
  float cb[SY][SX], cr[SY][SX];
#pragma unroll
  for (int dy = 0; dy < SY; ++dy)
#pragma unroll
    for (int dx = 0; dx < SX; ++dx) {
      const int py = SY * by + dy, px = SX * bx + dx;
      const float *p = xh.p + ((int64_t)py * xh.W + px) * xh.cs + xh.co;
      float y;
      if constexpr (FROM_RGB) {
        rgb_to_ycc(p[0], p[1], p[2], y, cb[dy][dx], cr[dy][dx]);
      } else {
        y = p[0];
        cb[dy][dx] = p[1];
        cr[dy][dx] = p[2];
      }
      qst(out + (int64_t)py * w + px, clamp01(y), mx);
    }
  const bool seq = FROM_RGB && cw == 1;
  qst(out + plane + b, clamp01(foot_mean<SX, SY>(cb, seq)), mx);
  qst(out + plane + n + b, clamp01(foot_mean<SX, SY>(cr, seq)), mx);
}

// 4:4:4, 4:2:2 or 4:2:0
bool layout_ok(int sub_x, int sub_y) {
  return (sub_x == 1 && sub_y == 1) || (sub_x == 2 && (sub_y == 1 || sub_y == 2));
}

bool yuvp_ok(int h, int w, int depth, int sub_x, int sub_y) {
  return layout_ok(sub_x, sub_y) && depth_ok(depth, 8) && h >= 1 && w >= 1 && h % sub_y == 0 && w % sub_x == 0;
}

FSample sample_of(int depth) { return depth == 8 ? FS_U8 : FS_U16; }

// LAUNCH(T, SX, SY) for the instantiations an entry point can reach: uint8 and
// uint16 samples at the three layouts, and for fp32 planes at 4:2:0 FLOAT_CASE
// (the launch, or a return where there is none); anything else is
// DCVC_HIP_EINVAL
#define YUVP_LAYOUTS(T, LAUNCH) \
  do {                          \
    if (sub_x == 1) {           \
      LAUNCH(T, 1, 1);          \
    } else if (sub_y == 1) {    \
      LAUNCH(T, 2, 1);          \
    } else {                    \
      LAUNCH(T, 2, 2);          \
    }                           \
  } while (0)
#define YUVP_DISPATCH(s, LAUNCH, FLOAT_CASE)                   \
  do {                                                         \
    if ((s) == FS_U8) {                                        \
      YUVP_LAYOUTS(uint8_t, LAUNCH);                           \
    } else if ((s) == FS_U16) {                                \
      YUVP_LAYOUTS(uint16_t, LAUNCH);                          \
    } else if ((s) == FS_F32 && sub_x == 2 && sub_y == 2) {    \
      FLOAT_CASE;                                              \
    } else {                                                   \
      return DCVC_HIP_EINVAL;                                  \
    }                                                          \
    DCVC_LAUNCH_CHECK();                                       \
  } while (0)

}  // namespace

int dcvc_internal_yuv_ingest(FSample s, float mx, int sub_x, int sub_y, const void *y, const void *uv, int h, int w,
                             FView out, hipStream_t st) {
  if (!layout_ok(sub_x, sub_y)) return DCVC_HIP_EINVAL;
  const unsigned g = item_blocks((int64_t)out.H * out.W);
  if (!g) return DCVC_HIP_EINVAL;
#define LAUNCH(T, SX, SY)                                                                                    \
  hipLaunchKernelGGL((yuvp_kernel<T, SX, SY>), dim3(g), dim3(ITEM_BLOCK), 0, st, static_cast<const T *>(y), \
                     static_cast<const T *>(uv), h, w, mx, out)
  YUVP_DISPATCH(s, LAUNCH, LAUNCH(float, 2, 2));
#undef LAUNCH
  return DCVC_HIP_OK;
}

int dcvc_internal_yuv_ingest_rgb(FSample s, float mx, int sub_x, int sub_y, const void *y, const void *uv, int h,
                                 int w, FView out, float *rgb_planes, hipStream_t st) {
  if (!layout_ok(sub_x, sub_y)) return DCVC_HIP_EINVAL;
  const unsigned g = cf_blocks((int64_t)out.H * out.W);
  const double zy = zoom_ratio(h / sub_y), zx = zoom_ratio(w / sub_x);
#define LAUNCH(T, SX, SY)                                                                                       \
  hipLaunchKernelGGL((yuvp_rgb_kernel<T, SX, SY>), dim3(g), dim3(CF_BLOCK), 0, st, static_cast<const T *>(y), \
                     static_cast<const T *>(uv), h, w, mx, zy, zx, out, rgb_planes)
  YUVP_DISPATCH(s, LAUNCH, LAUNCH(float, 2, 2));
#undef LAUNCH
  return DCVC_HIP_OK;
}

int dcvc_internal_yuv_sse(FSample s, float mx, int sub_x, int sub_y, FView xh, const void *y, const void *uv, int h,
                          int w, double *workspace, double *out3, hipStream_t st) {
  if (!layout_ok(sub_x, sub_y)) return DCVC_HIP_EINVAL;
  const int bh = (xh.H + sub_y - 1) / sub_y, bw = (xh.W + sub_x - 1) / sub_x;
  const unsigned g = sse_blocks((int64_t)bh * bw);
#define LAUNCH(T, SX, SY)                                                               \
  hipLaunchKernelGGL((sse_yuvp_kernel<T, SX, SY>), dim3(g), dim3(SSE_BLOCK), 0, st, xh, \
                     static_cast<const T *>(y), static_cast<const T *>(uv), h, w, mx, bh, bw, workspace)
  YUVP_DISPATCH(s, LAUNCH, LAUNCH(float, 2, 2));
#undef LAUNCH
  hipLaunchKernelGGL(sse_final_kernel, dim3(1), dim3(256), 0, st, workspace, (int)g, out3);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

int dcvc_internal_yuv_write(FSample s, float mx, int sub_x, int sub_y, bool from_rgb, FView xh, int h, int w,
                            void *out, hipStream_t st) {
  if (!layout_ok(sub_x, sub_y)) return DCVC_HIP_EINVAL;
  const unsigned g = item_blocks((int64_t)(h / sub_y) * (w / sub_x));
  if (!g) return DCVC_HIP_EINVAL;
#define LAUNCH(T, SX, SY)                                                                                       \
  do {                                                                                                          \
    if (from_rgb)                                                                                               \
      hipLaunchKernelGGL((recon_yuvp_kernel<T, SX, SY, true>), dim3(g), dim3(ITEM_BLOCK), 0, st, xh, h, w, mx,  \
                         static_cast<T *>(out));                                                                \
    else                                                                                                        \
      hipLaunchKernelGGL((recon_yuvp_kernel<T, SX, SY, false>), dim3(g), dim3(ITEM_BLOCK), 0, st, xh, h, w, mx, \
                         static_cast<T *>(out));                                                                \
  } while (0)
  YUVP_DISPATCH(s, LAUNCH, return DCVC_HIP_EINVAL);
#undef LAUNCH
  return DCVC_HIP_OK;
}

extern "C" int dcvc_yuvp_to_nhwc(const void *y, const void *uv, int h, int w, int depth, int sub_x, int sub_y,
                                 float *out, int H, int W, int cstride, int coff, void *stream) {
  if (!y || !uv || !view_ok(out, H, W, cstride, coff) || !yuvp_ok(h, w, depth, sub_x, sub_y) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_ingest(sample_of(depth), max_val(depth), sub_x, sub_y, y, uv, h, w,
                                  fvs(out, H, W, cstride, coff), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_yuvp_to_rgb_nhwc(const void *y, const void *uv, int h, int w, int depth, int sub_x, int sub_y,
                                     float *out, int H, int W, int cstride, int coff, float *rgb_planes,
                                     void *stream) {
  if (!y || !uv || !rgb_planes || !view_ok(out, H, W, cstride, coff) || !yuvp_ok(h, w, depth, sub_x, sub_y) ||
      H < h || W < w)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_ingest_rgb(sample_of(depth), max_val(depth), sub_x, sub_y, y, uv, h, w,
                                      fvs(out, H, W, cstride, coff), rgb_planes,
                                      reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_yuvp_sse(float *x_hat, int H, int W, int cstride, int coff, const void *y, const void *uv, int h,
                             int w, int depth, int sub_x, int sub_y, double *workspace, double *out3, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !y || !uv || !workspace || !out3 ||
      !yuvp_ok(h, w, depth, sub_x, sub_y) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_sse(sample_of(depth), max_val(depth), sub_x, sub_y, fvs(x_hat, H, W, cstride, coff), y, uv,
                               h, w, workspace, out3, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dcvc_recon_to_yuvp(const float *x_hat, int H, int W, int cstride, int coff, int h, int w, int depth,
                                  int sub_x, int sub_y, int from_rgb, void *out, void *stream) {
  if (!view_ok(x_hat, H, W, cstride, coff) || !out || !yuvp_ok(h, w, depth, sub_x, sub_y) || H < h || W < w)
    return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_write(sample_of(depth), max_val(depth), sub_x, sub_y, from_rgb != 0,
                                 fvs(x_hat, H, W, cstride, coff), h, w, out, reinterpret_cast<hipStream_t>(stream));
}
