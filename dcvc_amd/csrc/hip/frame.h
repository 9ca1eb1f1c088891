// Helpers shared by the harness-side frame kernels (frame.hip, crossfmt.hip,
// frame16.hip, chroma.hip): the NHWC frame view, sample access (a uint8 /
// uint16 / fp32 source sample as the reader's float, a value as the writer's
// uint8 / uint16 sample), scipy's order-0 zoom index map, the fixed-order
// squared-error reduction, the argument predicates of the entry points, and
// the one host launcher each operation has.
#pragma once
#include "common.h"

struct FView {
  float *p;
  int H, W, cs, co;
};

// The sample type of a source or an output file: uint8, little-endian uint16
// of 9..16 bits (mx = max_val(depth)), or fp32 planes already in [0, 1].
enum FSample { FS_U8, FS_U16, FS_F32 };

// One host launcher per operation; every extern "C" entry point of the four
// files is its argument check and a call to one of these.  Each is defined
// once, next to its kernel template (the kernels are file-local: a template
// instantiated from two files would be compiled twice).  (sub_x, sub_y) is the
// chroma layout, (1, 1) | (2, 1) | (2, 2); fp32 sources exist at (2, 2) only.
// chroma.hip:
int dcvc_internal_yuv_ingest(FSample s, float mx, int sub_x, int sub_y, const void *y, const void *uv, int h, int w,
                             FView out, hipStream_t st);
int dcvc_internal_yuv_ingest_rgb(FSample s, float mx, int sub_x, int sub_y, const void *y, const void *uv, int h,
                                 int w, FView out, float *rgb_planes, hipStream_t st);
int dcvc_internal_yuv_sse(FSample s, float mx, int sub_x, int sub_y, FView xh, const void *y, const void *uv, int h,
                          int w, double *workspace, double *out3, hipStream_t st);
int dcvc_internal_yuv_write(FSample s, float mx, int sub_x, int sub_y, bool from_rgb, FView xh, int h, int w,
                            void *out, hipStream_t st);
// frame.hip:
int dcvc_internal_rgb_sse(FSample s, float mx, FView xh, const void *src, int h, int w, double *workspace,
                          double *out3, hipStream_t st);
// crossfmt.hip: uint8 HWC or uint16 planar RGB, from an RGB or a YUV 4:4:4
// frame; the float64 MS-SSIM planes of a YUV420 (uv set) or an RGB source
int dcvc_internal_rgb_write(FSample s, float mx, bool from_yuv, FView xh, int h, int w, void *out, hipStream_t st);
int dcvc_internal_msssim_planes(FSample s, FView xh, const void *src, const void *uv, int h, int w, double *sp,
                                double *rp, hipStream_t st);

namespace {

__device__ __forceinline__ float u8f(uint8_t v) { return (float)v / 255.f; }

// a 9..16-bit sample with mx = float32((1 << depth) - 1): one IEEE division
__device__ __forceinline__ float u16f(uint16_t v, float mx) { return (float)v / mx; }

// a source sample as the reader's float; only a uint16 sample needs mx
__device__ __forceinline__ float smp(uint8_t v, float = 0.f) { return u8f(v); }
__device__ __forceinline__ float smp(uint16_t v, float mx) { return u16f(v, mx); }
__device__ __forceinline__ float smp(float v, float = 0.f) { return v; }

// scipy.ndimage.zoom(uv, (1, 2, 2), order=0) as ycbcr420_to_444(order=0)
// calls it (DCVC-DC/src/transforms/functional.py:61-72): output index i of an
// axis of length 2n samples input index round(i * (n - 1) / (2n - 1)).  The
// product i(n-1)/(2n-1) is never a half-integer (2i(n-1) is even, (2n-1)
// odd) and lies at least 1/(2(2n-1)) from one, so the double evaluation
// rounds exactly as scipy's does.
__device__ __forceinline__ int zoom_src(int i, int n) {
  if (n <= 1) return 0;
  const double z = (double)(n - 1) / (double)(2 * n - 1);
  return (int)floor((double)i * z + 0.5);
}

constexpr int SSE_BLOCK = 256;
constexpr int SSE_MAX_BLOCKS = 1024;

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Block sum of three doubles in a fixed order: wave shuffles, then the four
// wave results in index order.  Thread 0 writes part[3 * blockIdx.x + c].
__device__ inline void block_sum3(double a0, double a1, double a2, double *part) {
  __shared__ double red[SSE_BLOCK / 64][3];
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  a2 = wave_sum(a2);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[wv][0] = a0;
    red[wv][1] = a1;
    red[wv][2] = a2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int i = 0; i < SSE_BLOCK / 64; ++i) s += red[i][threadIdx.x];
    part[3 * blockIdx.x + threadIdx.x] = s;
  }
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ uint8_t q255(float v) {
  return (uint8_t)fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f);  // np.clip(np.rint(v * 255), 0, 255)
}

__device__ __forceinline__ uint16_t q16(float v, float mx) {
  return (uint16_t)fminf(fmaxf(rintf(v * mx), 0.f), mx);  // np.clip(np.rint(v * max_val), 0, max_val)
}

// a value as the writer's sample
__device__ __forceinline__ void qst(uint8_t *o, float v, float) { *o = q255(v); }
__device__ __forceinline__ void qst(uint16_t *o, float v, float mx) { *o = q16(v, mx); }

// Fixed-order final reduction of the per-block partials: out[c] = sum_b part[3b + c]
// (launched by the two distortion launchers; the other includers do not use it).
[[maybe_unused]] __global__ void __launch_bounds__(256) sse_final_kernel(const double *part, int nb, double *out) {
  __shared__ double red[4][3];
  double a[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] += part[3 * b + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = wave_sum(a[c]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < 3; ++c) red[wv][c] = a[c];
  __syncthreads();
  if (threadIdx.x < 3) out[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                                          red[3][threadIdx.x];
}

inline bool frame_ok(const dcvc_tensor &t) {
  return t.ptr && t.dtype == DCVC_F32 && t.C == 3 && t.H > 0 && t.W > 0 && t.coff >= 0 && t.coff + 3 <= t.cstride;
}

inline FView fv(const dcvc_tensor &t) { return FView{reinterpret_cast<float *>(t.ptr), t.H, t.W, t.cstride, t.coff}; }

// The same 3-channel fp32 frame view handed over as scalars (the entry points
// of the 9..16-bit sources): base pointer, H, W, channel stride and offset.
inline bool view_ok(const float *p, int H, int W, int cs, int co) {
  return p && H > 0 && W > 0 && co >= 0 && co + 3 <= cs;
}

inline FView fvs(const float *p, int H, int W, int cs, int co) { return FView{const_cast<float *>(p), H, W, cs, co}; }

inline bool even_frame(int h, int w) { return h >= 2 && w >= 2 && !(h & 1) && !(w & 1); }

// lo = 9: the uint16-only entry points; lo = 8: those that also take uint8
inline bool depth_ok(int depth, int lo) { return depth >= lo && depth <= 16; }

inline float max_val(int depth) { return (float)((1 << depth) - 1); }

// the grid of a kernel that runs one item per thread; 0: it would not fit
constexpr int ITEM_BLOCK = 256;

inline unsigned item_blocks(int64_t n) {
  const int64_t g = (n + ITEM_BLOCK - 1) / ITEM_BLOCK;
  return g > 0 && g <= 0x7fffffff ? (unsigned)g : 0;
}

inline unsigned sse_blocks(int64_t n) {
  const int64_t g = (n + SSE_BLOCK - 1) / SSE_BLOCK;
  return (unsigned)(g < SSE_MAX_BLOCKS ? (g > 0 ? g : 1) : SSE_MAX_BLOCKS);
}

}  // namespace
