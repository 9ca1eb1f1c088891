// Colour and chroma-resampling arithmetic shared by the frame kernels that
// convert between YCbCr and RGB or resample chroma (chroma.hip, crossfmt.hip):
// BT.709 in numpy's operation order, the 2x2 block mean, scipy's order-1 zoom
// taps, and the launch helpers.
//
// Every value is bit-equal to the reference's numpy / scipy result
// (DCVC-DC/src/transforms/functional.py:16-58), so the arithmetic is written
// operation by operation in numpy's order with contraction into FMAs switched
// off (numpy rounds after every ufunc).
#pragma once
#include "frame.h"

namespace {

// ITU-R BT.709 (functional.py:10-13).  numpy multiplies float32 arrays by
// these Python doubles as float32 scalars: each constant is the double
// expression rounded once to fp32.
constexpr float KR = (float)0.2126, KG = (float)0.7152, KB = (float)0.0722;
constexpr float C_CR = (float)(2.0 - 2.0 * 0.2126), C_CB = (float)(2.0 - 2.0 * 0.0722);
constexpr float D_CB = (float)(1.0 - 0.0722), D_CR = (float)(1.0 - 0.2126);

// r = y + (2 - 2 Kr) (cr - 0.5); b = y + (2 - 2 Kb) (cb - 0.5);
// g = (y - Kr r - Kb b) / Kg; clip (functional.py:52-57)
__device__ __forceinline__ void ycc_to_rgb(float y, float cb, float cr, float &r, float &g, float &b) {
#pragma clang fp contract(off)
  const float tr = cr - 0.5f, tb = cb - 0.5f;
  const float pr = C_CR * tr, pb = C_CB * tb;
  const float rr = y + pr, bb = y + pb;
  const float m1 = KR * rr, m2 = KB * bb;
  const float d1 = y - m1;
  const float d2 = d1 - m2;
  r = clamp01(rr);
  g = clamp01(d2 / KG);
  b = clamp01(bb);
}

// y = Kr r + Kg g + Kb b; cb = 0.5 (b - y) / (1 - Kb) + 0.5;
// cr = 0.5 (r - y) / (1 - Kr) + 0.5, unclipped (functional.py:25-29)
__device__ __forceinline__ void rgb_to_ycc(float r, float g, float b, float &y, float &cb, float &cr) {
#pragma clang fp contract(off)
  const float m0 = KR * r, m1 = KG * g, m2 = KB * b;
  const float s0 = m0 + m1;
  y = s0 + m2;
  const float db = b - y, dr = r - y;
  const float hb = 0.5f * db, hr = 0.5f * dr;
  const float qb = hb / D_CB, qr = hr / D_CR;
  cb = qb + 0.5f;
  cr = qr + 0.5f;
}

// float32 mean of a 2x2 block as numpy's mean(axis=(-1, -3)) forms it:
// (x00 + x01) + (x10 + x11), except for a
// chroma plane one column wide (seq), whose four values numpy reduces as one
// contiguous run, ((x00 + x01) + x10) + x11
__device__ __forceinline__ float mean4(float x00, float x01, float x10, float x11, bool seq) {
  const float s = seq ? ((x00 + x01) + x10) + x11 : (x00 + x01) + (x10 + x11);
  return s / 4.f;
}

// scipy.ndimage.zoom(order=1) along one axis of length n doubled to 2n: output
// index i samples at cc = i * z, z = (n - 1) / (2n - 1) formed first in double
// (on the host: zoom_ratio); taps floor(cc) and floor(cc) + 1.  scipy weighs
// a tap k by 1 - |k - cc|: w0 = 1 - f and w1 = 1 - w0, which is not always f
// in the last double bit, and that bit decides fp32 ties such as (2a + b) / 3.
// n = 1: z = 0, both outputs take tap 0.
struct Tap {
  int i0, i1;
  double w0, w1;
};

__device__ __forceinline__ Tap zoom1_tap(int i, int n, double z) {
#pragma clang fp contract(off)
  const double cc = (double)i * z;
  const double fl = floor(cc);
  const double f = cc - fl;
  const int i0 = max((int)fl, 0);
  Tap t;
  t.i0 = min(i0, n - 1);
  t.i1 = min(i0 + 1, n - 1);
  t.w0 = 1.0 - f;
  t.w1 = 1.0 - t.w0;
  return t;
}

// the four products (v * w_row) * w_col summed in double in scipy's order
// (r0, c0), (r0, c1), (r1, c0), (r1, c1), rounded once to fp32
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, const Tap &tr, const Tap &tc) {
#pragma clang fp contract(off)
  const double p00 = ((double)v00 * tr.w0) * tc.w0;
  const double p01 = ((double)v01 * tr.w0) * tc.w1;
  const double p10 = ((double)v10 * tr.w1) * tc.w0;
  const double p11 = ((double)v11 * tr.w1) * tc.w1;
  double t = p00;
  t = t + p01;
  t = t + p10;
  t = t + p11;
  return (float)t;
}

// clipped mean of channel c of the 2x2 block (by, bx) of a 4:4:4 frame, the
// values as given (ycbcr444_to_420's chroma sample)
__device__ __forceinline__ float block_mean(const FView &xh, int by, int bx, int c, bool seq) {
  const float *p0 = xh.p + ((int64_t)(2 * by) * xh.W + 2 * bx) * xh.cs + xh.co + c;
  const float *p1 = p0 + (int64_t)xh.W * xh.cs;
  return clamp01(mean4(p0[0], p0[xh.cs], p1[0], p1[xh.cs], seq));
}

// (n - 1) / (2n - 1), the ratio scipy's zoom forms before it multiplies
inline double zoom_ratio(int n) { return n > 1 ? (double)(n - 1) / (double)(2 * n - 1) : 0.0; }

constexpr int CF_BLOCK = 256;
constexpr int64_t CF_MAX_BLOCKS = 65536;

inline unsigned cf_blocks(int64_t n) {
  const int64_t g = (n + CF_BLOCK - 1) / CF_BLOCK;
  return (unsigned)(g < CF_MAX_BLOCKS ? (g > 0 ? g : 1) : CF_MAX_BLOCKS);
}

}  // namespace
