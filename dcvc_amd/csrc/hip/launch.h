// Host-side helpers shared by the launchers (no device code): the CU count,
// the split-fp16 weight layout, and the view checks and parameter fill of the
// split-family conv entry points (tconv, nconv, wconv, xconv, dconv, sconv,
// sgemm).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/dcvc_hip.h"

// Compute units of the current device, queried once per process (the
// persistent kernels size their grids by it).  0 when the query fails (the
// next call asks again).
inline int dcvc_cu_count() {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    cus = prop.multiProcessorCount;
  }
  return cus;
}

// The DCVC_F16X3 weight layout of dcvc_conv_pack_weights (conv.hip
// pack_f16x3 writes it, the split kernels read it): one chunk per 32 input
// channels, each a hi block [rows][cout][32] then a lo block of the same
// shape.  A full chunk has one row per tap; a last chunk of <= 16 (<= 8)
// channels packs 2 (4) taps per row.
struct SplitWLayout {
  int nch;         // 32-channel input chunks
  int tpk_last;    // taps per row of the last chunk: 4, 2 or 1
  int rows_last;   // rows of the last chunk
  int nst;         // rows of all chunks, the K stages: (nch - 1) * kt + rows_last
  int64_t wchunk;  // halves of a full chunk (hi and lo)
  int64_t halves;  // halves of the whole tensor
  int64_t bytes;
  bool fits_i32;   // bytes < 2^31 - 64: a 32-bit buffer offset reaches every piece
};

inline SplitWLayout split_wlayout(int cin, int cout, int kh, int kw) {
  SplitWLayout l;
  const int kt = kh * kw;
  l.nch = (cin + 31) / 32;
  const int vcl = cin - 32 * (l.nch - 1);
  l.tpk_last = vcl <= 8 ? 4 : vcl <= 16 ? 2 : 1;
  l.rows_last = (kt + l.tpk_last - 1) / l.tpk_last;
  l.nst = (l.nch - 1) * kt + l.rows_last;
  l.wchunk = (int64_t)2 * kt * cout * 32;
  l.halves = (int64_t)(l.nch - 1) * l.wchunk + (int64_t)2 * l.rows_last * cout * 32;
  l.bytes = l.halves * 2;
  l.fits_i32 = l.bytes < ((int64_t)1 << 31) - 64;
  return l;
}

// An fp32 view read or written in 16-byte pieces, `elems` channels apart (4:
// every piece, 8: pairs of pieces): the base pointer and every pixel's window
// start are aligned.  (The dtype is the caller's check.)
inline bool f32_pieces_ok(const dcvc_tensor &t, int elems) {
  return (uintptr_t)t.ptr % 16 == 0 && t.cstride % elems == 0 && t.coff % elems == 0;
}
// the kernels compute a leaky ReLU as max(v, slope * v): exact for these slopes
inline bool lrelu_exact(float slope) { return slope >= 0.f && slope <= 1.f; }

// The members every split-family parameter struct has, from the call's
// arguments: input, weights, output and first residual views, epilogue
// constants.  The map sizes stay with the launcher (sgemm.hip counts pixels;
// the output size depends on the strides and paddings a family takes).  SP keeps void pointers where
// the others keep float pointers, hence the casts through the members' own
// types.  Absent residuals stay null with zero strides.
template <class P>
void fill_conv_views(P &p, const dcvc_conv_args *a) {
  p.x = reinterpret_cast<decltype(p.x)>(a->x.ptr);
  p.xcs = a->x.cstride;
  p.xco = a->x.coff;
  p.w = reinterpret_cast<decltype(p.w)>(a->w);
  p.bias = a->bias;
  p.scale = a->scale;
  p.y = reinterpret_cast<decltype(p.y)>(a->y.ptr);
  p.ycs = a->y.cstride;
  p.yco = a->y.coff;
  if (a->res.ptr) {
    p.res = reinterpret_cast<decltype(p.res)>(a->res.ptr);
    p.rcs = a->res.cstride;
    p.rco = a->res.coff;
  }
  p.in_slope = a->in_slope;
  p.act = a->act;
  p.slope = a->slope;
}
// ... and the second residual (every family but wconv takes one)
template <class P>
void fill_res2_view(P &p, const dcvc_conv_args *a) {
  if (a->res2.ptr) {
    p.res2 = reinterpret_cast<decltype(p.res2)>(a->res2.ptr);
    p.r2cs = a->res2.cstride;
    p.r2co = a->res2.coff;
  }
}
