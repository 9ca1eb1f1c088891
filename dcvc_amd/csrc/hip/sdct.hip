// The tail of a feature-rate DepthConv in split-fp16 arithmetic
// (DCVC-DC/src/models/layers.py:135-163), for the blocks sdc.hip cannot take
// (128 channels wide, or cin != cout at 64 / 128 channels: the decoder's
// reconstruction UNets and the mv branch):
//   out = conv2(dw3x3(t) + bdw) + b2 + idn
//   idn = adaptor(x) + ba   (ADAPT)   |   idn = x
// t = lrelu(conv1(x) + b1) comes from the previous launch.  Unfused this is a
// depthwise launch, the adaptor 1x1 and the conv2 1x1 with the residual: the
// depthwise output and the identity map each make an fp32 round trip through
// memory to be read once.  sldc_kernel (slffn.hip) fuses the adaptor-free
// case for the latent maps, one 32-pixel run per one-shot workgroup; on a map
// 16 times larger it re-stages its tables and re-streams the conv2 fragments
// 4080 times and issues every depthwise tap as its own global load.
//
// Here one persistent workgroup per CU (8 waves) walks 8 x 16 pixel tiles:
//   * the conv2 (and adaptor) weights live in registers for the launch: wave
//     w owns output rows [16 rb, 16 rb + 16) of every K chunk (packed MFMA A
//     fragments, dcvc_frag_pack_weights) for NPB of the tile's 8 pixel rows;
//   * a tile is a chain of stages, one per 32-channel K chunk: first the
//     adaptor's chunks of x (ADAPT), then conv2's chunks of t.  A stage's
//     fp32 input (the 10 x 18 halo of t, or the 8 x 16 tile of x) is loaded
//     into registers two stages ahead (across tile boundaries too), parked
//     in one of two LDS halo buffers one stage ahead, turned into a split
//     (hi, lo) fp16 image in one of two LDS image buffers (the depthwise in
//     fp32 VALU: a thread owns 4 channels of two vertically adjacent pixels,
//     so a halo row is read from memory once per tile and from LDS 1.5 times
//     per output row), and multiplied: one barrier per stage;
//   * ADAPT: the adaptor's result stays in registers as idn; otherwise the
//     epilogue's x is loaded before the last chunk's MFMAs.
// Arithmetic: the depthwise is dw8_kernel's (misc.hip) fp32 fma chain from 0
// over the taps (dy, dx) ascending, then + bdw.  dw8_kernel skips a tap that
// falls outside the map; here such a tap reads a zero: fma(w, 0, acc) = acc
// bit for bit for finite w (acc is never -0: the chain starts at +0 and an
// exact cancellation rounds to +0).  Both GEMMs are dconv.hip's / sgemm.hip's
// products (xh wh into the main accumulator; xl wh, then xh wl into the
// correction accumulator) over K chunks of 32 ascending, and the epilogues
// theirs: idn = (am + 2^-11 ac) + ba, out = idn + ((cm + 2^-11 cc) + b2).  So
// the output is bit-identical to the unfused launches.
#include "common.h"
#include "launch.h"
#include "options.h"
#include "split.h"

namespace {

constexpr int kNW = 8, kNT = kNW * 64;
constexpr int TH = 8, TW = 16;               // pixel tile
constexpr int HWD = TW + 2;                  // halo row pitch in pixels
constexpr int HP = (TH + 2) * HWD;           // 180 halo pixels
constexpr int TP = TH * TW;                  // 128 tile pixels
// a buffer offset past any num_records: the load returns zeros, the store is dropped
constexpr int kOob = 0x7fffffe0;

struct TailP {
  const float *t;
  int H, W, tcs, tco, tbytes;
  const float *x;
  int xcs, xco, xbytes;
  float *y;
  int ycs, yco, ybytes;
  const float *w9, *bdw, *b2, *ba;   // depthwise taps [9][C], biases
  const uint16_t *w2, *wa;           // conv2 [COUT][C], adaptor [COUT][CX] as packed fragments
  int txt, ntile;                    // tiles per tile row, tiles
  int *ovf;                          // fp16 range guard (split.h SplitRange)
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, bytes, 0x00020000);
}

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

template <int C, int CX, int COUT, bool ADAPT>
constexpr size_t tail_lds() {
  return (size_t)2 * HP * 32 * 4 + (size_t)4 * TP * 32 * 2 + (size_t)(10 * C + 2 * COUT) * 4;
}

template <int C, int CX, int COUT, bool ADAPT>
__global__ void __launch_bounds__(kNT) sdct_kernel(TailP p) {
  SplitRange rg(p.ovf);
  constexpr int KA = ADAPT ? CX / 32 : 0, KC = C / 32, NS = KA + KC;   // stages of a tile
  static_assert(NS % 2 == 0 && NS >= 2, "a tile starts in LDS buffer 0");
  static_assert(ADAPT || (CX == C && COUT == C), "without an adaptor x is the identity");
  constexpr int NRB = COUT / 16;      // 16-row blocks of the output channels
  static_assert(kNW % NRB == 0, "a wave owns one row block");
  constexpr int NPB = TH / (kNW / NRB);   // tile rows (16-pixel blocks) per wave
  extern __shared__ __align__(16) unsigned char smem[];
  float *Hb = reinterpret_cast<float *>(smem);                    // [2][HP][32] fp32 stage input
  uint16_t *Db = reinterpret_cast<uint16_t *>(Hb + 2 * HP * 32);  // [2][hi, lo][TP][32] split image
  float *Lw9 = reinterpret_cast<float *>(Db + 4 * TP * 32);       // [9][C]
  float *Lbd = Lw9 + 9 * C;                                       // [C]
  float *Lb2 = Lbd + C, *Lba = Lb2 + COUT;                        // [COUT] each

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int rb = wave % NRB, pb0 = (wave / NRB) * NPB;
  const int G = gridDim.x;
  const __amdgpu_buffer_rsrc_t tr = rsrc(p.t + p.tco, p.tbytes);
  const __amdgpu_buffer_rsrc_t xr = rsrc(p.x + p.xco, p.xbytes);
  const __amdgpu_buffer_rsrc_t yr = rsrc(p.y + p.yco, p.ybytes);

  // the wave's weight fragments: rows [16 rb, 16 rb + 16) of every K chunk
  f16x8 w2h[KC], w2l[KC], wah[KA ? KA : 1], wal[KA ? KA : 1];
  {
    const __amdgpu_buffer_rsrc_t wr = rsrc(p.w2, COUT * C * 4);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const int o = ((rb * KC + kc) * 1024 + lane * 8) * 2;
      w2h[kc] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wr, o, 0, 0));
      w2l[kc] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wr, o + 1024, 0, 0));
    }
    if constexpr (ADAPT) {
      const __amdgpu_buffer_rsrc_t ar = rsrc(p.wa, COUT * CX * 4);
#pragma unroll
      for (int kc = 0; kc < KA; ++kc) {
        const int o = ((rb * KA + kc) * 1024 + lane * 8) * 2;
        wah[kc] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(ar, o, 0, 0));
        wal[kc] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(ar, o + 1024, 0, 0));
      }
    }
  }
  // the lane's output channels: 16 rb + 4 g .. + 3
  const int n = rb * 16 + 4 * g;
  for (int i = tid; i < 9 * C; i += kNT) Lw9[i] = p.w9[i];
  for (int i = tid; i < C; i += kNT) Lbd[i] = p.bdw[i];
  for (int i = tid; i < COUT; i += kNT) {
    Lb2[i] = p.b2[i];
    Lba[i] = ADAPT ? p.ba[i] : 0.f;
  }

  // stage s of the tile at (y0, x0): its fp32 input into pre, 16-byte piece u
  // = tid + 512 i.  Adaptor stage: piece (pixel u >> 3, channels 4 (u & 7))
  // of the tile; conv2 stage: the same of the halo.  Outside the map: zeros.
  f32x4 pre[3];
  auto issue = [&](int s, int y0, int x0) __attribute__((always_inline)) {
    if (s < KA) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int u = tid + i * kNT, px = u >> 3, q = u & 7;
        const int yy = y0 + (px >> 4), xx = x0 + (px & 15);
        const bool ok = yy < p.H && xx < p.W;
        const int o = ok ? ((yy * p.W + xx) * p.xcs + s * 32 + q * 4) * 4 : kOob;
        pre[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int u = tid + i * kNT, hp = u >> 3, q = u & 7;
        const int hy = hp / HWD, hx = hp - hy * HWD;
        const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
        const bool ok = u < HP * 8 && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
        const int o = ok ? ((yy * p.W + xx) * p.tcs + (s - KA) * 32 + q * 4) * 4 : kOob;
        pre[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(tr, o, 0, 0));
      }
    }
  };
  // pre (stage s) into halo buffer s & 1, piece u at 4 u floats
  auto stash = [&](int s) __attribute__((always_inline)) {
    float *Hs = Hb + (s & 1) * HP * 32;
#pragma unroll
    for (int i = 0; i < (s < KA ? 2 : 3); ++i) {
      const int u = tid + i * kNT;
      if (i < 2 || u < HP * 8) *reinterpret_cast<f32x4 *>(Hs + u * 4) = pre[i];
    }
  };
  // 4 channels 4 q .. + 3 of the chunk, pixel px of the tile, split into image buffer s & 1
  auto put4 = [&](int s, int px, int q, const float *v) __attribute__((always_inline)) {
    uint16_t *Dh = Db + (s & 1) * 2 * TP * 32, *Dl = Dh + TP * 32;
    rg.add4(v);
    const auto h0 = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]);
    const auto h1 = __builtin_amdgcn_cvt_pkrtz(v[2], v[3]);
    const uint32_t l0 = pk(split_lo(v[0], (float)h0[0]), split_lo(v[1], (float)h0[1]));
    const uint32_t l1 = pk(split_lo(v[2], (float)h1[0]), split_lo(v[3], (float)h1[1]));
    const int off = swz(px, q >> 1) + (q & 1) * 4;
    *reinterpret_cast<u32x2_t *>(Dh + off) = u32x2_t{__builtin_bit_cast(uint32_t, h0), __builtin_bit_cast(uint32_t, h1)};
    *reinterpret_cast<u32x2_t *>(Dl + off) = u32x2_t{l0, l1};
  };
  // stage s: halo buffer -> split image (adaptor stage: x as it is; conv2
  // stage: the depthwise conv of channels 4 q .. + 3 of the chunk at column
  // cx, rows 2 rp and 2 rp + 1 of the tile)
  auto image = [&](int s, int y0, int x0) __attribute__((always_inline)) {
    const float *Hs = Hb + (s & 1) * HP * 32;
    if (s < KA) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int u = tid + i * kNT;
        const f32x4 a = *reinterpret_cast<const f32x4 *>(Hs + u * 4);
        const float v[4] = {a[0], a[1], a[2], a[3]};
        put4(s, u >> 3, u & 7, v);
      }
    } else {
      const int q = tid & 7, cx = (tid >> 3) & 15, rp = tid >> 7;
      const int c0 = (s - KA) * 32 + q * 4;
      // halo row by halo row (tap row hr of the upper pixel, hr - 1 of the
      // lower one), fenced: read all at once the 12 pixels and 9 taps take
      // 84 registers beside the accumulators and the weight fragments
      f32x4 wv[2][3];
      float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int hr = 0; hr < 4; ++hr) {
        if (hr < 3) {
#pragma unroll
          for (int dx = 0; dx < 3; ++dx)
            wv[hr & 1][dx] = *reinterpret_cast<const f32x4 *>(Lw9 + (hr * 3 + dx) * C + c0);
        }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const f32x4 a = *reinterpret_cast<const f32x4 *>(Hs + ((2 * rp + hr) * HWD + cx + dx) * 32 + q * 4);
          if (hr < 3) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a0[e] = __builtin_fmaf(wv[hr & 1][dx][e], a[e], a0[e]);
          }
          if (hr > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a1[e] = __builtin_fmaf(wv[(hr - 1) & 1][dx][e], a[e], a1[e]);
          }
        }
        sched_fence();
      }
      const f32x4 bd = *reinterpret_cast<const f32x4 *>(Lbd + c0);
      const bool okx = x0 + cx < p.W;
      const bool ok0 = okx && y0 + 2 * rp < p.H, ok1 = okx && y0 + 2 * rp + 1 < p.H;
      float v0[4], v1[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v0[e] = ok0 ? a0[e] + bd[e] : 0.f;
        v1[e] = ok1 ? a1[e] + bd[e] : 0.f;
      }
      put4(s, (2 * rp) * TW + cx, q, v0);
      put4(s, (2 * rp + 1) * TW + cx, q, v1);
    }
  };

  f32x4 am[NPB], ac[NPB], idn[NPB];
#pragma unroll
  for (int i = 0; i < NPB; ++i) {
    am[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    ac[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    idn[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  int tile = blockIdx.x;   // (the grid is no larger than the tile count)
  int ty = tile / p.txt;
  int y0 = ty * TH, x0 = (tile - ty * p.txt) * TW;
  issue(0, y0, x0);
  stash(0);
  issue(1, y0, x0);
  __syncthreads();

  for (; tile < p.ntile; tile += G) {
    const int nxt = tile + G;
    const bool more = nxt < p.ntile;
    const int nty = nxt / p.txt;
    const int ny0 = nty * TH, nx0 = (nxt - nty * p.txt) * TW;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      // halo buffer s & 1 holds stage s, pre stage s + 1 (in flight)
      image(s, y0, x0);
      if (s + 1 < NS || more) stash((s + 1) % NS);
      // (not __syncthreads(): its vmcnt(0) would wait for the loads in flight
      // and for the previous tile's stores; only the LDS traffic is ordered)
      wait_lgkm();
      raw_barrier();
      if (s + 2 < NS)
        issue(s + 2, y0, x0);
      else if (more)
        issue(s + 2 - NS, ny0, nx0);
      if (!ADAPT && s == NS - 1) {
        // the identity, for the epilogue
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
          const int yy = y0 + pb0 + i, xx = x0 + col;
          const bool ok = yy < p.H && xx < p.W;
          idn[i] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, ok ? ((yy * p.W + xx) * p.xcs + n) * 4 : kOob, 0, 0));
        }
      }
      {
        const uint16_t *Dh = Db + (s & 1) * 2 * TP * 32, *Dl = Dh + TP * 32;
        const f16x8 ah = s < KA ? wah[s < KA ? s : 0] : w2h[s < KA ? 0 : s - KA];
        const f16x8 al = s < KA ? wal[s < KA ? s : 0] : w2l[s < KA ? 0 : s - KA];
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
          const int o = swz((pb0 + i) * 16 + col, g);
          const f16x8 bh = *reinterpret_cast<const f16x8 *>(Dh + o);
          const f16x8 bl = *reinterpret_cast<const f16x8 *>(Dl + o);
          am[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, am[i], 0, 0, 0);
          ac[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, ac[i], 0, 0, 0);
          ac[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, ac[i], 0, 0, 0);
          // (image operands of at most 4 pixel blocks in registers at once)
          if ((i & 3) == 3) sched_fence();
        }
      }
      if (ADAPT && s == KA - 1) {
        // idn = adaptor(x) + ba
        const f32x4 bav = *reinterpret_cast<const f32x4 *>(Lba + n);
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
#pragma unroll
          for (int e = 0; e < 4; ++e) idn[i][e] = (am[i][e] + ac[i][e] * kLoInv) + bav[e];
          am[i] = f32x4{0.f, 0.f, 0.f, 0.f};
          ac[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      if (s == NS - 1) {
        // out = idn + ((acc) + b2): lane (col, g) of fragment i holds channels
        // n .. n + 3 of pixel (y0 + pb0 + i, x0 + col)
        const f32x4 b2v = *reinterpret_cast<const f32x4 *>(Lb2 + n);
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
          const int yy = y0 + pb0 + i, xx = x0 + col;
          const bool ok = yy < p.H && xx < p.W;
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = idn[i][e] + ((am[i][e] + ac[i][e] * kLoInv) + b2v[e]);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), yr,
                                                 ok ? ((yy * p.W + xx) * p.ycs + n) * 4 : kOob, 0, 0);
          am[i] = f32x4{0.f, 0.f, 0.f, 0.f};
          ac[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    y0 = ny0;
    x0 = nx0;
  }
}

DCVC_OPTION("dctail", g_enable, 1);   // 0: the feature-rate DepthConv tails to their earlier routes (sldc 128 / unfused)

template <int C, int CX, int COUT, bool ADAPT>
int run_tail(TailP p, hipStream_t st) {
  constexpr size_t lds = tail_lds<C, CX, COUT, ADAPT>();
  static_assert(lds <= 160 * 1024, "LDS of a CU");
  const int cus = dcvc_cu_count();
  if (cus <= 0) return DCVC_HIP_ELAUNCH;
  const int G = p.ntile < cus ? p.ntile : cus;
  auto kern = sdct_kernel<C, CX, COUT, ADAPT>;
  dcvc_note_kernel("sdct_kernel<%d, %d, %d, %s>@%lld", C, CX, COUT, bname(ADAPT), (long long)G * kNT);
  dcvc_ensure_lds(reinterpret_cast<const void *>(kern), 160 * 1024);
  hipLaunchKernelGGL(kern, dim3((unsigned)G), dim3(kNT), lds, st, p);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

}  // namespace

// dcvc_dw_conv2_split's feature-rate route (slffn.hip has the entry point and
// the argument checks that do not depend on the kernel): a->cx, a->cout set.
extern "C" int dcvc_internal_dctail(const dcvc_dwc_args *a, void *stream) {
  if (!g_enable) return DCVC_HIP_EUNSUPPORTED;
  const int c = a->c, cx = a->cx, cout = a->cout;
  const bool adapt = a->wa != nullptr;
  const bool inst = (c == 128 && cx == 128 && cout == 64 && adapt) || (c == 64 && cx == 64 && cout == 128 && adapt) ||
                    (c == 128 && cx == 128 && cout == 128 && !adapt);
  if (!inst) return DCVC_HIP_EUNSUPPORTED;
  if (!f32_pieces_ok(a->t, 4) || !f32_pieces_ok(a->r, 4) || !f32_pieces_ok(a->y, 4)) return DCVC_HIP_EUNSUPPORTED;
  auto al16 = [](const void *q) { return (uintptr_t)q % 16 == 0; };
  if (!al16(a->w9) || !al16(a->bdw) || !al16(a->b2) || !al16(a->w2) || (adapt && (!al16(a->wa) || !al16(a->ba))))
    return DCVC_HIP_EUNSUPPORTED;
  const int64_t npix = (int64_t)a->t.H * a->t.W;
  if (npix <= 0) return DCVC_HIP_OK;
  auto bytes = [&](const dcvc_tensor &v) { return (npix * v.cstride - v.coff) * 4; };
  if (bytes(a->t) > 0x7fff0000 || bytes(a->r) > 0x7fff0000 || bytes(a->y) > 0x7fff0000) return DCVC_HIP_EUNSUPPORTED;
  TailP p{};
  p.ovf = dcvc_internal_split_flag();
  p.t = reinterpret_cast<const float *>(a->t.ptr);
  p.H = a->t.H;
  p.W = a->t.W;
  p.tcs = a->t.cstride;
  p.tco = a->t.coff;
  p.tbytes = (int)bytes(a->t);
  p.x = reinterpret_cast<const float *>(a->r.ptr);
  p.xcs = a->r.cstride;
  p.xco = a->r.coff;
  p.xbytes = (int)bytes(a->r);
  p.y = reinterpret_cast<float *>(a->y.ptr);
  p.ycs = a->y.cstride;
  p.yco = a->y.coff;
  p.ybytes = (int)bytes(a->y);
  p.w9 = a->w9;
  p.bdw = a->bdw;
  p.b2 = a->b2;
  p.ba = a->ba;
  p.w2 = reinterpret_cast<const uint16_t *>(a->w2);
  p.wa = reinterpret_cast<const uint16_t *>(a->wa);
  p.txt = (a->t.W + TW - 1) / TW;
  p.ntile = p.txt * ((a->t.H + TH - 1) / TH);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (c == 128 && cout == 64) return run_tail<128, 128, 64, true>(p, st);
  if (c == 64) return run_tail<64, 64, 128, true>(p, st);
  return run_tail<128, 128, 128, false>(p, st);
}
