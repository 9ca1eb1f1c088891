// Order-independent 128-bit digest of an NHWC view (dcvc_digest): what the
// stand-alone encoder stores per frame and the stand-alone decoder verifies
// (INTEGRATION.md "DPB digest" is the normative definition).
//
// Every element contributes h = mix64(((u64)bits << 32 | index) + seed * PHI);
// the digest is (sum of h mod 2^64, xor of h).  Integer add and xor are
// associative and commutative, so any reduction order gives the same words:
// the kernels are deterministic by construction and use no atomics.
#include "common.h"
#include "launch.h"

namespace {

constexpr int kBlock = 256;
constexpr int kBlocksPerCu = 4;
constexpr int kMaxBlocks = 4096;
constexpr uint64_t kPhi = 0x9E3779B97F4A7C15ull;

struct View {
  const void *p;
  int H, W, C, cs, co;
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// bit pattern of an element, -0.0 folded onto +0.0
__device__ __forceinline__ uint32_t canon(uint32_t b) { return b == 0x80000000u ? 0u : b; }
__device__ __forceinline__ uint32_t canon(uint16_t b) { return b == 0x8000u ? 0u : (uint32_t)b; }

struct Acc {
  uint64_t s = 0, x = 0;
  __device__ __forceinline__ void add(uint32_t bits, uint32_t n, uint64_t off) {
    const uint64_t h = mix64((((uint64_t)bits << 32) | n) + off);
    s += h;
    x ^= h;
  }
};

// wave shuffles, then the block's waves through LDS; the result is valid in thread 0
__device__ __forceinline__ void block_reduce(Acc &a) {
  __shared__ uint64_t part[2][kBlock / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.s += __shfl_down((unsigned long long)a.s, o, 64);
    a.x ^= __shfl_down((unsigned long long)a.x, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[0][wave] = a.s;
    part[1][wave] = a.x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.s = part[0][0];
    a.x = part[1][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) {
      a.s += part[0][w];
      a.x ^= part[1][w];
    }
  }
}

template <typename T> struct Vec;
template <> struct Vec<float> {
  static constexpr int N = 4;
  typedef uint32_t bits;
  typedef uint32_t type __attribute__((ext_vector_type(4)));
};
template <> struct Vec<uint16_t> {
  static constexpr int N = 8;
  typedef uint16_t bits;
  typedef uint16_t type __attribute__((ext_vector_type(8)));
};

template <typename T>
__device__ __forceinline__ void add_vec(Acc &a, const View &v, uint32_t item, uint32_t per_pix, uint64_t off) {
  constexpr int N = Vec<T>::N;
  const uint32_t pix = item / per_pix, q = item - pix * per_pix;
  const typename Vec<T>::type d = *reinterpret_cast<const typename Vec<T>::type *>(
      reinterpret_cast<const T *>(v.p) + ((int64_t)pix * v.cs + v.co + q * N));
  const uint32_t n0 = pix * (uint32_t)v.C + q * N;
#pragma unroll
  for (int e = 0; e < N; ++e) a.add(canon((typename Vec<T>::bits)d[e]), n0 + e, off);
}

// 16 bytes per lane (4 fp32 / 8 bf16 channels); two loads in flight per pass
template <typename T>
__global__ void __launch_bounds__(kBlock) digest_vec_kernel(View v, uint64_t off, uint64_t *ws) {
  const uint32_t per_pix = (uint32_t)v.C / Vec<T>::N;
  const uint64_t items = (uint64_t)v.H * v.W * per_pix;
  const uint64_t T2 = (uint64_t)gridDim.x * kBlock;
  Acc a, b;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < items; i += 2 * T2) {
    add_vec<T>(a, v, (uint32_t)i, per_pix, off);
    if (i + T2 < items) add_vec<T>(b, v, (uint32_t)(i + T2), per_pix, off);
  }
  a.s += b.s;
  a.x ^= b.x;
  block_reduce(a);
  if (threadIdx.x == 0) {
    ws[2 * blockIdx.x] = a.s;
    ws[2 * blockIdx.x + 1] = a.x;
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) digest_scalar_kernel(View v, uint64_t off, uint64_t *ws) {
  const uint64_t n_all = (uint64_t)v.H * v.W * v.C;
  const uint64_t T1 = (uint64_t)gridDim.x * kBlock;
  Acc a;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_all; i += T1) {
    const uint32_t n = (uint32_t)i;
    const uint32_t pix = n / (uint32_t)v.C, c = n - pix * (uint32_t)v.C;
    a.add(canon(reinterpret_cast<const typename Vec<T>::bits *>(v.p)[(int64_t)pix * v.cs + v.co + c]), n, off);
  }
  block_reduce(a);
  if (threadIdx.x == 0) {
    ws[2 * blockIdx.x] = a.s;
    ws[2 * blockIdx.x + 1] = a.x;
  }
}

// one block: sums the partials and folds them into out
__global__ void __launch_bounds__(kBlock) digest_fold_kernel(const uint64_t *ws, int nblocks, uint64_t *out) {
  Acc a;
  for (int i = threadIdx.x; i < nblocks; i += kBlock) {
    a.s += ws[2 * i];
    a.x ^= ws[2 * i + 1];
  }
  block_reduce(a);
  if (threadIdx.x == 0) {
    out[0] += a.s;
    out[1] ^= a.x;
  }
}

}  // namespace

extern "C" int64_t dcvc_digest_workspace(void) { return (int64_t)2 * kMaxBlocks * sizeof(uint64_t); }

extern "C" int dcvc_digest_threads(void) {
  const int cus = dcvc_cu_count();
  if (cus <= 0) return DCVC_HIP_ELAUNCH;
  int64_t blocks = (int64_t)cus * kBlocksPerCu;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  if (blocks < 1) blocks = 1;
  return (int)(blocks * kBlock);
}

extern "C" int dcvc_digest(dcvc_tensor t, uint64_t seed, uint64_t *workspace, uint64_t *out, void *stream) {
  if (!t.ptr || !workspace || !out || t.H <= 0 || t.W <= 0 || t.C <= 0 || t.coff < 0 || t.coff + t.C > t.cstride)
    return DCVC_HIP_EINVAL;
  if (t.dtype != DCVC_F32 && t.dtype != DCVC_BF16) return DCVC_HIP_EUNSUPPORTED;
  const uint64_t n_all = (uint64_t)t.H * t.W * t.C;
  if (n_all >= (1ull << 32)) return DCVC_HIP_EINVAL;
  const int threads = dcvc_digest_threads();
  if (threads < 0) return threads;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const View v{t.ptr, t.H, t.W, t.C, t.cstride, t.coff};
  const uint64_t off = seed * kPhi;
  const int vn = t.dtype == DCVC_F32 ? 4 : 8;
  const bool vec = t.C % vn == 0 && t.coff % vn == 0 && t.cstride % vn == 0 && ((uintptr_t)t.ptr & 15) == 0;
  // the grid comes from the device (kBlocksPerCu blocks per CU), shrunk only
  // when the tensor has fewer work items than that many threads
  const uint64_t work = vec ? n_all / vn : n_all;
  int64_t grid = threads / kBlock;
  const int64_t need = (int64_t)((work + kBlock - 1) / kBlock);
  if (grid > need) grid = need;
  if (vec) {
    if (t.dtype == DCVC_F32)
      hipLaunchKernelGGL((digest_vec_kernel<float>), dim3((unsigned)grid), dim3(kBlock), 0, st, v, off, workspace);
    else
      hipLaunchKernelGGL((digest_vec_kernel<uint16_t>), dim3((unsigned)grid), dim3(kBlock), 0, st, v, off, workspace);
  } else {
    if (t.dtype == DCVC_F32)
      hipLaunchKernelGGL((digest_scalar_kernel<float>), dim3((unsigned)grid), dim3(kBlock), 0, st, v, off, workspace);
    else
      hipLaunchKernelGGL((digest_scalar_kernel<uint16_t>), dim3((unsigned)grid), dim3(kBlock), 0, st, v, off,
                         workspace);
  }
  DCVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(digest_fold_kernel, dim3(1), dim3(kBlock), 0, st, workspace, (int)grid, out);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}
