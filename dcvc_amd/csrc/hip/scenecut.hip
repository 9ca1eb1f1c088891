// Scene statistics of two co-located sample planes (dcvc_scene_stats): what
// the encoder's scene-cut detector reads per frame (INTEGRATION.md "Scene-cut
// keyframes" is the normative definition).
//
//   sad   = sum_i |cur[i] - prev[i]|
//   hdiff = sum_b |hist_cur[b] - hist_prev[b]|, 64 bins, bin = sample >> (depth - 6)
//
// Both are integers, and integer adds are associative: whatever the order of
// the reduction the two words equal a host restatement bit for bit, so a
// threshold decision never differs between the GPU and the host.  No global
// atomics and no zero-initialised output: every block writes one partial row
// (its 64-bit SAD and, per bin, the signed difference of its two counts) and a
// one-block kernel sums the rows, so each call rewrites everything it reads.
//
// The planes may start at any sample: the body is read in 16-byte pieces when
// both pointers are equally far from a 16-byte boundary (head and tail by
// single samples), and by single samples throughout when they are not.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxBlocks = 1024;
constexpr int kBins = 64;
// samples of one call: a bin's count, and a block's signed count difference, fit 32 bits
constexpr int64_t kMaxSamples = 0x7fffffff;

template <typename T> struct Piece;
template <> struct Piece<uint8_t> {
  static constexpr int N = 16;
  typedef uint8_t type __attribute__((ext_vector_type(16)));
};
template <> struct Piece<uint16_t> {
  static constexpr int N = 8;
  typedef uint16_t type __attribute__((ext_vector_type(8)));
};

// Where the 16-byte pieces lie: samples [0, head) and [head + N * pieces, n)
// are read one by one, the pieces between them as vectors.
struct Split {
  int64_t head, pieces, edge;   // edge = head + tail, the single samples
};

template <typename T>
Split split_of(const void *cur, const void *prev, int64_t n) {
  constexpr int N = Piece<T>::N;
  const uintptr_t a = (uintptr_t)cur & 15, b = (uintptr_t)prev & 15;
  if (a != b || a % sizeof(T)) return Split{n, 0, n};
  int64_t head = (int64_t)((16 - a) & 15) / (int64_t)sizeof(T);
  if (head > n) head = n;
  const int64_t pieces = (n - head) / N;
  return Split{head, pieces, n - pieces * N};
}

// One sample pair: the SAD term, and one count in each of the wave's two
// histograms (samples above max_val, which no reader clamps, count in bin 63).
__device__ __forceinline__ uint32_t add_pair(uint32_t a, uint32_t b, int shift, uint32_t *hc, uint32_t *hp) {
  atomicAdd(hc + min(a >> shift, (uint32_t)(kBins - 1)), 1u);
  atomicAdd(hp + min(b >> shift, (uint32_t)(kBins - 1)), 1u);
  return a > b ? a - b : b - a;
}

// One histogram pair per wave in LDS (a block-wide pair would serialise every
// wave of the block on one counter when a plane is flat), merged at the end.
// ws_sad[block] = the block's SAD, ws_diff[block][b] = hist_cur[b] - hist_prev[b]
// over the block's samples.
template <typename T>
__global__ void __launch_bounds__(kBlock) scene_stats_kernel(const T *__restrict__ cur, const T *__restrict__ prev,
                                                             int64_t n, Split sp, int shift, uint64_t *ws_sad,
                                                             int32_t *ws_diff) {
  constexpr int N = Piece<T>::N;
  typedef typename Piece<T>::type V;
  __shared__ uint32_t hist[kWaves][2][kBins];
  __shared__ uint64_t wsum[kWaves];
  for (int i = threadIdx.x; i < kWaves * 2 * kBins; i += kBlock) (&hist[0][0][0])[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t *hc = hist[wave][0], *hp = hist[wave][1];
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  uint64_t sad = 0;   // 64 bits: one 16-bit plane reaches n * 65535
  const T *cb = cur + sp.head, *pb = prev + sp.head;
  for (int64_t i = first; i < sp.pieces; i += stride) {
    const V a = *reinterpret_cast<const V *>(cb + i * N);
    const V b = *reinterpret_cast<const V *>(pb + i * N);
    uint32_t s = 0;   // at most 8 * 65535
#pragma unroll
    for (int e = 0; e < N; ++e) s += add_pair((uint32_t)a[e], (uint32_t)b[e], shift, hc, hp);
    sad += s;
  }
  const int64_t body = sp.pieces * N;
  for (int64_t j = first; j < sp.edge; j += stride) {
    const int64_t i = j < sp.head ? j : j + body;
    sad += add_pair((uint32_t)cur[i], (uint32_t)prev[i], shift, hc, hp);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sad += __shfl_down((unsigned long long)sad, o, 64);
  if (lane == 0) wsum[wave] = sad;
  __syncthreads();
  if (threadIdx.x < kBins) {
    int32_t d = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) d += (int32_t)hist[w][0][threadIdx.x] - (int32_t)hist[w][1][threadIdx.x];
    ws_diff[(int64_t)blockIdx.x * kBins + threadIdx.x] = d;
  }
  if (threadIdx.x == 0) {
    uint64_t s = wsum[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += wsum[w];
    ws_sad[blockIdx.x] = s;
  }
}

// One block: out2[0] = sum of the rows' SADs, out2[1] = sum_b |sum of the rows' differences of bin b|
__global__ void __launch_bounds__(kBlock) scene_final_kernel(const uint64_t *ws_sad, const int32_t *ws_diff,
                                                             int nblocks, int64_t *out2) {
  __shared__ int64_t part[kWaves][kBins];
  __shared__ uint64_t wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t sad = 0;
  for (int r = threadIdx.x; r < nblocks; r += kBlock) sad += ws_sad[r];
  int64_t d = 0;   // wave w sums bin `lane` over rows w, w + kWaves, ...
  for (int r = wave; r < nblocks; r += kWaves) d += ws_diff[(int64_t)r * kBins + lane];
  part[wave][lane] = d;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sad += __shfl_down((unsigned long long)sad, o, 64);
  if (lane == 0) wsum[wave] = sad;
  __syncthreads();
  if (wave == 0) {
    d = part[0][lane];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) d += part[w][lane];
    uint64_t h = (uint64_t)(d < 0 ? -d : d);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_down((unsigned long long)h, o, 64);
    if (lane == 0) {
      uint64_t s = wsum[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) s += wsum[w];
      out2[0] = (int64_t)s;
      out2[1] = (int64_t)h;
    }
  }
}

template <typename T>
int launch(const void *cur, const void *prev, int64_t n, int depth, void *workspace, int64_t *out2, hipStream_t st) {
  const Split sp = split_of<T>(cur, prev, n);
  const int64_t work = sp.pieces > sp.edge ? sp.pieces : sp.edge;
  int64_t grid = (work + kBlock - 1) / kBlock;
  if (grid > kMaxBlocks) grid = kMaxBlocks;
  if (grid < 1) grid = 1;
  uint64_t *ws_sad = reinterpret_cast<uint64_t *>(workspace);
  int32_t *ws_diff = reinterpret_cast<int32_t *>(ws_sad + kMaxBlocks);
  hipLaunchKernelGGL((scene_stats_kernel<T>), dim3((unsigned)grid), dim3(kBlock), 0, st,
                     reinterpret_cast<const T *>(cur), reinterpret_cast<const T *>(prev), n, sp, depth - 6, ws_sad,
                     ws_diff);
  DCVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(scene_final_kernel, dim3(1), dim3(kBlock), 0, st, ws_sad, ws_diff, (int)grid, out2);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

}  // namespace

extern "C" int64_t dcvc_scene_stats_workspace(void) {
  return (int64_t)kMaxBlocks * (sizeof(uint64_t) + kBins * sizeof(int32_t));
}

extern "C" int dcvc_scene_stats(const void *cur, const void *prev, int64_t n, int depth, void *workspace,
                                int64_t *out2, void *stream) {
  if (!cur || !prev || !workspace || !out2 || n < 1 || n > kMaxSamples || depth < 8 || depth > 16)
    return DCVC_HIP_EINVAL;
  if (((uintptr_t)workspace | (uintptr_t)out2) & 7) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (depth == 8) return launch<uint8_t>(cur, prev, n, depth, workspace, out2, st);
  if (((uintptr_t)cur | (uintptr_t)prev) & 1) return DCVC_HIP_EINVAL;
  return launch<uint16_t>(cur, prev, n, depth, workspace, out2, st);
}
