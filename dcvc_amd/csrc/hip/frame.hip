// Harness-side frame entry points of 8-bit sources: YUV420 source frames into
// the codec's NHWC input, the per-frame distortion of run_test (DCVC-DC/
// test_video.py:108-195) with the in-place clamp of the reconstruction, and
// the decoded frame as uint8 samples.  The RGB distortion kernel lives here;
// every YUV operation is the (2, 2) instantiation of chroma.hip's templates
// and the RGB writer is crossfmt.hip's, reached through frame.h's launchers.
#include "frame.h"

namespace {

// RGB: recon_frame.clamp_(0, 1) over the padded frame (test_video.py:169),
// then per channel sum((x_hat - x)^2) over the crop against a planar source,
// the difference and its square in fp32 as PSNR() forms them (:65-68), summed
// in fp64.  The block size, sse_blocks and the order of a thread's sums fix
// the fp64 result.
template <typename S>
__global__ void __launch_bounds__(SSE_BLOCK) sse_rgb_kernel(FView xh, const S *__restrict__ src, int h, int w,
                                                            float mx, double *part) {
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
      const float d0 = v0 - smp(src[o], mx), d1 = v1 - smp(src[plane + o], mx), d2 = v2 - smp(src[2 * plane + o], mx);
      a[0] += (double)(d0 * d0);
      a[1] += (double)(d1 * d1);
      a[2] += (double)(d2 * d2);
    }
  }
  block_sum3(a[0], a[1], a[2], part);
}

}  // namespace

int dcvc_internal_rgb_sse(FSample s, float mx, FView xh, const void *src, int h, int w, double *workspace,
                          double *out3, hipStream_t st) {
  const unsigned g = sse_blocks((int64_t)xh.H * xh.W);
#define LAUNCH(S)                                                                                                  \
  hipLaunchKernelGGL(sse_rgb_kernel<S>, dim3(g), dim3(SSE_BLOCK), 0, st, xh, static_cast<const S *>(src), h, w, mx, \
                     workspace)
  if (s == FS_U8)
    LAUNCH(uint8_t);
  else if (s == FS_U16)
    LAUNCH(uint16_t);
  else
    LAUNCH(float);
#undef LAUNCH
  DCVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sse_final_kernel, dim3(1), dim3(256), 0, st, workspace, (int)g, out3);
  DCVC_LAUNCH_CHECK();
  return DCVC_HIP_OK;
}

extern "C" int dcvc_yuv420_to_nhwc(const uint8_t *y, const uint8_t *uv, int h, int w, dcvc_tensor out,
                                   void *stream) {
  if (!y || !uv || !frame_ok(out) || !even_frame(h, w) || out.H < h || out.W < w) return DCVC_HIP_EINVAL;
  return dcvc_internal_yuv_ingest(FS_U8, max_val(8), 2, 2, y, uv, h, w, fv(out),
                                  reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dcvc_frame_sse_workspace(void) { return (int64_t)3 * SSE_MAX_BLOCKS * sizeof(double); }

extern "C" int dcvc_frame_sse(dcvc_tensor x_hat, const uint8_t *src, const uint8_t *uv, int h, int w, int yuv420,
                              double *workspace, double *out3, void *stream) {
  if (!frame_ok(x_hat) || !src || !workspace || !out3 || h <= 0 || w <= 0 || x_hat.H < h || x_hat.W < w)
    return DCVC_HIP_EINVAL;
  if (yuv420 && (!uv || !even_frame(h, w) || !even_frame(x_hat.H, x_hat.W))) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (yuv420) return dcvc_internal_yuv_sse(FS_U8, max_val(8), 2, 2, fv(x_hat), src, uv, h, w, workspace, out3, st);
  return dcvc_internal_rgb_sse(FS_U8, max_val(8), fv(x_hat), src, h, w, workspace, out3, st);
}

extern "C" int dcvc_recon_to_u8(dcvc_tensor x_hat, int h, int w, int yuv420, uint8_t *out, void *stream) {
  if (!frame_ok(x_hat) || !out || h <= 0 || w <= 0 || x_hat.H < h || x_hat.W < w) return DCVC_HIP_EINVAL;
  if (yuv420 && !even_frame(h, w)) return DCVC_HIP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (yuv420) return dcvc_internal_yuv_write(FS_U8, max_val(8), 2, 2, false, fv(x_hat), h, w, out, st);
  return dcvc_internal_rgb_write(FS_U8, max_val(8), false, fv(x_hat), h, w, out, st);
}
