// Iso-surface ray casting: the per-ray search around the density kernels (include/codenerf.h, "Iso-surface
// ray casting").
//
// bracket: one wave per ray.  Lanes stride over the ray's S densities, 64 a round (coalesced at stride 1);
// a round's `sigma >= level` is one ballot whose lowest set bit is the crossing -- wave-uniform, and the
// search stops at the first round that has one.  step and shade: one thread per ray, a few dozen bytes
// each; they are launch-latency bound at any ray count a view has.  No kernel here uses LDS, an atomic or a
// workspace, and each launches over exactly n_rays rows whatever the rays hit.
#include <limits.h>
#include <math.h>

#include "cn_common.h"

namespace {

constexpr int kRayWaves = 4;               // rays (waves) per 256-thread block, as cn_sample_span
constexpr int kMaxSearch = 1024;
constexpr int kRowBlock = 256;             // rays per block of the per-ray kernels

// s is known: not a culled slot's marker, not NaN.
__device__ __forceinline__ bool known(float s) { return s > CN_EMPTY_SIGMA_RAW; }

__global__ __launch_bounds__(64 * kRayWaves) void surface_bracket_kernel(
    const float* __restrict__ sigma, int sigma_stride, const float* __restrict__ z, int64_t n_rays, int n_samples,
    float level, float* __restrict__ bracket, int* __restrict__ hit) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRayWaves) + (threadIdx.x >> 6);
  if (r >= n_rays) return;                 // wave-uniform
  const int64_t row = r * n_samples;
  int j = -1;
  for (int j0 = 0; j0 < n_samples; j0 += 64) {
    const int s = j0 + lane;
    const bool reached = s < n_samples && sigma[(row + s) * sigma_stride] >= level;     // false for NaN
    const unsigned long long m = __ballot(reached);
    if (m) {
      j = j0 + __builtin_ctzll(m);
      break;
    }
  }
  const int lo = j < 0 ? n_samples - 1 : max(j - 1, 0);
  const int hi = j < 0 ? n_samples - 1 : j;
  if (lane < 4) {
    const int64_t k = row + ((lane & 1) ? hi : lo);
    bracket[4 * r + lane] = lane < 2 ? z[k] : sigma[k * sigma_stride];
  }
  if (lane == 0) hit[r] = j < 0 ? 0 : (j == 0 ? 2 : 1);
}

__global__ __launch_bounds__(kRowBlock) void surface_step_kernel(
    const float* __restrict__ ro, const float* __restrict__ rd, const int* __restrict__ hit,
    const float* __restrict__ probe, int probe_stride, float level, int finish, int64_t n_rays,
    float4* __restrict__ bracket, float* __restrict__ t, float* __restrict__ pts) {
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRowBlock) + threadIdx.x;
  if (r >= n_rays) return;
  float4 b = bracket[r];                   // t_lo, t_hi, s_lo, s_hi
  if (probe && hit[r] == 1) {
    const float tp = t[r];
    const float sp = probe[r * probe_stride];
    if (sp >= level) {
      b.y = tp;
      b.w = sp;
    } else {                               // below the level, or NaN
      b.x = tp;
      b.z = sp;
    }
    bracket[r] = b;
  }
  float w = 0.5f;
  if (finish) {
    const float ds = __fsub_rn(b.w, b.z);
    w = 1.0f;
    if (known(b.z) && !(ds <= 0.0f)) {
      const float q = __fdiv_rn(__fsub_rn(level, b.z), ds);
      const float q0 = q > 0.0f ? q : 0.0f;          // max(q, 0): 0 for a NaN quotient
      w = q0 < 1.0f ? q0 : 1.0f;
    }
  }
  const float tn = __fadd_rn(b.x, __fmul_rn(w, __fsub_rn(b.y, b.x)));
  t[r] = tn;
#pragma unroll
  for (int c = 0; c < 3; ++c) pts[3 * r + c] = __fadd_rn(ro[3 * r + c], __fmul_rn(rd[3 * r + c], tn));
}

__global__ __launch_bounds__(kRowBlock) void surface_shade_kernel(
    const float4* __restrict__ raw, const int* __restrict__ hit, const float* __restrict__ t, float bg0, float bg1,
    float bg2, int64_t n_rays, float* __restrict__ rgb, float* __restrict__ depth, float* __restrict__ pts) {
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRowBlock) + threadIdx.x;
  if (r >= n_rays) return;
  if (hit[r] != 0) {
    const float4 v = raw[r];
    rgb[3 * r + 0] = cn::widened_sigmoid(v.x);
    rgb[3 * r + 1] = cn::widened_sigmoid(v.y);
    rgb[3 * r + 2] = cn::widened_sigmoid(v.z);
    depth[r] = t[r];
  } else {
    rgb[3 * r + 0] = bg0;
    rgb[3 * r + 1] = bg1;
    rgb[3 * r + 2] = bg2;
    depth[r] = INFINITY;
    const float nan = __builtin_nanf("");
    pts[3 * r + 0] = nan;
    pts[3 * r + 1] = nan;
    pts[3 * r + 2] = nan;
  }
}

bool stride_ok(int64_t stride) { return stride == 1 || stride == 4; }

}  // namespace

extern "C" int cn_surface_bracket(const float* sigma, int64_t sigma_stride, const float* z, int64_t n_rays,
                                  int64_t n_samples, float level, float* bracket, int32_t* hit, cn_stream_t stream) {
  CN_CHECK_ARG(sigma && z && bracket && hit);
  CN_CHECK_ARG(n_rays > 0 && n_samples >= 2 && n_samples <= kMaxSearch && stride_ok(sigma_stride) && isfinite(level));
  const int64_t ray_blocks = cn::ceil_div(n_rays, kRayWaves);
  CN_CHECK_ARG(ray_blocks <= INT_MAX && n_rays <= INT64_MAX / (4 * kMaxSearch));
  hipLaunchKernelGGL(surface_bracket_kernel, dim3(static_cast<unsigned>(ray_blocks)), dim3(64 * kRayWaves), 0,
                     cn::as_stream(stream), sigma, static_cast<int>(sigma_stride), z, n_rays,
                     static_cast<int>(n_samples), level, bracket, hit);
  return cn::launch_status();
}

extern "C" int cn_surface_step(const float* ro, const float* rd, const int32_t* hit, const float* probe_sigma,
                               int64_t probe_stride, float level, int finish, int64_t n_rays, float* bracket, float* t,
                               float* pts, cn_stream_t stream) {
  CN_CHECK_ARG(ro && rd && hit && bracket && t && pts);
  CN_CHECK_ARG(n_rays > 0 && stride_ok(probe_stride) && isfinite(level) && (finish == 0 || finish == 1));
  CN_CHECK_ARG(cn::aligned16(bracket));
  const int64_t blocks = cn::ceil_div(n_rays, kRowBlock);
  CN_CHECK_ARG(blocks <= INT_MAX);
  hipLaunchKernelGGL(surface_step_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kRowBlock), 0,
                     cn::as_stream(stream), ro, rd, hit, probe_sigma, static_cast<int>(probe_stride), level, finish,
                     n_rays, reinterpret_cast<float4*>(bracket), t, pts);
  return cn::launch_status();
}

extern "C" int cn_surface_shade(const float* raw, const int32_t* hit, const float* t, const float* background,
                                int64_t n_rays, float* rgb, float* depth, float* pts, cn_stream_t stream) {
  CN_CHECK_ARG(raw && hit && t && background && rgb && depth && pts);
  CN_CHECK_ARG(n_rays > 0 && cn::aligned16(raw));
  const int64_t blocks = cn::ceil_div(n_rays, kRowBlock);
  CN_CHECK_ARG(blocks <= INT_MAX);
  hipLaunchKernelGGL(surface_shade_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kRowBlock), 0,
                     cn::as_stream(stream), reinterpret_cast<const float4*>(raw), hit, t, background[0], background[1],
                     background[2], n_rays, rgb, depth, pts);
  return cn::launch_status();
}
