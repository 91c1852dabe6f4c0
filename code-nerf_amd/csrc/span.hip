// Per-ray depth spans from occupancy grids, and the coarse depths stratified inside them
// (include/codenerf.h, "Per-ray depth spans").
//
// One wave per ray.  The ray's P probe depths are looked up in every object's grid, 64 probes a
// round: a round's occupied probes are one ballot, whose lowest / highest set bits give the first and
// last occupied probe -- wave-uniform, no reduction across waves, no atomics, no workspace.  The wave
// then writes its ray's Nc depths, lanes strided over the samples.  The kernel is latency bound on
// the grid words (L2-resident: 256 KiB at G = 128); the K grids' descriptors travel by value in the
// kernel argument.
#include <limits.h>
#include <math.h>

#include "cn_common.h"

namespace {

constexpr int kRayWaves = 4;               // rays (waves) per 256-thread block, as the occupancy passes
constexpr int kMaxProbes = 1024;
constexpr int kMaxSpanSamples = 512;       // as cn_volume_render

struct SpanGrids {
  const unsigned* bits[CN_MAX_SCENE_OBJECTS];
  int g[CN_MAX_SCENE_OBJECTS];
  float lo[CN_MAX_SCENE_OBJECTS];
  float inv_cell[CN_MAX_SCENE_OBJECTS];
};

// Probe depth j of [near, far]: near + j step, the last one far itself.
__device__ __forceinline__ float probe_depth(int j, int n_probes, float near, float far, float step) {
  return j == n_probes - 1 ? far : __fadd_rn(near, __fmul_rn(static_cast<float>(j), step));
}

__global__ __launch_bounds__(64 * kRayWaves) void sample_span_kernel(
    const float* __restrict__ ro, const float* __restrict__ rd, int64_t n_rays, SpanGrids grids, int n_objects,
    float near, float far, float step, int n_probes, int nc, const float* __restrict__ t_rand,
    float* __restrict__ z_out, float* __restrict__ span, int* __restrict__ probe_range) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRayWaves) + (threadIdx.x >> 6);
  if (r >= n_rays) return;                 // wave-uniform
  int first = -1, last = -1;
  for (int j0 = 0; j0 < n_probes; j0 += 64) {      // n_probes is a multiple of 64: no partial round
    const float d = probe_depth(j0 + lane, n_probes, near, far, step);
    bool occ = false;
#pragma unroll 1                           // one object's descriptor and ray in SGPRs at a time
    for (int k = 0; k < n_objects; ++k) {
      const float* o = ro + 3 * (k * n_rays + r);
      const float* v = rd + 3 * (k * n_rays + r);
      occ = occ || cn::occupied(grids.bits[k], grids.g[k], grids.lo[k], grids.inv_cell[k],
                                cn::mul_add_rn(v[0], d, o[0]), cn::mul_add_rn(v[1], d, o[1]),
                                cn::mul_add_rn(v[2], d, o[2]));
    }
    const unsigned long long m = __ballot(occ);
    if (m) {
      if (first < 0) first = j0 + __builtin_ctzll(m);
      last = j0 + 63 - __builtin_clzll(m);
    }
  }
  // a miss (first = last = -1) keeps the whole range
  const int a = first < 0 ? 0 : max(first - 1, 0);
  const int b = first < 0 ? n_probes - 1 : min(last + 1, n_probes - 1);
  const float t_lo = probe_depth(a, n_probes, near, far, step);
  const float t_hi = probe_depth(b, n_probes, near, far, step);
  const float w = __fdiv_rn(__fsub_rn(t_hi, t_lo), static_cast<float>(nc - 1));
  float* zr = z_out + r * nc;
  const float* tr = t_rand ? t_rand + r * nc : nullptr;
  for (int i = lane; i < nc; i += 64) {
    float z = t_hi;                        // the last sample sits on t_hi exactly
    if (i < nc - 1) {
      const float t = __fadd_rn(static_cast<float>(i), tr ? tr[i] : 0.0f);
      const float v = __fadd_rn(t_lo, __fmul_rn(t, w));
      z = v > t_hi ? t_hi : v;
    }
    zr[i] = z;
  }
  if (lane < 2) {
    span[2 * r + lane] = lane ? t_hi : t_lo;
    probe_range[2 * r + lane] = lane ? last : first;
  }
}

}  // namespace

extern "C" int cn_sample_span(const float* ro, const float* rd, int64_t n_rays, const uint32_t* const* bits,
                              const int64_t* g, const float* lo, const float* inv_cell, int n_objects, float near,
                              float far, int64_t n_probes, int64_t nc, const float* t_rand, float* z_out, float* span,
                              int32_t* probe_range, cn_stream_t stream) {
  CN_CHECK_ARG(ro && rd && bits && g && lo && inv_cell && z_out && span && probe_range);
  CN_CHECK_ARG(n_objects >= 1 && n_objects <= CN_MAX_SCENE_OBJECTS && n_rays > 0);
  CN_CHECK_ARG(n_probes >= 64 && n_probes <= kMaxProbes && n_probes % 64 == 0 && nc >= 2 && nc <= kMaxSpanSamples);
  CN_CHECK_ARG(isfinite(near) && isfinite(far) && near >= 0.0f && far > near);
  const int64_t ray_blocks = cn::ceil_div(n_rays, kRayWaves);
  CN_CHECK_ARG(ray_blocks <= INT_MAX && n_rays <= INT64_MAX / (3 * CN_MAX_SCENE_OBJECTS));
  SpanGrids grids = {};
  for (int k = 0; k < n_objects; ++k) {
    CN_CHECK_ARG(bits[k] && cn::grid_ok(g[k]) && isfinite(lo[k]) && isfinite(inv_cell[k]));
    grids.bits[k] = bits[k];
    grids.g[k] = static_cast<int>(g[k]);
    grids.lo[k] = lo[k];
    grids.inv_cell[k] = inv_cell[k];
  }
  const float step = (far - near) / static_cast<float>(n_probes - 1);      // fp32, each op rounded
  hipLaunchKernelGGL(sample_span_kernel, dim3(static_cast<unsigned>(ray_blocks)), dim3(64 * kRayWaves), 0,
                     cn::as_stream(stream), ro, rd, n_rays, grids, n_objects, near, far, step,
                     static_cast<int>(n_probes), static_cast<int>(nc), t_rand, z_out, span, probe_range);
  return cn::launch_status();
}
