// Shared helpers for the gfx950 kernels of libcodenerf_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codenerf.h"

#define CN_CHECK_ARG(cond)          \
  do {                              \
    if (!(cond)) return CN_EINVAL;  \
  } while (0)

#define CN_TRY(x)                 \
  do {                            \
    const int rc_ = (x);          \
    if (rc_ != CN_OK) return rc_; \
  } while (0)

namespace cn {

constexpr int kWave = 64;

inline hipStream_t as_stream(cn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Launch status: hipGetLastError after a launch (sticky errors surface too).
inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? CN_OK : static_cast<int>(e);
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Grid for a grid-stride elementwise kernel: at most 256 CUs x 8 blocks.
// NULL counts as aligned (an optional output).
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline unsigned elementwise_grid(int64_t n, int block) {
  int64_t g = ceil_div(n, block);
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return static_cast<unsigned>(g);
}

// Compute units of the current device (256 if the query fails), cached per device for the whole
// library.
inline int64_t cu_count() {
  static int n[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (n[dev] == 0) {
    int v = 0;
    n[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return n[dev];
}

// Workgroups of a persistent grid over m rows in tiles of `tile`: one per CU (the kernels hold a
// CU's LDS and every SIMD's registers), never more than there are tiles, nor than `cap`.
inline unsigned persistent_grid(int64_t m, int64_t tile, int64_t cap = INT64_MAX) {
  int64_t g = ceil_div(m, tile);
  const int64_t cus = cu_count();
  if (g > cus) g = cus;
  if (g > cap) g = cap;
  return static_cast<unsigned>(g);
}

// Exact fp32 a*b then +c with two roundings (never contracted into an FMA):
// matches torch's separate mul and add kernels bit for bit.
__device__ __forceinline__ float mul_add_rn(float a, float b, float c) {
  return __fadd_rn(__fmul_rn(a, b), c);
}

// An occupancy grid's resolution: a multiple of 32 in [32, 512] (include/codenerf.h).
inline bool grid_ok(int64_t g) { return g >= 32 && g <= 512 && g % 32 == 0; }

// The occupancy lookup of include/codenerf.h: u_d = (p_d - lo) inv_cell, each op rounded; inside iff
// 0 <= u_d < G on every axis (false for NaN), cell floor(u_d).
__device__ __forceinline__ bool occupied(const unsigned* __restrict__ bits, int g, float lo, float inv_cell,
                                         float p0, float p1, float p2) {
  const float u0 = __fmul_rn(__fsub_rn(p0, lo), inv_cell);
  const float u1 = __fmul_rn(__fsub_rn(p1, lo), inv_cell);
  const float u2 = __fmul_rn(__fsub_rn(p2, lo), inv_cell);
  const float gf = static_cast<float>(g);
  const bool inside = u0 >= 0.0f && u0 < gf && u1 >= 0.0f && u1 < gf && u2 >= 0.0f && u2 < gf;
  if (!inside) return false;
  const unsigned i0 = static_cast<unsigned>(static_cast<int>(floorf(u0)));
  const unsigned i1 = static_cast<unsigned>(static_cast<int>(floorf(u1)));
  const unsigned i2 = static_cast<unsigned>(static_cast<int>(floorf(u2)));
  const unsigned c = (i0 * g + i1) * g + i2;      // < G^3 <= 2^27
  return (bits[c >> 5] >> (c & 31)) & 1u;
}

// torch.nn.functional.softplus(x) with beta 1, threshold 20 (volumetric_render.py:32):
// log1p(e), e = expf(x), as log(u) + (e - (u - 1)) / u with u = fl(1 + e) -- the rounding of u
// compensated to first order -- on the hardware log2 (v_log_f32) instead of the libm log1pf, whose
// extended-precision path was ~60 of volume_render's ~220 VALU instructions per sample.
__device__ __forceinline__ float softplus20(float x) {
  if (x > 20.0f) return x;
  const float e = expf(x);
  const float u = 1.0f + e;
  const float c = (e - (u - 1.0f)) * __builtin_amdgcn_rcpf(u);
  return fmaf(__builtin_amdgcn_logf(u), 0.693147180559945309f, c);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// sigmoid on the hardware exp2 / reciprocal (v_exp_f32, v_rcp_f32: 1 ulp each) instead of the
// libm expf and the IEEE division (~25 instructions).  The argument rounding of -x log2(e) moves
// e^-x by <= |x| 2^-24 relative, so the result stays within ~2e-7 of the exact sigmoid
// (saturated where |x| is large); volume_render's colours and their gradients use it.
__device__ __forceinline__ float sigmoid_hw(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}

// A raw colour channel as it is shown (volumetric_render.py:28): sigmoid(x) * 1.002 - 0.001, the product
// and the difference each rounded -- what cn_volume_render composites and cn_surface_shade writes.
__device__ __forceinline__ float widened_sigmoid(float x) {
  return __fsub_rn(__fmul_rn(sigmoid_hw(x), 1.002f), 0.001f);
}

}  // namespace cn
