// Volume integration: volume_render (view_synthesis/nerf/volumetric_render.py:36-66).
//
// The exclusive prefix of sigma*delta -- transmittance = exp(-[0, cumsum(sigma*delta)[:-1]]) --
// is a scan over the lanes' run totals followed by the in-run prefix (layout below).
#include "cn_common.h"

namespace {

// L lanes per ray: 16 (one DPP row; 4 rays per wave, 16 per 256-thread block) for S <= 128, 64
// (the whole wave; 4 rays per block) above, so a lane's run stays <= 8 samples in registers at
// every S <= 512.  Lane i of a ray owns the contiguous run of samples [i run, (i + 1) run),
// run = ceil(S / L) <= K; its next sample's depth (z[j + 1] past the run) comes from lane i + 1 by
// DPP (a lane shuffle when L = 64) instead of a second load; the exclusive prefix of sigma*delta
// over the lanes' run totals is a 4-step DPP row scan (in double, as torch's CPU cumsum
// accumulates, Q13) plus, for L = 64, the earlier rows' totals read back as scalars; the per-ray
// sums are DPP row reductions (plus the row totals for L = 64) -- no LDS traffic in any
// cross-lane step.
// Algorithmic bytes per ray: 12 (rd) + 20*S in (raw + z), 4*S + 20 out.
constexpr int kMaxRun = 8;
constexpr int kMaxSamples = 64 * kMaxRun;  // 512

// Raw rows, depths and weights cross the kernel once: non-temporal 16-B loads and stores (streamed
// past the caches) -- the C2 launch 91 -> 86 us alone, 83 -> 74 us with the grouped launch (r04,
// tools/volume_timing.py, HIP-event medians).
typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4* p) {
  const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store4(float4 v, float4* p) {
  __builtin_nontemporal_store(nt_f4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_f4*>(p));
}

template <int CTRL>
__device__ __forceinline__ float dppf(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ double dppd(double x) {
  const long long v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(v & 0xffffffff), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(v >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}
// Inclusive prefix over the 16 lanes of the row (row_shr: lane i reads lane i - n, 0 below the row).
__device__ __forceinline__ double row_inclusive_scan(double x) {
  x += dppd<0x111>(x);
  x += dppd<0x112>(x);
  x += dppd<0x114>(x);
  x += dppd<0x118>(x);
  return x;
}
// Inclusive suffix over the row (row_shl: lane i reads lane i + n, 0 past the row).
__device__ __forceinline__ float row_inclusive_suffix(float x) {
  x += dppf<0x101>(x);
  x += dppf<0x102>(x);
  x += dppf<0x104>(x);
  x += dppf<0x108>(x);
  return x;
}
// Sum over the row's 16 lanes, valid in lane 15.
__device__ __forceinline__ float row_sum(float x) {
  x += dppf<0x111>(x);
  x += dppf<0x112>(x);
  x += dppf<0x114>(x);
  x += dppf<0x118>(x);
  return x;
}

__device__ __forceinline__ float lanef(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}
__device__ __forceinline__ double laned(double x, int l) {
  const long long v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane(static_cast<int>(v & 0xffffffff), l);
  const int hi = __builtin_amdgcn_readlane(static_cast<int>(v >> 32), l);
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

// The ray-level cross-lane steps over its L lanes.  L = 16: the row steps.  L = 64 (one ray per
// wave): the row step, then the other rows' totals -- uniform, read back by readlane -- added in
// a fixed order.
template <int L>
__device__ __forceinline__ double ray_exclusive_scan(double v) {
  const double x = row_inclusive_scan(v);
  if constexpr (L == 16) {
    return x - v;
  } else {
    const int row = (threadIdx.x & 63) >> 4;
    const double t0 = laned(x, 15), t1 = laned(x, 31), t2 = laned(x, 47);
    double off = 0.0;
    if (row > 0) off += t0;
    if (row > 1) off += t1;
    if (row > 2) off += t2;
    return (x - v) + off;
  }
}
template <int L>
__device__ __forceinline__ float ray_exclusive_suffix(float v) {
  const float x = row_inclusive_suffix(v);
  if constexpr (L == 16) {
    return x - v;
  } else {  // row totals: the inclusive suffix in each row's lane 0
    const int row = (threadIdx.x & 63) >> 4;
    const float t1 = lanef(x, 16), t2 = lanef(x, 32), t3 = lanef(x, 48);
    float off = 0.0f;
    if (row < 3) off += t3;
    if (row < 2) off += t2;
    if (row < 1) off += t1;
    return (x - v) + off;
  }
}
// The ray's sum over its L lanes: valid in lane 15 of the row (L = 16) / every lane (L = 64).
template <int L>
__device__ __forceinline__ float ray_sum(float x) {
  x = row_sum(x);
  if constexpr (L == 64) x = ((lanef(x, 15) + lanef(x, 31)) + lanef(x, 47)) + lanef(x, 63);
  return x;
}
// ... valid in every lane of the ray.
template <int L>
__device__ __forceinline__ float ray_sum_all(float x) {
  if constexpr (L == 16) return __shfl(row_sum(x), (threadIdx.x & 63) | 15);
  else return ray_sum<64>(x);
}
// Lane + 1's value (the next run's first depth); 0 (L = 16) or the lane's own value (L = 64) past
// the ray's last lane, where it is never used.
template <int L>
__device__ __forceinline__ float next_lane(float x) {
  if constexpr (L == 16) return dppf<0x101>(x);
  else return __shfl_down(x, 1);
}

// Load this lane's run of depths (zero past S): 16-B vector loads when the run is a multiple of
// 4 aligned to 16 B (every S % 4 == 0 with run % 4 == 0: S = 64, 128 -- the C2 / C3 shapes),
// element loads otherwise.
template <int K>
__device__ __forceinline__ void load_depths(const float* zr, int j0, int run, int S_in, float (&zz)[K]) {
  if (K % 4 == 0 && run % 4 == 0 && (S_in & 3) == 0 && j0 + run <= S_in) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * q < run) v = nt_load4(reinterpret_cast<const float4*>(zr + j0) + q);
      zz[4 * q] = v.x;
      zz[4 * q + 1] = v.y;
      zz[4 * q + 2] = v.z;
      zz[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < K; ++i) zz[i] = (i < run && j0 + i < S_in) ? zr[j0 + i] : 0.0f;
  }
}

template <int K>
__device__ __forceinline__ void load_run(const float* zr, const float4* rr, int j0, int run, int S_in, float (&zz)[K],
                                         float4 (&rv)[K]) {
  load_depths<K>(zr, j0, run, S_in, zz);
#pragma unroll
  for (int i = 0; i < K; ++i)
    rv[i] = (i < run && j0 + i < S_in) ? rr[j0 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Raw rows through LDS: a lane's run of float4 samples is 16 run bytes apart from its
// neighbour's, so per-lane loads of it touch every cache line run times.  The wave's rays' rows
// (64 / L of them) are ONE contiguous (64 / L) S float4 block: lane l copies quads l + 64 t with
// coalesced 16-B loads into LDS slot pad(q) = q + q / 4 (a padding quad after every four: runs of
// four then sit 5 quads apart, conflict-free across a 16-lane group), and each lane then reads
// its own run from there.  The backward stores d raw back the same way.  <= 64 K quads per wave.
__device__ __forceinline__ int pad4(int q) { return q + (q >> 2); }


template <int K>
__device__ __forceinline__ void stage_rows_in(const float4* __restrict__ src, int nq, float4* sl, int lane) {
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const int q = lane + 64 * t;
    if (q < nq) sl[pad4(q)] = nt_load4(src + q);
  }
}

template <int K>
__device__ __forceinline__ void stage_rows_out(float4* __restrict__ dst, int nq, const float4* sl, int lane) {
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const int q = lane + 64 * t;
    if (q < nq) dst[q] = sl[pad4(q)];
  }
}

// This lane's run of raw rows from the wave's LDS copy (q0: the run's first quad in the wave block).
template <int K>
__device__ __forceinline__ void load_raw_lds(const float4* sl, int q0, int j0, int run, int S_in, float4 (&rv)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) rv[i] = (i < run && j0 + i < S_in) ? sl[pad4(q0 + i)] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// A raw row's density and colour channel (volumetric_render.py:32 and :28), shared by the plain and the
// composed render: shifted_softplus(x) = softplus(x - 1); widened_sigmoid(x) = sigmoid(x) * 1.002 - 0.001.
__device__ __forceinline__ float raw_sigma(float x) { return cn::softplus20(__fsub_rn(x, 1.0f)); }
__device__ __forceinline__ float raw_colour(float x) { return cn::widened_sigmoid(x); }

// This lane's run of weights: 16-B stores where the run is aligned (see load_depths).  S: the samples
// that contribute (0 for the sample-free S_in == 1).
template <int K>
__device__ __forceinline__ void store_run_weights(float* __restrict__ weights, int64_t r, int j0, int run, int S_in,
                                                  int S, const float (&wv)[K]) {
  float* wr = weights + r * S_in;
  if (K % 4 == 0 && run % 4 == 0 && (S_in & 3) == 0 && j0 + run <= S_in && S > 0) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q)
      if (4 * q < run)
        nt_store4(make_float4(wv[4 * q], wv[4 * q + 1], wv[4 * q + 2], wv[4 * q + 3]),
                                    reinterpret_cast<float4*>(wr + j0) + q);
  } else {
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (i < run && j0 + i < S) wr[j0 + i] = wv[i];
  }
}

// The ray's maps from its summed colour, depth and opacity (the lane that holds the sums stores).
__device__ __forceinline__ void store_ray_maps(int64_t r, float cr, float cg, float cb, float dep, float ac,
                                               float* __restrict__ rgb, float* __restrict__ disp,
                                               float* __restrict__ acc, float* __restrict__ depth) {
  rgb[3 * r] = cr;
  rgb[3 * r + 1] = cg;
  rgb[3 * r + 2] = cb;
  depth[r] = dep;
  acc[r] = ac;
  // (:63) torch.max propagates NaN: disp is NaN when acc == 0
  const float q = dep / ac;
  disp[r] = (q != q) ? q : 1.0f / fmaxf(1e-10f, q);
}

// One lane's part of a ray (lane sub of its L): the run's depths zz and raw rows rv loaded, |rd| = nrm.
template <int K, bool FULL, int L>
__device__ __forceinline__ void render_run(const float (&zz)[K], const float4 (&rv)[K], int S_in, int64_t r, float nrm,
                                           float* __restrict__ rgb, float* __restrict__ disp, float* __restrict__ acc,
                                           float* __restrict__ weights, float* __restrict__ depth) {
  const int sub = threadIdx.x & (L - 1);
  // S == 1: the reference's dists = cat(z[1:] - z[:-1], full_like(that[..., :1], 1e10))
  // is EMPTY (both pieces are 0 wide), so no sample contributes (rgb = acc = depth = 0,
  // disp = NaN, weights (R, 0)).  Reproduced by treating the ray as sample-free.
  // FULL (S_in == 16 K: every lane's run is K samples): the run / bounds tests fold away
  const int S = FULL ? L * K : (S_in == 1 ? 0 : S_in);
  const int run = FULL ? K : (S_in + L - 1) / L;
  const int j0 = sub * run;
  float sd[K], wv[K];
  const float znext = next_lane<L>(zz[0]);  // the first depth of lane sub + 1's run
  double run_sum = 0.0;  // sum of this run's sigma*delta that feeds later transmittances
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = j0 + i;
    sd[i] = 0.0f;
    if (i < run && j < S) {
      // dists = [z[1:] - z[:-1], 1e10] (:41-44), delta = dists * |rd| (:45)
      const float zn = (i + 1 < run) ? zz[(i + 1) % K] : znext;
      const float dist = (j + 1 < S) ? __fsub_rn(zn, zz[i]) : 1e10f;
      const float sigma = raw_sigma(rv[i].w);  // shifted_softplus (:32)
      sd[i] = __fmul_rn(sigma, __fmul_rn(dist, nrm));
      if (j + 1 < S) run_sum += static_cast<double>(sd[i]);
    }
  }
  double prefix = ray_exclusive_scan<L>(run_sum);

  float cr = 0.f, cg = 0.f, cb = 0.f, dep = 0.f, ac = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = j0 + i;
    wv[i] = 0.0f;
    if (i < run && j < S) {
      const float trans = expf(-static_cast<float>(prefix));      // (:54-57)
      const float alpha = __fsub_rn(1.0f, expf(-sd[i]));           // (:58)
      const float w = __fmul_rn(alpha, trans);                     // (:59)
      // widened_sigmoid (:28): sigmoid(x) * 1.002 - 0.001
      const float c0 = raw_colour(rv[i].x), c1 = raw_colour(rv[i].y), c2 = raw_colour(rv[i].z);
      cr += w * c0;
      cg += w * c1;
      cb += w * c2;
      dep += w * zz[i];
      ac += w;
      wv[i] = w;
      if (j + 1 < S) prefix += static_cast<double>(sd[i]);
    }
  }
  if (weights) store_run_weights<K>(weights, r, j0, run, S_in, S, wv);
  cr = ray_sum<L>(cr);
  cg = ray_sum<L>(cg);
  cb = ray_sum<L>(cb);
  dep = ray_sum<L>(dep);
  ac = ray_sum<L>(ac);
  if (sub == (L == 16 ? 15 : 63)) store_ray_maps(r, cr, cg, cb, dep, ac, rgb, disp, acc, depth);
}

template <int K, bool FULL, int L>
__global__ __launch_bounds__(256) void volume_render_kernel(
    const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rd,
    int64_t n_rays, int S_in, float* __restrict__ rgb, float* __restrict__ disp,
    float* __restrict__ acc, float* __restrict__ weights, float* __restrict__ depth) {
  static_assert(K <= kMaxRun && (L == 16 || L == 64) && (!FULL || L == 16), "instance");
  if (FULL) S_in = L * K;  // the host dispatches FULL only for S == 16 K: lets every bound fold
  __shared__ float4 slds[4 * 80 * K];  // per wave: <= 64 K quads, padded 5 / 4
  const int sub = threadIdx.x & (L - 1), lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int64_t rw0 = r - lane / L;  // the wave's first ray
  float4* sl = slds + (threadIdx.x >> 6) * 80 * K;
  if (rw0 < n_rays)
    stage_rows_in<K>(reinterpret_cast<const float4*>(raw) + rw0 * S_in,
                     static_cast<int>(min<int64_t>(64 / L, n_rays - rw0)) * S_in, sl, lane);
  // lanes read quads other lanes wrote: keep the staging stores ahead of the reads (no instruction;
  // LDS operations of one wave then execute in program order)
  __builtin_amdgcn_wave_barrier();
  if (r >= n_rays) return;  // whole rays leave together: the cross-lane steps never read an exited lane
  const int run = FULL ? K : (S_in + L - 1) / L;
  const int j0 = sub * run;
  const float* zr = z + r * S_in;
  const float d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
  const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
  float zz[K];
  float4 rv[K];
  load_depths<K>(zr, j0, run, S_in, zz);
  load_raw_lds<K>(sl, (lane / L) * S_in + j0, j0, run, S_in, rv);
  render_run<K, FULL, L>(zz, rv, S_in, r, nrm, rgb, disp, acc, weights, depth);
}

// S = 16 K with n_rays % 4 == 0 (dispatched for S = 64: the C2 / C3 / C5 coarse launches; at K = 8
// the staged rows would cost the occupancy): wave w renders G groups of 4 rays, groups
// w + g W of the grid's W waves.  Every group's raw rows, depths and directions are loaded up front,
// so the later groups' loads are in flight while the wave integrates the earlier ones.
template <int K, int G>
__global__ __launch_bounds__(256) void volume_render_groups_kernel(
    const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rd, int64_t n_rays,
    float* __restrict__ rgb, float* __restrict__ disp, float* __restrict__ acc, float* __restrict__ weights,
    float* __restrict__ depth) {
  constexpr int L = 16, S = L * K;
  __shared__ float4 slds[4 * 80 * K];
  const int lane = threadIdx.x & 63, sub = lane & 15;
  float4* sl = slds + (threadIdx.x >> 6) * 80 * K;
  const int64_t n_waves = (int64_t)gridDim.x * 4, wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  float4 stg[G][K];
  float zz[G][K], dv[G][3];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    // past the end: a copy of the last group (no branch around the loads, so the arrays stay in registers)
    const int64_t rw0 = min(4 * (wave + g * n_waves), n_rays - 4);
    const float4* src = reinterpret_cast<const float4*>(raw) + rw0 * S;
#pragma unroll
    for (int t = 0; t < K; ++t) stg[g][t] = nt_load4(src + lane + 64 * t);
    const int64_t r = rw0 + lane / L;
    float zl[K];
    load_depths<K>(z + r * S, sub * K, K, S, zl);
#pragma unroll
    for (int i = 0; i < K; ++i) zz[g][i] = zl[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) dv[g][d] = rd[3 * r + d];
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t rw0 = 4 * (wave + g * n_waves);
    if (rw0 >= n_rays) continue;  // wave-uniform
#pragma unroll
    for (int t = 0; t < K; ++t) sl[pad4(lane + 64 * t)] = stg[g][t];
    __builtin_amdgcn_wave_barrier();
    float4 rv[K];
    load_raw_lds<K>(sl, (lane / L) * S + sub * K, sub * K, K, S, rv);
    __builtin_amdgcn_wave_barrier();
    float zg[K];
#pragma unroll
    for (int i = 0; i < K; ++i) zg[i] = zz[g][i];
    const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dv[g][0], dv[g][0]), __fmul_rn(dv[g][1], dv[g][1])),
                                           __fmul_rn(dv[g][2], dv[g][2])));
    render_run<K, true, L>(zg, rv, S, rw0 + lane / L, nrm, rgb, disp, acc, weights, depth);
  }
}

}  // namespace

// Instances: S = 64 / 128 (every C2-C5 coarse / merged shape) take the FULL 16-lane ones; other
// S <= 128 the 16-lane ones with run <= 4 / 8; S <= 512 (the 32 + 160 and 64 + 128 merged
// shapes: S = 192) the 64-lane ones with run <= 4 / 8.
#define CN_VOLUME_DISPATCH(KERNEL, S, N, STREAM, ...)                                                      \
  do {                                                                                                      \
    const dim3 g16(static_cast<unsigned>(cn::ceil_div((N), 16))), g64(static_cast<unsigned>(cn::ceil_div((N), 4))); \
    if ((S) == 64) hipLaunchKernelGGL((KERNEL<4, true, 16>), g16, dim3(256), 0, STREAM, __VA_ARGS__);      \
    else if ((S) == 128) hipLaunchKernelGGL((KERNEL<8, true, 16>), g16, dim3(256), 0, STREAM, __VA_ARGS__); \
    else if ((S) <= 64) hipLaunchKernelGGL((KERNEL<4, false, 16>), g16, dim3(256), 0, STREAM, __VA_ARGS__); \
    else if ((S) <= 128) hipLaunchKernelGGL((KERNEL<8, false, 16>), g16, dim3(256), 0, STREAM, __VA_ARGS__); \
    else if ((S) <= 256) hipLaunchKernelGGL((KERNEL<4, false, 64>), g64, dim3(256), 0, STREAM, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<8, false, 64>), g64, dim3(256), 0, STREAM, __VA_ARGS__);                \
  } while (0)

extern "C" int cn_volume_render(const float* raw, const float* z, const float* rd, int64_t n_rays,
                                int64_t n_samples, float* rgb, float* disp, float* acc,
                                float* weights, float* depth, cn_stream_t stream) {
  CN_CHECK_ARG(raw && z && rd && rgb && disp && acc && depth);
  CN_CHECK_ARG(n_rays > 0 && n_samples > 0 && n_samples <= kMaxSamples);
  CN_CHECK_ARG(cn::aligned16(raw) && cn::aligned16(z) && cn::aligned16(weights));
  if (n_samples == 64 && n_rays % 4 == 0) {  // C2 / C5 coarse: two ray groups per wave
    constexpr int G = 2;
    const int64_t waves = cn::ceil_div(n_rays / 4, G);
    hipLaunchKernelGGL((volume_render_groups_kernel<4, G>), dim3(static_cast<unsigned>(cn::ceil_div(waves, 4))),
                       dim3(256), 0, cn::as_stream(stream), raw, z, rd, n_rays, rgb, disp, acc, weights, depth);
    return cn::launch_status();
  }
  CN_VOLUME_DISPATCH(volume_render_kernel, n_samples, n_rays, cn::as_stream(stream), raw, z, rd, n_rays,
                     static_cast<int>(n_samples), rgb, disp, acc, weights, depth);
  return cn::launch_status();
}

// ---------------------------------------------------------------- scene composition
// cn_volume_render_compose: the raw rows of n_objects objects at the same depths become one ray integral
// (the rule is in include/codenerf.h).  volume_render_kernel's geometry -- L lanes per ray, a run of
// <= K samples per lane, the wave's rows staged through LDS -- with each object's rows staged in turn
// through the same LDS block.  Per sample a lane keeps the summed density, the colour numerator, the
// count of active objects and the last active object's colour (the mix's three cases), and every
// object's own density for the shares: NOBJ * K <= 64 values.  NOBJ bounds n_objects at compile time, so
// every array is indexed statically and stays in registers.
// Algorithmic bytes per ray: 12 (rd) + (16 n_objects + 4) S in, 4 S + 20 + 4 n_objects out.
namespace {

struct ComposeRaws {
  const float* p[CN_MAX_SCENE_OBJECTS];
};
// The objects' uniform scales (cn_volume_render_compose_scaled): read by the SCALED instances only, whose
// density is softplus20(xs - 1) / s_k; the others are the unscaled entries' kernels as they were.
struct ComposeScales {
  float s[CN_MAX_SCENE_OBJECTS];
};

// HOST scales into the kernel argument; false for one that is NaN, infinite or <= 0.
inline bool read_scales(const float* scales, int n_objects, ComposeScales& sc) {
  for (int k = 0; k < n_objects; ++k) {
    const float v = scales[k];
    if (!(v - v == 0.0f && v > 0.0f)) return false;
    sc.s[k] = v;
  }
  return true;
}

template <bool SCALED>
__device__ __forceinline__ float object_sigma(float xs, float scale) {
  if constexpr (SCALED) return __fdiv_rn(raw_sigma(xs), scale);
  else return raw_sigma(xs);
}

// SCALED instances ask for two waves per SIMD (<= 256 registers): the divisions' temporaries would otherwise take
// the <8, 64, 8> instance past it.  The unscaled instances keep the default bound and their code.
template <int K, int L, int NOBJ, bool SCALED>
__global__ __launch_bounds__(256, SCALED ? 2 : 1) void volume_render_compose_kernel(
    ComposeRaws raws, ComposeScales scales, int n_objects, const float* __restrict__ z, const float* __restrict__ rd,
    int64_t n_rays,
    int S_in, float* __restrict__ rgb, float* __restrict__ disp, float* __restrict__ acc,
    float* __restrict__ weights, float* __restrict__ depth, float* __restrict__ acc_objects) {
  static_assert(K <= kMaxRun && (L == 16 || L == 64) && NOBJ >= 1 && NOBJ <= CN_MAX_SCENE_OBJECTS, "instance");
  __shared__ float4 slds[4 * 80 * K];  // per wave: one object's <= 64 K quads, padded 5 / 4
  const int sub = threadIdx.x & (L - 1), lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int64_t rw0 = r - lane / L;  // the wave's first ray
  if (rw0 >= n_rays) return;         // the whole wave
  const int nq = static_cast<int>(min<int64_t>(64 / L, n_rays - rw0)) * S_in;  // the wave's valid quads
  float4* sl = slds + (threadIdx.x >> 6) * 80 * K;
  // a ray past n_rays (L = 16 only) copies its share of every object's rows, accumulates nothing and
  // leaves before the cross-lane steps, with its whole row
  const bool live = r < n_rays;
  const int S = S_in == 1 ? 0 : S_in;  // see render_run: S == 1 has no contributing sample
  const int run = (S_in + L - 1) / L;
  const int j0 = sub * run;
  const int q0 = (lane / L) * S_in + j0;  // this run's first quad in the wave block
  float zz[K];
  float nrm = 0.0f;
  if (live) {
    load_depths<K>(z + r * S_in, j0, run, S_in, zz);
    const float d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
    nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
  }

  float sig[K], num[K][3], lone[K][3], sk[NOBJ][K];
  int cnt[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    sig[i] = 0.0f;
    cnt[i] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) num[i][c] = lone[i][c] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < NOBJ; ++k) {
#pragma unroll
    for (int i = 0; i < K; ++i) sk[k][i] = 0.0f;
    if (k >= n_objects) continue;  // uniform
    // the previous object's LDS reads stay ahead of these stores, and these stores ahead of the reads
    // (no instruction: the LDS operations of one wave execute in program order)
    __builtin_amdgcn_wave_barrier();
    stage_rows_in<K>(reinterpret_cast<const float4*>(raws.p[k]) + rw0 * S_in, nq, sl, lane);
    __builtin_amdgcn_wave_barrier();
    if (!live) continue;
    float4 rv[K];
    load_raw_lds<K>(sl, q0, j0, run, S_in, rv);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if (i < run && j0 + i < S) {
        const float s = object_sigma<SCALED>(rv[i].w, scales.s[k]);
        sk[k][i] = s;
        sig[i] = __fadd_rn(sig[i], s);
        if (s != 0.0f) {  // active (a NaN density is)
          const float c0 = raw_colour(rv[i].x), c1 = raw_colour(rv[i].y), c2 = raw_colour(rv[i].z);
          cnt[i] += 1;
          lone[i][0] = c0;
          lone[i][1] = c1;
          lone[i][2] = c2;
          num[i][0] = __fadd_rn(num[i][0], __fmul_rn(s, c0));
          num[i][1] = __fadd_rn(num[i][1], __fmul_rn(s, c1));
          num[i][2] = __fadd_rn(num[i][2], __fmul_rn(s, c2));
        }
      }
    }
  }
  if (!live) return;  // whole rays leave together: the cross-lane steps never read an exited lane

  // from here render_run's arithmetic on the summed density and the mixed colour
  float sd[K], wv[K];
  const float znext = next_lane<L>(zz[0]);
  double run_sum = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = j0 + i;
    sd[i] = 0.0f;
    if (i < run && j < S) {
      const float zn = (i + 1 < run) ? zz[(i + 1) % K] : znext;
      const float dist = (j + 1 < S) ? __fsub_rn(zn, zz[i]) : 1e10f;
      sd[i] = __fmul_rn(sig[i], __fmul_rn(dist, nrm));
      if (j + 1 < S) run_sum += static_cast<double>(sd[i]);
    }
  }
  double prefix = ray_exclusive_scan<L>(run_sum);

  float cr = 0.f, cg = 0.f, cb = 0.f, dep = 0.f, ac = 0.f, ao[NOBJ];
#pragma unroll
  for (int k = 0; k < NOBJ; ++k) ao[k] = 0.0f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = j0 + i;
    wv[i] = 0.0f;
    if (i < run && j < S) {
      const float trans = expf(-static_cast<float>(prefix));
      const float alpha = __fsub_rn(1.0f, expf(-sd[i]));
      const float w = __fmul_rn(alpha, trans);
      // no active object: no colour; one: its colour as it is; more: the density-weighted mean
      float c0 = lone[i][0], c1 = lone[i][1], c2 = lone[i][2];
      if (cnt[i] > 1) {
        c0 = __fdiv_rn(num[i][0], sig[i]);
        c1 = __fdiv_rn(num[i][1], sig[i]);
        c2 = __fdiv_rn(num[i][2], sig[i]);
      }
      cr += w * c0;
      cg += w * c1;
      cb += w * c2;
      dep += w * zz[i];
      ac += w;
      wv[i] = w;
#pragma unroll
      for (int k = 0; k < NOBJ; ++k) {
        const float share = sk[k][i] != 0.0f ? (cnt[i] > 1 ? __fdiv_rn(sk[k][i], sig[i]) : 1.0f) : 0.0f;
        ao[k] += w * share;
      }
      if (j + 1 < S) prefix += static_cast<double>(sd[i]);
    }
  }
  if (weights) store_run_weights<K>(weights, r, j0, run, S_in, S, wv);
  cr = ray_sum<L>(cr);
  cg = ray_sum<L>(cg);
  cb = ray_sum<L>(cb);
  dep = ray_sum<L>(dep);
  ac = ray_sum<L>(ac);
#pragma unroll
  for (int k = 0; k < NOBJ; ++k) ao[k] = ray_sum<L>(ao[k]);
  if (sub == (L == 16 ? 15 : 63)) {
    store_ray_maps(r, cr, cg, cb, dep, ac, rgb, disp, acc, depth);
    if (acc_objects) {
#pragma unroll
      for (int k = 0; k < NOBJ; ++k)
        if (k < n_objects) acc_objects[k * n_rays + r] = ao[k];
    }
  }
}

template <int NOBJ, bool SCALED>
void launch_compose(const ComposeRaws& raws, const ComposeScales& scales, int n_objects, const float* z, const float* rd,
                    int64_t n_rays, int S, float* rgb, float* disp, float* acc, float* weights, float* depth,
                    float* acc_objects, hipStream_t stream) {
  const dim3 g16(static_cast<unsigned>(cn::ceil_div(n_rays, 16))), g64(static_cast<unsigned>(cn::ceil_div(n_rays, 4)));
#define CN_COMPOSE_LAUNCH(K, L, GRID)                                                                         \
  hipLaunchKernelGGL((volume_render_compose_kernel<K, L, NOBJ, SCALED>), GRID, dim3(256), 0, stream, raws, scales, \
                     n_objects, z, rd, n_rays, S, rgb, disp, acc, weights, depth, acc_objects)
  if (S <= 64) CN_COMPOSE_LAUNCH(4, 16, g16);
  else if (S <= 128) CN_COMPOSE_LAUNCH(8, 16, g16);
  else if (S <= 256) CN_COMPOSE_LAUNCH(4, 64, g64);
  else CN_COMPOSE_LAUNCH(8, 64, g64);
#undef CN_COMPOSE_LAUNCH
}

// The two entries' body: scales NULL is the unscaled entry.
int compose_entry(const float* const* raws, const float* scales, bool scaled, int n_objects, const float* z,
                  const float* rd, int64_t n_rays, int64_t n_samples, float* rgb, float* disp, float* acc,
                  float* weights, float* depth, float* acc_objects, cn_stream_t stream) {
  CN_CHECK_ARG(raws && z && rd && rgb && disp && acc && depth && (scales || !scaled));
  CN_CHECK_ARG(n_objects >= 1 && n_objects <= CN_MAX_SCENE_OBJECTS);
  CN_CHECK_ARG(n_rays > 0 && n_samples > 0 && n_samples <= kMaxSamples);
  CN_CHECK_ARG(cn::aligned16(z) && cn::aligned16(weights));
  ComposeRaws p = {};
  ComposeScales sc = {};
  for (int k = 0; k < n_objects; ++k) {
    CN_CHECK_ARG(raws[k] && cn::aligned16(raws[k]));
    p.p[k] = raws[k];
  }
  if (scaled) CN_CHECK_ARG(read_scales(scales, n_objects, sc));
  const int s = static_cast<int>(n_samples);
  hipStream_t st = cn::as_stream(stream);
#define CN_COMPOSE(NOBJ)                                                                                              \
  do {                                                                                                                \
    if (scaled) launch_compose<NOBJ, true>(p, sc, n_objects, z, rd, n_rays, s, rgb, disp, acc, weights, depth, acc_objects, st); \
    else launch_compose<NOBJ, false>(p, sc, n_objects, z, rd, n_rays, s, rgb, disp, acc, weights, depth, acc_objects, st);       \
  } while (0)
  // the object count's compile-time bound: 1, 2, 4 or 8
  if (n_objects == 1) CN_COMPOSE(1);
  else if (n_objects == 2) CN_COMPOSE(2);
  else if (n_objects <= 4) CN_COMPOSE(4);
  else CN_COMPOSE(8);
#undef CN_COMPOSE
  return cn::launch_status();
}

}  // namespace

extern "C" int cn_volume_render_compose(const float* const* raws, int n_objects, const float* z, const float* rd,
                                        int64_t n_rays, int64_t n_samples, float* rgb, float* disp, float* acc,
                                        float* weights, float* depth, float* acc_objects, cn_stream_t stream) {
  return compose_entry(raws, nullptr, false, n_objects, z, rd, n_rays, n_samples, rgb, disp, acc, weights, depth,
                       acc_objects, stream);
}

extern "C" int cn_volume_render_compose_scaled(const float* const* raws, const float* scales, int n_objects,
                                               const float* z, const float* rd, int64_t n_rays, int64_t n_samples,
                                               float* rgb, float* disp, float* acc, float* weights, float* depth,
                                               float* acc_objects, cn_stream_t stream) {
  return compose_entry(raws, scales, true, n_objects, z, rd, n_rays, n_samples, rgb, disp, acc, weights, depth,
                       acc_objects, stream);
}

// ---------------------------------------------------------------- backward
// Gradient of volume_render (volumetric_render.py:36-66) w.r.t. raw and rd.
// With sd_i = sigma_i delta_i, T_i = exp(-sum_{j<i} sd_j), w_i = (1 - e^{-sd_i}) T_i:
//   G_i = g_w_i + g_rgb . c_i + g_depth z_i + g_acc          (dL/dw_i)
//   dL/dsd_i = G_i T_i e^{-sd_i} - sum_{j>i} G_j w_j          (reverse ray scan)
//   d raw_i[0:3] = w_i g_rgb 1.002 s(1-s);  d raw_i[3] = dL/dsd_i delta_i softplus'(raw_i[3]-1)
//   d rd = (sum_i dL/dsd_i sigma_i dist_i) rd/|rd|
// g_disp folds into g_depth / g_acc through disp = 1/max(1e-10, depth/acc).
// z is never differentiated (the reference detaches its samples).  Same layout as the forward.
namespace {

// The device arithmetic volume_render_backward_kernel and volume_render_compose_backward_kernel share: every
// function is the plain kernel's own expressions (the build does not contract, so the bits are its bits).

// The forward's weights again, from this lane's run of densities sig (0 outside the run): dist, sd, the
// transmittances tr, the weights w, and the ray's depth / acc in every lane of the ray.
template <int K, int L>
__device__ __forceinline__ void backward_weights(const float (&zz)[K], const float (&sig)[K], int S, int run, int j0,
                                                 float nrm, float (&dist)[K], float (&sd)[K], float (&w)[K],
                                                 float (&tr)[K], float& dep_out, float& ac_out) {
  const float znext = next_lane<L>(zz[0]);
  double run_sum = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = j0 + i;
    sd[i] = 0.0f;
    dist[i] = 0.0f;
    if (i < run && j < S) {
      const float zn = (i + 1 < run) ? zz[(i + 1) % K] : znext;
      dist[i] = (j + 1 < S) ? __fsub_rn(zn, zz[i]) : 1e10f;
      sd[i] = __fmul_rn(sig[i], __fmul_rn(dist[i], nrm));
      if (j + 1 < S) run_sum += static_cast<double>(sd[i]);
    }
  }
  double prefix = ray_exclusive_scan<L>(run_sum);
  float dep = 0.f, ac = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = j0 + i;
    w[i] = 0.0f;
    tr[i] = 0.0f;
    if (i < run && j < S) {
      tr[i] = expf(-static_cast<float>(prefix));
      w[i] = __fmul_rn(__fsub_rn(1.0f, expf(-sd[i])), tr[i]);
      dep += w[i] * zz[i];
      ac += w[i];
      if (j + 1 < S) prefix += static_cast<double>(sd[i]);
    }
  }
  dep_out = ray_sum_all<L>(dep);
  ac_out = ray_sum_all<L>(ac);
}

// The ray's upstream gradients (a NULL one is zero), g_disp folded into g_depth / g_acc.
struct RayGrads {
  float r0, r1, r2, dep, acc;
};
__device__ __forceinline__ RayGrads ray_grads(int64_t r, float dep, float ac, const float* __restrict__ g_rgb,
                                              const float* __restrict__ g_disp, const float* __restrict__ g_acc,
                                              const float* __restrict__ g_depth) {
  RayGrads g;
  g.r0 = g_rgb ? g_rgb[3 * r] : 0.f;
  g.r1 = g_rgb ? g_rgb[3 * r + 1] : 0.f;
  g.r2 = g_rgb ? g_rgb[3 * r + 2] : 0.f;
  g.dep = g_depth ? g_depth[r] : 0.f;
  g.acc = g_acc ? g_acc[r] : 0.f;
  if (g_disp) {
    const float q = dep / ac;
    if (q > 1e-10f) {  // d(1/q)/dq = -1/q^2; below the clamp torch routes the gradient to the constant
      const float gq = -g_disp[r] / (q * q);
      g.dep += gq / ac;
      g.acc += gq * (-dep / (ac * ac));
    }
  }
  return g;
}

// G = dL/dw of a sample of colour (c0, c1, c2) at depth zv with weight gradient gw.
__device__ __forceinline__ float weight_grad(const RayGrads& g, float c0, float c1, float c2, float zv, float gw) {
  return g.r0 * c0 + g.r1 * c1 + g.r2 * c2 + g.dep * zv + g.acc + gw;
}

// d raw colour channel from the channel's sigmoid s: w g 1.002 s (1 - s).
__device__ __forceinline__ float colour_grad(float w, float g, float s) { return w * g * 1.002f * s * (1.0f - s); }

// softplus20'(x - 1) of a raw density x.
__device__ __forceinline__ float sigma_slope(float xs) {
  const float x = xs - 1.0f;
  return x > 20.0f ? 1.0f : cn::sigmoid_hw(x);
}

// dL/dsd per sample from G (the reverse ray scan), and this lane's part of sum dL/dsd sigma dist.
template <int K, int L>
__device__ __forceinline__ void backward_dsd(const float (&G)[K], const float (&w)[K], const float (&tr)[K],
                                             const float (&sd)[K], const float (&sig)[K], const float (&dist)[K], int S,
                                             int run, int j0, float (&dsd)[K], float& gnorm_out) {
  float gw_run = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i)
    if (i < run && j0 + i < S) gw_run += G[i] * w[i];
  float suffix = ray_exclusive_suffix<L>(gw_run);  // sum of G_j w_j over later lanes' runs
  float gnorm = 0.f;
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    dsd[i] = 0.0f;
    if (i < run && j0 + i < S) {
      dsd[i] = G[i] * tr[i] * expf(-sd[i]) - suffix;
      suffix += G[i] * w[i];
      gnorm += dsd[i] * sig[i] * dist[i];
    }
  }
  gnorm_out = gnorm;
}

// d rd = (sum dL/dsd sigma dist) rd / |rd| from the lane that holds the ray's sum: one writer per ray.
__device__ __forceinline__ void store_d_rd(float* __restrict__ d_rd, int64_t r, float gnorm, float nrm, float d0,
                                           float d1, float d2, int accumulate_rd) {
  const float inv = nrm > 0.f ? gnorm / nrm : 0.f;
  if (accumulate_rd) {      // the caller's running sum of the ray's gradients
    d_rd[3 * r] += inv * d0;
    d_rd[3 * r + 1] += inv * d1;
    d_rd[3 * r + 2] += inv * d2;
  } else {
    d_rd[3 * r] = inv * d0;
    d_rd[3 * r + 1] = inv * d1;
    d_rd[3 * r + 2] = inv * d2;
  }
}

template <int K, bool FULL, int L>
__global__ __launch_bounds__(256) void volume_render_backward_kernel(
    const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rd,
    int64_t n_rays, int S_in, const float* __restrict__ g_rgb, const float* __restrict__ g_disp,
    const float* __restrict__ g_acc, const float* __restrict__ g_w, const float* __restrict__ g_depth,
    float* __restrict__ d_raw, float* __restrict__ d_rd, int accumulate_rd) {
  static_assert(K <= kMaxRun && (L == 16 || L == 64) && (!FULL || L == 16), "instance");
  if (FULL) S_in = L * K;  // as in the forward
  __shared__ float4 slds[4 * 80 * K];  // per wave: raw in, then d raw out (forward's layout)
  const int sub = threadIdx.x & (L - 1), lane = threadIdx.x & 63;
  const int64_t r_ = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int64_t rw0 = r_ - lane / L;
  if (rw0 >= n_rays) return;  // the whole wave
  const int nq = static_cast<int>(min<int64_t>(64 / L, n_rays - rw0)) * S_in;  // the wave's valid quads
  float4* sl = slds + (threadIdx.x >> 6) * 80 * K;
  stage_rows_in<K>(reinterpret_cast<const float4*>(raw) + rw0 * S_in, nq, sl, lane);
  __builtin_amdgcn_wave_barrier();  // cross-lane LDS reads follow (see the forward)
  // a ray past n_rays (L = 16 only) stays alive as a copy of the last ray, nothing stored, so the
  // wave's coalesced d raw copy-out runs in every lane
  const bool live = r_ < n_rays;
  const int64_t r = live ? r_ : n_rays - 1;
  const int S = FULL ? L * K : (S_in == 1 ? 0 : S_in);  // see the forward: S == 1 has no contributing sample
  const int run = FULL ? K : (S_in + L - 1) / L;
  const int j0 = sub * run;
  const float* zr = z + r * S_in;
  const float4* rr = reinterpret_cast<const float4*>(raw) + r * S_in;
  const float d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
  const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));

  float sd[K], zz[K], dist[K], sig[K], w[K], tr[K];
  float4 rv[K];
  const int q0 = (lane / L) * S_in + j0;  // this run's first quad in the wave block
  load_depths<K>(zr, j0, run, S_in, zz);
  if (live) load_raw_lds<K>(sl, q0, j0, run, S_in, rv);
  else load_run<K>(zr, rr, j0, run, S_in, zz, rv);  // the last ray again (not in this wave's block)
#pragma unroll
  for (int i = 0; i < K; ++i) sig[i] = (i < run && j0 + i < S) ? raw_sigma(rv[i].w) : 0.0f;
  float dep, ac;
  backward_weights<K, L>(zz, sig, S, run, j0, nrm, dist, sd, w, tr, dep, ac);
  const RayGrads g = ray_grads(r, dep, ac, g_rgb, g_disp, g_acc, g_depth);
  // G_i and the per-sample colour gradients
  float G[K], dsd[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = j0 + i;
    G[i] = 0.0f;
    if (i < run && j < S) {
      const float s0 = cn::sigmoid_hw(rv[i].x), s1 = cn::sigmoid_hw(rv[i].y), s2 = cn::sigmoid_hw(rv[i].z);
      const float c0 = s0 * 1.002f - 0.001f, c1 = s1 * 1.002f - 0.001f, c2 = s2 * 1.002f - 0.001f;
      G[i] = weight_grad(g, c0, c1, c2, zz[i], g_w ? g_w[r * S_in + j] : 0.f);
      rv[i].x = colour_grad(w[i], g.r0, s0);  // reuse rv for d_raw[0:3]
      rv[i].y = colour_grad(w[i], g.r1, s1);
      rv[i].z = colour_grad(w[i], g.r2, s2);
    }
  }
  float gnorm;
  backward_dsd<K, L>(G, w, tr, sd, sig, dist, S, run, j0, dsd, gnorm);
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    const int j = j0 + i;
    if (i < run && j < S) {
      float4 o = rv[i];
      o.w = dsd[i] * (dist[i] * nrm) * sigma_slope(rv[i].w);
      if (live) sl[pad4(q0 + i)] = o;
    } else if (i < run && j < S_in) {
      if (live) sl[pad4(q0 + i)] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __builtin_amdgcn_wave_barrier();  // the copy-out reads quads other lanes wrote
  stage_rows_out<K>(reinterpret_cast<float4*>(d_raw) + rw0 * S_in, nq, sl, lane);
  gnorm = ray_sum<L>(gnorm);
  if (live && sub == (L == 16 ? 15 : 63) && d_rd) store_d_rd(d_rd, r, gnorm, nrm, d0, d1, d2, accumulate_rd);
}

}  // namespace

extern "C" int cn_volume_render_backward(const float* raw, const float* z, const float* rd,
                                         int64_t n_rays, int64_t n_samples, const float* g_rgb,
                                         const float* g_disp, const float* g_acc,
                                         const float* g_weights, const float* g_depth,
                                         float* d_raw, float* d_rd, int accumulate_rd, cn_stream_t stream) {
  CN_CHECK_ARG(raw && z && rd && d_raw && (accumulate_rd == 0 || accumulate_rd == 1));
  CN_CHECK_ARG(n_rays > 0 && n_samples > 0 && n_samples <= kMaxSamples);
  CN_CHECK_ARG(cn::aligned16(raw) && cn::aligned16(z) && cn::aligned16(d_raw));
  CN_VOLUME_DISPATCH(volume_render_backward_kernel, n_samples, n_rays, cn::as_stream(stream), raw, z, rd, n_rays,
                     static_cast<int>(n_samples), g_rgb, g_disp, g_acc, g_weights, g_depth, d_raw, d_rd,
                     accumulate_rd);
  return cn::launch_status();
}

// ---------------------------------------------------------------- scene composition, backward
// Gradient of cn_volume_render_compose w.r.t. every object's raw rows and rd (the rule is in
// include/codenerf.h): the composition read as real functions, every sample's active set held fixed.  The
// forward's geometry.  Pass 1 stages each object's rows in turn and keeps, per sample, the summed density, the
// colour numerator, the count of active objects, the last active colour and (with g_acc_objects) the
// density-weighted sum of the objects' mask gradients; then the plain backward's arithmetic on the summed
// density and the mixed colour gives dL/dsd; pass 2 stages each object's rows again, recomputes its density
// and colours (nothing per object stays in registers between the passes) and sends its d raw rows out through
// the same LDS block.  With one active object at a sample its row gets volume_render_backward_kernel's bits.
// Algorithmic bytes per ray: 12 (rd) + (32 n_objects + 4) S in, 16 n_objects S + 12 out, plus the upstream rows.
namespace {

struct ComposeGrads {
  float* p[CN_MAX_SCENE_OBJECTS];
};

// SCALED (cn_volume_render_compose_scaled_backward): the density is softplus20(xs - 1) / s_k, the density's
// gradient goes back through that division, and with scale_partials every wave leaves, per object, its sum of
// -d sigma_k sigma_k / s_k at scale_partials[k * n_waves + wave] (n_waves = the waves that hold a ray): lanes in
// the row tree's order, the rows ascending, no atomics.
template <int K, int L, int NOBJ, bool SCALED>
__global__ __launch_bounds__(256) void volume_render_compose_backward_kernel(
    ComposeRaws raws, ComposeScales scales, int n_objects, const float* __restrict__ z, const float* __restrict__ rd,
    int64_t n_rays, int S_in, const float* __restrict__ g_rgb, const float* __restrict__ g_disp,
    const float* __restrict__ g_acc, const float* __restrict__ g_w, const float* __restrict__ g_depth,
    const float* __restrict__ g_ao, ComposeGrads d_raws, float* __restrict__ d_rd, int accumulate_rd,
    float* __restrict__ scale_partials) {
  static_assert(K <= kMaxRun && (L == 16 || L == 64) && NOBJ >= 1 && NOBJ <= CN_MAX_SCENE_OBJECTS, "instance");
  __shared__ float4 slds[4 * 80 * K];  // per wave: one object's rows in, then its d raw rows out
  const int sub = threadIdx.x & (L - 1), lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int64_t rw0 = r - lane / L;  // the wave's first ray
  if (rw0 >= n_rays) return;         // the whole wave
  const int nq = static_cast<int>(min<int64_t>(64 / L, n_rays - rw0)) * S_in;  // the wave's valid quads
  float4* sl = slds + (threadIdx.x >> 6) * 80 * K;
  // a ray past n_rays (L = 16 only) takes part in the wave's copies alone: whole rows of 16 lanes skip the
  // arithmetic together, so no cross-lane step reads one
  const bool live = r < n_rays;
  const int S = S_in == 1 ? 0 : S_in;  // see render_run: S == 1 has no contributing sample
  const int run = (S_in + L - 1) / L;
  const int j0 = sub * run;
  const int q0 = (lane / L) * S_in + j0;  // this run's first quad in the wave block
  float zz[K];
  float nrm = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
#pragma unroll
  for (int i = 0; i < K; ++i) zz[i] = 0.0f;
  if (live) {
    load_depths<K>(z + r * S_in, j0, run, S_in, zz);
    d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
    nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
  }
  float gao[NOBJ];  // the ray's mask gradients
#pragma unroll
  for (int k = 0; k < NOBJ; ++k) gao[k] = (g_ao && live && k < n_objects) ? g_ao[k * n_rays + r] : 0.0f;

  // pass 1: the forward's mix
  float sig[K], num[K][3], lone[K][3], aon[K], alone[K];
  int cnt[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    sig[i] = aon[i] = alone[i] = 0.0f;
    cnt[i] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) num[i][c] = lone[i][c] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < NOBJ; ++k) {
    if (k >= n_objects) continue;  // uniform
    __builtin_amdgcn_wave_barrier();  // (see the forward)
    stage_rows_in<K>(reinterpret_cast<const float4*>(raws.p[k]) + rw0 * S_in, nq, sl, lane);
    __builtin_amdgcn_wave_barrier();
    if (!live) continue;
    float4 rv[K];
    load_raw_lds<K>(sl, q0, j0, run, S_in, rv);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if (i < run && j0 + i < S) {
        const float s = object_sigma<SCALED>(rv[i].w, scales.s[k]);
        sig[i] = __fadd_rn(sig[i], s);
        if (s != 0.0f) {  // active (a NaN density is)
          const float c0 = raw_colour(rv[i].x), c1 = raw_colour(rv[i].y), c2 = raw_colour(rv[i].z);
          cnt[i] += 1;
          lone[i][0] = c0;
          lone[i][1] = c1;
          lone[i][2] = c2;
          num[i][0] = __fadd_rn(num[i][0], __fmul_rn(s, c0));
          num[i][1] = __fadd_rn(num[i][1], __fmul_rn(s, c1));
          num[i][2] = __fadd_rn(num[i][2], __fmul_rn(s, c2));
          alone[i] = gao[k];
          aon[i] += gao[k] * s;
        }
      }
    }
  }

  // dL/dsd from the summed density and the mixed colour: the plain backward's arithmetic
  float dist[K], w[K], dsd[K];
  float gnorm = 0.0f;
  RayGrads g = {};
#pragma unroll
  for (int i = 0; i < K; ++i) dist[i] = w[i] = dsd[i] = 0.0f;
  if (live) {
    float sd[K], tr[K], G[K];
    float dep, ac;
    backward_weights<K, L>(zz, sig, S, run, j0, nrm, dist, sd, w, tr, dep, ac);
    g = ray_grads(r, dep, ac, g_rgb, g_disp, g_acc, g_depth);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int j = j0 + i;
      G[i] = 0.0f;
      if (i < run && j < S) {
        // the mixed colour, kept in lone for pass 2; sum_k g_acc_objects[k] share_k in alone
        if (cnt[i] > 1) {
          lone[i][0] = __fdiv_rn(num[i][0], sig[i]);
          lone[i][1] = __fdiv_rn(num[i][1], sig[i]);
          lone[i][2] = __fdiv_rn(num[i][2], sig[i]);
          alone[i] = aon[i] / sig[i];
        }
        G[i] = weight_grad(g, lone[i][0], lone[i][1], lone[i][2], zz[i], g_w ? g_w[r * S_in + j] : 0.f);
        if (g_ao) G[i] += alone[i];
      }
    }
    backward_dsd<K, L>(G, w, tr, sd, sig, dist, S, run, j0, dsd, gnorm);
    gnorm = ray_sum<L>(gnorm);
    if (sub == (L == 16 ? 15 : 63) && d_rd) store_d_rd(d_rd, r, gnorm, nrm, d0, d1, d2, accumulate_rd);
  }

  // pass 2: every object's d raw rows
#pragma unroll
  for (int k = 0; k < NOBJ; ++k) {
    if (k >= n_objects) continue;  // uniform
    __builtin_amdgcn_wave_barrier();  // the previous object's copy-out reads stay ahead of these stores
    stage_rows_in<K>(reinterpret_cast<const float4*>(raws.p[k]) + rw0 * S_in, nq, sl, lane);
    __builtin_amdgcn_wave_barrier();
    float dscale = 0.0f;  // SCALED: this lane's part of d_scales[k]
    if (live) {
      float4 rv[K];
      load_raw_lds<K>(sl, q0, j0, run, S_in, rv);
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const int j = j0 + i;
        if (!(i < run && j < S_in)) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);  // an inactive object's row, and the sample-free S_in == 1
        const float s = j < S ? object_sigma<SCALED>(rv[i].w, scales.s[k]) : 0.0f;
        if (s != 0.0f) {
          const float s0 = cn::sigmoid_hw(rv[i].x), s1 = cn::sigmoid_hw(rv[i].y), s2 = cn::sigmoid_hw(rv[i].z);
          if (cnt[i] > 1) {
            const float share = __fdiv_rn(s, sig[i]), ws = w[i] * share;
            const float c0 = s0 * 1.002f - 0.001f, c1 = s1 * 1.002f - 0.001f, c2 = s2 * 1.002f - 0.001f;
            o.x = colour_grad(ws, g.r0, s0);
            o.y = colour_grad(ws, g.r1, s1);
            o.z = colour_grad(ws, g.r2, s2);
            // through the mixed colour and the shares: w (g_rgb . (c_k - c) + g_ao[k] - sum_j g_ao[j] share_j) / sigma
            float mixg = g.r0 * (c0 - lone[i][0]) + g.r1 * (c1 - lone[i][1]) + g.r2 * (c2 - lone[i][2]);
            if (g_ao) mixg += gao[k] - alone[i];
            const float dsig = dsd[i] * (dist[i] * nrm) + w[i] * mixg / sig[i];
            o.w = dsig * sigma_slope(rv[i].w);
            if constexpr (SCALED) dscale -= dsig * s / scales.s[k];
          } else {  // the only active object: the plain backward's row
            o.x = colour_grad(w[i], g.r0, s0);
            o.y = colour_grad(w[i], g.r1, s1);
            o.z = colour_grad(w[i], g.r2, s2);
            const float dsig = dsd[i] * (dist[i] * nrm);
            o.w = dsig * sigma_slope(rv[i].w);
            if constexpr (SCALED) dscale -= dsig * s / scales.s[k];
          }
          if constexpr (SCALED) o.w = o.w / scales.s[k];
        }
        sl[pad4(q0 + i)] = o;
      }
    }
    __builtin_amdgcn_wave_barrier();  // the copy-out reads quads other lanes wrote
    stage_rows_out<K>(reinterpret_cast<float4*>(d_raws.p[k]) + rw0 * S_in, nq, sl, lane);
    if constexpr (SCALED) {
      if (scale_partials) {  // uniform; every lane of the wave is here (a ray past n_rays holds 0)
        const float t = ray_sum<64>(dscale);
        const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        const int64_t n_waves = (n_rays + (64 / L - 1)) / (64 / L);
        if (lane == 63) scale_partials[k * n_waves + wave] = t;
      }
    }
  }
}

// d_scales[k] from the waves' partials, one block per object: lane t sums partials t, t + 256, ... in ascending
// order, then a fixed tree over the block's lanes.
__global__ __launch_bounds__(256) void compose_scales_reduce_kernel(const float* __restrict__ partials, int64_t n_waves,
                                                                    float* __restrict__ d_scales) {
  __shared__ float red[256];
  const int k = blockIdx.x;
  float acc = 0.0f;
  for (int64_t b = threadIdx.x; b < n_waves; b += 256) acc += partials[k * n_waves + b];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) d_scales[k] = red[0];
}

// The waves that hold a ray: cn_volume_render_compose_scaled_backward's partials per object.
inline int64_t compose_waves(int64_t n_rays, int64_t n_samples) {
  return cn::ceil_div(n_rays, (int64_t)(n_samples <= 128 ? 4 : 1));
}

template <int NOBJ, bool SCALED>
void launch_compose_backward(const ComposeRaws& raws, const ComposeScales& scales, int n_objects, const float* z,
                             const float* rd, int64_t n_rays, int S, const float* g_rgb, const float* g_disp,
                             const float* g_acc, const float* g_w, const float* g_depth, const float* g_ao,
                             const ComposeGrads& d_raws, float* d_rd, int accumulate_rd, float* scale_partials,
                             hipStream_t stream) {
  const dim3 g16(static_cast<unsigned>(cn::ceil_div(n_rays, 16))), g64(static_cast<unsigned>(cn::ceil_div(n_rays, 4)));
#define CN_COMPOSE_BWD_LAUNCH(K, L, GRID)                                                                            \
  hipLaunchKernelGGL((volume_render_compose_backward_kernel<K, L, NOBJ, SCALED>), GRID, dim3(256), 0, stream, raws,   \
                     scales, n_objects, z, rd, n_rays, S, g_rgb, g_disp, g_acc, g_w, g_depth, g_ao, d_raws, d_rd,      \
                     accumulate_rd, scale_partials)
  if (S <= 64) CN_COMPOSE_BWD_LAUNCH(4, 16, g16);
  else if (S <= 128) CN_COMPOSE_BWD_LAUNCH(8, 16, g16);
  else if (S <= 256) CN_COMPOSE_BWD_LAUNCH(4, 64, g64);
  else CN_COMPOSE_BWD_LAUNCH(8, 64, g64);
#undef CN_COMPOSE_BWD_LAUNCH
}

// The two entries' body: scaled false is the unscaled entry (no scales, d_scales or workspace).
int compose_backward_entry(const float* const* raws, const float* scales, bool scaled, int n_objects, const float* z,
                           const float* rd, int64_t n_rays, int64_t n_samples, const float* g_rgb, const float* g_disp,
                           const float* g_acc, const float* g_weights, const float* g_depth, const float* g_acc_objects,
                           float* const* d_raws, float* d_rd, int accumulate_rd, float* d_scales, float* workspace,
                           cn_stream_t stream) {
  CN_CHECK_ARG(raws && d_raws && z && rd && (accumulate_rd == 0 || accumulate_rd == 1) && (scales || !scaled));
  CN_CHECK_ARG(n_objects >= 1 && n_objects <= CN_MAX_SCENE_OBJECTS);
  CN_CHECK_ARG(n_rays > 0 && n_samples > 0 && n_samples <= kMaxSamples);
  CN_CHECK_ARG(cn::aligned16(z) && (!d_scales || workspace));
  ComposeRaws p = {};
  ComposeGrads d = {};
  ComposeScales sc = {};
  for (int k = 0; k < n_objects; ++k) {
    CN_CHECK_ARG(raws[k] && cn::aligned16(raws[k]) && d_raws[k] && cn::aligned16(d_raws[k]));
    p.p[k] = raws[k];
    d.p[k] = d_raws[k];
  }
  if (scaled) CN_CHECK_ARG(read_scales(scales, n_objects, sc));
  const int s = static_cast<int>(n_samples);
  hipStream_t st = cn::as_stream(stream);
  float* partials = d_scales ? workspace : nullptr;
#define CN_COMPOSE_BWD(NOBJ)                                                                                          \
  do {                                                                                                                \
    if (scaled)                                                                                                       \
      launch_compose_backward<NOBJ, true>(p, sc, n_objects, z, rd, n_rays, s, g_rgb, g_disp, g_acc, g_weights, g_depth, \
                                          g_acc_objects, d, d_rd, accumulate_rd, partials, st);                       \
    else                                                                                                              \
      launch_compose_backward<NOBJ, false>(p, sc, n_objects, z, rd, n_rays, s, g_rgb, g_disp, g_acc, g_weights, g_depth, \
                                           g_acc_objects, d, d_rd, accumulate_rd, nullptr, st);                       \
  } while (0)
  // the object count's compile-time bound, as the forward
  if (n_objects == 1) CN_COMPOSE_BWD(1);
  else if (n_objects == 2) CN_COMPOSE_BWD(2);
  else if (n_objects <= 4) CN_COMPOSE_BWD(4);
  else CN_COMPOSE_BWD(8);
#undef CN_COMPOSE_BWD
  if (partials)
    hipLaunchKernelGGL(compose_scales_reduce_kernel, dim3(n_objects), dim3(256), 0, st, partials,
                       compose_waves(n_rays, n_samples), d_scales);
  return cn::launch_status();
}

}  // namespace

extern "C" int cn_volume_render_compose_backward(const float* const* raws, int n_objects, const float* z,
                                                 const float* rd, int64_t n_rays, int64_t n_samples,
                                                 const float* g_rgb, const float* g_disp, const float* g_acc,
                                                 const float* g_weights, const float* g_depth,
                                                 const float* g_acc_objects, float* const* d_raws, float* d_rd,
                                                 int accumulate_rd, cn_stream_t stream) {
  return compose_backward_entry(raws, nullptr, false, n_objects, z, rd, n_rays, n_samples, g_rgb, g_disp, g_acc,
                                g_weights, g_depth, g_acc_objects, d_raws, d_rd, accumulate_rd, nullptr, nullptr, stream);
}

extern "C" int64_t cn_volume_render_compose_scaled_backward_workspace_floats(int64_t n_rays, int64_t n_samples,
                                                                             int n_objects) {
  if (n_rays <= 0 || n_samples <= 0 || n_samples > kMaxSamples || n_objects < 1 || n_objects > CN_MAX_SCENE_OBJECTS)
    return -1;
  return compose_waves(n_rays, n_samples) * n_objects;
}

extern "C" int cn_volume_render_compose_scaled_backward(const float* const* raws, const float* scales, int n_objects,
                                                        const float* z, const float* rd, int64_t n_rays,
                                                        int64_t n_samples, const float* g_rgb, const float* g_disp,
                                                        const float* g_acc, const float* g_weights,
                                                        const float* g_depth, const float* g_acc_objects,
                                                        float* const* d_raws, float* d_rd, int accumulate_rd,
                                                        float* d_scales, float* workspace, cn_stream_t stream) {
  return compose_backward_entry(raws, scales, true, n_objects, z, rd, n_rays, n_samples, g_rgb, g_disp, g_acc,
                                g_weights, g_depth, g_acc_objects, d_raws, d_rd, accumulate_rd, d_scales, workspace,
                                stream);
}
