// Occupancy-grid sample culling for the inference render.
//
// A grid is G^3 cells over the cube [-bound, bound]^3, one bit per cell: cell (ix, iy, iz) is bit
// c & 31 of 32-bit word c >> 5, c = (ix G + iy) G + iz.  Three passes around the unchanged field
// kernels:
//   build   node densities -> the bit words (a wave's ballot is two words);
//   cull    every ray sample looked up; the kept ones compacted, in ascending sample order, into
//           (point, Q1 view-direction row, code row) triples -- a points-mode input of the field
//           kernels with n_samples = 1 -- and the kept masks / ray offsets left in a workspace;
//   expand  the compact (M', 4) result gathered back to (R, S, 4), culled slots the empty row.
// All three are bandwidth / latency bound: one wave per ray, ballots and mbcnt ranks, no atomics, so
// the compact order (and with it every output) is deterministic.
//
// Weight-bounded colour culling (cn_weight_cull, cn_scatter_rgb) reuses passes 2 and 3 and the
// workspace: its pass 1 decides from a ray's volume-render weights instead of a grid, and the
// compact field result goes back through a colours-only scatter instead of the expand.
#include <limits.h>

#include "cn_common.h"

namespace {

constexpr int kMaxSamples = 512;           // as cn_volume_render
constexpr int kRayWaves = 4;               // rays (waves) per 256-thread block
constexpr int kScanThreads = 1024;
constexpr int kScanPerThread = 4;
constexpr int kScanPart = kScanThreads * kScanPerThread;   // rays per scan partition (4096)

__host__ __device__ inline int64_t mask_words(int64_t n_samples) { return (n_samples + 63) / 64; }

// Workspace: the rays' exclusive kept-sample offsets (int32, padded to 16 B), then their kept masks
// (mask_words(S) 64-bit words per ray, bit s & 63 of word s >> 6).
__host__ __device__ inline int64_t offsets_bytes(int64_t n_rays) { return (n_rays * 4 + 15) / 16 * 16; }

inline bool sizes_ok(int64_t n_rays, int64_t n_samples) {
  return n_rays > 0 && n_samples >= 1 && n_samples <= kMaxSamples && n_rays <= INT_MAX / n_samples;
}

// Lanes of this wave below the caller's whose bit is set in m.
__device__ __forceinline__ int rank_below(unsigned long long m) {
  return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u)));
}

// One thread per cell, c = its global index, so a wave's ballot is words c >> 5 and (c >> 5) + 1
// (G^3 is a multiple of 64: no partial wave).  Occupied: any node of [i - d, i + 1 + d]^3 (clamped
// to the node grid) above the threshold, or NaN.
__global__ __launch_bounds__(256) void occupancy_build_kernel(const float* __restrict__ nodes, int g, float threshold,
                                                              int dilate, unsigned* __restrict__ bits) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  const int iz = static_cast<int>(c % g), iy = static_cast<int>((c / g) % g), ix = static_cast<int>(c / (g * g));
  const int n = g + 1;
  const int x0 = max(ix - dilate, 0), x1 = min(ix + 1 + dilate, g);
  const int y0 = max(iy - dilate, 0), y1 = min(iy + 1 + dilate, g);
  const int z0 = max(iz - dilate, 0), z1 = min(iz + 1 + dilate, g);
  bool occ = false;
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) {
      const float* row = nodes + (static_cast<size_t>(x) * n + y) * n;
      for (int z = z0; z <= z1; ++z) {
        const float v = row[z];
        occ = occ || v > threshold || v != v;
      }
    }
  const unsigned long long b = __ballot(occ);
  const int lane = threadIdx.x & 63;
  if ((lane & 31) == 0) bits[c >> 5] = static_cast<unsigned>(b >> lane);
}

// Pass 1, one wave per ray: the kept mask of each 64 samples (a ballot) and the ray's kept count.
__global__ __launch_bounds__(64 * kRayWaves) void occupancy_mask_kernel(
    const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ z, int64_t n_rays, int n_samples,
    const unsigned* __restrict__ bits, int g, float lo, float inv_cell, int* __restrict__ counts,
    unsigned long long* __restrict__ masks) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRayWaves) + (threadIdx.x >> 6);
  if (r >= n_rays) return;                 // wave-uniform
  const float o0 = ro[3 * r], o1 = ro[3 * r + 1], o2 = ro[3 * r + 2];
  const float d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
  const int nw = static_cast<int>(mask_words(n_samples));
  int total = 0;
  for (int w = 0; w < nw; ++w) {
    const int s = 64 * w + lane;
    bool keep = false;
    if (s < n_samples) {
      const float zv = z[r * n_samples + s];
      keep = cn::occupied(bits, g, lo, inv_cell, cn::mul_add_rn(d0, zv, o0), cn::mul_add_rn(d1, zv, o1),
                      cn::mul_add_rn(d2, zv, o2));
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) masks[r * nw + w] = m;
    total += __popcll(m);
  }
  if (lane == 0) counts[r] = total;
}

// Pass 2, one workgroup: the ray counts -> their exclusive prefix sums, in place, a partition of
// kScanPart rays per round with the running total carried over; the grand total is M'.
__global__ __launch_bounds__(kScanThreads) void occupancy_scan_kernel(int* __restrict__ offsets, int64_t n_rays,
                                                                       int64_t* __restrict__ count) {
  __shared__ int s_wave[kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int64_t base = 0; base < n_rays; base += kScanPart) {
    const int64_t i0 = base + static_cast<int64_t>(tid) * kScanPerThread;
    int v[kScanPerThread];
    int t = 0;
#pragma unroll
    for (int q = 0; q < kScanPerThread; ++q) {
      v[q] = i0 + q < n_rays ? offsets[i0 + q] : 0;
      t += v[q];
    }
    int incl = t;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(incl, off);
      if (lane >= off) incl += u;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) {
      const int x = s_wave[k];
      before += k < wv ? x : 0;
      all += x;
    }
    int run = carry + before + incl - t;
#pragma unroll
    for (int q = 0; q < kScanPerThread; ++q) {
      if (i0 + q < n_rays) offsets[i0 + q] = run;
      run += v[q];
    }
    carry += all;
    __syncthreads();                       // s_wave is rewritten next round
  }
  if (tid == 0) count[0] = carry;
}

// Pass 3, one wave per ray: kept sample k goes to compact row offset[r] + (kept samples of the ray
// before it), an mbcnt rank: ascending k.
__global__ __launch_bounds__(64 * kRayWaves) void occupancy_emit_kernel(
    const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ z, int64_t n_rays, int n_samples,
    int64_t chunk_rows, const int64_t* __restrict__ code_index, const int* __restrict__ offsets,
    const unsigned long long* __restrict__ masks, int* __restrict__ sample_index, float* __restrict__ pts,
    float* __restrict__ vdir, int64_t* __restrict__ code_out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRayWaves) + (threadIdx.x >> 6);
  if (r >= n_rays) return;                 // wave-uniform
  const int nw = static_cast<int>(mask_words(n_samples));
  const float o0 = ro[3 * r], o1 = ro[3 * r + 1], o2 = ro[3 * r + 2];
  const float d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
  // Q1 (decode_sample, mlp_common.h): sample row k of a chunk takes the view direction of ray k mod Rc
  const int64_t base = (r / chunk_rows) * chunk_rows;
  const int64_t rcnt = min(chunk_rows, n_rays - base);
  const int64_t code = code_index ? code_index[r] : r;
  int64_t j0 = offsets[r];
  for (int w = 0; w < nw; ++w) {
    const unsigned long long m = masks[r * nw + w];
    const int s = 64 * w + lane;
    if ((m >> lane) & 1ull) {
      const int64_t j = j0 + rank_below(m);
      const float zv = z[r * n_samples + s];
      // (r - base) S + s <= r S + s < n_rays S <= INT_MAX (sizes_ok): a 32-bit remainder
      const int64_t dray = base + static_cast<unsigned>((r - base) * n_samples + s) % static_cast<unsigned>(rcnt);
      sample_index[j] = static_cast<int>(r * n_samples + s);
      pts[3 * j] = cn::mul_add_rn(d0, zv, o0);
      pts[3 * j + 1] = cn::mul_add_rn(d1, zv, o1);
      pts[3 * j + 2] = cn::mul_add_rn(d2, zv, o2);
      vdir[3 * j] = rd[3 * dray];
      vdir[3 * j + 1] = rd[3 * dray + 1];
      vdir[3 * j + 2] = rd[3 * dray + 2];
      if (code_out) code_out[j] = code;
    }
    j0 += __popcll(m);
  }
}

// The gather back, one wave per ray: a kept sample's compact row, else the empty row; one 16-B
// store per lane (1 KiB per wave instruction).
__global__ __launch_bounds__(64 * kRayWaves) void occupancy_expand_kernel(
    const float4* __restrict__ raw_compact, const int* __restrict__ offsets, const unsigned long long* __restrict__ masks,
    int64_t n_rays, int n_samples, float4* __restrict__ raw) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRayWaves) + (threadIdx.x >> 6);
  if (r >= n_rays) return;                 // wave-uniform
  const int nw = static_cast<int>(mask_words(n_samples));
  int64_t j0 = offsets[r];
  for (int w = 0; w < nw; ++w) {
    const unsigned long long m = masks[r * nw + w];
    const int s = 64 * w + lane;
    if (s < n_samples) {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, CN_EMPTY_SIGMA_RAW);
      if ((m >> lane) & 1ull) v = raw_compact[j0 + rank_below(m)];
      raw[r * n_samples + s] = v;
    }
    j0 += __popcll(m);
  }
}

// Weight culling, pass 1, one wave per ray: sample i is kept iff w_i > 0, w_i >= eps_weight and
// tail_i = sum_{k >= i} (double)w_k >= eps_tail (NaN fails each).  The 64-sample words are taken from
// the last to the first; in a word the doubles go through an inclusive suffix scan across the lanes
// (log-step shuffles: lane l adds lanes l + 1, l + 2, l + 4, ...), then the sum of the later words
// (the previous word's lane-0 tail) is added.  Masks and counts as occupancy_mask_kernel leaves them.
__global__ __launch_bounds__(64 * kRayWaves) void weight_mask_kernel(
    const float* __restrict__ weights, int64_t n_rays, int n_samples, float eps_weight, double eps_tail,
    int* __restrict__ counts, unsigned long long* __restrict__ masks) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRayWaves) + (threadIdx.x >> 6);
  if (r >= n_rays) return;                 // wave-uniform
  const int nw = static_cast<int>(mask_words(n_samples));
  double carry = 0.0;
  int total = 0;
  for (int w = nw - 1; w >= 0; --w) {
    const int s = 64 * w + lane;
    const float wv = s < n_samples ? weights[r * n_samples + s] : 0.0f;
    double tail = static_cast<double>(wv);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double u = __shfl_down(tail, off);
      if (lane + off < 64) tail += u;
    }
    tail += carry;
    carry = __shfl(tail, 0);
    const bool keep = wv > 0.0f && wv >= eps_weight && tail >= eps_tail;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) masks[r * nw + w] = m;
    total += __popcll(m);
  }
  if (lane == 0) counts[r] = total;
}

// The colours of the kept rows back into raw (n_slots, 4): one thread per compact row, a 16-B load
// and a 12-B store; component 3 (sigma_raw) and every other row are not written.
__global__ __launch_bounds__(256) void scatter_rgb_kernel(const float4* __restrict__ raw_compact,
                                                          const int* __restrict__ sample_index, int n_rows,
                                                          float* __restrict__ raw, int n_slots) {
  const int j = static_cast<int>(blockIdx.x * 256u + threadIdx.x);
  if (j >= n_rows) return;
  const int k = sample_index[j];
  if (static_cast<unsigned>(k) >= static_cast<unsigned>(n_slots)) return;   // never a store outside raw
  const float4 v = raw_compact[j];
  *reinterpret_cast<float3*>(raw + 4 * static_cast<size_t>(k)) = make_float3(v.x, v.y, v.z);
}

// scatter_rgb_kernel with the row count in device memory (cn_scatter_rgb_counted): the launch covers
// n_rows_max rows, the rows past min(max(count[0], 0), n_rows_max) read no index and store nothing.
__global__ __launch_bounds__(256) void scatter_rgb_counted_kernel(const float4* __restrict__ raw_compact,
                                                                  const int* __restrict__ sample_index,
                                                                  const int64_t* __restrict__ count, int n_rows_max,
                                                                  float* __restrict__ raw, int n_slots) {
  const int64_t c = count[0];
  const int n_rows = c < 0 ? 0 : (c < n_rows_max ? static_cast<int>(c) : n_rows_max);
  const int j = static_cast<int>(blockIdx.x * 256u + threadIdx.x);
  if (j >= n_rows) return;
  const int k = sample_index[j];
  if (static_cast<unsigned>(k) >= static_cast<unsigned>(n_slots)) return;   // never a store outside raw
  const float4 v = raw_compact[j];
  *reinterpret_cast<float3*>(raw + 4 * static_cast<size_t>(k)) = make_float3(v.x, v.y, v.z);
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// What the two cull entries share: their common argument rules ...
inline bool cull_args_ok(const float* ro, const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                         int64_t chunk_rows, const void* workspace, const int64_t* count,
                         const int32_t* sample_index, const float* pts, const float* vdir) {
  return ro && rd && z && workspace && count && sample_index && pts && vdir && sizes_ok(n_rays, n_samples) &&
         chunk_rows > 0 && aligned8(workspace) && aligned8(count) && cn::ceil_div(n_rays, kRayWaves) <= INT_MAX;
}

inline int* ws_offsets(void* workspace) { return static_cast<int*>(workspace); }

inline unsigned long long* ws_masks(void* workspace, int64_t n_rays) {
  return reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + offsets_bytes(n_rays));
}

// ... and passes 2 and 3 over the masks and counts their pass 1 left in the workspace.
inline int launch_scan_emit(const float* ro, const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                            int64_t chunk_rows, const int64_t* code_index, void* workspace, int64_t* count,
                            int32_t* sample_index, float* pts, float* vdir, int64_t* code_out, hipStream_t st) {
  const unsigned ray_blocks = static_cast<unsigned>(cn::ceil_div(n_rays, kRayWaves));
  int* offsets = ws_offsets(workspace);
  hipLaunchKernelGGL(occupancy_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, offsets, n_rays, count);
  hipLaunchKernelGGL(occupancy_emit_kernel, dim3(ray_blocks), dim3(64 * kRayWaves), 0, st, ro, rd, z, n_rays,
                     static_cast<int>(n_samples), chunk_rows, code_index, offsets, ws_masks(workspace, n_rays),
                     sample_index, pts, vdir, code_out);
  return cn::launch_status();
}

}  // namespace

extern "C" int64_t cn_occupancy_cull_workspace_bytes(int64_t n_rays, int64_t n_samples) {
  if (!sizes_ok(n_rays, n_samples)) return -1;
  return offsets_bytes(n_rays) + n_rays * mask_words(n_samples) * 8;
}

extern "C" int cn_occupancy_build(const float* nodes, int64_t g, float threshold, int dilate, uint32_t* bits,
                                  cn_stream_t stream) {
  CN_CHECK_ARG(nodes && bits && cn::grid_ok(g) && dilate >= 0 && dilate <= 2);
  const unsigned blocks = static_cast<unsigned>(g * g * g / 256);      // g % 32 == 0: exact
  hipLaunchKernelGGL(occupancy_build_kernel, dim3(blocks), dim3(256), 0, cn::as_stream(stream), nodes,
                     static_cast<int>(g), threshold, dilate, bits);
  return cn::launch_status();
}

extern "C" int cn_occupancy_cull(const float* ro, const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                                 int64_t chunk_rows, const int64_t* code_index, const uint32_t* bits, int64_t g,
                                 float lo, float inv_cell, void* workspace, int64_t* count, int32_t* sample_index,
                                 float* pts, float* vdir, int64_t* code_out, cn_stream_t stream) {
  CN_CHECK_ARG(bits && cn::grid_ok(g));
  CN_CHECK_ARG(cull_args_ok(ro, rd, z, n_rays, n_samples, chunk_rows, workspace, count, sample_index, pts, vdir));
  hipStream_t st = cn::as_stream(stream);
  hipLaunchKernelGGL(occupancy_mask_kernel, dim3(static_cast<unsigned>(cn::ceil_div(n_rays, kRayWaves))),
                     dim3(64 * kRayWaves), 0, st, ro, rd, z, n_rays, static_cast<int>(n_samples), bits,
                     static_cast<int>(g), lo, inv_cell, ws_offsets(workspace), ws_masks(workspace, n_rays));
  return launch_scan_emit(ro, rd, z, n_rays, n_samples, chunk_rows, code_index, workspace, count, sample_index, pts,
                          vdir, code_out, st);
}

extern "C" int cn_weight_cull(const float* weights, const float* ro, const float* rd, const float* z, int64_t n_rays,
                              int64_t n_samples, int64_t chunk_rows, const int64_t* code_index, float eps_weight,
                              double eps_tail, void* workspace, int64_t* count, int32_t* sample_index, float* pts,
                              float* vdir, int64_t* code_out, cn_stream_t stream) {
  CN_CHECK_ARG(weights && eps_weight >= 0.0f && eps_tail >= 0.0);          // a NaN threshold fails
  CN_CHECK_ARG(cull_args_ok(ro, rd, z, n_rays, n_samples, chunk_rows, workspace, count, sample_index, pts, vdir));
  hipStream_t st = cn::as_stream(stream);
  hipLaunchKernelGGL(weight_mask_kernel, dim3(static_cast<unsigned>(cn::ceil_div(n_rays, kRayWaves))),
                     dim3(64 * kRayWaves), 0, st, weights, n_rays, static_cast<int>(n_samples), eps_weight, eps_tail,
                     ws_offsets(workspace), ws_masks(workspace, n_rays));
  return launch_scan_emit(ro, rd, z, n_rays, n_samples, chunk_rows, code_index, workspace, count, sample_index, pts,
                          vdir, code_out, st);
}

extern "C" int cn_scatter_rgb(const float* raw_compact, const int32_t* sample_index, int64_t n_rows, float* raw,
                              int64_t n_slots, cn_stream_t stream) {
  CN_CHECK_ARG(raw_compact && sample_index && raw && n_slots <= INT_MAX && n_rows >= 1 && n_rows <= n_slots);
  CN_CHECK_ARG(cn::aligned16(raw_compact) && cn::aligned16(raw));
  hipLaunchKernelGGL(scatter_rgb_kernel, dim3(static_cast<unsigned>(cn::ceil_div(n_rows, 256))), dim3(256), 0,
                     cn::as_stream(stream), reinterpret_cast<const float4*>(raw_compact), sample_index,
                     static_cast<int>(n_rows), raw, static_cast<int>(n_slots));
  return cn::launch_status();
}

extern "C" int cn_scatter_rgb_counted(const float* raw_compact, const int32_t* sample_index, const int64_t* count,
                                      int64_t n_rows_max, float* raw, int64_t n_slots, cn_stream_t stream) {
  CN_CHECK_ARG(raw_compact && sample_index && raw && n_slots <= INT_MAX && n_rows_max >= 1 && n_rows_max <= n_slots);
  CN_CHECK_ARG(count && aligned8(count) && cn::aligned16(raw_compact) && cn::aligned16(raw));
  hipLaunchKernelGGL(scatter_rgb_counted_kernel, dim3(static_cast<unsigned>(cn::ceil_div(n_rows_max, 256))), dim3(256),
                     0, cn::as_stream(stream), reinterpret_cast<const float4*>(raw_compact), sample_index, count,
                     static_cast<int>(n_rows_max), raw, static_cast<int>(n_slots));
  return cn::launch_status();
}

extern "C" int cn_occupancy_expand(const float* raw_compact, const void* workspace, int64_t n_rays, int64_t n_samples,
                                   float* raw, cn_stream_t stream) {
  CN_CHECK_ARG(workspace && raw && sizes_ok(n_rays, n_samples));
  CN_CHECK_ARG(aligned8(workspace) && cn::aligned16(raw) && cn::aligned16(raw_compact));
  const int64_t ray_blocks = cn::ceil_div(n_rays, kRayWaves);
  CN_CHECK_ARG(ray_blocks <= INT_MAX);
  const int* offsets = static_cast<const int*>(workspace);
  const unsigned long long* masks =
      reinterpret_cast<const unsigned long long*>(static_cast<const char*>(workspace) + offsets_bytes(n_rays));
  hipLaunchKernelGGL(occupancy_expand_kernel, dim3(static_cast<unsigned>(ray_blocks)), dim3(64 * kRayWaves), 0,
                     cn::as_stream(stream), reinterpret_cast<const float4*>(raw_compact), offsets, masks, n_rays,
                     static_cast<int>(n_samples), reinterpret_cast<float4*>(raw));
  return cn::launch_status();
}

// ---------------------------------------------------------------- backward of the compact rows
namespace {

// cn_occupancy_expand's backward, one wave per ray as the expand: a kept sample's gradient row to its compact
// row; a culled slot's is dropped (the empty row is a constant).
__global__ __launch_bounds__(64 * kRayWaves) void occupancy_gather_kernel(
    const float4* __restrict__ g_raw, const int* __restrict__ offsets, const unsigned long long* __restrict__ masks,
    int64_t n_rays, int n_samples, float4* __restrict__ g_compact) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * static_cast<int64_t>(kRayWaves) + (threadIdx.x >> 6);
  if (r >= n_rays) return;                 // wave-uniform
  const int nw = static_cast<int>(mask_words(n_samples));
  int64_t j0 = offsets[r];
  for (int w = 0; w < nw; ++w) {
    const unsigned long long m = masks[r * nw + w];
    const int s = 64 * w + lane;
    if (s < n_samples && ((m >> lane) & 1ull)) g_compact[j0 + rank_below(m)] = g_raw[r * n_samples + s];
    j0 += __popcll(m);
  }
}

// The compact row of kept sample s of a ray whose first row is j0: the kept samples before it.
__device__ __forceinline__ int64_t row_of(const unsigned long long* __restrict__ m, int64_t j0, int s) {
  for (int w = 0; w < (s >> 6); ++w) j0 += __popcll(m[w]);
  return j0 + __popcll(m[s >> 6] & ((1ull << (s & 63)) - 1ull));
}

// cn_occupancy_cull's backward: one lane per (ray, component), every sum sequential in the header's order.
__global__ __launch_bounds__(256) void occupancy_cull_backward_kernel(
    const float* __restrict__ g_pts, const float* __restrict__ g_vdir, const float* __restrict__ z, int64_t n_rays,
    int n_samples, int64_t chunk_rows, const int* __restrict__ offsets, const unsigned long long* __restrict__ masks,
    float* __restrict__ d_ro, float* __restrict__ d_rd) {
  const int64_t t = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (t >= 3 * n_rays) return;
  const int64_t r = t / 3;
  const int c = static_cast<int>(t - 3 * r);
  const int nw = static_cast<int>(mask_words(n_samples));
  float so = 0.0f, sp = 0.0f, sv = 0.0f;
  if (g_pts) {
    int64_t j = offsets[r];
    for (int w = 0; w < nw; ++w) {
      unsigned long long m = masks[r * nw + w];
      while (m) {                          // ascending samples: ascending rows
        const int s = 64 * w + __builtin_ctzll(m);
        m &= m - 1;
        const float g = g_pts[3 * j + c];
        so = __fadd_rn(so, g);
        sp = __fadd_rn(sp, __fmul_rn(z[r * n_samples + s], g));
        ++j;
      }
    }
  }
  if (g_vdir) {
    // the samples whose Q1 view-direction ray is r: k' = (r - base) + i rcnt of the chunk, ascending
    const int64_t base = (r / chunk_rows) * chunk_rows;
    const int64_t rcnt = min(chunk_rows, n_rays - base);
    for (int i = 0; i < n_samples; ++i) {
      const int64_t kk = (r - base) + i * rcnt;          // < rcnt S
      const int64_t rr = base + kk / n_samples;
      const int s = static_cast<int>(kk % n_samples);
      const unsigned long long* m = masks + rr * nw;
      if ((m[s >> 6] >> (s & 63)) & 1ull) sv = __fadd_rn(sv, g_vdir[3 * row_of(m, offsets[rr], s) + c]);
    }
  }
  if (d_ro) d_ro[t] = so;
  if (d_rd) d_rd[t] = __fadd_rn(sp, sv);
}

}  // namespace

extern "C" int cn_occupancy_gather(const float* g_raw, const void* workspace, int64_t n_rays, int64_t n_samples,
                                   float* g_compact, cn_stream_t stream) {
  CN_CHECK_ARG(g_raw && workspace && g_compact && sizes_ok(n_rays, n_samples));
  CN_CHECK_ARG(aligned8(workspace) && cn::aligned16(g_raw) && cn::aligned16(g_compact));
  const int64_t ray_blocks = cn::ceil_div(n_rays, kRayWaves);
  CN_CHECK_ARG(ray_blocks <= INT_MAX);
  const int* offsets = static_cast<const int*>(workspace);
  const unsigned long long* masks =
      reinterpret_cast<const unsigned long long*>(static_cast<const char*>(workspace) + offsets_bytes(n_rays));
  hipLaunchKernelGGL(occupancy_gather_kernel, dim3(static_cast<unsigned>(ray_blocks)), dim3(64 * kRayWaves), 0,
                     cn::as_stream(stream), reinterpret_cast<const float4*>(g_raw), offsets, masks, n_rays,
                     static_cast<int>(n_samples), reinterpret_cast<float4*>(g_compact));
  return cn::launch_status();
}

extern "C" int cn_occupancy_cull_backward(const float* g_pts, const float* g_vdir, const float* z, const void* workspace,
                                          int64_t n_rays, int64_t n_samples, int64_t chunk_rows, float* d_ro,
                                          float* d_rd, cn_stream_t stream) {
  CN_CHECK_ARG(z && workspace && (d_ro || d_rd) && sizes_ok(n_rays, n_samples) && chunk_rows > 0);
  CN_CHECK_ARG(aligned8(workspace));
  const int64_t blocks = cn::ceil_div(3 * n_rays, 256);
  CN_CHECK_ARG(blocks <= INT_MAX);
  const int* offsets = static_cast<const int*>(workspace);
  const unsigned long long* masks =
      reinterpret_cast<const unsigned long long*>(static_cast<const char*>(workspace) + offsets_bytes(n_rays));
  hipLaunchKernelGGL(occupancy_cull_backward_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                     cn::as_stream(stream), g_pts, g_vdir, z, n_rays, static_cast<int>(n_samples), chunk_rows, offsets,
                     masks, d_ro, d_rd);
  return cn::launch_status();
}
