// Ray generation: RaySampler (view_synthesis/nerf/ray_sampler.py).
//
// Memory-bound and tiny (24 B/ray written); one lane per pixel / ray with the
// 3-float records read and written by consecutive lanes.
#include "cn_common.h"

namespace {

// ray_sampler.py:35-51 — meshgrid(indexing='xy'): pixel p = h*W + w,
// dir = ((w - cx)/f, -(h - cy)/f, -1); no +0.5 centre (quirk Q3).
__global__ void ray_directions_kernel(int64_t height, int64_t width, float focal, float cx,
                                      float cy, float* __restrict__ dirs) {
  const int64_t n = height * width;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const float w = static_cast<float>(p % width);
    const float h = static_cast<float>(p / width);
    dirs[3 * p + 0] = __fdiv_rn(__fsub_rn(w, cx), focal);
    dirs[3 * p + 1] = __fdiv_rn(-__fsub_rn(h, cy), focal);
    dirs[3 * p + 2] = -1.0f;
  }
}

// ray_sampler.py:95-98 — rd[b,p,:] = R_b d_p (einsum 'hwij,bji->bhwj'),
// ro[b,p,:] = t_b.
__global__ void ray_bundle_kernel(const float* __restrict__ dirs, int64_t hw,
                                  const float* __restrict__ c2w, int64_t batch,
                                  float* __restrict__ ro, float* __restrict__ rd) {
  const int64_t n = hw * batch;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / hw, p = q % hw;
    const float* T = c2w + 16 * b;
    const float d0 = dirs[3 * p], d1 = dirs[3 * p + 1], d2 = dirs[3 * p + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float acc = __fmul_rn(d0, T[4 * j + 0]);
      acc = __fadd_rn(acc, __fmul_rn(d1, T[4 * j + 1]));
      acc = __fadd_rn(acc, __fmul_rn(d2, T[4 * j + 2]));
      rd[3 * q + j] = acc;
      ro[3 * q + j] = T[4 * j + 3];
    }
  }
}

// ray_sampler.py:77-80 — per-image fancy-index gather.  Indices out of
// [0, hw) produce NaN rays (the host wrapper validates them first).
__global__ void gather_rays_kernel(const float* __restrict__ ro, const float* __restrict__ rd,
                                   int64_t batch, int64_t hw,
                                   const int64_t* __restrict__ sel, int64_t s,
                                   float* __restrict__ ro_out, float* __restrict__ rd_out) {
  const int64_t n = batch * s;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / s;
    const int64_t p = sel[q];
    const bool ok = p >= 0 && p < hw;
    const int64_t src = (b * hw + (ok ? p : 0)) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      ro_out[3 * q + j] = ok ? ro[src + j] : __int_as_float(0x7fc00000);
      rd_out[3 * q + j] = ok ? rd[src + j] : __int_as_float(0x7fc00000);
    }
  }
}

}  // namespace

extern "C" int cn_ray_directions(int64_t height, int64_t width, float focal, float cx,
                                 float cy, float* dirs, cn_stream_t stream) {
  CN_CHECK_ARG(height > 0 && width > 0 && dirs != nullptr && focal != 0.0f);
  const int64_t n = height * width;
  hipLaunchKernelGGL(ray_directions_kernel, dim3(cn::elementwise_grid(n, 256)), dim3(256), 0,
                     cn::as_stream(stream), height, width, focal, cx, cy, dirs);
  return cn::launch_status();
}

extern "C" int cn_ray_bundle(const float* dirs, int64_t hw, const float* c2w, int64_t batch,
                             float* ro, float* rd, cn_stream_t stream) {
  CN_CHECK_ARG(hw > 0 && batch > 0 && dirs && c2w && ro && rd);
  const int64_t n = hw * batch;
  hipLaunchKernelGGL(ray_bundle_kernel, dim3(cn::elementwise_grid(n, 256)), dim3(256), 0,
                     cn::as_stream(stream), dirs, hw, c2w, batch, ro, rd);
  return cn::launch_status();
}

extern "C" int cn_gather_rays(const float* ro, const float* rd, int64_t batch, int64_t hw,
                              const int64_t* select_inds, int64_t sample_size, float* ro_out,
                              float* rd_out, cn_stream_t stream) {
  CN_CHECK_ARG(batch > 0 && hw > 0 && sample_size > 0 && sample_size <= hw);
  CN_CHECK_ARG(ro && rd && select_inds && ro_out && rd_out);
  const int64_t n = batch * sample_size;
  hipLaunchKernelGGL(gather_rays_kernel, dim3(cn::elementwise_grid(n, 256)), dim3(256), 0,
                     cn::as_stream(stream), ro, rd, batch, hw, select_inds, sample_size, ro_out,
                     rd_out);
  return cn::launch_status();
}

// ---------------------------------------------------------------- scene objects
namespace {

struct ObjectPoses {
  float p[CN_MAX_SCENE_OBJECTS][12];  // R row-major (object to world), then t
};
struct ObjectScales {
  float s[CN_MAX_SCENE_OBJECTS];  // a similarity pose's 13th float (read by the SCALED instances only)
};

// Host poses of `stride` (12 or 13) floats each into the kernels' argument structs; false for an entry that is
// not finite or a scale that is not > 0.
inline bool read_poses(const float* poses, int n_objects, int stride, ObjectPoses& p, ObjectScales& sc) {
  for (int k = 0; k < n_objects; ++k) {
    for (int e = 0; e < 12; ++e) {
      const float v = poses[stride * k + e];
      if (!(v - v == 0.0f)) return false;  // finite
      p.p[k][e] = v;
    }
    const float v = stride == 13 ? poses[13 * k + 12] : 1.0f;
    if (!(v - v == 0.0f && v > 0.0f)) return false;
    sc.s[k] = v;
  }
  return true;
}

// World rays in every object's frame: the inverse rigid map R^T (x - t), every operation rounded
// (include/codenerf.h).  One lane per ray, the object is the block's y index.  SCALED: a similarity pose, the
// result divided by the object's scale.
template <bool SCALED>
__global__ __launch_bounds__(256) void object_rays_kernel(const float* __restrict__ ro, const float* __restrict__ rd,
                                                          int64_t n_rays, ObjectPoses poses, ObjectScales scales,
                                                          float* __restrict__ ro_out, float* __restrict__ rd_out) {
  const int k = blockIdx.y;
  const float sc = SCALED ? scales.s[k] : 1.0f;
  float m[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) m[e] = poses.p[k][e];
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n_rays; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = k * n_rays + r;
    const float d0 = __fsub_rn(ro[3 * r], m[9]), d1 = __fsub_rn(ro[3 * r + 1], m[10]);
    const float d2 = __fsub_rn(ro[3 * r + 2], m[11]);
    const float v0 = rd[3 * r], v1 = rd[3 * r + 1], v2 = rd[3 * r + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float uo = __fadd_rn(__fadd_rn(__fmul_rn(d0, m[i]), __fmul_rn(d1, m[3 + i])), __fmul_rn(d2, m[6 + i]));
      const float uv = __fadd_rn(__fadd_rn(__fmul_rn(v0, m[i]), __fmul_rn(v1, m[3 + i])), __fmul_rn(v2, m[6 + i]));
      ro_out[3 * q + i] = SCALED ? __fdiv_rn(uo, sc) : uo;
      rd_out[3 * q + i] = SCALED ? __fdiv_rn(uv, sc) : uv;
    }
  }
}

}  // namespace

extern "C" int cn_object_rays(const float* ro, const float* rd, int64_t n_rays, const float* poses, int n_objects,
                              float* ro_out, float* rd_out, cn_stream_t stream) {
  CN_CHECK_ARG(ro && rd && poses && ro_out && rd_out && n_rays > 0);
  CN_CHECK_ARG(n_objects >= 1 && n_objects <= CN_MAX_SCENE_OBJECTS);
  ObjectPoses p = {};
  ObjectScales sc = {};
  CN_CHECK_ARG(read_poses(poses, n_objects, 12, p, sc));
  hipLaunchKernelGGL(object_rays_kernel<false>, dim3(cn::elementwise_grid(n_rays, 256), n_objects), dim3(256), 0,
                     cn::as_stream(stream), ro, rd, n_rays, p, sc, ro_out, rd_out);
  return cn::launch_status();
}

extern "C" int cn_object_rays_scaled(const float* ro, const float* rd, int64_t n_rays, const float* poses,
                                     int n_objects, float* ro_out, float* rd_out, cn_stream_t stream) {
  CN_CHECK_ARG(ro && rd && poses && ro_out && rd_out && n_rays > 0);
  CN_CHECK_ARG(n_objects >= 1 && n_objects <= CN_MAX_SCENE_OBJECTS);
  ObjectPoses p = {};
  ObjectScales sc = {};
  CN_CHECK_ARG(read_poses(poses, n_objects, 13, p, sc));
  hipLaunchKernelGGL(object_rays_kernel<true>, dim3(cn::elementwise_grid(n_rays, 256), n_objects), dim3(256), 0,
                     cn::as_stream(stream), ro, rd, n_rays, p, sc, ro_out, rd_out);
  return cn::launch_status();
}

// ---------------------------------------------------------------- backward
namespace {

// get_bundle backward (ray_sampler.py:97-98): d R_b[j][i] = sum_p g_rd[b,p,j] d_p[i],
// d t_b[j] = sum_p g_ro[b,p,j] into d_c2w (B,4,4) rows 0..2 (row 3 untouched).
// One block per image, one reduction of 12 sums over its pixels.
__global__ __launch_bounds__(256) void ray_bundle_backward_kernel(const float* __restrict__ dirs, int64_t hw,
                                                                  const float* __restrict__ g_ro,
                                                                  const float* __restrict__ g_rd,
                                                                  float* __restrict__ d_c2w) {
  __shared__ float red[12][256];
  const int64_t b = blockIdx.x;
  float acc[12] = {0};
  for (int64_t p = threadIdx.x; p < hw; p += blockDim.x) {
    const float d0 = dirs[3 * p], d1 = dirs[3 * p + 1], d2 = dirs[3 * p + 2];
    const int64_t q = b * hw + p;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float g = g_rd ? g_rd[3 * q + j] : 0.0f;
      acc[4 * j + 0] += g * d0;
      acc[4 * j + 1] += g * d1;
      acc[4 * j + 2] += g * d2;
      acc[4 * j + 3] += g_ro ? g_ro[3 * q + j] : 0.0f;
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < 12; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 12) d_c2w[16 * b + threadIdx.x] += red[threadIdx.x][0];
}

// sample gather backward (ray_sampler.py:77-80): a scatter-add.  The sampler's indices within
// an image are a permutation prefix (unique), but the entry takes any index list (cn_pose_rays
// does too), so two rays may select one pixel: the adds are float atomics.  A destination with a
// single source gets one add onto its running value, bitwise the plain sum; out-of-range indices
// (NaN rows in the forward) contribute nothing.
__global__ void gather_rays_backward_kernel(const float* __restrict__ g_o, const float* __restrict__ g_d,
                                            int64_t batch, int64_t hw, const int64_t* __restrict__ sel, int64_t s,
                                            float* __restrict__ d_ro, float* __restrict__ d_rd) {
  const int64_t n = batch * s;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / s, p = sel[q];
    if (p < 0 || p >= hw) continue;
    const int64_t dst = (b * hw + p) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (d_ro && g_o) atomicAdd(&d_ro[dst + j], g_o[3 * q + j]);
      if (d_rd && g_d) atomicAdd(&d_rd[dst + j], g_d[3 * q + j]);
    }
  }
}

}  // namespace

extern "C" int cn_ray_bundle_backward(const float* dirs, int64_t hw, int64_t batch, const float* g_ro,
                                      const float* g_rd, float* d_c2w, cn_stream_t stream) {
  CN_CHECK_ARG(dirs && d_c2w && hw > 0 && batch > 0 && batch < (1ll << 31) && (g_ro || g_rd));
  hipLaunchKernelGGL(ray_bundle_backward_kernel, dim3(static_cast<unsigned>(batch)), dim3(256), 0,
                     cn::as_stream(stream), dirs, hw, g_ro, g_rd, d_c2w);
  return cn::launch_status();
}

extern "C" int cn_gather_rays_backward(const float* g_ro, const float* g_rd, int64_t batch, int64_t hw,
                                       const int64_t* select_inds, int64_t sample_size, float* d_ro, float* d_rd,
                                       cn_stream_t stream) {
  CN_CHECK_ARG(batch > 0 && hw > 0 && sample_size > 0 && sample_size <= hw && select_inds);
  const int64_t n = batch * sample_size;
  hipLaunchKernelGGL(gather_rays_backward_kernel, dim3(cn::elementwise_grid(n, 256)), dim3(256), 0,
                     cn::as_stream(stream), g_ro, g_rd, batch, hw, select_inds, sample_size, d_ro, d_rd);
  return cn::launch_status();
}

// ---------------------------------------------------------------- scene objects, backward
// Gradient of cn_object_rays (the rule is in include/codenerf.h).  One lane per ray sums the objects'
// gradients into the ray's d ro / d rd (one writer per element) and forms the ray's 12 pose terms per object;
// a block's lanes walk the rays in a fixed stride, its 12 sums per object are reduced by the fixed LDS tree of
// ray_bundle_backward_kernel into the workspace's block partials, and a second launch reduces the partials, one
// block per object, in the same fixed order: no atomics, two runs give the same bits.  cn_object_rays_scaled_backward
// is the SCALED instance: the gradients divided by the object's scale first, and the scale's own sum as a 13th.
namespace {

constexpr int kPoseBlocks = 256;  // at most: block partials per object

inline int pose_blocks(int64_t n_rays) {
  return static_cast<int>(cn::ceil_div(n_rays, 256) < kPoseBlocks ? cn::ceil_div(n_rays, 256) : kPoseBlocks);
}

// The tree over the block's 256 lanes of N sums each -> out[0..N) (from lanes 0..N-1).  N: 12 for a rigid
// pose, 13 with the scale's sum.
template <int N>
__device__ __forceinline__ void reduce_sums(float (&red)[N][256], const float (&acc)[N], float* __restrict__ out) {
#pragma unroll
  for (int e = 0; e < N; ++e) red[e][threadIdx.x] = acc[e];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
#pragma unroll
      for (int e = 0; e < N; ++e) red[e][threadIdx.x] += red[e][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < N) out[threadIdx.x] = red[threadIdx.x][0];
  __syncthreads();  // red is rewritten by the next object
}

// SCALED: similarity poses -- the upstream gradients divided by the object's scale first, and a 13th sum.
template <bool SCALED>
__global__ __launch_bounds__(256) void object_rays_backward_kernel(
    const float* __restrict__ g_ro, const float* __restrict__ g_rd, const float* __restrict__ ro,
    const float* __restrict__ rd, int64_t n_rays, ObjectPoses poses, ObjectScales scales, int n_objects,
    float* __restrict__ d_ro, float* __restrict__ d_rd, int accumulate, float* __restrict__ partials) {
  constexpr int N = SCALED ? 13 : 12;
  __shared__ float red[N][256];
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t first = blockIdx.x * (int64_t)256 + threadIdx.x;
  // the rays' own gradients: sum_k R_k g_k, ascending k
  if (d_ro || d_rd) {
    for (int64_t r = first; r < n_rays; r += stride) {
      float so[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
      for (int k = 0; k < n_objects; ++k) {
        const float* m = poses.p[k];
        const int64_t q = 3 * (k * n_rays + r);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          float go = g_ro ? g_ro[q + i] : 0.0f, gv = g_rd ? g_rd[q + i] : 0.0f;
          if constexpr (SCALED) {
            go = __fdiv_rn(go, scales.s[k]);
            gv = __fdiv_rn(gv, scales.s[k]);
          }
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            so[j] += m[3 * j + i] * go;
            sv[j] += m[3 * j + i] * gv;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (d_ro) d_ro[3 * r + j] = accumulate ? d_ro[3 * r + j] + so[j] : so[j];
        if (d_rd) d_rd[3 * r + j] = accumulate ? d_rd[3 * r + j] + sv[j] : sv[j];
      }
    }
  }
  if (!partials) return;  // uniform: no pose gradient wanted
  for (int k = 0; k < n_objects; ++k) {
    const float* m = poses.p[k];
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.0f;
    for (int64_t r = first; r < n_rays; r += stride) {
      const int64_t q = 3 * (k * n_rays + r);
      float go[3], gv[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        go[i] = g_ro ? g_ro[q + i] : 0.0f;
        gv[i] = g_rd ? g_rd[q + i] : 0.0f;
      }
      if constexpr (SCALED) {
        // the forward's outputs again (its expressions), against the gradients as they came; then g' = g / s
        const float sc = scales.s[k];
        const float e0 = __fsub_rn(ro[3 * r], m[9]), e1 = __fsub_rn(ro[3 * r + 1], m[10]);
        const float e2 = __fsub_rn(ro[3 * r + 2], m[11]);
        const float v0 = rd[3 * r], v1 = rd[3 * r + 1], v2 = rd[3 * r + 2];
        float t = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float uo = __fadd_rn(__fadd_rn(__fmul_rn(e0, m[i]), __fmul_rn(e1, m[3 + i])), __fmul_rn(e2, m[6 + i]));
          const float uv = __fadd_rn(__fadd_rn(__fmul_rn(v0, m[i]), __fmul_rn(v1, m[3 + i])), __fmul_rn(v2, m[6 + i]));
          t += __fdiv_rn(uo, sc) * go[i] + __fdiv_rn(uv, sc) * gv[i];
          go[i] = __fdiv_rn(go[i], sc);
          gv[i] = __fdiv_rn(gv[i], sc);
        }
        acc[12] -= t / sc;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float dj = ro[3 * r + j] - m[9 + j], vj = rd[3 * r + j];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          acc[3 * j + i] += dj * go[i] + vj * gv[i];
          acc[9 + j] -= m[3 * j + i] * go[i];
        }
      }
    }
    reduce_sums<N>(red, acc, partials + ((int64_t)k * gridDim.x + blockIdx.x) * N);
  }
}

// Stage 2, one block per object: lane t sums the block partials t, t + 256, ... (at most one with
// kPoseBlocks = 256), then the tree.
template <int N>
__global__ __launch_bounds__(256) void object_poses_reduce_kernel(const float* __restrict__ partials, int n_blocks,
                                                                  float* __restrict__ d_poses) {
  __shared__ float red[N][256];
  const int k = blockIdx.x;
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.0f;
  for (int b = threadIdx.x; b < n_blocks; b += 256)
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] += partials[((int64_t)k * n_blocks + b) * N + e];
  reduce_sums<N>(red, acc, d_poses + N * k);
}

}  // namespace

extern "C" int64_t cn_object_rays_backward_workspace_floats(int64_t n_rays, int n_objects) {
  if (n_rays <= 0 || n_objects < 1 || n_objects > CN_MAX_SCENE_OBJECTS) return -1;
  return (int64_t)pose_blocks(n_rays) * n_objects * 12;
}

extern "C" int cn_object_rays_backward(const float* g_ro_obj, const float* g_rd_obj, const float* ro, const float* rd,
                                       int64_t n_rays, const float* poses, int n_objects, float* d_ro, float* d_rd,
                                       int accumulate, float* d_poses, float* workspace, cn_stream_t stream) {
  CN_CHECK_ARG(ro && rd && poses && n_rays > 0 && (accumulate == 0 || accumulate == 1));
  CN_CHECK_ARG(n_objects >= 1 && n_objects <= CN_MAX_SCENE_OBJECTS);
  CN_CHECK_ARG(d_ro || d_rd || d_poses);
  CN_CHECK_ARG(!d_poses || workspace);
  ObjectPoses p = {};
  ObjectScales sc = {};
  CN_CHECK_ARG(read_poses(poses, n_objects, 12, p, sc));
  const int blocks = pose_blocks(n_rays);
  hipStream_t st = cn::as_stream(stream);
  hipLaunchKernelGGL(object_rays_backward_kernel<false>, dim3(blocks), dim3(256), 0, st, g_ro_obj, g_rd_obj, ro, rd,
                     n_rays, p, sc, n_objects, d_ro, d_rd, accumulate, d_poses ? workspace : nullptr);
  if (d_poses)
    hipLaunchKernelGGL(object_poses_reduce_kernel<12>, dim3(n_objects), dim3(256), 0, st, workspace, blocks, d_poses);
  return cn::launch_status();
}

extern "C" int64_t cn_object_rays_scaled_backward_workspace_floats(int64_t n_rays, int n_objects) {
  if (n_rays <= 0 || n_objects < 1 || n_objects > CN_MAX_SCENE_OBJECTS) return -1;
  return (int64_t)pose_blocks(n_rays) * n_objects * 13;
}

extern "C" int cn_object_rays_scaled_backward(const float* g_ro_obj, const float* g_rd_obj, const float* ro,
                                              const float* rd, int64_t n_rays, const float* poses, int n_objects,
                                              float* d_ro, float* d_rd, int accumulate, float* d_poses,
                                              float* workspace, cn_stream_t stream) {
  CN_CHECK_ARG(ro && rd && poses && n_rays > 0 && (accumulate == 0 || accumulate == 1));
  CN_CHECK_ARG(n_objects >= 1 && n_objects <= CN_MAX_SCENE_OBJECTS);
  CN_CHECK_ARG(d_ro || d_rd || d_poses);
  CN_CHECK_ARG(!d_poses || workspace);
  ObjectPoses p = {};
  ObjectScales sc = {};
  CN_CHECK_ARG(read_poses(poses, n_objects, 13, p, sc));
  const int blocks = pose_blocks(n_rays);
  hipStream_t st = cn::as_stream(stream);
  hipLaunchKernelGGL(object_rays_backward_kernel<true>, dim3(blocks), dim3(256), 0, st, g_ro_obj, g_rd_obj, ro, rd,
                     n_rays, p, sc, n_objects, d_ro, d_rd, accumulate, d_poses ? workspace : nullptr);
  if (d_poses)
    hipLaunchKernelGGL(object_poses_reduce_kernel<13>, dim3(n_objects), dim3(256), 0, st, workspace, blocks, d_poses);
  return cn::launch_status();
}
