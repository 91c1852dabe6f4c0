// Code-conditioned MLP: CodeNeRFModel (view_synthesis/models/model.py:123-194)
// fused with the positional encoding and Q1 view-direction mapping of
// forward_pass (view_synthesis/nerf/__init__.py:94-134).
//
// Per sample the reference evaluates 9 Linear layers over concatenated inputs.
// Three of them (the code layers, model.py:174-177) and the code halves of
// layer_xyz2 / fc_out / fc_rgb depend only on the object's codes, so they are
// folded once per code row into bias vectors (cn_code_bias).  The remaining
// per-sample work -- 63->256, 256->256, 256->257, (256+27)->256, 256->256,
// 256->3 -- is 286,208 MAC = 572,416 FLOP per sample and runs on fp32 MFMA
// (v_mfma_f32_32x32x2_f32, exact f32 products, ~157 TFLOP/s peak on gfx950).
//
// Kernel shape: 256-thread workgroup = 4 waves, one wave per SIMD (the layer's
// 256-wide input and output tiles take ~300 VGPRs), 32 samples per wave, 128
// per workgroup.  Activations never leave registers: each layer's accumulator
// is the next layer's B operand (mlp_layout.h).  Weights (1.25 MiB packed,
// resident in every XCD's L2) stream through a double-buffered LDS ring in
// chunks of 16 k-steps; each chunk is 128-144 MFMAs per wave (8-9 K cycles),
// its successor is loaded into registers while it runs and written to LDS
// behind it.
#include "mlp_common.h"

namespace cn {
namespace mlp {

// ---------------------------------------------------------------- packing

__global__ void pack_kernel(Params P, float* __restrict__ packed) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < kPackedFloats;
       idx += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (idx >= kBiasXyz1) {
      const int j = idx - kBiasXyz1;
      v = j < 256 ? P.p[kBXyz1][j] : (j < 512 ? P.p[kBDir1][j - 256] : P.p[kBDir2][j - 512]);
    } else {
      constexpr int offs[kNumLayers + 1] = {layer_offset(0), layer_offset(1), layer_offset(2),
                                            layer_offset(3), layer_offset(4), layer_offset(5),
                                            layer_offset(6)};
      int l = 0;
      while (l + 1 < kNumLayers && idx >= offs[l + 1]) ++l;
      int rem = idx - offs[l];
      const int nbp = kBlocksPad[l];
      const int ob = rem % nbp;
      rem /= nbp;
      const int lane = rem % 64, t = rem / 64;
      const int i = lane & 31, h = lane >> 5;
      int row = -1, col = -1, in_dim = 0;
      const float* W = nullptr;
      switch (l) {
        case kXyz1: W = P.p[kWXyz1]; in_dim = kDimXyz; row = 32 * ob + i; col = k_from_enc(t, h, 15); break;
        case kXyz2: W = P.p[kWXyz2]; in_dim = kHidden + kCode; row = 32 * ob + i; col = k_from_acc(t, h); break;
        case kOut:
          W = P.p[kWOut]; in_dim = kHidden + kCode; col = k_from_acc(t, h);
          row = ob < 8 ? 1 + 32 * ob + i : ((ob == 8 && i == 0) ? 0 : -1);
          break;
        case kDir1:
          W = P.p[kWDir1]; in_dim = kCode + kDimDir; row = 32 * ob + i;
          if (t < 128) {
            col = k_from_acc(t, h);
          } else {
            const int e = k_from_enc(t - 128, h, 6);
            col = e < 0 ? -1 : kCode + e;
          }
          break;
        case kDir2: W = P.p[kWDir2]; in_dim = kHidden; row = 32 * ob + i; col = k_from_acc(t, h); break;
        default: W = P.p[kWRgb]; in_dim = kHidden + kCode; row = (ob == 0 && i < 3) ? i : -1; col = k_from_acc(t, h); break;
      }
      if (row >= 0 && col >= 0) v = W[row * in_dim + col];
    }
    packed[idx] = v;
  }
}

// ---------------------------------------------------------------- code bias
// (code_bias_block, mlp_common.h: one workgroup of kCbThreads per (code, slice))

__global__ __launch_bounds__(kCbThreads) void code_bias_kernel(Params P, const float* __restrict__ z_s,
                                                               const float* __restrict__ z_t,
                                                               float* __restrict__ out) {
  code_bias_block(P, z_s, z_t, out, blockIdx.x);
}

// ---------------------------------------------------------------- field kernel

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kTile = 32 * kWaves;          // samples per workgroup
constexpr int kChunkSteps = 16;
constexpr int kMaxChunkFloats = kChunkSteps * 64 * 12;  // fc_out chunks (nbp 12)

struct Chunk {
  int layer, t0, steps;
};

// The weight stream: every layer in 16-k-step chunks (layer_dir1 ends with
// its 14-step view-direction chunk).
constexpr int kNumChunks = 2 + 8 + 8 + 9 + 8 + 8;
__host__ __device__ constexpr Chunk chunk_at(int c) {
  return c < 2 ? Chunk{kXyz1, 16 * c, 16}
       : c < 10 ? Chunk{kXyz2, 16 * (c - 2), 16}
       : c < 18 ? Chunk{kOut, 16 * (c - 10), 16}
       : c < 27 ? Chunk{kDir1, 16 * (c - 18), c == 26 ? 14 : 16}
       : c < 35 ? Chunk{kDir2, 16 * (c - 27), 16}
                : Chunk{kRgb, 16 * (c - 35), 16};
}
__host__ __device__ constexpr int chunk_floats(int c) {
  return chunk_at(c).steps * 64 * kBlocksPad[chunk_at(c).layer];
}
__host__ __device__ constexpr int chunk_src(int c) {
  return layer_offset(chunk_at(c).layer) + chunk_at(c).t0 * 64 * kBlocksPad[chunk_at(c).layer];
}
// float4 loads per thread to stage a chunk
__host__ __device__ constexpr int chunk_loads(int c) { return (chunk_floats(c) / 4 + kThreads - 1) / kThreads; }
constexpr int kMaxLoads = (kMaxChunkFloats / 4) / kThreads;  // 12

struct State {
  float* save_row;   // this sample's row of plane 0 of FieldArgs::save (or null)
  int64_t plane;     // floats between save planes
  floatx16 act[8];   // layer input (B operands), 256 features x 32 samples
  floatx16 acc[9];   // layer output accumulators
  floatx16 denc;     // view-direction encoding (14 k-steps of layer_dir1)
  float4 stage[kMaxLoads];
  float sigma;
  int lane, h;
  int64_t cb_row;    // code-bias row (floats offset)
  float vd[3];       // unit view direction of this sample's Q1 ray
};

template <int C>
__device__ __forceinline__ void load_chunk(State& s, const float* __restrict__ packed) {
  constexpr int n4 = chunk_floats(C) / 4;
  const float4* src = reinterpret_cast<const float4*>(packed + chunk_src(C));
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < chunk_loads(C); ++i) {
    const int q = i * kThreads + tid;
    if (n4 % kThreads == 0 || q < n4) s.stage[i] = src[q];
  }
}

template <int C>
__device__ __forceinline__ void store_chunk(State& s, float* lds) {
  constexpr int n4 = chunk_floats(C) / 4;
  float4* dst = reinterpret_cast<float4*>(lds);
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < chunk_loads(C); ++i) {
    const int q = i * kThreads + tid;
    if (n4 % kThreads == 0 || q < n4) dst[q] = s.stage[i];
  }
}

// Bias-initialised accumulators for layer L (acc = b, then acc += W x).
template <int L>
__device__ __forceinline__ void init_acc(State& s, const FieldArgs& a) {
  const float* cb = a.code_bias + s.cb_row;
  const float* base = L == kXyz1 ? a.packed + kBiasXyz1
                    : L == kXyz2 ? cb + kCbXyz2
                    : L == kOut ? cb + kCbFeat
                    : L == kDir1 ? a.packed + kBiasDir1
                    : L == kDir2 ? a.packed + kBiasDir2
                                 : cb + kCbRgb;
  if constexpr (L == kRgb) {
    // block 0 rows 0..2 (lane half 0, registers 0..2)
    s.acc[0] = floatx16{0};
    if (s.h == 0) {
      s.acc[0][0] = base[0];
      s.acc[0][1] = base[1];
      s.acc[0][2] = base[2];
    }
  } else {
#pragma unroll
    for (int ob = 0; ob < 8; ++ob) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 b = *reinterpret_cast<const float4*>(base + 32 * ob + 8 * q + 4 * s.h);
        s.acc[ob][4 * q + 0] = b.x;
        s.acc[ob][4 * q + 1] = b.y;
        s.acc[ob][4 * q + 2] = b.z;
        s.acc[ob][4 * q + 3] = b.w;
      }
    }
    if constexpr (L == kOut) {
      s.acc[8] = floatx16{0};
      if (s.h == 0) s.acc[8][0] = cb[kCbSigma];
    }
  }
}

// B operand of k-step t (global within layer L).
template <int L, int T>
__device__ __forceinline__ float b_operand(const State& s) {
  if constexpr (L == kXyz1) {
    return s.act[T >> 4][T & 15];
  } else if constexpr (L == kDir1 && T >= 128) {
    return s.denc[T - 128];
  } else {
    return s.act[T >> 4][T & 15];
  }
}

template <int C, int T>
__device__ __forceinline__ void mfma_step(State& s, const float* lds) {
  constexpr Chunk ch = chunk_at(C);
  constexpr int L = ch.layer;
  constexpr int nbp = kBlocksPad[L];
  constexpr int nb = kBlocks[L];
  const float* ap = lds + (T * 64 + s.lane) * nbp;
  float a[nbp];
  if constexpr (nbp % 4 == 0) {
#pragma unroll
    for (int j = 0; j < nbp / 4; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(ap + 4 * j);
      a[4 * j] = v.x; a[4 * j + 1] = v.y; a[4 * j + 2] = v.z; a[4 * j + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < nbp; ++j) a[j] = ap[j];
  }
  const float b = b_operand<L, ch.t0 + T>(s);
#pragma unroll
  for (int ob = 0; ob < nb; ++ob) s.acc[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ob], b, s.acc[ob], 0, 0, 0);
}

template <int C, int T>
__device__ __forceinline__ void mfma_steps(State& s, const float* lds) {
  if constexpr (T < chunk_at(C).steps) {
    mfma_step<C, T>(s, lds);
    mfma_steps<C, T + 1>(s, lds);
  }
}

template <int N>
__device__ __forceinline__ void put_act(State& s, const float* v) {
#pragma unroll
  for (int t = 0; t < N; ++t) s.act[t >> 4][t & 15] = v[t];
}

// Training mode: the layer's post-activation outputs, row-major (m, 256) per layer.
template <int L>
__device__ __forceinline__ void save_layer(const State& s) {
  if constexpr (L != kRgb) {
    if (s.save_row) {
      float* dst = s.save_row + L * s.plane;
#pragma unroll
      for (int ob = 0; ob < 8; ++ob)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(dst + 32 * ob + 8 * q + 4 * s.h) =
              make_float4(s.act[ob][4 * q], s.act[ob][4 * q + 1], s.act[ob][4 * q + 2], s.act[ob][4 * q + 3]);
    }
  }
}

template <int L>
__device__ __forceinline__ void finish_layer(State& s) {
  if constexpr (L == kOut) {
#pragma unroll
    for (int ob = 0; ob < 8; ++ob) s.act[ob] = s.acc[ob];  // feat: no activation
    s.sigma = s.acc[8][0];
  } else if constexpr (L != kRgb) {
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r)  // ReLU as v_max_i32 on the bits (fmaxf: canonicalize + max)
        s.act[ob][r] = __int_as_float(max(__float_as_int(s.acc[ob][r]), 0));
  }
}

template <int MODE, int C>
__device__ __forceinline__ void run_chunks(State& s, const FieldArgs& a, float* lds0, float* lds1) {
  if constexpr (C < kNumChunks) {
    constexpr Chunk ch = chunk_at(C);
    float* cur = (C & 1) ? lds1 : lds0;
    float* nxt = (C & 1) ? lds0 : lds1;
    if constexpr (ch.t0 == 0) init_acc<ch.layer>(s, a);
    if constexpr (C + 1 < kNumChunks) load_chunk<C + 1>(s, a.packed);
    if constexpr (ch.layer == kDir1 && ch.t0 == 0 && MODE != kFromEncoded) {
      float v[14];
      encode_pairs<6, 4>(s.vd, a.fd, s.h, v);
#pragma unroll
      for (int t = 0; t < 14; ++t) s.denc[t] = v[t];
    }
    mfma_steps<C, 0>(s, cur);
    constexpr bool last_of_layer = (C + 1 == kNumChunks) || chunk_at(C + 1).layer != ch.layer;
    if constexpr (last_of_layer) {
      finish_layer<ch.layer>(s);
      save_layer<ch.layer>(s);
    }
    if constexpr (C + 1 < kNumChunks) {
      store_chunk<C + 1>(s, nxt);
      __syncthreads();
    }
    run_chunks<MODE, C + 1>(s, a, lds0, lds1);
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads, 1) void field_kernel(FieldArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2][kMaxChunkFloats];
  State s;
  s.lane = threadIdx.x & 63;
  s.h = s.lane >> 5;
  const int wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * kTile + wave * 32 + (s.lane & 31);
  const bool valid = row < a.m;
  const int64_t rc = valid ? row : a.m - 1;
  s.save_row = (a.save && valid) ? a.save + row * 256 : nullptr;
  s.plane = a.m * 256;

  // ---- per-sample inputs
  const SampleIn in = decode_sample<MODE>(a, rc);
  float enc[32];
  if constexpr (MODE == kFromEncoded) {
    const float* xr = a.x + rc * (kDimXyz + kDimDir);
    gather_pairs<15>(xr, 0, s.h, enc);
    float d[14];
    gather_pairs<6>(xr, kDimXyz, s.h, d);
#pragma unroll
    for (int t = 0; t < 14; ++t) s.denc[t] = d[t];
  } else {
    encode_pairs<15, 10>(in.x, a.fx, s.h, enc);
#pragma unroll
    for (int j = 0; j < 3; ++j) s.vd[j] = in.vd[j];
  }
  put_act<32>(s, enc);
  s.cb_row = code_row(a, in.code_of) * kCbStride;

  // ---- weight stream prologue: chunk 0 into buffer 0
  load_chunk<0>(s, a.packed);
  store_chunk<0>(s, lds[0]);
  __syncthreads();
  run_chunks<MODE, 0>(s, a, lds[0], lds[1]);

  // ---- raw = [rgb(3), sigma]: block 0 rows 0..2 of fc_rgb live in lane half 0
  if (valid && s.h == 0) {
    float4 o;
    o.x = s.acc[0][0];
    o.y = s.acc[0][1];
    o.z = s.acc[0][2];
    o.w = s.sigma;
    reinterpret_cast<float4*>(a.raw)[row] = o;
  }
}


// ---------------------------------------------------------------- launchers (entry points: field_api.hip)

static_assert(kPackedFloats == 327424, "packed layout changed: update docs");
static_assert(kCbStride == CN_CODE_BIAS_STRIDE, "code-bias stride mismatch");

int launch_pack_v1(const Params& P, float* packed, hipStream_t st) {
  hipLaunchKernelGGL(pack_kernel, dim3(cn::elementwise_grid(kPackedFloats, 256)), dim3(256), 0, st, P, packed);
  return cn::launch_status();
}

int launch_code_bias(const Params& P, const float* z_s, const float* z_t, int64_t n_codes, float* out,
                     hipStream_t st) {
  hipLaunchKernelGGL(code_bias_kernel, dim3(static_cast<unsigned>(n_codes * kCbSlices)), dim3(kCbThreads), 0, st, P,
                     z_s, z_t, out);
  return cn::launch_status();
}

int launch_field_v1(int mode, FieldArgs& a, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(cn::ceil_div(a.m, kTile))), b(kThreads);
  return launch_any_mode(mode, [&](auto M) { hipLaunchKernelGGL(field_kernel<M.value>, grid, b, 0, st, a); });
}

}  // namespace mlp
}  // namespace cn
