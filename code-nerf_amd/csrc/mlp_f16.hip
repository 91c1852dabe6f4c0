// fp16 inference field kernel (CN_FMT_F16): the fused posenc + CodeNeRF MLP of mlp_x3.hip with every
// GEMM as ONE product on v_mfma_f32_32x32x16_f16 (fp32 accumulate).  Forward only: no masks, no
// saved planes, no backward.
//
// The rule (include/codenerf.h, tests/field_f16_cases.py).  The six GEMM weight matrices are rounded
// to fp16 (round to nearest even) at pack time; every vector an MFMA reads -- the 63 position
// encodings, h1, h2, feat, the 27 view encodings, v1, v2 -- is rounded to fp16 (RNE, v_cvt_pk_f16_f32)
// where it is read.  Everything else is fp32 and unrounded: the encodings' arithmetic, every bias
// (the accumulators start from the fp32 values through an fp32 MFMA, b x 1.0), the per-code terms
// and the accumulation.  sigma_raw (fc_out row 0) is an fp32 dot product over the unrounded h2.
// ReLU is v_max_f32(x, 0): a NaN becomes 0.
//
// Register dataflow (mlp_layout.h; the f16 and bf16 forms of the instruction share the operand
// layout).  A 32x32 fp32 accumulator block's registers 0..7 / 8..15 are the next layer's B operand
// for k-steps 2b / 2b+1, so a block converts in place to 8 dwords of packed fp16 (max + one
// v_cvt_pk_f16_f32 per pair) and activations never leave registers.  The last chunk of a layer runs
// its MFMAs block by block instead of k-step by k-step, so that the blocks it has finished convert
// in the issue gaps of the blocks still running; only the last pair converts in the open.
//
// Weight stream.  Chunk = 2 k-steps x 8 blocks x 64 lanes quads = 16 KiB, fragment-major (a wave's
// ds_read_b128 of one fragment is 1 KiB contiguous); 36 chunks in the order mlp_x3.hip shares with
// this file (mlp_stream.h: the schedule, the bias paths, the LDS reads and waits).  A 4-slot LDS
// ring is filled by LDS-DMA, 4 pieces of 1 KiB per wave and chunk.  Chunk c is split by ONE barrier
// M_c after its 4th MFMA group (of 8): chunk c+1 landed for every wave (counted vmcnt(4): chunk
// c+2's pieces are the younger ones) and every wave is done with chunk c-1.  Groups 0, 1 of chunk c
// issue pieces 2, 3 of chunk c+2, groups 4, 5 pieces 0, 1 of chunk c+3 (the slot of chunk c-1), and
// group 7 already reads chunk c+1's first A fragments.  No ordinary global load is live in the
// stream, so the counted waits are exact.
//
// Persistent tiles: one workgroup per CU, 128-sample tiles (32 per wave), a cyclic stream (36 chunks,
// a multiple of the ring) whose last three chunks prefetch the next tile's first three.  The layers
// are unrolled (a layer is a third of mlp_x3.hip's in instructions).
#include "mlp_stream.h"

namespace cn {
namespace mlp {
namespace f16 {

using namespace stream;
using namespace stream32;

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kBlk = 8;                            // 32-row output blocks per k-step
constexpr int kQuadsPerStep = 64 * kBlk;           // one k-step of a chunk (8 KiB)
constexpr int kChunkQuads = 2 * kQuadsPerStep;     // 1024 quads = 16 KiB
constexpr int kDmaPerWave = kChunkQuads / 64 / 4;  // 4
constexpr int kQuads = kChunks * kChunkQuads;
constexpr int kBiasXyz1 = kQuads * 4;  // floats
constexpr int kPackedFloats = kBiasXyz1 + kConsts;

__global__ void pack_f16_kernel(Params P, float* __restrict__ packed) {
  unsigned short* q16 = reinterpret_cast<unsigned short*>(packed);
  const int n_elems = kQuads * 8;  // fp16 elements
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n_elems + kConsts; idx += gridDim.x * blockDim.x) {
    if (idx >= n_elems) {
      const int j = idx - n_elems;
      float v;
      if (j < 256) v = P.p[kBXyz1][j];
      else if (j < 512) v = P.p[kBDir1][j - 256];
      else if (j < 768) v = P.p[kBDir2][j - 512];
      else {
        const int t = j - kSigmaOff, h = t >> 7, b = (t >> 4) & 7, r = t & 15;
        v = P.p[kWOut][acc_row(b, r, h)];  // fc_out row 0 at input feature acc_row(b, r, h) of h2
      }
      packed[kBiasXyz1 + j] = v;
      continue;
    }
    const int quad = idx >> 3, e = idx & 7;
    const int c = quad / kChunkQuads;
    int r = quad % kChunkQuads;
    const int T = r / kQuadsPerStep;
    r %= kQuadsPerStep;
    const int frag = r / 64, lane = r % 64;  // fragment-major: 1 KiB per block
    int l, ks, ob;
    chunk_map(c, T, frag, l, ks, ob);
    const int i = lane & 31, h = lane >> 5;
    const int col = in_col(l, ks, h, e);
    int row = -1, in_dim = 0;
    const float* W = nullptr;
    switch (l) {
      case kXyz1: W = P.p[kWXyz1]; in_dim = kDimXyz; row = 32 * ob + i; break;
      case kXyz2: W = P.p[kWXyz2]; in_dim = kHidden + kCode; row = 32 * ob + i; break;
      case kOut: W = P.p[kWOut]; in_dim = kHidden + kCode; row = 1 + 32 * ob + i; break;
      case kDir1: W = P.p[kWDir1]; in_dim = kCode + kDimDir; row = 32 * ob + i; break;
      case kDir2: W = P.p[kWDir2]; in_dim = kHidden; row = 32 * ob + i; break;
      default: W = P.p[kWRgb]; in_dim = kHidden + kCode; row = i < 3 ? i : -1; break;
    }
    const float w = (row >= 0 && col >= 0) ? W[row * in_dim + col] : 0.0f;
    const _Float16 hw = static_cast<_Float16>(w);  // round to nearest even; beyond the range: +-inf
    q16[idx] = __builtin_bit_cast(unsigned short, hw);
  }
}

// ---------------------------------------------------------------- kernel

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kTile = 32 * kWaves;
constexpr int kRing = 4;
constexpr int kLdsQuads = kRing * kChunkQuads;  // 64 KiB ring
// after the ring: the constant vectors (1024), then each wave's code row
constexpr int kBiasLds = kConsts + kWaves * kCbStride;

struct State {
  floatx16 acc[8];
  unsigned hb[8][8];  // per block: the 16 activations as packed fp16, dwords 0-3 k-step 2b, 4-7 k-step 2b+1
  unsigned xb[16];    // the position encodings' 4 k-steps
  unsigned db[8];     // the view encodings' 2 k-steps
  float sigma, sig;   // fc_out row 0; running partial of this lane half
  int lane, h, wave;
  int crow;           // this lane's code-bias row
  bool uniform_code;  // all 32 samples of the wave use one code row
  halfx8 pre[2];      // next chunk's group-0 A fragments, read by the chunk before it
  __amdgpu_buffer_rsrc_t wsrc;  // the packed stream as a buffer resource
  unsigned voff;      // this lane's byte offset inside a 1 KiB-per-wave piece row
};

__device__ __forceinline__ halfx8 b_of(const unsigned* w) {
  const u32x4 u = {w[0], w[1], w[2], w[3]};
  return __builtin_bit_cast(halfx8, u);
}

// Two fp32 values -> one dword of fp16 (RNE), pinned where it is written (LLVM would otherwise sink
// the conversion to the operand's first use, out of the MFMA gaps it is meant to fill).
__device__ __forceinline__ unsigned pack_pair(float x, float y) {
  const f32x2 v = {x, y};
  const halfx2 hv = __builtin_convertvector(v, halfx2);
  unsigned u = __builtin_bit_cast(unsigned, hv);
  asm volatile("" : "+v"(u));
  return u;
}

// One LDS-DMA piece: 1 KiB per wave (16 B per lane) of chunk `cn`, piece `i` (quads [i*256, i*256+256)
// of the chunk; this wave moves quads i*256 + wave*64 + lane).
__device__ __forceinline__ void dma_piece(const State& s, float4* lds, int cn, int i) {
  dma_quads<kChunkQuads, kRing>(s.wsrc, s.wave, s.voff, lds, cn, cn, i * 256);
}

// The pieces running chunk c issues: groups 0, 1 pieces 2, 3 of chunk c+2, groups 4, 5 pieces 0, 1 of
// chunk c+3, wrapping into the next tile's first chunks (kChunks is a multiple of kRing).
struct Dma {
  const State& s;
  float4* lds;
  int ca, cb;  // c+2, c+3 mod kChunks
  template <int G>
  __device__ __forceinline__ void piece() const {
    if constexpr (G < 2) dma_piece(s, lds, ca, 2 + G);
    else if constexpr (G == 4 || G == 5) dma_piece(s, lds, cb, G - 4);
  }
};
template <int G>
constexpr bool has_piece() { return G < 2 || G == 4 || G == 5; }

__device__ __forceinline__ Dma dma_for(const State& s, float4* lds, int c) {
  return Dma{s, lds, wrap_chunk(c + 2), wrap_chunk(c + 3)};
}

// M_c is chunk_barrier<kMidOut>: chunk c+2's 4 pieces are the younger ones.
constexpr int kMidOut = 4;

// Biases.  acc starts as the fp32 value b through ONE fp32 MFMA per output block: A holds b_i at
// k = 0 (lane half 0), B holds 1.0 at k = 0, so D = b exactly -- no 16-bit operand is involved.
__device__ __forceinline__ floatx16 bias_mfma(const State& s, float v) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(s.h == 0 ? v : 0.0f, s.h == 0 ? 1.0f : 0.0f, floatx16{0}, 0, 0, 0);
}

template <int LAYER>
__device__ __forceinline__ void init_acc(State& s, const FieldArgs& a, const float* blds) {
  constexpr bool per_code = LAYER == kXyz2 || LAYER == kOut;
  if (!per_code || s.uniform_code) {
    float v[8];
    bias_values(s, blds, LAYER, v);
#pragma unroll
    for (int ob = 0; ob < 8; ++ob) s.acc[ob] = bias_mfma(s, v[ob]);
  } else {
    init_acc_per_lane(s, a, LAYER);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// Block B of a finished layer -> its 8 dwords of fp16 operands; SIG (layer_xyz2): the sigma dot
// product's terms over the unrounded values alongside.
template <int B, bool RELU, bool SIG>
__device__ __forceinline__ void conv_block(State& s, const float* blds) {
  float w[16];
  if constexpr (SIG) lds_read16(blds + kSigmaOff + (s.h * 8 + B) * 16, w);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float x = s.acc[B][2 * q], y = s.acc[B][2 * q + 1];
    if constexpr (RELU) {
      x = vmax(x, 0.0f);
      y = vmax(y, 0.0f);
    }
    if constexpr (SIG) {
      s.sig = fmaf(w[2 * q], x, s.sig);
      s.sig = fmaf(w[2 * q + 1], y, s.sig);
    }
    s.hb[B][q] = pack_pair(x, y);
  }
}

struct NoFill {
  template <int G>
  __device__ __forceinline__ void step() {}
  static constexpr int kValu = 0;
};

// Last chunk of a layer (block-major groups: pair P's MFMAs are groups 2P, 2P+1): block G - 2 is
// finished when group G starts.
template <bool RELU, bool SIG>
struct ConvFill {
  State& s;
  const float* blds;
  template <int G>
  __device__ __forceinline__ void step() {
    if constexpr (G >= 2) conv_block<G - 2, RELU, SIG>(s, blds);
  }
  static constexpr int kValu = 12;
};

// Scheduling pattern of one group: the next group's 2 A reads and the group's DMA piece first, then 2
// MFMAs, each followed by up to N VALU.
template <int N, bool READS, bool DMA>
__device__ __forceinline__ void group_pattern() {
  if (READS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
  if (DMA) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (N > 0) __builtin_amdgcn_sched_group_barrier(0x002, N, 0);
  }
}

// Fragment order of a chunk's 8 groups of 2 MFMAs.  k-major: group g = (T = g / 4, pair P = g % 4);
// block-major: (P = g / 2, T = g % 2).  Fragment (T, block) lies at quad (8 T + block) * 64.
template <bool BLOCK_MAJOR, int G>
struct GroupOf {
  static constexpr int T = BLOCK_MAJOR ? G % 2 : G / 4;
  static constexpr int P = BLOCK_MAJOR ? G / 2 : G % 4;
};

template <int T, int P>
__device__ __forceinline__ void load_a(const float4* slot_lane, halfx8* a) {
  a[0] = __builtin_bit_cast(halfx8, slot_lane[(8 * T + 2 * P) * 64]);
  a[1] = __builtin_bit_cast(halfx8, slot_lane[(8 * T + 2 * P + 1) * 64]);
}

__device__ __forceinline__ floatx16 mfma(halfx8 a, halfx8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// One 2-k-step chunk against the 8 output blocks: 8 groups of 2 MFMAs; the A fragments of group g+1
// are read during group g (group 7 reads the next chunk's group 0 into s.pre); fill.step<g>() is VALU
// work placed in group g's MFMA issue gaps; M_c sits between groups 3 and 4.  SELF: group 0's
// fragments are read here (first chunk of a tile) instead of arriving in s.pre.
template <bool BLOCK_MAJOR, bool SELF, typename Fill>
__device__ __forceinline__ void run_chunk(State& s, float4* lds, int& c, halfx8 b0, halfx8 b1, Fill& fill) {
  const float4* slot = lds + (c & (kRing - 1)) * kChunkQuads + s.lane;
  const float4* nslot = lds + ((c + 1) & (kRing - 1)) * kChunkQuads + s.lane;
  const Dma dma = dma_for(s, lds, c);
  halfx8 a0[2], a1[2];
  if constexpr (SELF) {
    load_a<0, 0>(slot, a0);
  } else {
    a0[0] = s.pre[0];
    a0[1] = s.pre[1];
  }
  __builtin_amdgcn_sched_barrier(0);
#define CN_GROUP(G, CUR, NXT)                                                              \
  {                                                                                        \
    typedef GroupOf<BLOCK_MAJOR, (G)> g;                                                   \
    typedef GroupOf<BLOCK_MAJOR, ((G) + 1) % 8> n;                                         \
    if constexpr ((G) < 7) load_a<n::T, n::P>(slot, NXT);                                  \
    else load_a<0, 0>(nslot, s.pre);                                                       \
    const halfx8 b = g::T ? b1 : b0;                                                       \
    s.acc[2 * g::P] = mfma(CUR[0], b, s.acc[2 * g::P]);                                    \
    s.acc[2 * g::P + 1] = mfma(CUR[1], b, s.acc[2 * g::P + 1]);                            \
    dma.template piece<(G)>();                                                             \
    fill.template step<(G)>();                                                             \
    group_pattern<Fill::kValu, true, has_piece<(G)>()>();                                  \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    if constexpr ((G) == 3) chunk_barrier<kMidOut>();                                      \
  }
  CN_GROUP(0, a0, a1)
  CN_GROUP(1, a1, a0)
  CN_GROUP(2, a0, a1)
  CN_GROUP(3, a1, a0)
  CN_GROUP(4, a0, a1)
  CN_GROUP(5, a1, a0)
  CN_GROUP(6, a0, a1)
  CN_GROUP(7, a1, a0)
#undef CN_GROUP
  ++c;
}

// A 256-input layer: its bias, (layer_dir1: the view-direction chunk,) 7 k-major chunks on blocks
// 0..6 of the previous layer's operands, the block-major last chunk converting the finished blocks,
// then the last pair's conversion.
template <int LAYER>
__device__ __forceinline__ void layer_256(State& s, const FieldArgs& a, float4* lds, const float* blds, int& c) {
  constexpr bool relu = LAYER != kOut;   // fc_out's feat goes on without an activation
  constexpr bool sig = LAYER == kXyz2;   // its outputs are h2: sigma's operand
  init_acc<LAYER>(s, a, blds);
  NoFill nf;
  if constexpr (LAYER == kDir1) run_chunk<false, false>(s, lds, c, b_of(s.db), b_of(s.db + 4), nf);
#define CN_CHUNK(J) run_chunk<false, false>(s, lds, c, b_of(s.hb[J]), b_of(s.hb[J] + 4), nf);
  CN_CHUNK(0) CN_CHUNK(1) CN_CHUNK(2) CN_CHUNK(3) CN_CHUNK(4) CN_CHUNK(5) CN_CHUNK(6)
#undef CN_CHUNK
  ConvFill<relu, sig> cf{s, blds};
  if constexpr (sig) s.sig = 0.0f;
  run_chunk<true, false>(s, lds, c, b_of(s.hb[7]), b_of(s.hb[7] + 4), cf);
  conv_block<6, relu, sig>(s, blds);
  conv_block<7, relu, sig>(s, blds);
  if constexpr (sig) s.sigma = s.sig + __shfl_xor(s.sig, 32);
}

// One 128-sample tile: inputs, encodings, the six layers (chunks 0..35 of the stream, which also
// prefetch chunks 0..2 for the next tile), the raw store.
template <int MODE>
__device__ __forceinline__ void field_tile(State& s, const FieldArgs& a, float4* lds, float* blds, int64_t tile) {
  s.sig = 0.0f;
  s.sigma = 0.0f;
  const int64_t row = tile * kTile + s.wave * 32 + (s.lane & 31);
  const bool valid = row < a.m;
  const int64_t rc = valid ? row : a.m - 1;

  // ---- per-sample inputs and this wave's code row (ordinary loads; the DMA in flight -- chunks
  // 0..2 of this tile -- retires with them)
  const SampleIn in = decode_sample<MODE>(a, rc);
  s.crow = static_cast<int>(code_row(a, in.code_of));
  const int crow0 = __builtin_amdgcn_readfirstlane(s.crow);
  // wave-uniform by construction; readfirstlane makes it an SGPR so the bias fast/slow choice is a
  // scalar branch
  s.uniform_code = __builtin_amdgcn_readfirstlane(__ballot(s.crow != crow0) == 0 ? 1 : 0) != 0;
  float cbr[9];
  {
    const float* src = a.code_bias + (int64_t)crow0 * kCbStride;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int j = s.lane + 64 * k;
      cbr[k] = (s.uniform_code && j < kCbStride) ? src[j] : 0.0f;
    }
  }
  float enc[32];
  float dv[16];
  if constexpr (MODE == kFromEncoded) {
    const float* xr = a.x + rc * (kDimXyz + kDimDir);
    gather_pairs<15>(xr, 0, s.h, enc);
    gather_pairs<6>(xr, kDimXyz, s.h, dv);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every ordinary load has landed
  int c = 0;

  // ---- encodings (fp32 VALU), rounded to fp16 where the MFMAs read them
  if constexpr (MODE != kFromEncoded) {
    encode_pairs<15, 10>(in.x, a.fx, s.h, enc);
    encode_pairs<6, 4>(in.vd, a.fd, s.h, dv);
  }
  dv[14] = 0.0f;
  dv[15] = 0.0f;
#pragma unroll
  for (int q = 0; q < 16; ++q) s.xb[q] = pack_pair(enc[2 * q], enc[2 * q + 1]);
#pragma unroll
  for (int q = 0; q < 8; ++q) s.db[q] = pack_pair(dv[2 * q], dv[2 * q + 1]);
  // this wave's code row: read back only by this wave (LDS is in order per wave)
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int j = s.lane + 64 * k;
    if (j < kCbStride) blds[kConsts + s.wave * kCbStride + j] = cbr[k];
  }

  // ---- layer_xyz1 (63 -> 256): 4 k-steps of encoding
  {
    init_acc<kXyz1>(s, a, blds);
    NoFill nf;
    if (tile == static_cast<int64_t>(blockIdx.x)) {
      // the workgroup's first tile: chunk 0 was primed, no chunk before it read its first fragments
      run_chunk<false, true>(s, lds, c, b_of(s.xb), b_of(s.xb + 4), nf);
    } else {
      run_chunk<false, false>(s, lds, c, b_of(s.xb), b_of(s.xb + 4), nf);
    }
    ConvFill<true, false> cf{s, blds};
    run_chunk<true, false>(s, lds, c, b_of(s.xb + 8), b_of(s.xb + 12), cf);
    conv_block<6, true, false>(s, blds);
    conv_block<7, true, false>(s, blds);
  }

  layer_256<kXyz2>(s, a, lds, blds, c);
  layer_256<kOut>(s, a, lds, blds, c);
  layer_256<kDir1>(s, a, lds, blds, c);
  layer_256<kDir2>(s, a, lds, blds, c);

  // sigma's code / bias term (cn_code_bias: b_out[0] + W_out[0, 256:] zs2)
  if (s.uniform_code) s.sigma += lds_read1(blds + kConsts + s.wave * kCbStride + kCbSigma);
  else s.sigma += a.code_bias[(int64_t)s.crow * kCbStride + kCbSigma];

  // ---- fc_rgb (256 -> 3): one chunk holding its 16 k-steps of block 0 (fragment f = k-step f), on
  // four accumulators; it prefetches chunk 2 of the next tile like any other chunk
  {
    if (s.uniform_code) {
      const int i = s.lane & 31;
      const float v = lds_read1(blds + kConsts + s.wave * kCbStride + kCbRgb + (i < 3 ? i : 0));
      s.acc[0] = bias_mfma(s, i < 3 ? v : 0.0f);
    } else {
      init_acc_per_lane(s, a, kRgb);
    }
    s.acc[1] = floatx16{0};
    s.acc[2] = floatx16{0};
    s.acc[3] = floatx16{0};
    const Dma dma = dma_for(s, lds, c);
    const float4* slot = lds + (c & (kRing - 1)) * kChunkQuads + s.lane;
    const float4* nslot = lds + ((c + 1) & (kRing - 1)) * kChunkQuads + s.lane;
    // group 0's fragments (k-steps 0, 1) arrived in s.pre
#define CN_RGB(G)                                                                                          \
  {                                                                                                        \
    const halfx8 f0 = (G) == 0 ? s.pre[0] : __builtin_bit_cast(halfx8, slot[(2 * (G)) * 64]);              \
    const halfx8 f1 = (G) == 0 ? s.pre[1] : __builtin_bit_cast(halfx8, slot[(2 * (G) + 1) * 64]);          \
    s.acc[(2 * (G)) & 3] = mfma(f0, b_of(s.hb[G]), s.acc[(2 * (G)) & 3]);                                  \
    s.acc[(2 * (G) + 1) & 3] = mfma(f1, b_of(s.hb[G] + 4), s.acc[(2 * (G) + 1) & 3]);                      \
    dma.template piece<(G)>();                                                                             \
    if constexpr ((G) == 3) chunk_barrier<kMidOut>();                                                      \
  }
    CN_RGB(0) CN_RGB(1) CN_RGB(2) CN_RGB(3) CN_RGB(4) CN_RGB(5) CN_RGB(6) CN_RGB(7)
#undef CN_RGB
    load_a<0, 0>(nslot, s.pre);  // the next tile's chunk 0 (landed: M_35)
    ++c;
  }

  if (valid && s.h == 0) {
    float4 o;
    o.x = (s.acc[0][0] + s.acc[1][0]) + (s.acc[2][0] + s.acc[3][0]);
    o.y = (s.acc[0][1] + s.acc[1][1]) + (s.acc[2][1] + s.acc[3][1]);
    o.z = (s.acc[0][2] + s.acc[1][2]) + (s.acc[2][2] + s.acc[3][2]);
    o.w = s.sigma;
    reinterpret_cast<float4*>(a.raw)[row] = o;
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads, 1) void field_f16_kernel(FieldArgs a) {
  // ONE LDS object (a second one makes hipcc wait vmcnt(0) before every ring read): the DMA ring,
  // then the constant vectors and code rows
  __shared__ __attribute__((aligned(16))) float4 lds[kLdsQuads + kBiasLds / 4];
  float* blds = reinterpret_cast<float*>(lds + kLdsQuads);
  State s;
  s.lane = threadIdx.x & 63;
  s.h = s.lane >> 5;
  s.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  s.wsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.packed), 0, kPackedFloats * 4, 0x00020000);
  s.voff = static_cast<unsigned>(s.wave * 64 + s.lane) * 16u;

  // constant vectors (biases, sigma weights) once per workgroup, then prime the ring
#pragma unroll
  for (int k = 0; k < kConsts / kThreads; ++k) blds[k * kThreads + threadIdx.x] = a.packed[kBiasXyz1 + k * kThreads + threadIdx.x];
  __syncthreads();
  // prime: chunks 0 and 1 and pieces 0, 1 of chunk 2 (chunk 0's groups 0, 1 issue the rest)
#pragma unroll
  for (int i = 0; i < kDmaPerWave; ++i) dma_piece(s, lds, 0, i);
#pragma unroll
  for (int i = 0; i < kDmaPerWave; ++i) dma_piece(s, lds, 1, i);
#pragma unroll
  for (int i = 0; i < kDmaPerWave / 2; ++i) dma_piece(s, lds, 2, i);
  // chunk 0 landed for every wave before any wave reads it (later chunks: M_c)
  asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");

  const int64_t n_tiles = (a.m + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) field_tile<MODE>(s, a, lds, blds, tile);
  // the last tile prefetched chunks 0..2 of a tile that does not exist: they must land before the
  // workgroup's LDS is released
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

static_assert(kDmaPerWave == 4, "DMA pieces per wave and chunk: groups 0, 1, 4, 5");
static_assert(kChunks % kRing == 0, "cyclic stream: chunk c + 36 reuses chunk c's ring slot");
static_assert(kBiasLds * 4 + kLdsQuads * 16 <= 160 * 1024, "LDS budget");
static_assert(kBiasLds % 4 == 0, "the constants follow the ring as whole quads");

}  // namespace f16

int64_t packed_floats_f16() { return f16::kPackedFloats; }

int launch_pack_f16(const Params& P, float* packed, hipStream_t st) {
  const int64_t n = (int64_t)f16::kQuads * 8 + f16::kConsts;
  hipLaunchKernelGGL(f16::pack_f16_kernel, dim3(cn::elementwise_grid(n, 256)), dim3(256), 0, st, P, packed);
  return cn::launch_status();
}

int launch_field_f16(int mode, FieldArgs& a, hipStream_t st) {
  const dim3 grid(cn::persistent_grid(a.m, f16::kTile)), b(f16::kThreads);
  return launch_any_mode(mode, [&](auto M) {
    hipLaunchKernelGGL(f16::field_f16_kernel<M.value>, grid, b, 0, st, a);
  });
}

}  // namespace mlp
}  // namespace cn
