// What the streamed field kernels share: the LDS reads and waits that keep hipcc from draining the
// LDS-DMA ring, the one LDS-DMA instruction, the 32x32 family's chunk schedule and bias paths, and the
// 16x16 family's stream layout and encoding maps.
// The kernels, their MFMA groups and their per-variant piece schedules stay in mlp_x3.hip,
// mlp_f16.hip, mlp_x3w.hip and mlp_f32.hip; DESIGN ("One header for the weight stream") lists what
// was left per variant and why.
#pragma once

#include "mlp_common.h"

namespace cn {
namespace mlp {

// ---------------------------------------------------------------- stateless helpers
namespace stream {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ float vmax(float x, float lo) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(lo));
  return r;
}

__device__ __forceinline__ unsigned short bf16_bits(float x) {
  const __bf16 b = static_cast<__bf16>(x);
  return __builtin_bit_cast(unsigned short, b);
}

// One LDS-DMA wave-instruction: 1 KiB (16 B per lane) from quads [q, q + 64 * waves) of packed chunk
// `src` into the same quads of ring slot cn & (RING - 1); this wave moves quads q + wave * 64 + lane
// (voff = (wave * 64 + lane) * 16).  The source offset is wave-uniform: readfirstlane puts it in an
// SGPR, the instruction's scalar offset.
template <int CHUNK_QUADS, int RING>
__device__ __forceinline__ void dma_quads(__amdgpu_buffer_rsrc_t rsrc, int wave, unsigned voff, float4* lds, int cn,
                                          int src, int q) {
  const unsigned soff = __builtin_amdgcn_readfirstlane((unsigned)(src * CHUNK_QUADS + q) * 16u);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(lds + (cn & (RING - 1)) * CHUNK_QUADS + q + wave * 64),
                                           16, voff, soff, 0, 0);
}

// M_c: chunk c+1 landed for every wave (all but this wave's OUT youngest DMA
// pieces retired), every wave is past chunk c-1, and every LDS read of this
// wave (incl. the asynchronous sigma-weight reads) has returned.  One asm
// statement, so no LDS read can be scheduled across it.
template <int OUT>
__device__ __forceinline__ void chunk_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(OUT) : "memory");
  __builtin_amdgcn_sched_barrier(0);  // nothing (ring reads included) is scheduled above the wait
}

// Small LDS reads outside the ring (biases, sigma weights).  Inline asm: hipcc
// cannot prove them disjoint from the in-flight DMA and would otherwise wait
// vmcnt(0), draining the ring.
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return static_cast<unsigned>(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) void*)p));
}

// 8 floats at p + 32*ob (ob = 0..7), one LDS round trip.
__device__ __forceinline__ void lds_read8_stride32(const float* p, float* v) {
  asm volatile(
      "ds_read_b32 %0, %8\n\tds_read_b32 %1, %8 offset:128\n\tds_read_b32 %2, %8 offset:256\n\t"
      "ds_read_b32 %3, %8 offset:384\n\tds_read_b32 %4, %8 offset:512\n\tds_read_b32 %5, %8 offset:640\n\t"
      "ds_read_b32 %6, %8 offset:768\n\tds_read_b32 %7, %8 offset:896\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
      : "v"(lds_addr(p))
      : "memory");
}

// 16 consecutive floats (64 B aligned), one LDS round trip.
__device__ __forceinline__ void lds_read16(const float* p, float* v) {
  u32x4 a, b, c, d;
  asm volatile(
      "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\t"
      "ds_read_b128 %3, %4 offset:48\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
      : "v"(lds_addr(p))
      : "memory");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = __uint_as_float(a[i]);
    v[4 + i] = __uint_as_float(b[i]);
    v[8 + i] = __uint_as_float(c[i]);
    v[12 + i] = __uint_as_float(d[i]);
  }
}

// The same without a wait: the values are first used after the next chunk
// barrier, whose lgkmcnt(0) covers them (volatile asm keeps the order).
__device__ __forceinline__ void lds_read16_async(const float* p, float* v) {
  u32x4 a, b, c, d;
  asm volatile(
      "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\t"
      "ds_read_b128 %3, %4 offset:48"
      : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
      : "v"(lds_addr(p))
      : "memory");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = __uint_as_float(a[i]);
    v[4 + i] = __uint_as_float(b[i]);
    v[8 + i] = __uint_as_float(c[i]);
    v[12 + i] = __uint_as_float(d[i]);
  }
}

__device__ __forceinline__ float lds_read1(const float* p) {
  float v;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(lds_addr(p)) : "memory");
  return v;
}

}  // namespace stream

// ---------------------------------------------------------------- the 32x32 family's layout
// mlp_x3.hip and mlp_f16.hip: 36 chunks of 2 k-steps x 8 output blocks in one order, the same
// constants after the stream, the same bias paths.  A chunk's size (hi / lo fragments or one) and
// its piece schedule are the variant's own.
namespace stream32 {

// stream: xyz1 2 | xyz2 8 | fc_out 8 | layer_dir1 view-dir k-steps 1 | layer_dir1 8 | layer_dir2 8 | fc_rgb 1
constexpr int kChunkL1 = 2, kChunkL2 = 10, kChunkDir = 18, kChunkL3 = 19, kChunkL4 = 27, kChunkRgb = 35;
constexpr int kChunks = 36;
constexpr int kSigmaOff = 768;         // after b_xyz1, b_dir1, b_dir2: fc_out row 0 over h2, [h][b][reg]
constexpr int kConsts = 1024;

static_assert(kChunkRgb + 1 == kChunks, "chunk schedule");

// Input feature of lane half h, element j, k-step s of layer l (-1 = zero pad).
__host__ __device__ constexpr int in_col(int l, int s, int h, int j) {
  if (l == kXyz1) return k_from_enc(8 * s + j, h, 15);
  if (l == kDir1 && s >= 16) {
    const int t = 8 * (s - 16) + j;
    if (t >= 14) return -1;
    const int e = k_from_enc(t, h, 6);
    return e < 0 ? -1 : kCode + e;
  }
  return acc_row(s >> 1, 8 * (s & 1) + j, h);
}

// (chunk, step-in-chunk T, slot j) -> (layer, k-step, output block)
__device__ void chunk_map(int c, int T, int j, int& l, int& ks, int& ob) {
  ob = j;
  if (c < kChunkL1) { l = kXyz1; ks = 2 * c + T; }
  else if (c < kChunkL2) { l = kXyz2; ks = 2 * (c - kChunkL1) + T; }
  else if (c < kChunkDir) { l = kOut; ks = 2 * (c - kChunkL2) + T; }
  else if (c == kChunkDir) { l = kDir1; ks = 16 + T; }
  else if (c < kChunkL4) { l = kDir1; ks = 2 * (c - kChunkL3) + T; }
  else if (c < kChunkRgb) { l = kDir2; ks = 2 * (c - kChunkL4) + T; }
  else { l = kRgb; ks = 8 * T + j; ob = 0; }
}

// Chunk counter c + 2 or c + 3 wrapped into the next tile's first chunks (kChunks is a multiple of
// the ring, so the ring slot is unchanged by the wrap).
__device__ __forceinline__ int wrap_chunk(int c) { return c < kChunks ? c : c - kChunks; }

// Bias vector of `layer` for this lane's 8 blocks.
template <typename S>
__device__ __forceinline__ void bias_values(const S& s, const float* blds, int layer, float* v) {
  const bool per_code = (layer == kXyz2 || layer == kOut);
  const float* src = per_code ? blds + kConsts + s.wave * kCbStride + (layer == kXyz2 ? kCbXyz2 : kCbFeat)
                              : blds + (layer == kXyz1 ? 0 : (layer == kDir1 ? 256 : 512));
  stream::lds_read8_stride32(src + (s.lane & 31), v);
}

// Slow path (a wave whose samples use several code rows): per-lane loads.
template <typename S>
__device__ __forceinline__ void init_acc_per_lane(S& s, const FieldArgs& a, int layer) {
  const float* base = a.code_bias + (int64_t)s.crow * kCbStride;
  if (layer == kRgb) {
    s.acc[0] = floatx16{0};
    if (s.h == 0) {
      s.acc[0][0] = base[kCbRgb];
      s.acc[0][1] = base[kCbRgb + 1];
      s.acc[0][2] = base[kCbRgb + 2];
    }
  } else {
    const float* b = base + (layer == kXyz2 ? kCbXyz2 : kCbFeat);
#pragma unroll
    for (int ob = 0; ob < 8; ++ob) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(b + 32 * ob + 8 * q + 4 * s.h);
        s.acc[ob][4 * q + 0] = v.x;
        s.acc[ob][4 * q + 1] = v.y;
        s.acc[ob][4 * q + 2] = v.z;
        s.acc[ob][4 * q + 3] = v.w;
      }
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): nothing pending leaks out
}

}  // namespace stream32

// ---------------------------------------------------------------- the 16x16 family's layout
// mlp_f32.hip (w16) and mlp_x3w.hip: 8 waves of 16 samples, 36 chunks of 32 KiB in one order through
// a 4-slot ring in 4 pieces per wave, the same constants after the stream, the same encoding maps.
namespace stream16 {

constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kTile = 16 * kWaves;         // samples per workgroup tile
constexpr int kChunkQuads = 32 * 64;       // 2048 float4 = 32 KiB
constexpr int kRing = 4;
constexpr int kPiecesPerWave = kChunkQuads / (64 * kWaves);   // 4 x 1 KiB per wave per chunk
// the stream: xyz1 2 | xyz2 8 | fc_out 8 | dir1 8 | dir1 view-dir 1 | dir2 8 | rgb 1
constexpr int kCL2 = 2, kCL3 = 10, kCL4 = 18, kCDir = 26, kCL5 = 27, kCRgb = 35, kChunks = 36;
constexpr int kStreamFloats = kChunks * kChunkQuads * 4;
// constants after the stream: b_xyz1 | b_dir1 | b_dir2 | sigma weights (fc_out row 0 over
// h2, [g][ob][r] = W_out[0][16 ob + 4 g + r])
constexpr int kCB1 = 0, kCBD1 = 256, kCBD2 = 512, kCSig = 768, kConsts = 1024;

static_assert(kChunks % kRing == 0, "cyclic stream: chunk c + 36 reuses chunk c's ring slot");
static_assert(kPiecesPerWave == 4, "4 DMA wave-instructions per chunk per wave");

// xyz encoding column (position_embed.py:44-53: x_d -> d, sin(f_k x_d) -> 3+6k+d,
// cos(f_k x_d) -> 6+6k+d) fed at k-step t (0..15) by lane group g: sines of pairs
// p = 4i + g at t = i, cosines at t = 8 + i; groups 2, 3 have 7 pairs and put the raw
// inputs in the free k-steps 7 / 15 (x0, x1 | x2, pad).
__host__ __device__ constexpr int col_enc_xyz(int t, int g) {
  const int i = t & 7, p = 4 * i + g;
  if (p < 30) return (t < 8 ? 3 : 6) + 6 * (p / 3) + p % 3;
  return t < 8 ? (g == 2 ? 0 : 2) : (g == 2 ? 1 : -1);
}

// View-direction encoding column (27 wide) at k-step s (0..6) of the view-dir chunk:
// sines of pairs p = 4i + g at s = i (i < 3), cosines at s = 3 + i, raw component g at s = 6.
__host__ __device__ constexpr int col_enc_dir(int s, int g) {
  if (s < 6) {
    const int p = 4 * (s % 3) + g;
    return (s < 3 ? 3 : 6) + 6 * (p / 3) + p % 3;
  }
  return (s == 6 && g < 3) ? g : -1;
}

}  // namespace stream16

}  // namespace mlp
}  // namespace cn
