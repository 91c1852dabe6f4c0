// Iso-surface extraction on the device: a node grid (N, N, N) -- what density_grid leaves in HBM -- to
// a triangle mesh, by marching tetrahedra on the Kuhn split of each cell.  include/codenerf.h holds the
// semantics; tests/isosurface_cases.py states them in numpy and every result equals that bit for bit.
//
// Five launches over the nodes in workgroups of kBlock consecutive node indices (coalesced along iz),
// in the compaction idiom of occupancy.hip -- classify, scan, emit:
//   classify  node -> its word: the 7-bit mask of the active edges it owns, its cell's triangle count
//             and the cell's 8 inside bits; and the workgroup's vertex and triangle sums;
//   scan      two workgroups, one per sum array: exclusive prefix sums in rounds of kScanPart with the
//             running total carried over, as occupancy_scan_kernel; the totals are V and T;
//   offsets   node -> its exclusive vertex and face offsets: a scan inside the workgroup on top of
//             the workgroup's offset;
//   vertices  node -> the vertices of its active edges, at offset + rank of the edge bit in the mask;
//   faces     cell (the thread of its lower node) -> its triangles; the vertex id of edge (a, d) is
//             offset[a] + popcount(mask[a] below bit d), read from the neighbours' words.
// The first three are cn_isosurface_count, the last two cn_isosurface_emit, which only reads the
// workspace.  No atomics, no workgroup waits on another, plain vector stores, no LDS beyond the
// wave sums of a workgroup.  All bandwidth / latency bound.
#include <limits.h>
#include <math.h>

#include "cn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMinN = 2, kMaxN = 513;      // 513^3 * 7 vertices and 512^3 * 12 faces are below 2^31
constexpr int kBlock = 256;                // nodes per workgroup
constexpr int kScanThreads = 1024;
constexpr int kScanPerThread = 4;
constexpr int kScanPart = kScanThreads * kScanPerThread;   // workgroup sums per scan round (4096)

// The node word: bits 0..6 the active-edge mask (bit d: the edge to corner d + 1), bits 7..10 the
// cell's triangle count (0..12), bits 11..18 the cell's inside bits (bit 11 + k: corner k).
constexpr int kTriShift = 7, kCornerShift = 11;

inline bool size_ok(int64_t n) { return n >= kMinN && n <= kMaxN; }
__host__ __device__ inline int64_t pad16(int64_t bytes) { return (bytes + 15) / 16 * 16; }
inline int64_t n_blocks(int64_t nodes) { return (nodes + kBlock - 1) / kBlock; }

// Workspace: words (int32 per node) | vertex offsets (per node) | face offsets (per node) | vertex
// sums (per workgroup) | face sums (per workgroup), each padded to 16 B.
struct Workspace {
  uint32_t* words;
  int* voff;
  int* foff;
  int* sums;               // the vertex sums, then (sums_stride ints on) the face sums
  int64_t sums_stride;
};

inline Workspace carve(void* workspace, int64_t nodes) {
  char* p = static_cast<char*>(workspace);
  const int64_t per_node = pad16(4 * nodes), per_block = pad16(4 * n_blocks(nodes));
  Workspace w;
  w.words = reinterpret_cast<uint32_t*>(p);
  w.voff = reinterpret_cast<int*>(p + per_node);
  w.foff = reinterpret_cast<int*>(p + 2 * per_node);
  w.sums = reinterpret_cast<int*>(p + 3 * per_node);
  w.sums_stride = per_block / 4;
  return w;
}

// ---- the split and its triangle table, derived at compile time from the rule of the header

// Corner j of tetrahedron tet, as a cube corner: tet is the tet-th permutation (a, b, c) of the axes
// (x, y, z) in lexicographic order; the corners are 0, bit(a), bit(a) | bit(b), 7; bit(x, y, z) = 4, 2, 1.
__host__ __device__ constexpr int tet_corner(int tet, int j) {
  const int a = tet / 2;
  const int b = tet % 2 ? (a == 2 ? 1 : 2) : (a == 0 ? 1 : 0);
  return j == 0 ? 0 : j == 1 ? (4 >> a) : j == 2 ? ((4 >> a) | (4 >> b)) : 7;
}

__host__ __device__ constexpr int corner_axis(int k, int c) { return (k >> (2 - c)) & 1; }

// A triangle is 3 edges of 6 bits (owner corner k | direction d << 3, the edge from corner k to corner
// k + d + 1), edge j in bits 6 j .. 6 j + 5, and bit 18 set; 0 is no triangle.
struct TriTable {
  uint32_t tri[6][16][2];
  bool oriented;           // no triangle had a normal at right angles to the inside -> outside direction
};

constexpr uint32_t kTriValid = 1u << 18;

constexpr TriTable make_tri_table() {
  TriTable t{};
  t.oriented = true;
  for (int tet = 0; tet < 6; ++tet)
    for (int p = 0; p < 16; ++p) {
      int in[4] = {}, out[4] = {}, ni = 0, no = 0;
      for (int j = 0; j < 4; ++j) {
        if ((p >> j) & 1) in[ni++] = j; else out[no++] = j;
      }
      // the rule's triangles as pairs of tetrahedron corners
      int e[2][3][2] = {};
      int count = 0;
      if (ni == 1 || ni == 3) {
        const int l = ni == 1 ? in[0] : out[0];
        const int* rest = ni == 1 ? out : in;                 // P < Q < R
        for (int j = 0; j < 3; ++j) { e[0][j][0] = l; e[0][j][1] = rest[j]; }
        count = 1;
      } else if (ni == 2) {
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        const int q[2][3][2] = {{{a, c}, {a, d}, {b, d}}, {{a, c}, {b, d}, {b, c}}};
        for (int r = 0; r < 2; ++r)
          for (int j = 0; j < 3; ++j) { e[r][j][0] = q[r][j][0]; e[r][j][1] = q[r][j][1]; }
        count = 2;
      }
      for (int r = 0; r < count; ++r) {
        // twice the midpoints; the direction (outside centroid - inside centroid) scaled by ni no
        int m[3][3] = {}, dir[3] = {};
        for (int c = 0; c < 3; ++c) {
          for (int j = 0; j < 3; ++j)
            m[j][c] = corner_axis(tet_corner(tet, e[r][j][0]), c) + corner_axis(tet_corner(tet, e[r][j][1]), c);
          int si = 0, so = 0;
          for (int j = 0; j < ni; ++j) si += corner_axis(tet_corner(tet, in[j]), c);
          for (int j = 0; j < no; ++j) so += corner_axis(tet_corner(tet, out[j]), c);
          dir[c] = so * ni - si * no;
        }
        const int u[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]};
        const int v[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
        const int dot = (u[1] * v[2] - u[2] * v[1]) * dir[0] + (u[2] * v[0] - u[0] * v[2]) * dir[1] +
                        (u[0] * v[1] - u[1] * v[0]) * dir[2];
        if (dot == 0) t.oriented = false;
        const int order[3] = {0, dot > 0 ? 1 : 2, dot > 0 ? 2 : 1};
        uint32_t word = kTriValid;
        for (int j = 0; j < 3; ++j) {
          const int i0 = e[r][order[j]][0], i1 = e[r][order[j]][1];
          const int lo = tet_corner(tet, i0 < i1 ? i0 : i1), hi = tet_corner(tet, i0 < i1 ? i1 : i0);
          word |= static_cast<uint32_t>(lo | ((hi - lo - 1) << 3)) << (6 * j);
        }
        t.tri[tet][p][r] = word;
      }
    }
  return t;
}

constexpr TriTable kTriTable = make_tri_table();
static_assert(kTriTable.oriented, "a triangle of the table has no orientation");

// ---- per-node work

// Linear node step to cube corner k.
__host__ __device__ __forceinline__ unsigned corner_step(unsigned k, unsigned n) {
  return (((k >> 2) & 1u) * n + ((k >> 1) & 1u)) * n + (k & 1u);
}

// Triangles of a tetrahedron with s of its 4 corners inside: 0, 1, 2, 1, 0.
__host__ __device__ __forceinline__ unsigned tet_triangles(unsigned s) { return s == 2u ? 2u : (s & 1u); }

__host__ __device__ __forceinline__ unsigned tet_pattern(unsigned corners, int tet) {
  return ((corners >> tet_corner(tet, 0)) & 1u) | (((corners >> tet_corner(tet, 1)) & 1u) << 1) |
         (((corners >> tet_corner(tet, 2)) & 1u) << 2) | (((corners >> tet_corner(tet, 3)) & 1u) << 3);
}

// The word of node idx = (ix n + iy) n + iz.  A corner is read only where it is inside the grid.
__host__ __device__ __forceinline__ uint32_t classify_node(const float* __restrict__ nodes, unsigned n, float iso, unsigned idx) {
  const unsigned iz = idx % n, iy = (idx / n) % n, ix = idx / (n * n);
  const unsigned high = (ix + 1 < n ? 4u : 0u) | (iy + 1 < n ? 2u : 0u) | (iz + 1 < n ? 1u : 0u);
  const unsigned in0 = nodes[idx] > iso ? 1u : 0u;
  unsigned corners = in0, mask = 0;
#pragma unroll
  for (unsigned k = 1; k < 8; ++k) {
    if ((k & high) == k) {
      const unsigned in = nodes[idx + corner_step(k, n)] > iso ? 1u : 0u;
      corners |= in << k;
      mask |= (in ^ in0) << (k - 1);
    }
  }
  unsigned tris = 0;
  if (high == 7u) {
#pragma unroll
    for (int tet = 0; tet < 6; ++tet) tris += tet_triangles(__builtin_popcount(tet_pattern(corners, tet)));
  }
  return mask | (tris << kTriShift) | (corners << kCornerShift);
}

// Vertices in the low half, triangles in the high half: a workgroup's sums (<= 1792 and <= 3072) and
// every partial sum on the way stay inside their halves.
__host__ __device__ __forceinline__ unsigned packed_counts(uint32_t word) {
  return __builtin_popcount(word & 127u) | (((word >> kTriShift) & 15u) << 16);
}

__global__ __launch_bounds__(kBlock) void isosurface_classify_kernel(const float* __restrict__ nodes, unsigned n,
                                                                     unsigned total, float iso,
                                                                     uint32_t* __restrict__ words, int* __restrict__ vsums,
                                                                     int* __restrict__ fsums) {
  __shared__ unsigned s_wave[kBlock / 64];
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  uint32_t word = 0;
  if (idx < total) {
    word = classify_node(nodes, n, iso, idx);
    words[idx] = word;
  }
  unsigned sum = packed_counts(word);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
#pragma unroll
    for (int k = 0; k < kBlock / 64; ++k) all += s_wave[k];
    vsums[blockIdx.x] = static_cast<int>(all & 0xffffu);
    fsums[blockIdx.x] = static_cast<int>(all >> 16);
  }
}

// Workgroup b scans sum array b (0 the vertices, 1 the faces) in place to exclusive offsets, a
// partition of kScanPart per round with the running total carried over; counts[b] = the total.
__global__ __launch_bounds__(kScanThreads) void isosurface_scan_kernel(int* __restrict__ sums, int64_t stride,
                                                                        int64_t n_sums, int64_t* __restrict__ counts) {
  __shared__ int s_wave[kScanThreads / 64];
  int* __restrict__ a = sums + blockIdx.x * stride;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int64_t base = 0; base < n_sums; base += kScanPart) {
    const int64_t i0 = base + static_cast<int64_t>(tid) * kScanPerThread;
    int v[kScanPerThread];
    int t = 0;
#pragma unroll
    for (int q = 0; q < kScanPerThread; ++q) {
      v[q] = i0 + q < n_sums ? a[i0 + q] : 0;
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
      if (i0 + q < n_sums) a[i0 + q] = run;
      run += v[q];
    }
    carry += all;
    __syncthreads();                       // s_wave is rewritten next round
  }
  if (tid == 0) counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kBlock) void isosurface_offsets_kernel(const uint32_t* __restrict__ words, unsigned total,
                                                                    const int* __restrict__ vsums,
                                                                    const int* __restrict__ fsums, int* __restrict__ voff,
                                                                    int* __restrict__ foff) {
  __shared__ unsigned s_wave[kBlock / 64];
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned own = idx < total ? packed_counts(words[idx]) : 0u;
  unsigned incl = own;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned u = __shfl_up(incl, off);
    if (lane >= off) incl += u;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  unsigned before = 0;
#pragma unroll
  for (int k = 0; k < kBlock / 64; ++k) before += k < wv ? s_wave[k] : 0u;
  const unsigned excl = before + incl - own;
  if (idx < total) {
    voff[idx] = vsums[blockIdx.x] + static_cast<int>(excl & 0xffffu);
    foff[idx] = fsums[blockIdx.x] + static_cast<int>(excl >> 16);
  }
}

// The vertices of node idx: t = (iso - v_a) / (v_b - v_a), pos_c = axis[a_c] + t (axis[b_c] - axis[a_c]),
// each operation rounded (contraction is off), a true division.  Row id is stored only below max_vertices.
__host__ __device__ __forceinline__ void node_vertices(const float* __restrict__ nodes, const float* __restrict__ axis,
                                                       unsigned n, float iso, const uint32_t* __restrict__ words,
                                                       const int* __restrict__ voff, int64_t max_vertices,
                                                       float* __restrict__ vertices, unsigned idx) {
  const unsigned mask = words[idx] & 127u;
  if (mask == 0) return;
  int64_t id = voff[idx];
  const unsigned iz = idx % n, iy = (idx / n) % n, ix = idx / (n * n);
  const float va = nodes[idx];
  const float num = iso - va;
  const float ax = axis[ix], ay = axis[iy], az = axis[iz];
  // an edge bit is set only where its upper node is inside the grid, so index + 1 is a node too
#pragma unroll
  for (unsigned k = 1; k < 8; ++k) {
    if ((mask >> (k - 1)) & 1u) {
      if (id >= max_vertices) return;
      const float t = num / (nodes[idx + corner_step(k, n)] - va);
      const float bx = (k & 4u) ? axis[ix + 1] : ax;
      const float by = (k & 2u) ? axis[iy + 1] : ay;
      const float bz = (k & 1u) ? axis[iz + 1] : az;
      float* row = vertices + 3 * id;
      row[0] = ax + t * (bx - ax);
      row[1] = ay + t * (by - ay);
      row[2] = az + t * (bz - az);
      ++id;
    }
  }
}

__global__ __launch_bounds__(kBlock) void isosurface_vertices_kernel(const float* __restrict__ nodes,
                                                                     const float* __restrict__ axis, unsigned n,
                                                                     unsigned total, float iso,
                                                                     const uint32_t* __restrict__ words,
                                                                     const int* __restrict__ voff, int64_t max_vertices,
                                                                     float* __restrict__ vertices) {
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx < total) node_vertices(nodes, axis, n, iso, words, voff, max_vertices, vertices, idx);
}

// The triangles of the cell whose lower node is idx (a node of a top face has triangle count 0).  Every
// edge of a cell's tetrahedra is owned by one of the cell's corners 0..6, all nodes of the grid.  Row f
// is stored only below max_faces.
__host__ __device__ __forceinline__ void cell_faces(unsigned n, const uint32_t* __restrict__ words,
                                                    const int* __restrict__ voff, const int* __restrict__ foff,
                                                    int64_t max_faces, int* __restrict__ faces, unsigned idx) {
  const uint32_t word = words[idx];
  if (((word >> kTriShift) & 15u) == 0) return;
  const unsigned corners = (word >> kCornerShift) & 255u;
  int64_t f = foff[idx];
#pragma unroll
  for (int tet = 0; tet < 6; ++tet) {
    const unsigned p = tet_pattern(corners, tet);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const uint32_t tri = kTriTable.tri[tet][p][r];
      if (tri & kTriValid) {
        if (f >= max_faces) return;
        int id[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const unsigned e = (tri >> (6 * j)) & 63u;
          const unsigned a = idx + corner_step(e & 7u, n);
          id[j] = voff[a] + __builtin_popcount(words[a] & ((1u << (e >> 3)) - 1u));
        }
        // cyclically, the smallest id first
        int v0 = id[0], v1 = id[1], v2 = id[2];
        if (id[1] < id[0] && id[1] < id[2]) {
          v0 = id[1]; v1 = id[2]; v2 = id[0];
        } else if (id[2] < id[0] && id[2] < id[1]) {
          v0 = id[2]; v1 = id[0]; v2 = id[1];
        }
        int* row = faces + 3 * f;
        row[0] = v0;
        row[1] = v1;
        row[2] = v2;
        ++f;
      }
    }
  }
}


// One thread per cell: the thread of its lower node.
__global__ __launch_bounds__(kBlock) void isosurface_faces_kernel(unsigned n, unsigned total,
                                                                  const uint32_t* __restrict__ words,
                                                                  const int* __restrict__ voff,
                                                                  const int* __restrict__ foff, int64_t max_faces,
                                                                  int* __restrict__ faces) {
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx < total) cell_faces(n, words, voff, foff, max_faces, faces, idx);
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" int64_t cn_isosurface_workspace_bytes(int64_t n) {
  if (!size_ok(n)) return -1;
  const int64_t nodes = n * n * n;
  return 3 * pad16(4 * nodes) + 2 * pad16(4 * n_blocks(nodes));
}

extern "C" int cn_isosurface_count(const float* nodes, int64_t n, float iso, void* workspace, int64_t* counts,
                                   cn_stream_t stream) {
  CN_CHECK_ARG(nodes && workspace && counts && size_ok(n) && isfinite(iso));
  CN_CHECK_ARG(aligned8(workspace) && aligned8(counts));
  const int64_t total = n * n * n;
  const unsigned blocks = static_cast<unsigned>(n_blocks(total));
  const Workspace w = carve(workspace, total);
  int* vsums = w.sums;
  int* fsums = w.sums + w.sums_stride;
  hipStream_t st = cn::as_stream(stream);
  hipLaunchKernelGGL(isosurface_classify_kernel, dim3(blocks), dim3(kBlock), 0, st, nodes, static_cast<unsigned>(n),
                     static_cast<unsigned>(total), iso, w.words, vsums, fsums);
  hipLaunchKernelGGL(isosurface_scan_kernel, dim3(2), dim3(kScanThreads), 0, st, w.sums, w.sums_stride,
                     static_cast<int64_t>(blocks), counts);
  hipLaunchKernelGGL(isosurface_offsets_kernel, dim3(blocks), dim3(kBlock), 0, st, w.words,
                     static_cast<unsigned>(total), vsums, fsums, w.voff, w.foff);
  return cn::launch_status();
}

extern "C" int cn_isosurface_emit(const float* nodes, const float* axis, int64_t n, float iso, const void* workspace,
                                  int64_t max_vertices, int64_t max_faces, float* vertices, int32_t* faces,
                                  cn_stream_t stream) {
  CN_CHECK_ARG(nodes && axis && workspace && size_ok(n) && isfinite(iso) && aligned8(workspace));
  CN_CHECK_ARG(max_vertices >= 0 && max_faces >= 0 && (vertices || max_vertices == 0) && (faces || max_faces == 0));
  const int64_t total = n * n * n;
  const unsigned blocks = static_cast<unsigned>(n_blocks(total));
  const Workspace w = carve(const_cast<void*>(workspace), total);
  hipStream_t st = cn::as_stream(stream);
  if (max_vertices > 0)
    hipLaunchKernelGGL(isosurface_vertices_kernel, dim3(blocks), dim3(kBlock), 0, st, nodes, axis,
                       static_cast<unsigned>(n), static_cast<unsigned>(total), iso, w.words, w.voff, max_vertices,
                       vertices);
  if (max_faces > 0)
    hipLaunchKernelGGL(isosurface_faces_kernel, dim3(blocks), dim3(kBlock), 0, st, static_cast<unsigned>(n),
                       static_cast<unsigned>(total), w.words, w.voff, w.foff, max_faces, faces);
  return cn::launch_status();
}
