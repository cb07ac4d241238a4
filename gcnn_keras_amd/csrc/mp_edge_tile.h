// The receiver-tile walk of the fused edge steps (csrc/mp_egnn.hip, mp_cgcnn.hip, mp_megnet.hip): per-receiver sums over a
// receiver-sorted edge list without atomics, so that two runs give equal bits.  Header-only: no kernels, no entry points.
//
// One workgroup walks tiles of TE sorted positions (position p is edge perm0[p]; ptr0 is the receivers' CSR over
// positions); one thread per output column adds the tile's values in list order.  When a receiver's segment ends, a
// receiver whose whole range [s0, s1) lies inside the tile is stored directly into the (N, W) output; one cut by a tile
// boundary leaves its partial sum in the (tiles, 2, W) workspace.  THE SLOT RULE: the first segment of a tile uses slot 0
// (head), any later one slot 1 (tail).  Only a tile's first and last segment can be cut, so the two never collide, and a
// receiver that owns a whole tile is its first segment.  The finishing kernel of each route takes a cut receiver's sum
// from cut_sum(): slot 0 of its first tile when its range starts on that tile's first position, else slot 1, plus slot 0
// of every later tile, added in tile order.
#pragma once
#include "mp_common.h"

namespace mp_tile {

constexpr int TE = 32;   // sorted positions per tile

// host side: tiles, bytes of the (tiles, 2, W) float workspace, and the sizes the kernels index with 32 bits
inline int64_t tiles_of(int64_t E) { return (E + TE - 1) / TE; }
inline size_t ws_bytes(int64_t E, int W) { return sizeof(float) * 2 * W * static_cast<size_t>(tiles_of(E)); }
inline bool sizes_ok(int64_t N, int64_t E) {
  return N >= 0 && E >= 0 && N < (int64_t(1) << 31) - 1 && E < (int64_t(1) << 31) - TE;
}

// Phase 0, thread t < TE: position p0 + t of a tile with nv valid positions -> receiver, sender, edge id.  r = -1 marks a
// row the tile skips: t >= nv, an edge id outside [0, E) (then e = 0) or a receiver or sender outside [0, N) (then s = 0).
struct Pos { int r, s, e; };
__device__ __forceinline__ Pos load_pos(const int32_t* col0, const int32_t* perm0, int N, int E, int p0, int t, int nv) {
  Pos p{-1, 0, 0};
  if (t < nv) {
    p.e = perm0 ? perm0[p0 + t] : p0 + t;
    if (p.e >= 0 && p.e < E) {
      p.r = col0[p.e];
      p.s = col0[E + p.e];
      if (p.r < 0 || p.r >= N || p.s < 0 || p.s >= N) { p.r = -1; p.s = 0; }
    } else {
      p.e = 0;
    }
  }
  return p;
}

// The walk of one thread (column `col` of width W).  step(e, r, v, range) takes position e of the tile with receiver r
// (-1: skipped row, -2: behind the last position) and its value v: flush(), which ends the open segment when r changes,
// then the in-order add.  range(cur, first) returns the CSR range {s0, s1} of receiver `cur`, whose segment began at
// tile position `first`.  For a kernel that owns the loop (MEGNet: unrolled over a preloaded column).
template <int W>
struct Walk {
  float* direct;   // (N, W)
  float* bnd;      // (tiles, 2, W)
  int tile, col;
  int cur = -1, first = 0;
  float sum = 0.0f;

  template <class Range>
  __device__ __forceinline__ void flush(int e, int r, const Range& range) {
    if (r != cur) {
      if (cur >= 0) {
        const int2 seg = range(cur, first);
        if (seg.x >= tile * TE && seg.y <= tile * TE + TE) direct[(size_t)cur * W + col] = sum;
        else bnd[((size_t)tile * 2 + (first == 0 ? 0 : 1)) * W + col] = sum;
      }
      cur = r; first = e; sum = 0.0f;
    }
  }
  template <class Range>
  __device__ __forceinline__ void step(int e, int r, float v, const Range& range) {
    flush(e, r, range);
    if (r >= 0) sum += v;
  }
};

// The whole loop over a tile of nv positions: recvL holds the tile's receivers (LDS), value(e) is position e's value in
// this thread's column, read behind the flush and for valid rows only; the CSR range is read from ptr0 when a segment
// ends.  A value lambda captures by value ([=]): captured by reference, egnn_edge_fwd_kernel compiled to 16 more VGPRs.
template <int W, class Value>
__device__ __forceinline__ void walk(const int* recvL, int nv, const int32_t* ptr0, float* direct, float* bnd, int tile,
                                     int col, const Value& value) {
  Walk<W> w{direct, bnd, tile, col};
  const auto range = [=](int cur, int) { return make_int2(ptr0[cur], ptr0[cur + 1]); };
  for (int e = 0; e <= nv; ++e) {
    const int r = e < nv ? recvL[e] : -2;
    w.flush(e, r, range);
    if (r >= 0) w.sum += value(e);
  }
}

// Finishing pass: the sum of column `col` of the receiver with the non-empty range [s0, s1).  False: the range lies inside
// one tile and the walk has stored the sum directly; true: *sum is the receiver's slots added in tile order.
template <int W>
__device__ __forceinline__ bool cut_sum(const float* __restrict__ bnd, int64_t s0, int64_t s1, int col, float* sum) {
  const int64_t t0 = s0 / TE, t1 = (s1 - 1) / TE;
  if (t0 == t1) return false;
  float u = bnd[((size_t)t0 * 2 + (s0 == t0 * TE ? 0 : 1)) * W + col];
  for (int64_t tt = t0 + 1; tt <= t1; ++tt) u += bnd[((size_t)tt * 2) * W + col];
  *sum = u;
  return true;
}

}  // namespace mp_tile
