// Parameter side of the reverse pass (what Keras' tape computes for Dense / Embedding / softmax under model.fit,
// kgcnn/layers/modules.py:15-90, :526-534, training/train_qm.py:164-166):
//
//   mp_dense_wgrad_f32        dW (K,U) = X^T G and db (U) = sum_r G[r] over R rows
//   mp_embedding_grad_f32     dTable[t] = sum_{i: number_i = t} G[i], node order within each type
//   mp_softmax_rows_grad_f32  out = y * (g - rowsum(g * y))
//   mp_directed_edge_wgrad_f32  mp_dense_wgrad_f32 whose X is the gathered difference h[send] - he[rev] of the directed
//                             edge update (kgcnn/literature/DMPNN.py:137-138), formed while a slab is staged
//
// Weight gradient: the reduction runs over the ROWS of x and g, so the MFMA's k dimension is the row index.  Both
// operands are k-contiguous in HBM in the wrong direction for a register load (x is (R,K) row-major), so a workgroup
// stages a 32-row slab of X (32 x 64 columns of K) and of G (32 x 64 columns of U) in LDS and reads them column-wise as
// the A (16 K-columns x 4 rows) and B (4 rows x 16 U-columns) operands of v_mfma_f32_16x16x4_f32: FP32 in, FP32
// accumulate, a row-ordered fma chain (the same precision class as mp_dense_f32).  One workgroup = 4 waves owns a
// 64 (K) x 64 (U) output tile, each wave a 32 x 32 quarter held in four independent 16 x 16 accumulators.
//
// Row split: the rows are cut into chunks - a function of (R, K, U) only - so that the grid fills the chip for few
// output tiles (SchNet's (26190, 128, 128) has 4); chunk c writes an FP32 slab, a second launch adds the slabs in chunk
// order.  The bias sum is taken from the G tiles already staged (workgroups of K-tile 0).  No atomics: the result is
// the same bits on every run and every stream.
#include "mp_common.h"
#include "../../include/mpengine/dmpnn.h"
#include "../../include/mpengine/index.h"
#include "../../include/mpengine/segment.h"
#include "../../include/mpengine/wgrad.h"

namespace {

using floatx4 = __attribute__((ext_vector_type(4))) float;

constexpr int WT = 64;           // output tile edge (K and U)
constexpr int BR = 32;           // rows per LDS stage (8 MFMA k-steps of 4 rows)
constexpr int LDW = WT + 16;     // padded LDS row: the 4 rows one MFMA reads start 16 banks apart
constexpr int64_t TARGET_WG = 512;   // ~2 workgroups per CU
constexpr int64_t MAX_CHUNKS = 512;  // bounds the workspace: chunks grow in rows, not in number, beyond this

struct WgradArgs {
  const float* x;   // (R, K)
  const float* g;   // (R, U)
  int64_t R, K, U;
  int64_t rows_per_chunk;   // multiple of BR
  float* dw;        // (K, U) destination of this launch (the final dW or the chunk's slab base)
  float* db;        // (U) destination of the bias sum (final db or the bias slab base), null: no bias
  int64_t dw_stride, db_stride;   // per-chunk stride of the slabs (0 when there is one chunk)
  // DIFF (mp_directed_edge_wgrad_f32): row r of x is x[send[r]] - x2[rev[r]], formed while the slab is staged
  const float* x2;        // (R, K), rows read at rev; a row with rev < 0 counts as zero
  const int32_t* send;    // (R) rows of x, inside [0, xrows) or clamped and flagged
  const int32_t* rev;     // (R) rows of x2, below R or clamped and flagged
  int64_t xrows;
  int32_t* flags;         // nullable
};

// Upper bound on the chunk count, non-decreasing in R (the workspace size is derived from it).
inline int64_t max_chunks(int64_t R, int64_t K, int64_t U) {
  const int64_t tiles = mp::ceil_div(K, WT) * mp::ceil_div(U, WT);
  const int64_t stages = mp::ceil_div(R, BR);
  int64_t c = mp::ceil_div(TARGET_WG, tiles);
  if (c > MAX_CHUNKS) c = MAX_CHUNKS;
  if (c > stages) c = stages;
  return c < 1 ? 1 : c;
}

// Rows per chunk (a multiple of BR) and the resulting chunk count (<= max_chunks).
inline void plan_chunks(int64_t R, int64_t K, int64_t U, int64_t* rows_per_chunk, int64_t* chunks) {
  const int64_t c = max_chunks(R, K, U);
  const int64_t stages = mp::ceil_div(R, BR);
  *rows_per_chunk = mp::ceil_div(stages, c) * BR;
  *chunks = mp::ceil_div(R, *rows_per_chunk);
}

// VEC: K % 4 == 0, U % 4 == 0 and 16-B aligned operands (16-B loads); the scalar path covers odd shapes (GCN's 1433
// input features, 7-class heads, U = 1).  Loads are unconditional from clamped addresses; what lies outside the chunk /
// the matrix is zeroed when the registers are written to LDS (rows beyond the chunk must be 0 in G for the bias sum).
// DIFF (VEC only): the A operand is a gathered difference, x[send[r]] - x2[rev[r]] (the directed edge update's input,
// csrc/mp_cmpnn.hip), never written to memory: a slab's row indices are read one slab ahead of its rows.
template <bool VEC, bool DIFF = false>
__global__ __launch_bounds__(256) void dense_wgrad_kernel(WgradArgs a) {
  static_assert(VEC || !DIFF, "the gathered difference is built for the 16-byte path");
  __shared__ __align__(16) float Xs[BR * LDW];
  __shared__ __align__(16) float Gs[BR * LDW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wk = wave >> 1, wu = wave & 1;
  const int64_t chunk = blockIdx.x;
  const int64_t k0 = static_cast<int64_t>(blockIdx.y) * WT;
  const int64_t u0 = static_cast<int64_t>(blockIdx.z) * WT;
  const int64_t R = a.R, K = a.K, U = a.U;
  const int64_t rbeg = chunk * a.rows_per_chunk;
  const int64_t rend = (rbeg + a.rows_per_chunk < R) ? rbeg + a.rows_per_chunk : R;
  const int64_t stages = (rend - rbeg + BR - 1) / BR;
  const bool do_bias = a.db != nullptr && blockIdx.y == 0;

  floatx4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  float bsum = 0.0f;

  constexpr int NV = (BR * WT) / (256 * 4);   // float4 per thread and tile
  constexpr int NS = (BR * WT) / 256;         // floats per thread and tile, scalar path
  float4 rx4[VEC ? NV : 1], rg4[VEC ? NV : 1];
  float rx[VEC ? 1 : NS], rg[VEC ? 1 : NS];
  float4 rx2[DIFF ? NV : 1];                       // the reverse rows of the difference
  int32_t is[DIFF ? NV : 1], ir[DIFF ? NV : 1];    // sender and reverse row of the NEXT slab to load
  int local_flags = 0;

  auto load_index = [&](int64_t r0) {
    if constexpr (DIFF) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int64_t gr = r0 + (tid + i * 256) / (WT / 4);
        const bool live = gr < rend;
        gr = gr < R ? gr : R - 1;
        int32_t s = a.send[gr], r = a.rev[gr];
        if (s < 0 || s >= a.xrows) { if (live) local_flags |= MP_FLAG_OOB; s = s < 0 ? 0 : static_cast<int32_t>(a.xrows - 1); }
        if (r >= R) { if (live) local_flags |= MP_FLAG_OOB; r = static_cast<int32_t>(R - 1); }
        is[i] = s;
        ir[i] = r;
      }
    }
  };

  auto load_tile = [&](int64_t r0) {
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int idx = tid + i * 256;
        const int r = idx / (WT / 4), c = (idx % (WT / 4)) * 4;
        int64_t gr = r0 + r, gk = k0 + c, gu = u0 + c;
        gr = gr < R ? gr : R - 1;
        gk = gk < K ? gk : K - 4;
        gu = gu < U ? gu : U - 4;
        if constexpr (DIFF) {
          rx4[i] = *reinterpret_cast<const float4*>(a.x + static_cast<int64_t>(is[i]) * K + gk);
          rx2[i] = *reinterpret_cast<const float4*>(a.x2 + static_cast<int64_t>(ir[i] < 0 ? 0 : ir[i]) * K + gk);
          if (ir[i] < 0) rx2[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          rx4[i] = make_float4(rx4[i].x - rx2[i].x, rx4[i].y - rx2[i].y, rx4[i].z - rx2[i].z, rx4[i].w - rx2[i].w);
        } else {
          rx4[i] = *reinterpret_cast<const float4*>(a.x + gr * K + gk);
        }
        rg4[i] = *reinterpret_cast<const float4*>(a.g + gr * U + gu);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int idx = tid + i * 256;
        const int r = idx / WT, c = idx % WT;
        int64_t gr = r0 + r, gk = k0 + c, gu = u0 + c;
        gr = gr < R ? gr : R - 1;
        gk = gk < K ? gk : K - 1;
        gu = gu < U ? gu : U - 1;
        rx[i] = a.x[gr * K + gk];
        rg[i] = a.g[gr * U + gu];
      }
    }
  };
  auto store_tile = [&](int64_t r0) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int idx = tid + i * 256;
        const int r = idx / (WT / 4), c = (idx % (WT / 4)) * 4;
        const bool row_ok = (r0 + r) < rend;
        if constexpr (DIFF) {   // selects on the values: a select between the two arrays' addresses costs a stack slot
          const bool okx = row_ok && (k0 + c) < K, okg = row_ok && (u0 + c) < U;
          const float4 vx = rx4[i], vg = rg4[i];
          *reinterpret_cast<float4*>(Xs + r * LDW + c) =
              make_float4(okx ? vx.x : 0.f, okx ? vx.y : 0.f, okx ? vx.z : 0.f, okx ? vx.w : 0.f);
          *reinterpret_cast<float4*>(Gs + r * LDW + c) =
              make_float4(okg ? vg.x : 0.f, okg ? vg.y : 0.f, okg ? vg.z : 0.f, okg ? vg.w : 0.f);
        } else {
          *reinterpret_cast<float4*>(Xs + r * LDW + c) = (row_ok && (k0 + c) < K) ? rx4[i] : z4;
          *reinterpret_cast<float4*>(Gs + r * LDW + c) = (row_ok && (u0 + c) < U) ? rg4[i] : z4;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int idx = tid + i * 256;
        const int r = idx / WT, c = idx % WT;
        const bool row_ok = (r0 + r) < rend;
        Xs[r * LDW + c] = (row_ok && (k0 + c) < K) ? rx[i] : 0.0f;
        Gs[r * LDW + c] = (row_ok && (u0 + c) < U) ? rg[i] : 0.0f;
      }
    }
  };

  if (stages > 0) {
    load_index(rbeg);
    load_tile(rbeg);
    if (stages > 1) load_index(rbeg + BR);
  }
  const int col = lane & 15, quad = lane >> 4;
  const float* xa = Xs + quad * LDW + wk * 32 + col;
  const float* gb = Gs + quad * LDW + wu * 32 + col;
  for (int64_t s = 0; s < stages; ++s) {
    const int64_t r0 = rbeg + s * BR;
    store_tile(r0);
    __syncthreads();
    if (s + 1 < stages) {
      load_tile(r0 + BR);   // next slab's loads in flight under this slab's MFMAs
      if (s + 2 < stages) load_index(r0 + 2 * BR);
    }
#pragma unroll
    for (int kk = 0; kk < BR / 4; ++kk) {
      const float a0 = xa[kk * 4 * LDW], a1 = xa[kk * 4 * LDW + 16];
      const float b0 = gb[kk * 4 * LDW], b1 = gb[kk * 4 * LDW + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (do_bias && wave == 0) {   // column sums of the staged G slab, rows in order
#pragma unroll 8
      for (int r = 0; r < BR; ++r) bsum += Gs[r * LDW + lane];
    }
    __syncthreads();
  }

  // C/D map of the 16x16 forms: row (K) = 4 * (lane >> 4) + q, column (U) = lane & 15
  float* dw = a.dw + chunk * a.dw_stride;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t u = u0 + wu * 32 + j * 16 + col;
    if (u >= U) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t k = k0 + wk * 32 + i * 16 + quad * 4 + q;
        if (k < K) dw[k * U + u] = acc[i][j][q];
      }
    }
  }
  if (do_bias && wave == 0 && u0 + lane < U) a.db[chunk * a.db_stride + u0 + lane] = bsum;
  if constexpr (DIFF) {
    if (a.flags != nullptr && blockIdx.y == 0 && blockIdx.z == 0) mp_publish_flags(a.flags, local_flags);
  }
}

// dW = sum_c slab[c], db = sum_c bslab[c], chunks added in order (fixed): the bits do not depend on scheduling.  One
// element per thread, 64-thread workgroups (a (128,128) dW is 16 k elements: 256 workgroups reach every CU, 256-thread
// ones would occupy 64), the loads of eight chunks issued before their in-order adds.
constexpr int REDUCE_BLOCK = 64;
__global__ __launch_bounds__(REDUCE_BLOCK) void wgrad_reduce_kernel(const float* __restrict__ slab,
                                                                    const float* __restrict__ bslab, int64_t chunks,
                                                                    int64_t KU, int64_t U, float* __restrict__ dw,
                                                                    float* __restrict__ db) {
  const int64_t total = KU + (db ? U : 0);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const bool is_w = t < KU;
    const float* src = is_w ? slab + t : bslab + (t - KU);
    const int64_t step = is_w ? KU : U;
    float s = 0.0f;
    int64_t c = 0;
    for (; c + 8 <= chunks; c += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[(c + j) * step];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; c < chunks; ++c) s += src[c * step];
    if (is_w) dw[t] = s;
    else db[t - KU] = s;
  }
}

// out = y * (g - sum_c g*y): one 64-lane wave per row (as softmax_rows_kernel), wave-wide sum by xor shuffles.
__global__ void softmax_rows_grad_kernel(const float* __restrict__ y, const float* __restrict__ g, int64_t R, int64_t C,
                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_global = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t r = wave_global; r < R; r += nwaves) {
    const float* yr = y + r * C;
    const float* gr = g + r * C;
    float dot = 0.0f;
    for (int64_t c = lane; c < C; c += 64) dot += gr[c] * yr[c];
    dot = mp_wave_sum(dot);
    for (int64_t c = lane; c < C; c += 64) out[r * C + c] = yr[c] * (gr[c] - dot);
  }
}

// Keras' int32 cast of the node numbers (truncation, as embedding_kernel); numbers outside [0, vocab) - rows the
// forward filled with zeros - go to the extra segment `vocab`, which is not reduced.
__global__ void embedding_ids_kernel(const float* __restrict__ numbers, int64_t N, int64_t vocab,
                                     int32_t* __restrict__ ids) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += stride) {
    const int64_t row = static_cast<int32_t>(numbers[i]);
    ids[i] = static_cast<int32_t>((row >= 0 && row < vocab) ? row : vocab);
  }
}


}  // namespace

extern "C" {

int mp_dense_wgrad_ws_bytes(int64_t R, int64_t K, int64_t U, size_t* bytes_out_host) {
  MP_REQUIRE(R >= 0 && K >= 1 && U >= 1 && bytes_out_host, "mp_dense_wgrad_ws_bytes: bad arguments");
  const int64_t c = max_chunks(R, K, U);
  *bytes_out_host = c > 1 ? sizeof(float) * static_cast<size_t>(c) * static_cast<size_t>(K * U + U) : 0;
  return MP_OK;
}

// Both entry points: the row split, the launch and the in-order reduction.  `diff` selects the gathered-difference A
// operand (a.x2 / a.send / a.rev / a.xrows / a.flags are set by the caller).
static int wgrad_launch(const char* what, WgradArgs a, bool diff, void* ws, size_t ws_bytes, mpStream_t stream) {
  const float* x = a.x;
  const float* g = a.g;
  const int64_t R = a.R, K = a.K, U = a.U;
  float* dw = a.dw;
  float* db = a.db;
  hipStream_t s = mp::as_stream(stream);
  if (R == 0) {   // empty sum
    MP_HIP(hipMemsetAsync(dw, 0, sizeof(float) * static_cast<size_t>(K * U), s));
    if (db) MP_HIP(hipMemsetAsync(db, 0, sizeof(float) * static_cast<size_t>(U), s));
    return MP_OK;
  }
  MP_REQUIRE(x && g, "%s: null pointer", what);
  const int64_t gk = mp::ceil_div(K, WT), gu = mp::ceil_div(U, WT);
  MP_REQUIRE(gk <= 65535 && gu <= 65535, "%s: K or U too large", what);
  int64_t rows_per_chunk = 0, chunks = 0;
  plan_chunks(R, K, U, &rows_per_chunk, &chunks);
  a.rows_per_chunk = rows_per_chunk;
  float* slab = nullptr;
  float* bslab = nullptr;
  if (chunks > 1) {
    size_t need = 0;
    int rc = mp_dense_wgrad_ws_bytes(R, K, U, &need);
    if (rc != MP_OK) return rc;
    MP_REQUIRE(ws && ws_bytes >= need, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    slab = static_cast<float*>(ws);
    bslab = slab + chunks * K * U;
    a.dw = slab;
    a.db = db ? bslab : nullptr;
    a.dw_stride = K * U;
    a.db_stride = U;
  }
  const bool vec = (K % 4 == 0) && (U % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0) &&
                   (reinterpret_cast<uintptr_t>(g) % 16 == 0);
  dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(gk), static_cast<unsigned>(gu));
  if (diff) {
    MP_REQUIRE(vec, "%s: widths are multiples of 4 and operands 16-byte aligned", what);
    dense_wgrad_kernel<true, true><<<grid, 256, 0, s>>>(a);
  } else if (vec) {
    dense_wgrad_kernel<true><<<grid, 256, 0, s>>>(a);
  } else {
    dense_wgrad_kernel<false><<<grid, 256, 0, s>>>(a);
  }
  int rc = mp::check_launch(what);
  if (rc != MP_OK || chunks == 1) return rc;
  wgrad_reduce_kernel<<<mp::grid_for(K * U + (db ? U : 0), REDUCE_BLOCK), REDUCE_BLOCK, 0, s>>>(slab, bslab, chunks,
                                                                                              K * U, U, dw, db);
  return mp::check_launch(what);
}

int mp_dense_wgrad_f32(const float* x, int64_t R, int64_t K, const float* g, int64_t U, float* dw, float* db, void* ws,
                       size_t ws_bytes, mpStream_t stream) {
  MP_REQUIRE(R >= 0 && K >= 1 && U >= 1, "mp_dense_wgrad_f32: bad sizes R=%lld K=%lld U=%lld", (long long)R,
             (long long)K, (long long)U);
  MP_REQUIRE(dw, "mp_dense_wgrad_f32: null dW");
  WgradArgs a{x, g, R, K, U, 0, dw, db, 0, 0, nullptr, nullptr, nullptr, 0, nullptr};
  return wgrad_launch("mp_dense_wgrad_f32", a, false, ws, ws_bytes, stream);
}

int mp_directed_edge_wgrad_ws_bytes(int64_t E, int64_t F, size_t* bytes_out_host) {
  MP_REQUIRE(E >= 0 && F >= 4 && F % 4 == 0 && bytes_out_host, "mp_directed_edge_wgrad_ws_bytes: bad arguments");
  return mp_dense_wgrad_ws_bytes(E, F, F, bytes_out_host);
}

int mp_directed_edge_wgrad_f32(const float* h, int64_t N, const float* he, int64_t E, int64_t F, const int32_t* send,
                               const int32_t* rev, const float* p, float* dw, float* db, void* ws, size_t ws_bytes,
                               int32_t* flags, mpStream_t stream) {
  const char* what = "mp_directed_edge_wgrad_f32";
  MP_REQUIRE(N >= 0 && E >= 0 && F >= 4 && F % 4 == 0, "%s: bad sizes N=%lld E=%lld F=%lld (F a multiple of 4)", what,
             (long long)N, (long long)E, (long long)F);
  MP_REQUIRE(N < (int64_t{1} << 31) - 1 && E < (int64_t{1} << 31) - 1, "%s: nodes and edges are indexed with 32 bits",
             what);
  MP_REQUIRE(dw, "%s: null dW", what);
  MP_REQUIRE(E == 0 || (h && he && send && rev && p && N > 0), "%s: null pointer, or edges and no node", what);
  MP_REQUIRE(mp::aligned16(h) && mp::aligned16(he) && mp::aligned16(p), "%s: operands must be 16-byte aligned", what);
  WgradArgs a{h, p, E, F, F, 0, dw, db, 0, 0, he, send, rev, N, flags};
  return wgrad_launch(what, a, true, ws, ws_bytes, stream);
}

int mp_softmax_rows_grad_f32(const float* y, const float* g, int64_t R, int64_t C, float* out, mpStream_t stream) {
  MP_REQUIRE(R >= 0 && C >= 1, "mp_softmax_rows_grad_f32: bad sizes");
  if (R == 0) return MP_OK;
  MP_REQUIRE(y && g && out, "mp_softmax_rows_grad_f32: null pointer");
  softmax_rows_grad_kernel<<<mp::grid_for(R * 64), 256, 0, mp::as_stream(stream)>>>(y, g, R, C, out);
  return mp::check_launch("mp_softmax_rows_grad_f32");
}

int mp_embedding_grad_ws_bytes(int64_t N, int64_t vocab, size_t* bytes_out_host) {
  MP_REQUIRE(N >= 0 && vocab >= 1 && bytes_out_host, "mp_embedding_grad_ws_bytes: bad arguments");
  size_t sort = 0;
  int rc = mp_sort_workspace_bytes(N, &sort);
  if (rc != MP_OK) return rc;
  const size_t n = static_cast<size_t>(N > 0 ? N : 1);
  *bytes_out_host = 3 * mp::align256(sizeof(int32_t) * n) + mp::align256(sizeof(int32_t) * static_cast<size_t>(vocab + 2)) + sort;
  return MP_OK;
}

int mp_embedding_grad_f32(const float* numbers, int64_t N, const float* g, int64_t vocab, int64_t dim, void* ws,
                          size_t ws_bytes, float* table_grad, mpStream_t stream) {
  MP_REQUIRE(vocab >= 1 && dim >= 1 && N >= 0, "mp_embedding_grad_f32: bad sizes");
  MP_REQUIRE(table_grad, "mp_embedding_grad_f32: null table gradient");
  hipStream_t s = mp::as_stream(stream);
  if (N == 0) {
    MP_HIP(hipMemsetAsync(table_grad, 0, sizeof(float) * static_cast<size_t>(vocab * dim), s));
    return MP_OK;
  }
  MP_REQUIRE(numbers && g && ws, "mp_embedding_grad_f32: null pointer");
  size_t need = 0;
  int rc = mp_embedding_grad_ws_bytes(N, vocab, &need);
  if (rc != MP_OK) return rc;
  MP_REQUIRE(ws_bytes >= need, "mp_embedding_grad_f32: workspace %zu < %zu bytes", ws_bytes, need);
  // stable sort by type + CSR + segment sum: rows of one type are added in node order
  char* p = static_cast<char*>(ws);
  const size_t nb = mp::align256(sizeof(int32_t) * static_cast<size_t>(N));
  int32_t* ids = reinterpret_cast<int32_t*>(p);
  int32_t* ids_sorted = reinterpret_cast<int32_t*>(p + nb);
  int32_t* perm = reinterpret_cast<int32_t*>(p + 2 * nb);
  int32_t* ptr = reinterpret_cast<int32_t*>(p + 3 * nb);
  void* sort_ws = p + 3 * nb + mp::align256(sizeof(int32_t) * static_cast<size_t>(vocab + 2));
  const size_t sort_bytes = ws_bytes - (3 * nb + mp::align256(sizeof(int32_t) * static_cast<size_t>(vocab + 2)));
  embedding_ids_kernel<<<mp::grid_for(N), 256, 0, s>>>(numbers, N, vocab, ids);
  rc = mp::check_launch("mp_embedding_grad_f32 (ids)");
  if (rc != MP_OK) return rc;
  rc = mp_sort_segments_i32(ids, N, ids_sorted, perm, sort_ws, sort_bytes, stream);
  if (rc != MP_OK) return rc;
  rc = mp_csr_from_sorted_i32(ids_sorted, N, vocab + 1, ptr, stream);
  if (rc != MP_OK) return rc;
  return mp_segment_reduce_csr_f32(MP_SUM, g, N, dim, ptr, perm, vocab, nullptr, 0, table_grad, stream);
}

}  // extern "C"
