// MEGNet (kgcnn/literature/Megnet.py:24-373, kgcnn/layers/conv/megnet_conv.py:96-111): the fused edge step of one
// MEGnetBlock, one launch plus a node-sized finishing pass:
//   z1[e]   = Pa[recv e] + Pb[send e] + edges[e] Wc + Pu[g(e)]
//   e'[e]   = act(act(z1[e]) W1 + b1) W2 + b2                                       (64 -> 32 -> 32, last layer linear)
//   pool[r] = mean or sum over {e : recv e = r} of e'[e], in list order; 0 for a receiver without edges
// Pa = v W_e[0:32], Pb = v W_e[32:64] (N, 64) and Pu = u W_e[96:128] + b0 (G, 64) are made by three Dense launches on row
// blocks of the first edge kernel (read in place), so the per-edge Dense on [v_i, v_j, e, u] is three gathered rows plus
// the 32-wide edge product.  g(e) is looked up in the edge tensor's own int64 row_splits: a tile may hold edges of several
// graphs, with edgeless graphs in between.
// One workgroup (4 waves) walks tiles of 32 receiver-sorted positions:
//   phase 0  receiver, sender, edge id, graph and the receiver's CSR range of each position, the edge-feature tile X
//            (32 x 32)                                                                                            -> LDS
//   phase 1  X Wc on the matrix pipe (v_mfma_f32_16x16x4_f32): wave w owns output columns [16w, 16w+16) of both row
//            blocks; the gathered rows are loaded ahead of the product, summed behind it, activated               -> LDS
//   phase 2  A1 W1 (32 x 64 x 32) and A2 W2 (32 x 32 x 32): wave w owns the 16 x 16 block (w >> 1, w & 1).  e' goes out
//            at its list position (through perm0) and into LDS for the walk
//   phase 3  per-receiver sums in list order by 32 threads (one per column): the walk step of csrc/mp_edge_tile.h,
//            which states the rule for receivers cut by a tile boundary.  No atomics: two runs give equal bits.
// The slabs of Wc, W1 and W2 a wave needs live in 8 + 16 + 8 registers per lane for the whole kernel.  The kernel is bound
// by the latency of its dependent loads (position -> indices -> rows), not by traffic, so the chain is kept short: with at
// most SPLITS_LDS graphs the row_splits are copied to LDS once per workgroup and g(e) is searched there (a search in
// global memory is log2(G) dependent round trips per tile), and the walk's CSR ranges are fetched with the indices.
// megnet_pool_kernel then takes every node's sum (direct, or the cut receiver's sum), zeroes the receivers without edges
// and divides by the edge count for the mean.
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/megnet.h"

namespace {

constexpr int FE = 32;   // edge width in
constexpr int H0 = 64;   // first layer of the edge chain
constexpr int H1 = 32;   // second layer
constexpr int H2 = 32;   // third layer = edge width out
constexpr int TE = mp_tile::TE;   // positions per tile
constexpr int SPLITS_LDS = 2048;   // row_splits entries held in LDS (as int32: E < 2^31); more graphs search in global memory
constexpr int XS = FE + 1;   // row strides in LDS
constexpr int A1S = H0 + 1;
constexpr int A2S = H1 + 1;
constexpr int MS = H2 + 1;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct EdgeArgs {
  const float* Pa;        // (N, 64), gathered by the receiver
  const float* Pb;        // (N, 64), gathered by the sender
  const float* Pu;        // (G, 64), first-layer bias folded in
  const int64_t* splits;  // (G+1) row_splits of the edge tensor
  const float* x;         // (E, 32) edge features
  const int32_t* col0;    // (2, E) receivers | senders
  const int32_t* ptr0;    // (N+1) CSR of col0 over sorted positions
  const int32_t* perm0;   // (E) sorted position -> edge, nullable
  const float* Wc;        // (32, 64)
  const float* W1;        // (64, 32)
  const float* b1;        // (32) nullable
  const float* W2;        // (32, 32)
  const float* b2;        // (32) nullable
  float* e_out;           // (E, 32)
  float* pool;            // (N, 32): sums of the receivers that lie inside one tile
  float* bnd;             // (tiles, 2, 32)
  int64_t G;
  int N, E;               // below 2^31 (checked on the host)
  int act;
  float alpha;
};

__global__ __launch_bounds__(256, 4) void megnet_edge_kernel(EdgeArgs a) {
  __shared__ float xL[TE * XS];
  __shared__ float a1L[TE * A1S];
  __shared__ float a2L[TE * A2S];
  __shared__ float mL[TE * MS];
  __shared__ int recvL[TE], sndL[TE], eidL[TE], gidL[TE], seg0L[TE], seg1L[TE];
  __shared__ int splitsL[SPLITS_LDS];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lc = lane & 15, kq = lane >> 4;
  const int col0 = 16 * wave + lc;                  // phase 1: column of the 64-wide first layer
  const int rb = wave >> 1, col = 16 * (wave & 1) + lc;   // phase 2: row block and column of the 32-wide layers

  // B operands: step s reads row 4s + (lane >> 4) of the wave's 16 columns
  float wc[FE / 4], w1[H0 / 4], w2[H1 / 4];
#pragma unroll
  for (int s = 0; s < FE / 4; ++s) wc[s] = a.Wc[(size_t)(4 * s + kq) * H0 + col0];
#pragma unroll
  for (int s = 0; s < H0 / 4; ++s) w1[s] = a.W1[(size_t)(4 * s + kq) * H1 + col];
#pragma unroll
  for (int s = 0; s < H1 / 4; ++s) w2[s] = a.W2[(size_t)(4 * s + kq) * H2 + col];
  const float bias1 = a.b1 ? a.b1[col] : 0.0f, bias2 = a.b2 ? a.b2[col] : 0.0f;

  const bool splits_in_lds = a.G + 1 <= SPLITS_LDS;
  if (splits_in_lds)
    for (int i = t; i <= static_cast<int>(a.G); i += 256) splitsL[i] = static_cast<int>(a.splits[i]);

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's walk is done with the tiles in LDS
    // phase 0
    int s0 = 0, s1 = 0;   // CSR range of the position's receiver (threads 0..31), needed by the walk only
    if (t < TE) {
      const mp_tile::Pos p = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p0, t, nv);
      int g = 0;   // read for valid rows only
      if (t < nv) {
        if (p.r >= 0) { s0 = a.ptr0[p.r]; s1 = a.ptr0[p.r + 1]; }
        if (splits_in_lds) {   // largest g in [0, G) with splits[g] <= e, as mp_owner_of
          int lo = 0, hi = static_cast<int>(a.G);
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (splitsL[mid] <= p.e) lo = mid; else hi = mid;
          }
          g = lo;
        } else {
          g = static_cast<int>(mp_owner_of(a.splits, a.G, p.e));
        }
      }
      recvL[t] = p.r; sndL[t] = p.s; eidL[t] = p.e; gidL[t] = g;
    }
    __syncthreads();
    // every global load of the tile is issued before the first one is waited for: the edge features (thread t holds
    // column t & 31 of rows (t >> 5) + 8j), then the gathered rows of phase 1
    float xv[TE * FE / 256];
#pragma unroll
    for (int j = 0; j < TE * FE / 256; ++j) {
      const int e = (t >> 5) + 8 * j;
      xv[j] = recvL[e] >= 0 ? a.x[(size_t)eidL[e] * FE + (t & (FE - 1))] : 0.0f;
    }
    // phase 1: the gathered rows first (C layout of 16x16x4: col = lane & 15, row = 4 * (lane >> 4) + i)
    float pa[2][4], pb[2][4], pu[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = 16 * b + 4 * kq + i;
        const bool ok = recvL[e] >= 0;
        pa[b][i] = ok ? a.Pa[(size_t)recvL[e] * H0 + col0] : 0.0f;
        pb[b][i] = ok ? a.Pb[(size_t)sndL[e] * H0 + col0] : 0.0f;
        pu[b][i] = ok ? a.Pu[(size_t)gidL[e] * H0 + col0] : 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < TE * FE / 256; ++j) xL[((t >> 5) + 8 * j) * XS + (t & (FE - 1))] = xv[j];
    if (t < TE) { seg0L[t] = s0; seg1L[t] = s1; }   // here, not in phase 0: the rows above do not wait for ptr0
    __syncthreads();
    {
      f32x4 acc[2];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[b][i] = 0.0f;
      const float* ap = xL + lc * XS + kq;
#pragma unroll
      for (int s = 0; s < FE / 4; ++s) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * s], wc[s], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[16 * XS + 4 * s], wc[s], acc[1], 0, 0, 0);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 16 * b + 4 * kq + i;
          const float z = ((pa[b][i] + pb[b][i]) + acc[b][i]) + pu[b][i];
          a1L[e * A1S + col0] = mp_apply_act(a.act, a.alpha, z);
        }
      }
    }
    __syncthreads();
    // phase 2
    {
      f32x4 acc;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = 0.0f;
      const float* ap = a1L + (16 * rb + lc) * A1S + kq;
#pragma unroll
      for (int s = 0; s < H0 / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * s], w1[s], acc, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a2L[(16 * rb + 4 * kq + i) * A2S + col] = mp_apply_act(a.act, a.alpha, acc[i] + bias1);
    }
    __syncthreads();
    {
      f32x4 acc;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = 0.0f;
      const float* ap = a2L + (16 * rb + lc) * A2S + kq;
#pragma unroll
      for (int s = 0; s < H1 / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * s], w2[s], acc, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = 16 * rb + 4 * kq + i;
        const bool ok = recvL[e] >= 0;
        const float v = ok ? acc[i] + bias2 : 0.0f;
        if (ok) a.e_out[(size_t)eidL[e] * H2 + col] = v;
        mL[e * MS + col] = v;
      }
    }
    __syncthreads();
    // phase 3
    if (t < H2) {
      float mv[TE];   // the thread's column: 32 independent LDS reads instead of one per dependent step
#pragma unroll
      for (int e = 0; e < TE; ++e) mv[e] = mL[e * MS + t];
      mp_tile::Walk<H2> w{a.pool, a.bnd, tile, t};
      const auto range = [&](int, int first) { return make_int2(seg0L[first], seg1L[first]); };
#pragma unroll
      for (int e = 0; e <= TE; ++e) {
        if (e > nv) break;
        w.step(e, e < nv ? recvL[e < TE ? e : 0] : -2, mv[e < TE ? e : 0], range);
      }
    }
  }
}

// pool of every node: direct, a cut receiver's sum, or 0 without edges; the mean divides by the count.
__global__ void megnet_pool_kernel(const int32_t* __restrict__ ptr0, int64_t N, const float* __restrict__ bnd, int mean,
                                   float* __restrict__ pool) {
  const int64_t total = N * H2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / H2;
    const int col = static_cast<int>(i - r * H2);
    const int64_t s0 = ptr0[r], s1 = ptr0[r + 1];
    float u = 0.0f;
    if (s1 > s0) {
      if (!mp_tile::cut_sum<H2>(bnd, s0, s1, col, &u)) u = pool[i];
      if (mean) u = u / static_cast<float>(s1 - s0);
    }
    pool[i] = u;
  }
}

}  // namespace

extern "C" {

int mp_megnet_edge_ws_bytes(int64_t E, size_t* bytes_out_host) {
  MP_REQUIRE(E >= 0 && bytes_out_host, "mp_megnet_edge_ws_bytes: bad arguments");
  *bytes_out_host = mp_tile::ws_bytes(E, H2);
  return MP_OK;
}

int mp_megnet_edge_f32(const float* Pa, const float* Pb, int64_t N, const float* Pu, const int64_t* edge_splits,
                       int64_t G, const float* edges, int Fn, int Fe, int Fu, const int32_t* cols, int64_t E,
                       const int32_t* ptr0, const int32_t* perm0, const float* Wc, const float* W1, const float* b1,
                       const float* W2, const float* b2, int units0, int units1, int units2, int act, float alpha,
                       int pool_op, float* ws, size_t ws_bytes, float* edges_out, float* pool_out, mpStream_t stream) {
  const char* what = "mp_megnet_edge_f32";
  MP_REQUIRE(mp_tile::sizes_ok(N, E) && G >= 0, "%s: bad sizes", what);
  MP_REQUIRE(Fn == 32 && Fe == FE && Fu == 32, "%s: the fused edge step takes node, edge and state widths 32 / 32 / 32, "
             "got %d / %d / %d", what, Fn, Fe, Fu);
  MP_REQUIRE(units0 == H0 && units1 == H1 && units2 == H2, "%s: the fused edge step takes the edge chain [64, 32, 32], "
             "got [%d, %d, %d]", what, units0, units1, units2);
  MP_REQUIRE(act >= 0 && act <= MP_ACT_LAST, "%s: unknown activation code %d", what, act);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: pooling is sum or mean, got op %d", what, pool_op);
  if (N == 0) return MP_OK;
  MP_REQUIRE(ptr0 && pool_out, "%s: null pointer", what);
  const size_t need = mp_tile::ws_bytes(E, H2);
  if (E > 0) {
    MP_REQUIRE(Pa && Pb && Pu && edge_splits && edges && cols && Wc && W1 && W2 && ws && edges_out, "%s: null pointer",
               what);
    MP_REQUIRE(G > 0, "%s: %lld edges in no graph", what, static_cast<long long>(E));
    MP_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", what, ws_bytes, need);
    EdgeArgs a{};
    a.Pa = Pa; a.Pb = Pb; a.Pu = Pu; a.splits = edge_splits; a.x = edges; a.col0 = cols; a.ptr0 = ptr0; a.perm0 = perm0;
    a.Wc = Wc; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.e_out = edges_out; a.pool = pool_out; a.bnd = ws; a.G = G;
    a.N = static_cast<int>(N); a.E = static_cast<int>(E); a.act = act; a.alpha = alpha;
    const int64_t tiles = mp_tile::tiles_of(E);
    megnet_edge_kernel<<<static_cast<unsigned>(tiles < 1024 ? tiles : 1024), 256, 0, mp::as_stream(stream)>>>(a);
    int rc = mp::check_launch(what);
    if (rc != MP_OK) return rc;
  }
  megnet_pool_kernel<<<mp::grid_for(N * H2), 256, 0, mp::as_stream(stream)>>>(ptr0, N, ws, pool_op == MP_MEAN ? 1 : 0,
                                                                              pool_out);
  return mp::check_launch("mp_megnet_edge_f32 (pool)");
}

}  // extern "C"
