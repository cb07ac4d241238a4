// Stage 0 of the fused SchNet forward with the node-input chain replaced by a row gather.
//
// The chain of csrc/mp_schnet_node.hip (NODE_IN) computes n = Embedding(Z) W0 + b0 and x = n Wx - functions of the node
// number alone.  A batch of 11.5 k nodes ran 720 sixteen-node tiles of two GEMMs to produce rows that are copies of at
// most vocab + 1 distinct ones.  Here the two GEMMs run once per weight update, for the vocabulary
// (mp_schnet_embed_table_f32: the SAME chain on the node numbers 0 .. vocab-1, -1, so every table row has the bits the
// chain writes for a node with that number), and a forward copies rows:
//
//   Tn[r] = emb[r] W0 + b0,  Tx[r] = Tn[r] Wx   (r < vocab);   row vocab = the chain's row for a number outside 0 .. vocab-1
//
// The node role needs no LDS, no barrier and ~40 registers: a half wave moves one 512-B row with 16-B accesses, every
// node-number load of a step is issued before the first row load, every row load before the first store.
#include "mp_common.h"
#include "mp_edge_prepare.h"
#include "../../include/mpengine/schnet.h"
#include "../../include/mpengine/schnet_model.h"

namespace {

constexpr int TF = 128;   // feature width of n and x
constexpr int GU = 4;     // rows of each table a half wave has in flight per step
typedef float f32x4 __attribute__((ext_vector_type(4)));   // (arrays of HIP's float4 class are not split into registers)

struct GatherArgs {
  int64_t N;
  const void* numbers;   // (N) float32 or int64 (numbers_i64)
  int numbers_i64;
  int vocab;
  const float* Tn;       // (vocab + 1, 128)
  const float* Tx;
  float* n;              // (N, 128)
  float* x;
};

// Node role.  Node numbers are cast as the chain's stage_load casts them (Keras Embedding: int32) and a number outside
// 0 .. vocab-1 selects row `vocab`.  Addresses are clamped, loads unconditional; only the stores are guarded.
__device__ __forceinline__ void node_gather_body(const GatherArgs& a, int64_t block, int64_t nblocks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, c = lane & 31;
  const int64_t per_block = static_cast<int64_t>(blockDim.x >> 6) * 2 * GU;
  const int64_t n_last = a.N > 0 ? a.N - 1 : 0;
  const f32x4* __restrict__ Tn4 = reinterpret_cast<const f32x4*>(a.Tn);
  const f32x4* __restrict__ Tx4 = reinterpret_cast<const f32x4*>(a.Tx);
  f32x4* __restrict__ n4 = reinterpret_cast<f32x4*>(a.n);
  f32x4* __restrict__ x4 = reinterpret_cast<f32x4*>(a.x);
  for (int64_t base = block * per_block; base < a.N; base += nblocks * per_block) {
    int z[GU];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int64_t node = base + (wave * GU + u) * 2 + half;
      const int64_t l = node < a.N ? node : n_last;
      z[u] = a.numbers_i64 ? static_cast<int>(static_cast<const int64_t*>(a.numbers)[l])
                           : static_cast<int>(static_cast<const float*>(a.numbers)[l]);
    }
    f32x4 vn[GU], vx[GU];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int64_t r = (z[u] < 0 || z[u] >= a.vocab) ? a.vocab : z[u];
      vn[u] = Tn4[r * (TF / 4) + c];
      vx[u] = Tx4[r * (TF / 4) + c];
    }
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int64_t node = base + (wave * GU + u) * 2 + half;
      if (node < a.N) {
        n4[node * (TF / 4) + c] = vn[u];
        x4[node * (TF / 4) + c] = vx[u];
      }
    }
  }
}

// Edge role: mp_prep::edge_prepare_body<true> (same arithmetic, same flags, same bits) with EU edges of a thread in
// flight at once.  The role runs on few workgroups - every one first stages both row-split arrays in LDS - so a union
// batch has four edges per thread; walked one after the other they are four chains of dependent round trips (index row ->
// owner search -> coordinates -> store: ~3.5 us each, 15.8 us for the launch).  Here the EU index rows, then the EU owner
// searches, then the 6 EU coordinate loads are issued together: one chain.  Addresses are clamped and loads unconditional;
// edges past the end repeat the last edge's work and only their stores and flags are guarded.  Requires M > 0, N > 0,
// G <= PREP_LDS_GRAPHS.
typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <int EU>
__device__ __forceinline__ void edge_role_body(const mp_prep::EdgePrepArgs& p, int64_t block, int64_t nblocks) {
  const int64_t M = p.M, G = p.G, N = p.N;
  __shared__ int64_t s_es[mp_prep::PREP_LDS_GRAPHS + 1];
  __shared__ int64_t s_ns[mp_prep::PREP_LDS_GRAPHS + 1];
  const int64_t stride = nblocks * blockDim.x;
  const int64_t e_first = block * blockDim.x + threadIdx.x;
  const i64x2* __restrict__ rows = reinterpret_cast<const i64x2*>(p.idx);
  i64x2 v_pre[EU], pv_pre[EU];
  auto fetch_rows = [&](int64_t e0) {
#pragma unroll
    for (int k = 0; k < EU; ++k) {
      const int64_t e = e0 + k * stride;
      const int64_t l = e < M ? e : M - 1;
      v_pre[k] = rows[l];
      pv_pre[k] = rows[l > 0 ? l - 1 : 0];
    }
  };
  fetch_rows(e_first);
  for (int i = threadIdx.x; i <= G; i += blockDim.x) {
    s_es[i] = p.edge_splits[i];
    s_ns[i] = p.node_splits[i];
  }
  __syncthreads();
  int local_flags = 0;
  for (int64_t e0 = e_first; e0 - (threadIdx.x & 63) < M; e0 += EU * stride) {
    i64x2 v[EU], pv[EU];
#pragma unroll
    for (int k = 0; k < EU; ++k) { v[k] = v_pre[k]; pv[k] = pv_pre[k]; }
    if (e0 + EU * stride - (threadIdx.x & 63) < M) fetch_rows(e0 + EU * stride);   // (wave-uniform) a next round exists
    int64_t si[EU], sj[EU];
#pragma unroll
    for (int k = 0; k < EU; ++k) {
      const int64_t e = e0 + k * stride;
      const bool live = e < M;
      const int64_t ec = live ? e : M - 1;
      const int g = mp_prep::owner_of_lds(s_es, static_cast<int>(G), ec);
      const int64_t base = s_ns[g];
      const int64_t n_g = s_ns[g + 1] - base;
      const int64_t g_start = s_es[g];
      int64_t i = v[k].x, j = v[k].y;
      if (i < 0 || i >= n_g || j < 0 || j >= n_g) {
        if (live) local_flags |= MP_FLAG_OOB;
        const int64_t hi = n_g > 0 ? n_g - 1 : 0;
        i = i < 0 ? 0 : (i > hi ? hi : i);
        j = j < 0 ? 0 : (j > hi ? hi : j);
      }
      si[k] = i + base;
      sj[k] = j + base;
      if (si[k] >= N) si[k] = N - 1;
      if (sj[k] >= N) sj[k] = N - 1;
      // receiver of the previous edge: only the same graph can break the order
      if (live && g_start < e && pv[k].x + base > si[k]) local_flags |= MP_FLAG_UNSORTED_COL0;
    }
    float ci[EU][3], cj[EU][3];
    if (p.dist) {
#pragma unroll
      for (int k = 0; k < EU; ++k) {
        const float* __restrict__ xi = p.xyz + si[k] * 3;
        const float* __restrict__ xj = p.xyz + sj[k] * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { ci[k][c] = xi[c]; cj[k][c] = xj[c]; }
      }
    }
#pragma unroll
    for (int k = 0; k < EU; ++k) {
      const int64_t e = e0 + k * stride;
      if (e < M) {
        p.recv[e] = static_cast<int32_t>(si[k]);
        p.send[e] = static_cast<int32_t>(sj[k]);
        if (p.dist) {
          const float dx = ci[k][0] - cj[k][0];
          const float dy = ci[k][1] - cj[k][1];
          const float dz = ci[k][2] - cj[k][2];
          p.dist[e] = sqrtf(fmaxf(dx * dx + dy * dy + dz * dz, 0.0f));
        }
      }
    }
  }
  mp_publish_flags(p.flags, local_flags);
}

// (256 threads, no register-heavy role: the launch shares a CU with the kernels of other launch sequences)
__global__ __launch_bounds__(256) void schnet_node_gather_kernel(GatherArgs a) {
  node_gather_body(a, blockIdx.x, gridDim.x);
}

template <int EU>
__global__ __launch_bounds__(256) void schnet_stage0_table_kernel(GatherArgs a, mp_prep::EdgePrepArgs p,
                                                                  int node_blocks) {
  if (static_cast<int>(blockIdx.x) < node_blocks) {
    node_gather_body(a, blockIdx.x, node_blocks);
  } else {
    edge_role_body<EU>(p, static_cast<int64_t>(blockIdx.x) - node_blocks,
                       static_cast<int64_t>(gridDim.x) - node_blocks);
  }
}

__global__ void table_numbers_kernel(float* __restrict__ numbers, int vocab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= vocab) numbers[i] = i < vocab ? static_cast<float>(i) : -1.0f;
}

constexpr int NODES_PER_BLOCK = (256 / 64) * 2 * GU;   // one step of a 256-thread workgroup

// Workgroup split of the one-launch stage 0.  Node role: one step per workgroup up to 512 of them (a union batch of
// 11.5 k nodes: 360) - the role holds no per-workgroup state, so the chain's one-workgroup-per-CU cap and the
// half-the-CUs rule of flag bit 9 (both there to amortise its weight slices) do not apply.  Edge role: one edge per thread
// up to EDGE_CAP workgroups; every edge workgroup first stages both row-split arrays in LDS, which is most of what a
// workgroup with few edges does, hence the cap: 128 workgroups of 256 threads, the thread count of the chain build's cap
// (64 of 512).  `several`: the cap bites, a thread has more than one edge (the build with four edges in flight per
// thread).
constexpr unsigned EDGE_CAP = 128;
void stage0_split(int64_t N, int64_t M, int* node_blocks, unsigned* grid, bool* several) {
  const int64_t nb = mp::ceil_div(N, NODES_PER_BLOCK);
  *node_blocks = static_cast<int>(nb < 512 ? nb : 512);
  unsigned eb = mp::grid_for(M);
  if (eb > EDGE_CAP) eb = EDGE_CAP;
  *grid = static_cast<unsigned>(*node_blocks) + eb;
  *several = M > static_cast<int64_t>(eb) * 256;
}

bool one_launch(int64_t N, int64_t M, int64_t G) {
  // outside the latency-bound regime the two stages run as their own (throughput-shaped) launches, as in
  // mp_schnet_stage0_f32
  return N > 0 && M > 0 && (N + 15) / 16 <= 1024 && G <= mp_prep::PREP_LDS_GRAPHS;
}

}  // namespace

extern "C" {

int mp_schnet_embed_table_f32(const float* emb, int vocab, int emb_dim, const float* W0, const float* b0,
                              const float* Wx, float* numbers_ws, float* n_table, float* x_table, int flags,
                              mpStream_t stream) {
  MP_REQUIRE(vocab >= 1 && vocab + 1 <= MP_SCHNET_TABLE_MAX_ROWS, "mp_schnet_embed_table_f32: vocab + 1 = %d rows, "
             "at most %d", vocab + 1, MP_SCHNET_TABLE_MAX_ROWS);
  MP_REQUIRE(numbers_ws && n_table && x_table, "mp_schnet_embed_table_f32: null pointer");
  table_numbers_kernel<<<(vocab + 256) / 256, 256, 0, mp::as_stream(stream)>>>(numbers_ws, vocab);
  int rc = mp::check_launch("mp_schnet_embed_table_f32");
  if (rc != MP_OK) return rc;
  return mp_schnet_node_in_f32(numbers_ws, vocab + 1, emb, vocab, emb_dim, W0, b0, Wx, n_table, x_table,
                               flags & (3 | 64), stream);
}

int mp_schnet_node_in_table_f32(const float* numbers, int64_t N, int vocab, const float* n_table, const float* x_table,
                                float* n_out, float* x_out, int flags, mpStream_t stream) {
  MP_REQUIRE(N >= 0 && vocab >= 1, "mp_schnet_node_in_table_f32: bad sizes");
  if (N == 0) return MP_OK;
  MP_REQUIRE(numbers && n_table && x_table && n_out && x_out, "mp_schnet_node_in_table_f32: null pointer");
  GatherArgs a{N, numbers, (flags & 256) ? 1 : 0, vocab, n_table, x_table, n_out, x_out};
  const int64_t nb = mp::ceil_div(N, NODES_PER_BLOCK);
  schnet_node_gather_kernel<<<static_cast<unsigned>(nb < 2048 ? nb : 2048), 256, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_schnet_node_in_table_f32");
}

int mp_schnet_stage0_table_f32(const float* numbers, int64_t N, int vocab, const float* n_table, const float* x_table,
                               float* n_out, float* x_out, const int64_t* idx, int64_t M, const int64_t* node_splits,
                               const int64_t* edge_splits, int64_t G, const float* xyz, int32_t* recv, int32_t* send,
                               float* dist, int32_t* flags, int flags_arg, mpStream_t stream) {
  MP_REQUIRE(N >= 0 && M >= 0 && G >= 0 && vocab >= 1, "mp_schnet_stage0_table_f32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31) && M < (int64_t{1} << 31), "mp_schnet_stage0_table_f32: N, M must fit int32");
  if (!one_launch(N, M, G)) {
    int rc = mp_edge_prepare_i64_f32(idx, M, node_splits, edge_splits, G, N, xyz, recv, send, dist, flags, stream);
    if (rc != MP_OK) return rc;
    return mp_schnet_node_in_table_f32(numbers, N, vocab, n_table, x_table, n_out, x_out, flags_arg, stream);
  }
  MP_REQUIRE(numbers && n_table && x_table && n_out && x_out && idx && node_splits && edge_splits && recv && send && flags,
             "mp_schnet_stage0_table_f32: null pointer");
  MP_REQUIRE((dist == nullptr) || (xyz != nullptr), "mp_schnet_stage0_table_f32: dist requested without coordinates");
  GatherArgs a{N, numbers, (flags_arg & 256) ? 1 : 0, vocab, n_table, x_table, n_out, x_out};
  mp_prep::EdgePrepArgs p{idx, M, node_splits, edge_splits, G, N, xyz, recv, send, dist, flags};
  int node_blocks;
  unsigned grid;
  bool several;
  stage0_split(N, M, &node_blocks, &grid, &several);
  if (several) schnet_stage0_table_kernel<4><<<grid, 256, 0, mp::as_stream(stream)>>>(a, p, node_blocks);
  else schnet_stage0_table_kernel<1><<<grid, 256, 0, mp::as_stream(stream)>>>(a, p, node_blocks);
  return mp::check_launch("mp_schnet_stage0_table_f32");
}

}  // extern "C"
