// Hierarchical pooling on ragged batches (kgcnn/layers/pool/topk.py): top-k node selection with the induced subgraph
// (PoolingTopK, topk.py:68-197), the reverse scatter (UnPoolingTopK, topk.py:252-287) and powers of the adjacency matrix
// on the edge list (AdjacencyPower, topk.py:330-391).  Nothing here forms a (Nmax, Nmax) or (M, 2, removed) tensor: every
// intermediate is linear in N, M or the size of the output.
//
// Selection.  s_i = sum_c (x[i,c] p[c]) / ||p||; the rank of node i is the number of nodes j of its graph with
// (s_j, j) < (s_i, i) - scores compare as floats (-0.0 == 0.0), ties go to the smaller index - so ranks are a permutation
// of 0..N_g-1 whatever the ties, with no sort.  nremove = rint(float(k) float(N_g)) (half to even), the kept nodes are the
// ranks >= nremove and new row new_splits[g] + rank - nremove holds them in ascending (s, i).  A block owns 256
// consecutive nodes and streams the scores of every graph its nodes belong to through LDS 256 at a time: no cap on N_g.
//
// Induced edges.  A lane group owns a NEW receiver, walks the OLD receiver's CSR bucket (in list order: through the stable
// permutation when the list is unsorted), counts the edges whose sender is kept; an int64 prefix sum; the same walk again
// compacts with ballot + popcount.  The output is sorted by new receiver and stable in the old order by construction.
//
// A . B (row-wise Gustavson).  A wave owns output row i and accumulates it in LDS, kAccFloats columns at a time (larger
// graphs run over column ranges): for every edge (i, j) of the left operand, in list order, the lanes run across the edges
// (j, k) of the right operand - distinct k without duplicate edges - and add a_ij b_jk.  The count pass counts the entries
// > eps (every non-zero entry for an intermediate power: a negative entry of A^2 still contributes to A^3, as in the dense
// product), the fill pass repeats the row in the same order (equal bits) and compacts in k order.
//
// No atomics on data; every sum runs in an order fixed by the inputs: equal bits on every call.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "mp_common.h"
#include "../../include/mpengine/topk.h"

namespace {

constexpr int kBlock = 256;
constexpr int kEdgeGroup = 16;                       // lanes per new receiver of the induced-edge walk
constexpr int kEdgeGroupsPerBlock = kBlock / kEdgeGroup;
constexpr int kProdWaves = kBlock / 64;              // output rows in flight per block of the product
constexpr int kAccFloats = MP_TOPK_ACC_FLOATS;       // row accumulator per wave, in floats

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// LDS written by one lane is read by another lane of the same wave: keep the compiler from moving accesses across
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------ selection
__global__ __launch_bounds__(kBlock) void topk_score_kernel(const float* __restrict__ x, int64_t N, int64_t F,
                                                            const float* __restrict__ p, float* __restrict__ score) {
  float sq = 0.0f;
  for (int64_t c = 0; c < F; ++c) sq += p[c] * p[c];
  const float norm = sqrtf(sq);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += stride) {
    const float* row = x + i * F;
    float s = 0.0f;
    for (int64_t c = 0; c < F; ++c) s += row[c] * p[c] / norm;   // topk.py:84: sum(n * p / norm_p)
    score[i] = s;
  }
}

// nkeep per graph (topk.py:96-98); counts[G] = 0 closes the exclusive scan
__global__ void topk_keep_kernel(const int64_t* __restrict__ splits, int64_t G, int64_t N, float k,
                                 int64_t* __restrict__ counts) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g <= G; g += stride) {
    int64_t keep = 0;
    if (g < G) {
      const int64_t n = clamp64(splits[g + 1], 0, N) - clamp64(splits[g], 0, N);
      if (n > 0) {
        const int64_t rem = clamp64(static_cast<int64_t>(rintf(k * static_cast<float>(n))), 0, n);
        keep = n - rem;
      }
    }
    counts[g] = keep;
  }
}

struct SelectArgs {
  const float* x;
  const float* score;
  const int64_t* splits;       // (G+1) old node splits
  const int64_t* new_splits;   // (G+1)
  int64_t N, F, G, Nk;
  int batch_indexing;
  float* out;                  // (Nk, F)
  int64_t* map_nodes;          // (Nk)
  int32_t* map_global;         // (Nk)
  int32_t* old2new;            // (N)
};

__global__ __launch_bounds__(kBlock) void topk_rank_kernel(SelectArgs a) {
  __shared__ float s_chunk[kBlock];
  __shared__ float s_gate[kBlock];
  __shared__ int64_t s_pos[kBlock];
  const int tid = threadIdx.x;
  for (int64_t tile = static_cast<int64_t>(blockIdx.x) * kBlock; tile < a.N; tile += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t tile_end = tile + kBlock < a.N ? tile + kBlock : a.N;
    const int64_t i = tile + tid;
    const float s_i = i < a.N ? a.score[i] : 0.0f;
    int64_t rank = 0, my_g = -1;
    for (int64_t g = mp_owner_of(a.splits, a.G, tile); g < a.G; ++g) {       // block-uniform loop
      const int64_t lo = clamp64(a.splits[g], 0, a.N), hi = clamp64(a.splits[g + 1], 0, a.N);
      if (lo >= tile_end) break;
      const bool mine = i < a.N && i >= lo && i < hi;
      if (mine) my_g = g;
      for (int64_t base = lo; base < hi; base += kBlock) {
        __syncthreads();
        if (base + tid < hi) s_chunk[tid] = a.score[base + tid];
        __syncthreads();
        if (mine) {
          const int n = static_cast<int>(hi - base < kBlock ? hi - base : kBlock);
          for (int t = 0; t < n; ++t) {
            const float s_j = s_chunk[t];
            rank += (s_j < s_i || (s_j == s_i && base + t < i)) ? 1 : 0;
          }
        }
      }
    }
    int64_t pos = -1;
    if (my_g >= 0) {
      const int64_t lo = clamp64(a.splits[my_g], 0, a.N), hi = clamp64(a.splits[my_g + 1], 0, a.N);
      const int64_t nlo = a.new_splits[my_g], nhi = a.new_splits[my_g + 1];
      const int64_t nremove = (hi - lo) - (nhi - nlo);
      if (rank >= nremove) pos = nlo + rank - nremove;
      if (pos < 0 || pos >= nhi || pos >= a.Nk) pos = -1;
      if (pos >= 0) {
        a.map_nodes[pos] = a.batch_indexing ? i : i - lo;
        a.map_global[pos] = static_cast<int32_t>(i);
      }
    }
    if (i < a.N) a.old2new[i] = static_cast<int32_t>(pos);
    __syncthreads();
    s_pos[tid] = pos;
    s_gate[tid] = 1.0f / (1.0f + expf(-s_i));   // topk.py:116
    __syncthreads();
    const int64_t elems = (tile_end - tile) * a.F;
    for (int64_t q = tid; q < elems; q += kBlock) {
      const int64_t r = q / a.F, c = q - r * a.F;
      const int64_t dst = s_pos[r];
      if (dst >= 0) a.out[dst * a.F + c] = a.x[(tile + r) * a.F + c] * s_gate[r];
    }
  }
}

// out[g] = off[clamp(splits[g])], g in [0, G]: row splits of a list that was built per row of `splits`' items
__global__ void topk_splits_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ splits, int64_t G,
                                   int64_t n, int64_t* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g <= G; g += stride)
    out[g] = off[clamp64(splits[g], 0, n)];
}

// ------------------------------------------------------------------------------------------------ induced edges
struct EdgeArgs {
  const int32_t* ptr0;         // (N+1) old receiver CSR
  const int32_t* perm0;        // (M) or null
  const int32_t* send;         // (M) shifted old sender column
  int64_t M, N;
  const int32_t* map_global;   // (Nk) new node -> old node
  const int32_t* old2new;      // (N) old node -> new node or -1
  int64_t Nk;
};

// old edge at bucket position p of new receiver t's old bucket, and whether it survives; *j_new: its new sender
__device__ __forceinline__ bool edge_kept(const EdgeArgs& a, int64_t p, int64_t end, int64_t* m_out, int32_t* j_new) {
  if (p >= end) return false;
  const int64_t m = a.perm0 ? static_cast<int64_t>(a.perm0[p]) : p;
  if (m < 0 || m >= a.M) return false;
  const int32_t j = a.send[m];
  if (j < 0 || j >= a.N) return false;
  const int32_t jn = a.old2new[j];
  if (jn < 0 || jn >= a.Nk) return false;
  *m_out = m;
  *j_new = jn;
  return true;
}

__device__ __forceinline__ void edge_bucket(const EdgeArgs& a, int64_t t, int64_t* begin, int64_t* end) {
  const int64_t i = a.map_global[t];
  int64_t b = 0, e = 0;
  if (i >= 0 && i < a.N) {
    b = clamp64(a.ptr0[i], 0, a.M);
    e = clamp64(a.ptr0[i + 1], 0, a.M);
  }
  *begin = b;
  *end = e;
}

__device__ __forceinline__ uint32_t edge_group_ballot(bool pred, int group_in_wave) {
  return static_cast<uint32_t>(__ballot(pred) >> (group_in_wave * kEdgeGroup)) & ((1u << kEdgeGroup) - 1u);
}

__global__ __launch_bounds__(kBlock) void topk_edges_count_kernel(EdgeArgs a, int64_t* __restrict__ counts) {
  const int lane = threadIdx.x & (kEdgeGroup - 1);
  const int group_in_wave = (threadIdx.x & 63) / kEdgeGroup;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEdgeGroupsPerBlock;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kEdgeGroupsPerBlock + threadIdx.x / kEdgeGroup; t < a.Nk; t += stride) {
    int64_t begin, end;
    edge_bucket(a, t, &begin, &end);
    int64_t cnt = 0;
    for (int64_t base = begin; base < end; base += kEdgeGroup) {
      int64_t m;
      int32_t jn;
      const bool keep = edge_kept(a, base + lane, end, &m, &jn);
      cnt += __popc(edge_group_ballot(keep, group_in_wave));
    }
    if (lane == 0) counts[t] = cnt;
  }
}

struct EdgeOut {
  const int64_t* off;              // (Nk+1)
  const int64_t* new_node_splits;  // (G+1)
  const int64_t* old_edge_splits;  // (G+1)
  int64_t G, Mk;
  const float* edges;              // (M, Fe)
  int64_t Fe;
  int batch_indexing;
  float* edges_out;                // (Mk, Fe)
  int64_t* idx_out;                // (Mk, 2)
  int64_t* map_edges;              // (Mk)
  int32_t* map_edges_global;       // (Mk) old batch-wide edge position
  int32_t* cols_out;               // (2, Mk)
  int32_t* ptr_out;                // (Nk+1)
  int32_t* edge_old2new;           // (M), pre-filled with -1; nullable
};

__global__ __launch_bounds__(kBlock) void topk_edges_fill_kernel(EdgeArgs a, EdgeOut o) {
  const int lane = threadIdx.x & (kEdgeGroup - 1);
  const int group_in_wave = (threadIdx.x & 63) / kEdgeGroup;
  const uint32_t below = (1u << lane) - 1u;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEdgeGroupsPerBlock;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kEdgeGroupsPerBlock + threadIdx.x / kEdgeGroup; t < a.Nk; t += stride) {
    int64_t pos = o.off[t];
    const int64_t pos_end = o.off[t + 1];
    if (lane == 0) {
      o.ptr_out[t] = static_cast<int32_t>(pos);
      if (t == a.Nk - 1) o.ptr_out[a.Nk] = static_cast<int32_t>(pos_end);
    }
    if (pos_end <= pos) continue;   // uniform over the group
    int64_t begin, end;
    edge_bucket(a, t, &begin, &end);
    const int64_t g = mp_owner_of(o.new_node_splits, o.G, t);
    const int64_t node_base = o.batch_indexing ? 0 : o.new_node_splits[g];
    const int64_t edge_base = o.batch_indexing ? 0 : o.old_edge_splits[g];
    for (int64_t base = begin; base < end; base += kEdgeGroup) {
      int64_t m = 0;
      int32_t jn = 0;
      bool keep = edge_kept(a, base + lane, end, &m, &jn);
      const uint32_t mask = edge_group_ballot(keep, group_in_wave);
      const int64_t row = pos + __popc(mask & below);
      pos += __popc(mask);
      keep = keep && row >= 0 && row < o.Mk && row < pos_end;   // rows stay inside what the count pass sized
      if (keep) {
        o.idx_out[2 * row] = t - node_base;
        o.idx_out[2 * row + 1] = jn - node_base;
        o.map_edges[row] = m - edge_base;
        o.map_edges_global[row] = static_cast<int32_t>(m);
        o.cols_out[row] = static_cast<int32_t>(t);
        o.cols_out[o.Mk + row] = jn;
        if (o.edge_old2new) o.edge_old2new[m] = static_cast<int32_t>(row);
      }
      // feature rows: the group copies the kept rows of this chunk one after the other, lanes across the columns
      const int64_t src_row = keep ? m : -1;
      for (int b = 0; b < kEdgeGroup; ++b) {
        const int64_t src = __shfl(src_row, b, kEdgeGroup);
        const int64_t dst = __shfl(row, b, kEdgeGroup);
        if (src < 0) continue;   // uniform over the group
        for (int64_t c = lane; c < o.Fe; c += kEdgeGroup) o.edges_out[dst * o.Fe + c] = o.edges[src * o.Fe + c];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ A . B
struct ProdArgs {
  const int32_t* ptrL;    // (N+1) row CSR of the left operand
  const int32_t* permL;   // (ML) or null
  const int32_t* colL;    // (ML) shifted column index of every left entry
  const float* valL;      // (ML, ldL): column 0 is the value
  int64_t ldL, ML;
  const int32_t* ptrR;    // right operand, same form; ptrR == null: the identity (thresholding alone)
  const int32_t* permR;
  const int32_t* colR;
  const float* valR;
  int64_t ldR, MR;
  int64_t N, G;
  const int64_t* node_splits;
  float eps;
  int keep_nonzero;   // intermediate power: keep every non-zero entry instead of the entries > eps
};

struct ProdOut {
  const int64_t* off;   // (N+1)
  int64_t Mo;
  int batch_indexing;
  float* vals;          // (Mo)
  int64_t* idx;         // (Mo, 2)
  int32_t* cols;        // (2, Mo)
  int32_t* ptr;         // (N+1)
};

template <bool kFill>
__global__ __launch_bounds__(kBlock) void adjacency_product_kernel(ProdArgs a, int64_t* __restrict__ counts, ProdOut o) {
  __shared__ float acc_all[kProdWaves][kAccFloats];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* acc = acc_all[wave];
  const uint64_t below = (uint64_t{1} << lane) - 1u;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kProdWaves;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kProdWaves + wave; row < a.N; row += stride) {   // wave-uniform
    const int64_t g = mp_owner_of(a.node_splits, a.G, row);
    const int64_t base = clamp64(a.node_splits[g], 0, a.N);
    const int64_t ng = clamp64(a.node_splits[g + 1], 0, a.N) - base;
    const int64_t lb = clamp64(a.ptrL[row], 0, a.ML), le = clamp64(a.ptrL[row + 1], 0, a.ML);
    int64_t cnt = 0, pos = 0, pos_end = 0;
    if (kFill) {
      pos = o.off[row];
      pos_end = o.off[row + 1];
      if (lane == 0) {
        o.ptr[row] = static_cast<int32_t>(pos);
        if (row == a.N - 1) o.ptr[a.N] = static_cast<int32_t>(pos_end);
      }
      if (pos_end <= pos) continue;
    }
    for (int64_t k0 = 0; k0 < ng; k0 += kAccFloats) {
      const int kn = static_cast<int>(ng - k0 < kAccFloats ? ng - k0 : kAccFloats);
      for (int c = lane; c < kn; c += 64) acc[c] = 0.0f;
      wave_lds_fence();
      for (int64_t p = lb; p < le; ++p) {                       // the row's entries in list order
        const int64_t e = a.permL ? static_cast<int64_t>(a.permL[p]) : p;
        if (e < 0 || e >= a.ML) continue;
        const int64_t j = a.colL[e];
        if (j < 0 || j >= a.N) continue;
        const float aij = a.valL[e * a.ldL];
        if (a.ptrR == nullptr) {
          const int64_t c = j - base - k0;
          if (lane == 0 && c >= 0 && c < kn) acc[c] = aij;      // tensor_scatter_nd_update (topk.py:356)
        } else {
          const int64_t rb = clamp64(a.ptrR[j], 0, a.MR), re = clamp64(a.ptrR[j + 1], 0, a.MR);
          for (int64_t q = rb + lane; q < re; q += 64) {        // lanes across the entries of row j: distinct columns
            const int64_t f = a.permR ? static_cast<int64_t>(a.permR[q]) : q;
            if (f < 0 || f >= a.MR) continue;
            const int64_t c = static_cast<int64_t>(a.colR[f]) - base - k0;
            if (c >= 0 && c < kn) acc[c] += aij * a.valR[f * a.ldR];
          }
        }
        wave_lds_fence();
      }
      for (int c0 = 0; c0 < kn; c0 += 64) {
        const int c = c0 + lane;
        const float v = c < kn ? acc[c] : 0.0f;
        const bool keep = c < kn && (a.keep_nonzero ? v != 0.0f : v > a.eps);   // topk.py:367
        const uint64_t mask = __ballot(keep);
        if (kFill) {
          const int64_t t = pos + __popcll(mask & below);
          pos += __popcll(mask);
          if (keep && t >= 0 && t < o.Mo && t < pos_end) {
            const int64_t col = base + k0 + c;
            o.vals[t] = v;
            o.idx[2 * t] = o.batch_indexing ? row : row - base;
            o.idx[2 * t + 1] = o.batch_indexing ? col : col - base;
            o.cols[t] = static_cast<int32_t>(row);
            o.cols[o.Mo + t] = static_cast<int32_t>(col);
          }
        } else {
          cnt += __popcll(mask);
        }
      }
      wave_lds_fence();
    }
    if (!kFill && lane == 0) counts[row] = cnt;
  }
}

// ------------------------------------------------------------------------------------------------ unpool
__global__ void topk_invert_kernel(const int64_t* __restrict__ map, int64_t Nk, const int64_t* __restrict__ new_splits,
                                   const int64_t* __restrict__ old_splits, int64_t G, int batch_indexing, int64_t N,
                                   int32_t* __restrict__ old2new) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < Nk; t += stride) {
    int64_t i = map[t];
    if (!batch_indexing) {
      const int64_t g = mp_owner_of(new_splits, G, t);
      const int64_t lo = old_splits[g], hi = old_splits[g + 1];
      i = (i >= 0 && i < hi - lo) ? i + lo : -1;
    }
    if (i >= 0 && i < N) old2new[i] = static_cast<int32_t>(t);
  }
}

// out[i] = (skip ? skip[i] : 0) + (old2new[i] >= 0 ? pooled[old2new[i]] : 0)   (topk.py:277 plus the model's LazyAdd)
__global__ __launch_bounds__(kBlock) void topk_unpool_kernel(const float* __restrict__ pooled, int64_t Nk, int64_t F,
                                                             const int32_t* __restrict__ old2new, int64_t N,
                                                             const float* __restrict__ skip, float* __restrict__ out) {
  const int64_t total = N * F;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int64_t i = q / F, c = q - i * F;
    const int64_t t = old2new[i];
    const float v = (t >= 0 && t < Nk) ? pooled[t * F + c] : 0.0f;
    out[q] = skip ? v + skip[q] : v;
  }
}

// counts (n+1, last = 0) -> off (n+1) on the workspace layout of mp_topk_workspace_bytes
int scan_counts(int64_t* counts, int64_t* off, int64_t n, void* ws, size_t ws_bytes, hipStream_t s) {
  const size_t counts_bytes = mp::align256(sizeof(int64_t) * static_cast<size_t>(n + 1));
  void* temp = static_cast<char*>(ws) + counts_bytes;
  size_t temp_bytes = ws_bytes - counts_bytes;
  MP_HIP(rocprim::exclusive_scan(temp, temp_bytes, counts, off, int64_t{0}, static_cast<size_t>(n + 1),
                                 rocprim::plus<int64_t>(), s, false));
  return MP_OK;
}

int check_ws(const char* what, int64_t n, void* ws, size_t ws_bytes) {
  size_t need = 0;
  int rc = mp_topk_workspace_bytes(n, &need);
  if (rc != MP_OK) return rc;
  MP_REQUIRE(ws != nullptr && ws_bytes >= need, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_topk_workspace_bytes(int64_t n, size_t* bytes_out_host) {
  MP_REQUIRE(bytes_out_host && n >= 0, "mp_topk_workspace_bytes: bad arguments");
  size_t temp = 0;
  hipError_t e = rocprim::exclusive_scan(nullptr, temp, static_cast<const int64_t*>(nullptr),
                                         static_cast<int64_t*>(nullptr), int64_t{0}, static_cast<size_t>(n + 1),
                                         rocprim::plus<int64_t>(), hipStream_t{nullptr}, false);
  if (e != hipSuccess) {
    mp::set_error("rocprim temp-size query failed: %s", hipGetErrorString(e));
    return MP_EHIP;
  }
  *bytes_out_host = mp::align256(temp) + mp::align256(sizeof(int64_t) * static_cast<size_t>(n + 1));
  return MP_OK;
}

int mp_topk_select_f32(const float* x, int64_t N, int64_t F, const float* p, const int64_t* node_splits, int64_t G,
                       float k, int64_t Nk, int batch_indexing, float* score, int64_t* new_splits, float* out,
                       int64_t* map_nodes, int32_t* map_global, int32_t* old2new, void* ws, size_t ws_bytes,
                       mpStream_t stream) {
  MP_REQUIRE(N >= 0 && F >= 1 && G >= 0 && Nk >= 0 && Nk <= N, "mp_topk_select_f32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31), "mp_topk_select_f32: N must fit int32");
  MP_REQUIRE(k >= 0.0f && k <= 1.0f, "mp_topk_select_f32: k = %g is outside [0, 1]", static_cast<double>(k));
  if (G == 0) return MP_OK;
  MP_REQUIRE(node_splits && new_splits, "mp_topk_select_f32: null splits");
  int rc = check_ws("mp_topk_select_f32", G, ws, ws_bytes);
  if (rc != MP_OK) return rc;
  hipStream_t s = mp::as_stream(stream);
  int64_t* counts = static_cast<int64_t*>(ws);
  topk_keep_kernel<<<mp::grid_for(G + 1), 256, 0, s>>>(node_splits, G, N, k, counts);
  rc = scan_counts(counts, new_splits, G, ws, ws_bytes, s);
  if (rc != MP_OK) return rc;
  if (N > 0) {
    MP_REQUIRE(x && p && score && map_global && old2new && (Nk == 0 || (out && map_nodes)),
               "mp_topk_select_f32: null pointer");
    topk_score_kernel<<<mp::grid_for(N), kBlock, 0, s>>>(x, N, F, p, score);
    const SelectArgs a{x, score, node_splits, new_splits, N, F, G, Nk, batch_indexing, out, map_nodes, map_global, old2new};
    topk_rank_kernel<<<mp::grid_for(N, kBlock), kBlock, 0, s>>>(a);
  }
  return mp::check_launch("mp_topk_select_f32");
}

int mp_topk_edges_count_i32(const int32_t* ptr0, const int32_t* perm0, const int32_t* send, int64_t M, int64_t N,
                            const int32_t* map_global, const int32_t* old2new, int64_t Nk, const int64_t* new_node_splits,
                            int64_t G, int64_t* off, int64_t* edge_splits_out, void* ws, size_t ws_bytes,
                            mpStream_t stream) {
  MP_REQUIRE(M >= 0 && N >= 0 && Nk >= 0 && Nk <= N && G >= 0, "mp_topk_edges_count_i32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31) && M < (int64_t{1} << 31), "mp_topk_edges_count_i32: N, M must fit int32");
  if (G == 0) return MP_OK;
  MP_REQUIRE(new_node_splits && off && edge_splits_out, "mp_topk_edges_count_i32: null pointer");
  MP_REQUIRE(Nk == 0 || M == 0 || (ptr0 && send && map_global && old2new), "mp_topk_edges_count_i32: null pointer");
  int rc = check_ws("mp_topk_edges_count_i32", Nk, ws, ws_bytes);
  if (rc != MP_OK) return rc;
  hipStream_t s = mp::as_stream(stream);
  int64_t* counts = static_cast<int64_t*>(ws);
  if (Nk == 0 || M == 0) {
    MP_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * static_cast<size_t>(Nk + 1), s));
  } else {
    MP_HIP(hipMemsetAsync(counts + Nk, 0, sizeof(int64_t), s));
    const EdgeArgs a{ptr0, perm0, send, M, N, map_global, old2new, Nk};
    topk_edges_count_kernel<<<mp::grid_for(Nk, kEdgeGroupsPerBlock), kBlock, 0, s>>>(a, counts);
  }
  rc = scan_counts(counts, off, Nk, ws, ws_bytes, s);
  if (rc != MP_OK) return rc;
  topk_splits_kernel<<<mp::grid_for(G + 1), 256, 0, s>>>(off, new_node_splits, G, Nk, edge_splits_out);
  return mp::check_launch("mp_topk_edges_count_i32");
}

int mp_topk_edges_fill_f32(const int32_t* ptr0, const int32_t* perm0, const int32_t* send, int64_t M, int64_t N,
                           const int32_t* map_global, const int32_t* old2new, int64_t Nk, const int64_t* new_node_splits,
                           const int64_t* old_edge_splits, int64_t G, const int64_t* off, int64_t Mk, const float* edges,
                           int64_t Fe, int batch_indexing, float* edges_out, int64_t* idx_out, int64_t* map_edges,
                           int32_t* map_edges_global, int32_t* cols_out, int32_t* ptr_out, int32_t* edge_old2new, mpStream_t stream) {
  MP_REQUIRE(M >= 0 && N >= 0 && Nk >= 0 && Nk <= N && G >= 0 && Mk >= 0 && Mk <= M && Fe >= 0,
             "mp_topk_edges_fill_f32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31) && M < (int64_t{1} << 31), "mp_topk_edges_fill_f32: N, M must fit int32");
  MP_REQUIRE(ptr_out != nullptr, "mp_topk_edges_fill_f32: null ptr_out");
  hipStream_t s = mp::as_stream(stream);
  if (edge_old2new && M > 0) MP_HIP(hipMemsetAsync(edge_old2new, 0xFF, sizeof(int32_t) * static_cast<size_t>(M), s));
  if (Nk == 0 || G == 0 || Mk == 0) {
    MP_HIP(hipMemsetAsync(ptr_out, 0, sizeof(int32_t) * static_cast<size_t>(Nk + 1), s));
    return MP_OK;
  }
  MP_REQUIRE(ptr0 && send && map_global && old2new && new_node_splits && old_edge_splits && off && idx_out &&
                 map_edges && map_edges_global && cols_out && (Fe == 0 || (edges && edges_out)),
             "mp_topk_edges_fill_f32: null pointer");
  const EdgeArgs a{ptr0, perm0, send, M, N, map_global, old2new, Nk};
  const EdgeOut o{off, new_node_splits, old_edge_splits, G, Mk, edges, Fe, batch_indexing, edges_out, idx_out,
                  map_edges, map_edges_global, cols_out, ptr_out, edge_old2new};
  topk_edges_fill_kernel<<<mp::grid_for(Nk, kEdgeGroupsPerBlock), kBlock, 0, s>>>(a, o);
  return mp::check_launch("mp_topk_edges_fill_f32");
}

int mp_adjacency_product_count_f32(const int32_t* ptrL, const int32_t* permL, const int32_t* colL, const float* valL,
                                   int64_t ldL, int64_t ML, const int32_t* ptrR, const int32_t* permR,
                                   const int32_t* colR, const float* valR, int64_t ldR, int64_t MR, int64_t N,
                                   const int64_t* node_splits, int64_t G, float eps, int keep_nonzero, int64_t* off,
                                   int64_t* edge_splits_out, void* ws, size_t ws_bytes, mpStream_t stream) {
  MP_REQUIRE(ML >= 0 && MR >= 0 && N >= 0 && G >= 0 && ldL >= 1 && ldR >= 1, "mp_adjacency_product_count_f32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31) && ML < (int64_t{1} << 31) && MR < (int64_t{1} << 31),
             "mp_adjacency_product_count_f32: N, M must fit int32");
  if (G == 0) return MP_OK;
  MP_REQUIRE(node_splits && off && edge_splits_out, "mp_adjacency_product_count_f32: null pointer");
  MP_REQUIRE(N == 0 || ptrL, "mp_adjacency_product_count_f32: null left CSR");
  MP_REQUIRE(ML == 0 || (colL && valL), "mp_adjacency_product_count_f32: null left operand");
  MP_REQUIRE(ptrR == nullptr || MR == 0 || (colR && valR), "mp_adjacency_product_count_f32: null right operand");
  int rc = check_ws("mp_adjacency_product_count_f32", N, ws, ws_bytes);
  if (rc != MP_OK) return rc;
  hipStream_t s = mp::as_stream(stream);
  int64_t* counts = static_cast<int64_t*>(ws);
  MP_HIP(hipMemsetAsync(counts + N, 0, sizeof(int64_t), s));
  if (N > 0) {
    const ProdArgs a{ptrL, permL, colL, valL, ldL, ML, ptrR, permR, colR, valR, ldR, MR, N, G, node_splits, eps, keep_nonzero};
    adjacency_product_kernel<false><<<mp::grid_for(N, kProdWaves), kBlock, 0, s>>>(a, counts, ProdOut{});
  }
  rc = scan_counts(counts, off, N, ws, ws_bytes, s);
  if (rc != MP_OK) return rc;
  topk_splits_kernel<<<mp::grid_for(G + 1), 256, 0, s>>>(off, node_splits, G, N, edge_splits_out);
  return mp::check_launch("mp_adjacency_product_count_f32");
}

int mp_adjacency_product_fill_f32(const int32_t* ptrL, const int32_t* permL, const int32_t* colL, const float* valL,
                                  int64_t ldL, int64_t ML, const int32_t* ptrR, const int32_t* permR,
                                  const int32_t* colR, const float* valR, int64_t ldR, int64_t MR, int64_t N,
                                  const int64_t* node_splits, int64_t G, float eps, int keep_nonzero, const int64_t* off, int64_t Mo,
                                  int batch_indexing, float* vals_out, int64_t* idx_out, int32_t* cols_out,
                                  int32_t* ptr_out, mpStream_t stream) {
  MP_REQUIRE(ML >= 0 && MR >= 0 && N >= 0 && G >= 0 && Mo >= 0 && ldL >= 1 && ldR >= 1,
             "mp_adjacency_product_fill_f32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31) && ML < (int64_t{1} << 31) && MR < (int64_t{1} << 31),
             "mp_adjacency_product_fill_f32: N, M must fit int32");
  MP_REQUIRE(Mo < (int64_t{1} << 31), "mp_adjacency_product_fill_f32: %lld entries do not fit the int32 plan columns",
             (long long)Mo);
  MP_REQUIRE(ptr_out != nullptr, "mp_adjacency_product_fill_f32: null ptr_out");
  hipStream_t s = mp::as_stream(stream);
  if (N == 0 || G == 0) {
    MP_HIP(hipMemsetAsync(ptr_out, 0, sizeof(int32_t) * static_cast<size_t>(N + 1), s));
    return MP_OK;
  }
  MP_REQUIRE(ptrL && node_splits && off, "mp_adjacency_product_fill_f32: null pointer");
  MP_REQUIRE(ML == 0 || (colL && valL), "mp_adjacency_product_fill_f32: null left operand");
  MP_REQUIRE(ptrR == nullptr || MR == 0 || (colR && valR), "mp_adjacency_product_fill_f32: null right operand");
  MP_REQUIRE(Mo == 0 || (vals_out && idx_out && cols_out), "mp_adjacency_product_fill_f32: null output");
  const ProdArgs a{ptrL, permL, colL, valL, ldL, ML, ptrR, permR, colR, valR, ldR, MR, N, G, node_splits, eps, keep_nonzero};
  const ProdOut o{off, Mo, batch_indexing, vals_out, idx_out, cols_out, ptr_out};
  adjacency_product_kernel<true><<<mp::grid_for(N, kProdWaves), kBlock, 0, s>>>(a, nullptr, o);
  return mp::check_launch("mp_adjacency_product_fill_f32");
}

int mp_topk_invert_map_i64(const int64_t* map, int64_t Nk, const int64_t* new_splits, const int64_t* old_splits, int64_t G,
                           int batch_indexing, int64_t N, int32_t* old2new, mpStream_t stream) {
  MP_REQUIRE(Nk >= 0 && N >= 0 && G >= 0, "mp_topk_invert_map_i64: bad sizes");
  MP_REQUIRE(Nk < (int64_t{1} << 31) && N < (int64_t{1} << 31), "mp_topk_invert_map_i64: sizes must fit int32");
  if (N == 0) return MP_OK;
  MP_REQUIRE(old2new != nullptr, "mp_topk_invert_map_i64: null pointer");
  hipStream_t s = mp::as_stream(stream);
  MP_HIP(hipMemsetAsync(old2new, 0xFF, sizeof(int32_t) * static_cast<size_t>(N), s));
  if (Nk == 0 || G == 0) return MP_OK;
  MP_REQUIRE(map && new_splits && old_splits, "mp_topk_invert_map_i64: null pointer");
  topk_invert_kernel<<<mp::grid_for(Nk), 256, 0, s>>>(map, Nk, new_splits, old_splits, G, batch_indexing, N, old2new);
  return mp::check_launch("mp_topk_invert_map_i64");
}

int mp_topk_unpool_f32(const float* pooled, int64_t Nk, int64_t F, const int32_t* old2new, int64_t N, const float* skip,
                       float* out, mpStream_t stream) {
  MP_REQUIRE(Nk >= 0 && N >= 0 && F >= 1, "mp_topk_unpool_f32: bad sizes");
  if (N == 0) return MP_OK;
  MP_REQUIRE(old2new && out && (Nk == 0 || pooled), "mp_topk_unpool_f32: null pointer");
  topk_unpool_kernel<<<mp::grid_for(N * F), kBlock, 0, mp::as_stream(stream)>>>(pooled, Nk, F, old2new, N, skip, out);
  return mp::check_launch("mp_topk_unpool_f32");
}

}  // extern "C"
