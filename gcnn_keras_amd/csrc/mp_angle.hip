// On-GPU SetAngle (kgcnn/graph/preprocessor.py:316-368 -> get_angle_indices, kgcnn/graph/adj.py:300-385, and get_angle,
// adj.py:388-415): the angle list of a whole ragged batch of edge lists, built on the device.
//
// The rule.  For edge n = (i, j) of a graph and edge_pairing in {"jk", "ik", "kj", "ki"}: pos_k is the position of k in
// the pairing, pos_fix the other one, pos_ij = 0 if "i" occurs in the pairing, else 1.  The partners of n are the edges
// m != n of the same graph with idx[m, pos_fix] == idx[n, pos_ij]; edges equal to (i, j) are left out unless multi
// edges are allowed, edges equal to (j, i) unless reverse edges are allowed.  Outputs: the node triple
// (i, j, idx[m, pos_k]) and the edge pair (n, m), ordered by n, then by m ascending (what check_sorted=True yields).
//
// The partners of n are one bucket of the edge list's CSR over column pos_fix (IndexPlan.csr(pos_fix): ptr, and the
// stable-sort perm when that column is unsorted - inside a bucket perm ascends in the edge index, which gives the
// order by m).  The ids are the plan's shifted, clamped int32 columns: graphs are disjoint in shifted ids, so a bucket
// holds edges of one graph only, and out-of-range input cannot address outside the buffers.
//
// Two passes around one int64 prefix sum, no atomics: a lane group of kGroup lanes owns edge n and walks its bucket in
// chunks of kGroup; pass 1 counts the kept partners, the scan gives off[n], pass 2 repeats the walk and compacts every
// chunk with a ballot + prefix popcount, so that neighbouring lanes write neighbouring rows, in order.  The output is
// the same on every run.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "mp_common.h"
#include "../../include/mpengine/geometry.h"

namespace {

constexpr int kGroup = 32;                 // lanes per edge: one chunk covers a molecular bucket (<= 32 neighbours)
constexpr int kBlock = 256;
constexpr int kGroupsPerBlock = kBlock / kGroup;

struct AngleArgs {
  const int32_t* col0;      // (M) shifted column 0 of the edge list
  const int32_t* col1;      // (M) shifted column 1
  const int32_t* ptr;       // (N+1) CSR over column pos_fix
  const int32_t* perm;      // (M) stable-sort permutation of column pos_fix, or null when it is sorted
  int64_t M, N;
  int pos_fix, pos_ij, pos_k, allow_multi, allow_reverse;
};

// The bucket [begin, end) of edge n, clamped to the edge list.
__device__ __forceinline__ void bucket_of(const AngleArgs& a, int32_t i_n, int32_t j_n, int64_t* begin, int64_t* end) {
  const int64_t key = a.pos_ij == 0 ? i_n : j_n;
  int64_t b = 0, e = 0;
  if (key >= 0 && key < a.N) {
    b = a.ptr[key];
    e = a.ptr[key + 1];
    if (b < 0) b = 0;
    if (e > a.M) e = a.M;
  }
  *begin = b;
  *end = e;
}

// Edge at bucket position p (p < end): its index m and whether the rule keeps it as a partner of n = (i_n, j_n).
__device__ __forceinline__ bool partner_at(const AngleArgs& a, int64_t p, int64_t n, int32_t i_n, int32_t j_n,
                                           int64_t* m_out, int32_t* k_out) {
  const int64_t m = a.perm ? static_cast<int64_t>(a.perm[p]) : p;
  if (m < 0 || m >= a.M || m == n) return false;
  const int32_t i_m = a.col0[m], j_m = a.col1[m];
  if (!a.allow_multi && i_m == i_n && j_m == j_n) return false;
  if (!a.allow_reverse && i_m == j_n && j_m == i_n) return false;
  *m_out = m;
  *k_out = a.pos_k == 0 ? i_m : j_m;
  return true;
}

// the kGroup ballot bits of this lane's group
__device__ __forceinline__ uint32_t group_ballot(bool pred, int group_in_wave) {
  return static_cast<uint32_t>(__ballot(pred) >> (group_in_wave * kGroup));
}

__global__ __launch_bounds__(kBlock) void angle_count_kernel(AngleArgs a, int64_t* __restrict__ counts) {
  const int lane = threadIdx.x & (kGroup - 1);
  const int group_in_wave = (threadIdx.x & 63) / kGroup;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupsPerBlock;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + threadIdx.x / kGroup; n < a.M; n += stride) {
    const int32_t i_n = a.col0[n], j_n = a.col1[n];
    int64_t begin, end;
    bucket_of(a, i_n, j_n, &begin, &end);
    int64_t cnt = 0;
    for (int64_t base = begin; base < end; base += kGroup) {
      int64_t m;
      int32_t k;
      const bool keep = base + lane < end && partner_at(a, base + lane, n, i_n, j_n, &m, &k);
      cnt += __popc(group_ballot(keep, group_in_wave));
    }
    if (lane == 0) counts[n] = cnt;
  }
}

struct AngleOut {
  const int64_t* off;          // (M+1) first output row of every edge
  const int64_t* node_splits;  // (G+1)
  const int64_t* edge_splits;  // (G+1)
  int64_t G, A;
  const float* xyz;            // (N,3), read for theta only
  int64_t* triples;            // (A,3) node ids local to the graph
  int64_t* pairs;              // (A,2) edge ids local to the graph
  int32_t* tcols;              // (3,A) shifted node ids
  int32_t* pcols;              // (2,A) shifted edge ids
  float* theta;                // (A)
};

// get_angle (adj.py:405-413) in the arithmetic of mp_vector_angle_f32: atan2(|v1 x v2|, v1 . v2), v1 = x_i - x_j,
// v2 = x_j - x_k
__device__ __forceinline__ float angle_ijk(const float* __restrict__ xyz, int64_t i, int64_t j, int64_t k) {
  const float xj[3] = {xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]};
  const float a[3] = {xyz[3 * i] - xj[0], xyz[3 * i + 1] - xj[1], xyz[3 * i + 2] - xj[2]};
  const float b[3] = {xj[0] - xyz[3 * k], xj[1] - xyz[3 * k + 1], xj[2] - xyz[3 * k + 2]};
  const float c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
  const float x = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const float y = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
  return atan2f(y, x);
}

__global__ __launch_bounds__(kBlock) void angle_fill_kernel(AngleArgs a, AngleOut o) {
  const int lane = threadIdx.x & (kGroup - 1);
  const int group_in_wave = (threadIdx.x & 63) / kGroup;
  const uint32_t below = (1u << lane) - 1u;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupsPerBlock;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + threadIdx.x / kGroup; n < a.M; n += stride) {
    int64_t pos = o.off[n];
    const int64_t pos_end = o.off[n + 1];
    if (pos_end <= pos) continue;   // no partners (uniform over the group)
    const int32_t i_n = a.col0[n], j_n = a.col1[n];
    int64_t begin, end;
    bucket_of(a, i_n, j_n, &begin, &end);
    const int64_t g = mp_owner_of(o.edge_splits, o.G, n);
    const int64_t node_base = o.node_splits[g], edge_base = o.edge_splits[g];
    for (int64_t base = begin; base < end; base += kGroup) {
      int64_t m = 0;
      int32_t k = 0;
      const bool keep = base + lane < end && partner_at(a, base + lane, n, i_n, j_n, &m, &k);
      const uint32_t mask = group_ballot(keep, group_in_wave);
      const int64_t t = pos + __popc(mask & below);
      pos += __popc(mask);
      if (!keep || t < 0 || t >= o.A || t >= pos_end) continue;   // rows stay inside what the count pass sized
      if (o.triples) {
        o.triples[3 * t] = i_n - node_base;
        o.triples[3 * t + 1] = j_n - node_base;
        o.triples[3 * t + 2] = k - node_base;
      }
      if (o.pairs) {
        o.pairs[2 * t] = n - edge_base;
        o.pairs[2 * t + 1] = m - edge_base;
      }
      if (o.tcols) {
        o.tcols[t] = i_n;
        o.tcols[o.A + t] = j_n;
        o.tcols[2 * o.A + t] = k;
      }
      if (o.pcols) {
        o.pcols[t] = static_cast<int32_t>(n);
        o.pcols[o.A + t] = static_cast<int32_t>(m);
      }
      if (o.theta) {
        const bool ok = i_n >= 0 && i_n < a.N && j_n >= 0 && j_n < a.N && k >= 0 && k < a.N;
        o.theta[t] = ok ? angle_ijk(o.xyz, i_n, j_n, k) : 0.0f;
      }
    }
  }
}

__global__ void angle_splits_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ edge_splits, int64_t G,
                                    int64_t M, int64_t* __restrict__ angle_splits) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g <= G; g += stride) {
    int64_t e = edge_splits[g];
    e = e < 0 ? 0 : (e > M ? M : e);
    angle_splits[g] = off[e];
  }
}

// CSR over column 0 of an output list from off: out[v] = off[at ? at[v] : v] for v in [0, n] (at: the edge list's
// column-0 CSR for the triples; identity for the pairs, whose column 0 is the edge index itself).
__global__ void angle_csr_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ at, int64_t n, int64_t M,
                                 int32_t* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; v <= n; v += stride) {
    int64_t e = at ? static_cast<int64_t>(at[v]) : v;
    e = e < 0 ? 0 : (e > M ? M : e);
    out[v] = static_cast<int32_t>(off[e]);
  }
}

int check_pairing(const char* what, int pos_fix, int pos_ij, int pos_k) {
  MP_REQUIRE((pos_fix == 0 || pos_fix == 1) && (pos_ij == 0 || pos_ij == 1) && pos_k == 1 - pos_fix,
             "%s: pos_fix, pos_ij must be 0 or 1 and pos_k the other position than pos_fix", what);
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_angle_list_workspace_bytes(int64_t M, size_t* bytes_out_host) {
  MP_REQUIRE(bytes_out_host && M >= 0, "mp_angle_list_workspace_bytes: bad arguments");
  size_t temp = 0;
  hipError_t e = rocprim::exclusive_scan(nullptr, temp, static_cast<const int64_t*>(nullptr),
                                         static_cast<int64_t*>(nullptr), int64_t{0}, static_cast<size_t>(M + 1),
                                         rocprim::plus<int64_t>(), hipStream_t{nullptr}, false);
  if (e != hipSuccess) {
    mp::set_error("rocprim temp-size query failed: %s", hipGetErrorString(e));
    return MP_EHIP;
  }
  *bytes_out_host = mp::align256(temp) + mp::align256(sizeof(int64_t) * static_cast<size_t>(M + 1));
  return MP_OK;
}

int mp_angle_list_count_i32(const int32_t* edge_cols, int64_t M, int64_t N, const int32_t* ptr, const int32_t* perm,
                            const int64_t* edge_splits, int64_t G, int pos_fix, int pos_ij, int allow_multi_edges,
                            int allow_reverse_edges, int64_t* off /* (M+1) */, int64_t* angle_splits /* (G+1) */,
                            void* ws, size_t ws_bytes, mpStream_t stream) {
  MP_REQUIRE(M >= 0 && N >= 0 && G >= 0, "mp_angle_list_count_i32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31) && M < (int64_t{1} << 31), "mp_angle_list_count_i32: N, M must fit int32");
  int rc = check_pairing("mp_angle_list_count_i32", pos_fix, pos_ij, 1 - pos_fix);
  if (rc != MP_OK) return rc;
  if (M == 0 || G == 0) return MP_OK;
  MP_REQUIRE(edge_cols && ptr && edge_splits && off && angle_splits && ws,
             "mp_angle_list_count_i32: null pointer");
  size_t need = 0;
  rc = mp_angle_list_workspace_bytes(M, &need);
  if (rc != MP_OK) return rc;
  MP_REQUIRE(ws_bytes >= need, "mp_angle_list_count_i32: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = mp::as_stream(stream);
  const size_t counts_bytes = mp::align256(sizeof(int64_t) * static_cast<size_t>(M + 1));
  int64_t* counts = static_cast<int64_t*>(ws);
  void* temp = static_cast<char*>(ws) + counts_bytes;
  size_t temp_bytes = ws_bytes - counts_bytes;
  MP_HIP(hipMemsetAsync(counts + M, 0, sizeof(int64_t), s));
  const AngleArgs a{edge_cols, edge_cols + M, ptr, perm, M, N, pos_fix, pos_ij, 1 - pos_fix, allow_multi_edges,
                    allow_reverse_edges};
  angle_count_kernel<<<mp::grid_for(M, kGroupsPerBlock), kBlock, 0, s>>>(a, counts);
  MP_HIP(rocprim::exclusive_scan(temp, temp_bytes, counts, off, int64_t{0}, static_cast<size_t>(M + 1),
                                 rocprim::plus<int64_t>(), s, false));
  angle_splits_kernel<<<mp::grid_for(G + 1), 256, 0, s>>>(off, edge_splits, G, M, angle_splits);
  return mp::check_launch("mp_angle_list_count_i32");
}

int mp_angle_list_fill_f32(const int32_t* edge_cols, int64_t M, int64_t N, const int32_t* ptr, const int32_t* perm,
                           const int64_t* node_splits, const int64_t* edge_splits, int64_t G, int pos_fix, int pos_ij,
                           int pos_k, int allow_multi_edges, int allow_reverse_edges, const int64_t* off, int64_t A,
                           const float* xyz, int64_t* triples, int64_t* pairs, int32_t* triple_cols,
                           int32_t* pair_cols, float* theta, const int32_t* edge_ptr0, int32_t* triple_ptr,
                           int32_t* pair_ptr, mpStream_t stream) {
  MP_REQUIRE(M >= 0 && N >= 0 && G >= 0 && A >= 0, "mp_angle_list_fill_f32: bad sizes");
  MP_REQUIRE(N < (int64_t{1} << 31) && M < (int64_t{1} << 31), "mp_angle_list_fill_f32: N, M must fit int32");
  MP_REQUIRE(A < (int64_t{1} << 31), "mp_angle_list_fill_f32: %lld angles do not fit the int32 plan columns",
             (long long)A);
  int rc = check_pairing("mp_angle_list_fill_f32", pos_fix, pos_ij, pos_k);
  if (rc != MP_OK) return rc;
  if (M == 0 || G == 0) return MP_OK;
  MP_REQUIRE(edge_cols && ptr && node_splits && edge_splits && off, "mp_angle_list_fill_f32: null pointer");
  MP_REQUIRE(theta == nullptr || xyz != nullptr, "mp_angle_list_fill_f32: theta requested without coordinates");
  MP_REQUIRE(triple_ptr == nullptr || edge_ptr0 != nullptr,
             "mp_angle_list_fill_f32: triple_ptr requested without the edge list's column-0 CSR");
  hipStream_t s = mp::as_stream(stream);
  if (triple_ptr) angle_csr_kernel<<<mp::grid_for(N + 1), 256, 0, s>>>(off, edge_ptr0, N, M, triple_ptr);
  if (pair_ptr) angle_csr_kernel<<<mp::grid_for(M + 1), 256, 0, s>>>(off, nullptr, M, M, pair_ptr);
  if (A > 0) {
    const AngleArgs a{edge_cols, edge_cols + M, ptr, perm, M, N, pos_fix, pos_ij, pos_k, allow_multi_edges,
                      allow_reverse_edges};
    const AngleOut o{off, node_splits, edge_splits, G, A, xyz, triples, pairs, triple_cols, pair_cols, theta};
    angle_fill_kernel<<<mp::grid_for(M, kGroupsPerBlock), kBlock, 0, s>>>(a, o);
  }
  return mp::check_launch("mp_angle_list_fill_f32");
}

}  // extern "C"
