/*
 * mpengine/topk.h - hierarchical pooling: top-k, induced edges, adjacency product.
 * Defined in csrc/: mp_topk.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_TOPK_H
#define MPENGINE_TOPK_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- hierarchical pooling: top-k, induced edges, A.B --- */
/* csrc/mp_topk.hip.  The three layers of kgcnn/layers/pool/topk.py on ragged rows, with no (Nmax, Nmax) and no
 * (M, 2, removed) intermediate.  Every entry that sizes an output by a data-dependent count is a count / fill pair around
 * one int64 prefix sum, with the workspace of mp_topk_workspace_bytes(n), n = the number of counted rows.  Ids are the
 * index plan's shifted, clamped int32 columns; batch_indexing != 0 writes int64 outputs as batch-wide ids, 0 as ids local
 * to the graph (node_indexing "batch" / "sample").  No atomics on data, equal bits on every call.
 *
 * mp_topk_select_f32 (PoolingTopK.call, topk.py:76-116, 178-183): score[i] = sum_c (x[i,c] p[c]) / ||p||; per graph
 *   nremove = rint(k N_g) in float32 (half to even), nkeep = N_g - nremove; new_splits (G+1) is their prefix sum and Nk
 *   must be its last entry (a pure function of the row lengths, computed by the caller on the host).  The rank of node i
 *   is the number of nodes j of its graph with (score_j, j) < (score_i, i): scores compare as floats (-0.0 == 0.0), equal
 *   scores order by ascending index; the nodes of rank >= nremove go to row new_splits[g] + rank - nremove, i.e. in
 *   ascending (score, index).  out (Nk, F) = x[i] sigmoid(score[i]); map_nodes (Nk) the old id (local or batch-wide);
 *   map_global (Nk) the old batch-wide id; old2new (N) the new batch-wide id or -1.  Non-finite scores are not supported
 *   (rows may then be overwritten; nothing is addressed out of range).  Any N_g: a graph's scores stream through LDS.
 * mp_topk_edges_count_i32 / mp_topk_edges_fill_f32 (topk.py:124-165, 184-189): the edges (i, j) with both ends kept,
 *   re-indexed, ordered by new receiver and stable in the old edge order.  ptr0 (N+1) / perm0 (M, nullable) is the old
 *   receiver CSR, send (M) the old sender column.  count: off (Nk+1) first output row of every new receiver,
 *   edge_splits_out (G+1); Mk = off[Nk] = edge_splits_out[G] is read by the caller.  fill: edges_out (Mk, Fe), idx_out
 *   (Mk, 2), map_edges (Mk) old edge position (local or batch-wide), map_edges_global (Mk) the batch-wide one, cols_out (2, Mk) shifted new ids, ptr_out (Nk+1) the
 *   new receiver CSR, edge_old2new (M, nullable) new edge row or -1.
 * mp_adjacency_product_count_f32 / _fill_f32 (AdjacencyPower.call, topk.py:345-386): C = L . R per graph on edge lists,
 *   L[i,j] = valL[e ldL] for the entry e = (i, j) = (row of the CSR ptrL / permL, colL[e]); R likewise; ptrR == null is
 *   R = identity (the thresholding alone).  Kept: the entries C[i,k] > eps (keep_nonzero != 0: the entries != 0, for an
 *   intermediate power), row-major, k ascending.  Duplicate (i, j)
 *   entries in an operand are not supported.  A wave owns a row with an accumulator of MP_TOPK_ACC_FLOATS floats in LDS;
 *   larger graphs run over column ranges, so N_g is not capped.  count: off (N+1), edge_splits_out (G+1).  fill: vals_out
 *   (Mo), idx_out (Mo, 2), cols_out (2, Mo), ptr_out (N+1) - the product's own row CSR, so that it can be the next L.
 * mp_topk_invert_map_i64: old2new (N) = -1, then old2new[old id of map[t]] = t for a (Nk) map of local or batch-wide ids.
 * mp_topk_unpool_f32 (UnPoolingTopK.call, topk.py:274-282): out (N, F) = (skip ? skip : 0) + (old2new[i] >= 0 ?
 *   pooled[old2new[i]] : 0) in one launch; skip (N, F, nullable) is the model's LazyAdd behind the layer. */
#define MP_TOPK_ACC_FLOATS 2048
int mp_topk_workspace_bytes(int64_t n, size_t* bytes_out_host);
int mp_topk_select_f32(const float* x, int64_t N, int64_t F, const float* p, const int64_t* node_splits, int64_t G,
                       float k, int64_t Nk, int batch_indexing, float* score, int64_t* new_splits, float* out,
                       int64_t* map_nodes, int32_t* map_global, int32_t* old2new, void* ws, size_t ws_bytes,
                       mpStream_t stream);
int mp_topk_edges_count_i32(const int32_t* ptr0, const int32_t* perm0, const int32_t* send, int64_t M, int64_t N,
                            const int32_t* map_global, const int32_t* old2new, int64_t Nk, const int64_t* new_node_splits,
                            int64_t G, int64_t* off, int64_t* edge_splits_out, void* ws, size_t ws_bytes,
                            mpStream_t stream);
int mp_topk_edges_fill_f32(const int32_t* ptr0, const int32_t* perm0, const int32_t* send, int64_t M, int64_t N,
                           const int32_t* map_global, const int32_t* old2new, int64_t Nk, const int64_t* new_node_splits,
                           const int64_t* old_edge_splits, int64_t G, const int64_t* off, int64_t Mk, const float* edges,
                           int64_t Fe, int batch_indexing, float* edges_out, int64_t* idx_out, int64_t* map_edges,
                           int32_t* map_edges_global, int32_t* cols_out, int32_t* ptr_out, int32_t* edge_old2new, mpStream_t stream);
int mp_adjacency_product_count_f32(const int32_t* ptrL, const int32_t* permL, const int32_t* colL, const float* valL,
                                   int64_t ldL, int64_t ML, const int32_t* ptrR, const int32_t* permR,
                                   const int32_t* colR, const float* valR, int64_t ldR, int64_t MR, int64_t N,
                                   const int64_t* node_splits, int64_t G, float eps, int keep_nonzero, int64_t* off,
                                   int64_t* edge_splits_out, void* ws, size_t ws_bytes, mpStream_t stream);
int mp_adjacency_product_fill_f32(const int32_t* ptrL, const int32_t* permL, const int32_t* colL, const float* valL,
                                  int64_t ldL, int64_t ML, const int32_t* ptrR, const int32_t* permR,
                                  const int32_t* colR, const float* valR, int64_t ldR, int64_t MR, int64_t N,
                                  const int64_t* node_splits, int64_t G, float eps, int keep_nonzero, const int64_t* off, int64_t Mo,
                                  int batch_indexing, float* vals_out, int64_t* idx_out, int32_t* cols_out,
                                  int32_t* ptr_out, mpStream_t stream);
int mp_topk_invert_map_i64(const int64_t* map, int64_t Nk, const int64_t* new_splits, const int64_t* old_splits, int64_t G,
                           int batch_indexing, int64_t N, int32_t* old2new, mpStream_t stream);
int mp_topk_unpool_f32(const float* pooled, int64_t Nk, int64_t F, const int32_t* old2new, int64_t N, const float* skip,
                       float* out, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_TOPK_H */
