/*
 * mpengine/index.h - index preparation, CSR offsets, stable segment sort.
 * Defined in csrc/: mp_index.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_INDEX_H
#define MPENGINE_INDEX_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- index ops ------------------------------ */
/* kgcnn/ops/partition.py:97-162 partition_row_indexing (row_splits target, row_splits index):
 * out[e,k] = idx[e,k] + direction * node_splits[graph_of_edge(e)], direction = +1 sample->batch, -1 batch->sample.
 * Bit-exact int64. */
int mp_shift_index_i64(const int64_t* idx, int64_t M, int K, const int64_t* node_splits, const int64_t* edge_splits,
                       int64_t G, int direction, int64_t* out, mpStream_t stream);

/* One pass over the API's (M,K) int64 sample indices that every gather / pooling call of the reference recomputes
 * (partition.py:140-155 + gather.py:228 column pick): writes shifted int32 columns cols[k*M + e], and ORs
 * MP_FLAG_* bits into *flags (caller zeroes it): out-of-range (clamped) and per-column sortedness (K<=2 tracked).
 * N = total node count (node_splits[G]). */
int mp_index_prepare_i64(const int64_t* idx, int64_t M, int K, const int64_t* node_splits, const int64_t* edge_splits,
                         int64_t G, int64_t N, int32_t* cols, int32_t* flags, mpStream_t stream);

/* CSR offsets ptr[0..N] from receiver-sorted segment ids (what tf.math.segment_* derives implicitly). */
int mp_csr_from_sorted_i32(const int32_t* seg, int64_t M, int64_t N, int32_t* ptr, mpStream_t stream);

/* Stable argsort by segment id = tf.argsort(stable=True) of kgcnn/layers/pooling.py:66; ws from mp_sort_workspace_bytes. */
int mp_sort_workspace_bytes(int64_t M, size_t* bytes_out_host);
int mp_sort_segments_i32(const int32_t* seg, int64_t M, int32_t* seg_sorted, int32_t* perm, void* ws, size_t ws_bytes,
                         mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_INDEX_H */
