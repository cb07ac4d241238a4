/*
 * mpengine/segment.h - segment reduce, pooling, segment softmax, relational scatter.
 * Defined in csrc/: mp_segment.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_SEGMENT_H
#define MPENGINE_SEGMENT_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- segment reduce ------------------------- */
/* Sorted segment reduce of kgcnn/layers/pooling.py:63-76 + ops/segment.py:39-46 fused with the has_unconnected
 * zero pad: out[n] = op_{e in [ptr[n], ptr[n+1])} (weight[r] *) data[r], r = perm ? perm[e] : e, accumulated
 * sequentially in edge order (the order tf.math.segment_* uses after the stable sort); empty rows give 0 for
 * every op.  weight (M) nullable multiplies BEFORE the reduce (pooling.py:152); normalize_by_weight divides by
 * sum(weight) with divide_no_nan (pooling.py:164-165).  N_out rows are written. */
int mp_segment_reduce_csr_f32(int op, const float* data, int64_t M, int64_t row_elems, const int32_t* ptr,
                              const int32_t* perm, int64_t N_out, const float* weight, int normalize_by_weight,
                              float* out, mpStream_t stream);

/* GCN aggregation, kgcnn/layers/conv/gcn_conv.py:87-89 in one pass: GatherNodesOutgoing + PoolingWeightedLocalEdges +
 * Activation: out[n] = act( op_{e in segment n} weight[e] * x[send[e]] ); the (M,F) gathered rows never exist
 * (20M + 8NF algorithmic bytes = 125 B/edge at config 5).  send in original edge order, ptr/perm as above. */
int mp_gather_segment_reduce_csr_f32(int op, const float* x, int64_t N, int64_t row_elems, const int32_t* send,
                                     int64_t M, const int32_t* ptr, const int32_t* perm, int64_t N_out,
                                     const float* weight, int normalize_by_weight, int act, float act_alpha, float* out,
                                     mpStream_t stream);

/* PoolingEmbedding / PoolingNodes, kgcnn/layers/pooling.py:215-218: per-graph reduce driven by int64 row_splits
 * (value_rowids never materialised).  Writes G rows (the host trims trailing empty graphs like TF does). */
int mp_pool_graph_f32(int op, const float* x, const int64_t* row_splits, int64_t G, int64_t row_elems,
                      const float* weight, float* out, mpStream_t stream);

/* segment_softmax, kgcnn/ops/segment.py:5-24, on CSR segments: out[r] = exp(a[r]-max_seg)/sum_seg exp(...). */
int mp_segment_softmax_csr_f32(const float* a, int64_t M, int64_t row_elems, const int32_t* ptr, const int32_t* perm,
                               int64_t N, float* out, mpStream_t stream);

/* Reverse rules of the attention pooling (PoolingLocalEdgesAttention, kgcnn/layers/pooling.py:464-546), for training
 * through the layer sequence; what tf.GradientTape derives for kgcnn/ops/segment.py:5-24 and the weighted segment sum.
 * mp_segment_softmax_csr_grad_f32: y = the softmax output (M, row_elems), g its upstream gradient:
 *   out_e = y_e (g_e - sum_{e' in segment of e} y_e' g_e'), the inner sum in list order over [ptr[n], ptr[n+1]) (through
 *   perm if given).  Rows outside every segment are not written.
 * mp_segment_weight_grad_f32: the weight gradient of out[n] = sum_{e: seg_ids[e] = n} w_e data[e]:
 *   out_e = sum_c g[seg_ids[e], c] data[e, c] in column order; g (N, row_elems), data (M, row_elems), seg_ids (M) in
 *   row order; a row whose id lies outside [0, N) gets 0. */
int mp_segment_softmax_csr_grad_f32(const float* y, const float* g, int64_t M, int64_t row_elems, const int32_t* ptr,
                                    const int32_t* perm, int64_t N, float* out, mpStream_t stream);
int mp_segment_weight_grad_f32(const float* g, const float* data, int64_t M, int64_t row_elems, const int32_t* seg_ids,
                               int64_t N, float* out, mpStream_t stream);

/* tensor_scatter_nd_{add,max,min}, kgcnn/ops/scatter.py:18-23 as used by RelationalPoolingLocalEdges
 * (pooling.py:658-666): out (N,R,F) must be zero-initialised by the caller; unsorted atomic scatter. */
int mp_scatter_relational_f32(int op, const float* edges, int64_t M, int64_t row_elems, const int32_t* recv,
                              const int32_t* relation, int64_t N, int64_t R, float* out, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_SEGMENT_H */
