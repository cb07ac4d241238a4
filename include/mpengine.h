/*
 * mpengine.h - C ABI of the MI355X-native message-passing engine (libmpengine.so).
 *
 * Drop-in boundary for the ragged scatter-gather hot path of kgcnn (Tacitus523/gcnn_keras):
 * every entry point replaces a short composition of TensorFlow ops inside one reference function,
 * cited as file:line relative to the reference tree.  The reference has no FFI of its own (it is
 * pure Python on TensorFlow); INTEGRATION.md shows the ctypes binding a maintainer adds to
 * kgcnn/layers/{gather,pooling}.py to route through this library.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (HIP, gfx950) unless the name ends in _host.  Plain pointers and
 *    sizes only; no framework types.  Values are float32 row-major; API indices / row_splits are int64
 *    exactly as the reference's RaggedTensor delivers them (kgcnn/data/utils.py:129-157).
 *  - Index convention: idx[e] = (i, j), column 0 = receiving node i, column 1 = sending node j
 *    (reference README.md:66); indices are per-graph local ("sample" indexing, kgcnn/layers/base.py:42-43).
 *  - Every call is asynchronous on the caller's stream (mpStream_t == hipStream_t), re-entrant, and keeps no
 *    pointer after it returns.  The caller allocates every input, output and workspace buffer.
 *  - Return: MP_OK or a negative status; mp_last_error() gives a thread-local message.  Host code maps
 *    MP_EINVAL -> ValueError/TypeError, MP_EINDEX -> IndexError (TF InvalidArgumentError), MP_EHIP -> RuntimeError.
 *  - Out-of-range indices never fault: they are clamped and recorded in a caller-provided device flag word
 *    (the analogue of ragged_validate / TF-GPU's silent zero fill); the caller decides when to read the flag.
 */
#ifndef MPENGINE_H
#define MPENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mpStream_t; /* hipStream_t */

enum mp_status { MP_OK = 0, MP_EINVAL = -1, MP_EINDEX = -2, MP_EHIP = -3, MP_ENOTSUP = -4 };

/* kgcnn/ops/segment.py:39-46 names -> op */
enum mp_reduce_op { MP_SUM = 0, MP_MEAN = 1, MP_MAX = 2, MP_MIN = 3 };

/* Activations reachable from SchNet / PaiNN / GCN configs (kgcnn/ops/activ.py:6-15, Keras strings) */
enum mp_activation {
  MP_ACT_LINEAR = 0, MP_ACT_RELU = 1, MP_ACT_SHIFTED_SOFTPLUS = 2, MP_ACT_SOFTPLUS = 3, MP_ACT_SWISH = 4,
  MP_ACT_SIGMOID = 5, MP_ACT_TANH = 6, MP_ACT_LEAKY_RELU = 7,
  MP_ACT_SOFTPLUS2 = 8, /* kgcnn/ops/activ.py:19-29: relu(x) + log(0.5 exp(-|x|) + 0.5) */
  MP_ACT_SELU = 9,      /* Keras "selu" (kgcnn/literature/NMPN.py:41): scale * (x > 0 ? x : alpha * (exp(x) - 1)) */
  MP_ACT_ELU = 10,      /* Keras "elu", alpha = 1 (kgcnn/layers/conv/attentivefp_conv.py:38): x > 0 ? x : exp(x) - 1 */
  MP_ACT_LAST = MP_ACT_ELU
};

enum mp_binary_op { MP_ADD = 0, MP_SUB = 1, MP_MUL = 2 };

/* bits of the device flag word written by mp_index_prepare_i64 */
enum mp_index_flag { MP_FLAG_OOB = 1, MP_FLAG_UNSORTED_COL0 = 2, MP_FLAG_UNSORTED_COL1 = 4 };
/* bit of the flag word of mp_scaler_apply: an atomic number inside [0, 95) that the fit did not see */
enum mp_scaler_flag { MP_FLAG_UNKNOWN_SPECIES = 8 };

/* element types of the host packer (mp_pack_*_host) */
enum mp_dtype { MP_DT_F32 = 0, MP_DT_F64 = 1, MP_DT_I32 = 2, MP_DT_I64 = 3 };

/* ---------------------------------------------------------------- runtime -------------------------------- */
const char* mp_last_error(void);
int mp_version(void);
/* Fills name (<= name_len bytes), CU count and LDS bytes per CU of the current HIP device. */
int mp_device_info(char* name_host, int name_len, int* num_cu_host, int* lds_bytes_host);

/* HIP-graph capture of a launch sequence on `stream` (replaces eager per-op dispatch of Keras/TF). */
int mp_graph_begin(mpStream_t stream);
int mp_graph_end(mpStream_t stream, void** graph_exec_out_host);
int mp_graph_launch(void* graph_exec, mpStream_t stream);
int mp_graph_destroy(void* graph_exec);

/* HIP events on the caller's stream, for timing inside bench.py. */
int mp_event_create(void** event_out_host);
int mp_event_record(void* event, mpStream_t stream);
int mp_event_elapsed_ms(void* start, void* stop, float* ms_out_host); /* synchronises on `stop` */
int mp_event_destroy(void* event);

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

/* ---------------------------------------------------------------- gather --------------------------------- */
/* tf.gather(node, idx[:, col], axis=0) of kgcnn/layers/gather.py:83,228 on prepared int32 columns:
 * out[(e*ncols + c)*row_elems + f] = x[cols[colsel[c]*M + e]*row_elems + f]; ncols=2, colsel={0,1} gives the
 * GatherNodes concat layout [x_i || x_j] (gather.py:88-90).  Bit-exact copy. */
int mp_gather_rows_f32(const float* x, int64_t N, int64_t row_elems, const int32_t* cols, int64_t M, int ncols,
                       const int32_t* colsel_host, float* out, mpStream_t stream);

/* Same, straight from the API's int64 sample indices with the shift fused (no prepared columns). */
int mp_gather_rows_i64_f32(const float* x, int64_t N, int64_t row_elems, const int64_t* idx, int64_t M, int K,
                           int col /* -1: all K columns, concat layout */, const int64_t* node_splits,
                           const int64_t* edge_splits, int64_t G, float* out, mpStream_t stream);

/* GatherState, kgcnn/layers/gather.py:363-369: out = repeat(state, row_lengths(splits), axis=0). */
int mp_repeat_rows_f32(const float* state, const int64_t* splits, int64_t G, int64_t row_elems, int64_t N, float* out,
                       mpStream_t stream);

/* Embedding lookup of float node numbers (cast to int32 like Keras Embedding; kgcnn/layers/modules.py:526-528). */
int mp_embedding_f32(const float* table, int64_t vocab, int64_t dim, const float* numbers, int64_t N, float* out,
                     int32_t* flags, mpStream_t stream);

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

/* ---------------------------------------------------------------- dense / elementwise -------------------- */
/* Keras Dense on flat values, kgcnn/layers/modules.py:85: out = act(x @ W + b); x (R,K), W (K,U) row-major
 * ("kernel" layout), b (U) nullable.  FP32 MFMA (v_mfma_f32_32x32x2_f32), k-ordered fma chain. */
int mp_dense_f32(const float* x, int64_t R, int64_t K, const float* W, const float* b, int64_t U, int act,
                 float act_alpha, float* out, mpStream_t stream);

/* Dense with a fused prologue / epilogue, for chains of Dense layers and their reverse pass (PAiNNconv / PAiNNUpdate,
 * kgcnn/layers/conv/painn_conv.py:98-99, 206-207; EnergyForceModel's tape, kgcnn/model/force.py:159-177):
 * in_mode 0: as mp_dense_f32; 1: x := in_act(x) while staging (x is a saved pre-activation); 2: x := x * in_act'(in_pre)
 * (in_pre (R,K): the reverse pass through an activation, fused into the GEMM with the transposed kernel).
 * Epilogue, in this order: out_pre (R,U) nullable receives the pre-activation x W + b; the result act(x W + b) is
 * multiplied by in_act'(grad_pre) if grad_pre (R,U) is given (the activation derivative applied where the upstream
 * gradient is produced); addend (R,U) nullable, may alias out, is added last. */
int mp_dense_ex_f32(const float* x, int64_t R, int64_t K, const float* W, const float* b, int64_t U, int act,
                    float act_alpha, int in_mode, int in_act, float in_alpha, const float* in_pre, const float* addend,
                    float* out_pre, const float* grad_pre, float* out, mpStream_t stream);

/* mp_dense_f32 for few output tiles and a long contraction (GCN's first layer, kgcnn/literature/GCN.py:95:
 * (2708,1433) x (1433,64) = 43 tiles of 64x64 for 256 CUs): the k range is cut into `splits` slices computed by separate
 * workgroups into the workspace (splits * R * U floats), a second kernel adds the slices in order and applies bias and
 * activation - deterministic, no atomics. */
int mp_dense_splitk_workspace_bytes(int64_t R, int64_t U, int splits, size_t* bytes_out_host);
int mp_dense_splitk_f32(const float* x, int64_t R, int64_t K, const float* W, const float* b, int64_t U, int act,
                        float act_alpha, int splits, void* ws, size_t ws_bytes, float* out, mpStream_t stream);

int mp_activation_f32(int act, float act_alpha, const float* x, int64_t n, float* out, mpStream_t stream);
int mp_softmax_rows_f32(const float* x, int64_t R, int64_t C, float* out, mpStream_t stream);
/* ---------------------------------------------------------------- parameter gradients (training) ------- */
/* What the Keras tape computes for the weights under model.fit (kgcnn/layers/modules.py:15-90 Dense, :526-534
 * Embedding; training/train_qm.py:164-166, training/train_citation.py:102-110).  csrc/mp_wgrad.hip.
 *
 * mp_dense_wgrad_f32: dW (K,U) = x^T g and, if db is not NULL, db (U) = sum_r g[r], over the R rows of x (R,K) and
 * g (R,U); FP32 MFMA with the row index as the reduction dimension.  The rows are cut into chunks (a function of R, K, U
 * only) whose partial products land in ws (mp_dense_wgrad_ws_bytes; 0 bytes when one chunk suffices) and are added in
 * chunk order by a second launch: deterministic, no atomics.  R = 0 writes zeros. */
int mp_dense_wgrad_ws_bytes(int64_t R, int64_t K, int64_t U, size_t* bytes_out_host);
int mp_dense_wgrad_f32(const float* x, int64_t R, int64_t K, const float* g, int64_t U, float* dw, float* db, void* ws,
                       size_t ws_bytes, mpStream_t stream);
/* Embedding table gradient: table_grad[t] (vocab,dim) = sum over i with int32(numbers[i]) = t of g[i] (N,dim), added in
 * node order for each t (stable sort by type + CSR + mp_segment_reduce_csr_f32); numbers outside [0, vocab) - zero
 * rows in mp_embedding_f32 - contribute nothing.  N = 0 writes zeros.  ws from mp_embedding_grad_ws_bytes. */
int mp_embedding_grad_ws_bytes(int64_t N, int64_t vocab, size_t* bytes_out_host);
int mp_embedding_grad_f32(const float* numbers, int64_t N, const float* g, int64_t vocab, int64_t dim, void* ws,
                          size_t ws_bytes, float* table_grad, mpStream_t stream);
/* Reverse of mp_softmax_rows_f32 from its output y: out (R,C) = y * (g - rowsum(g * y)). */
int mp_softmax_rows_grad_f32(const float* y, const float* g, int64_t R, int64_t C, float* out, mpStream_t stream);

/* GraphLayerNormalization over the last axis of the values (kgcnn/layers/norm.py:8-110 = Keras LayerNormalization):
 * out = (x - mean_row) * rsqrt(var_row + epsilon) * gamma + beta, biased variance; gamma / beta (C) nullable. */
int mp_layer_norm_f32(const float* x, int64_t R, int64_t C, const float* gamma, const float* beta, float epsilon,
                      float* out, mpStream_t stream);

/* Broadcasting binary op on (R, D1, D2) views: operand strides in elements, 0 = broadcast
 * (LazyAdd/LazySubtract/LazyMultiply of kgcnn/layers/modules.py:187-301, incl. PaiNN's (M,1,F)*(M,3,F)). */
int mp_binary_f32(int op, const float* a, const int64_t* a_strides_host, const float* b, const int64_t* b_strides_host,
                  int64_t R, int64_t D1, int64_t D2, float* out, mpStream_t stream);

/* Strided 2-D column-block copy: dst[r*dst_ld + dst_off + c] = src[r*src_ld + src_off + c], c < C
 * (LazyConcatenate modules.py:305-364 and SplitEmbedding painn_conv.py:329-340 on values). */
int mp_copy_cols_f32(const float* src, int64_t src_ld, int64_t src_off, float* dst, int64_t dst_ld, int64_t dst_off,
                     int64_t R, int64_t C, mpStream_t stream);

/* ---------------------------------------------------------------- geometry ------------------------------- */
/* EuclideanNorm._compute_euclidean_norm, kgcnn/layers/geom.py:181-193 on an (R, D, C) view reducing D:
 * out (R,C) = [1/]sqrt(relu(sum_d x^2) [+eps]). flags: bit0 invert, bit1 add_eps, bit2 no_nan, bit3 square_norm. */
int mp_euclidean_norm_f32(const float* x, int64_t R, int64_t D, int64_t C, int flags, float* out, mpStream_t stream);
/* ScalarProduct, geom.py:261: out (R,C) = sum_d a*b. */
int mp_scalar_product_f32(const float* a, const float* b, int64_t R, int64_t D, int64_t C, float* out,
                          mpStream_t stream);
/* GaussBasisLayer, geom.py:567-571. */
int mp_gauss_basis_f32(const float* d, int64_t M, int bins, float distance, float sigma, float offset, float* out,
                       mpStream_t stream);
/* BesselBasisLayer, geom.py:772-785 (poly envelope, frequencies (num_radial) trainable weight). */
int mp_bessel_basis_f32(const float* d, int64_t M, const float* frequencies, int num_radial, float cutoff,
                        int envelope_exponent, float* out, mpStream_t stream);
/* CosCutOffEnvelope, geom.py:831-837. */
int mp_cos_cutoff_f32(const float* d, int64_t n, float cutoff, float* out, mpStream_t stream);

/* Fused NodePosition -> LazySubtract -> EuclideanNorm (Schnet.py:116-117, PAiNN.py:116-118) on prepared columns:
 * dist (M) = ||x_i - x_j||, dir (M,3) nullable = (x_i-x_j)*divide_no_nan(1, dist). */
int mp_edge_geometry_f32(const float* xyz, int64_t N, const int32_t* recv, const int32_t* send, int64_t M,
                         float* dist, float* dir, mpStream_t stream);

/* ChangeTensorType ragged -> (padded, mask), kgcnn/layers/casting.py:79-84. */
int mp_ragged_to_padded_f32(const float* values, const int64_t* row_splits, int64_t G, int64_t Nmax, int64_t row_elems,
                            float* padded, float* mask, mpStream_t stream);

/* ---------------------------------------------------------------- fused SchNet path --------------------- */
/* mp_index_prepare_i64 for K = 2 fused with NodePosition -> LazySubtract -> EuclideanNorm
 * (kgcnn/literature/Schnet.py:116-117): recv (M), send (M) shifted int32 ids, dist (M) nullable = ||x_i - x_j||,
 * flags as mp_index_prepare_i64 (column 0 sortedness only). */
int mp_edge_prepare_i64_f32(const int64_t* idx, int64_t M, const int64_t* node_splits, const int64_t* edge_splits,
                            int64_t G, int64_t N, const float* xyz, int32_t* recv, int32_t* send, float* dist,
                            int32_t* flags, mpStream_t stream);

/* SchNetCFconv.call, kgcnn/layers/conv/schnet_conv.py:73-79, fused (F = units = 128, cfconv_pool = sum,
 * activation = shifted_softplus): out[i] += sum_{e: recv[e]=i} x[send[e]] * (ssp(rbf[e] W1 + b1) W2 + b2).
 * The filter-MLP weights (Keras layouts W1 (B,128), b1 (128)|NULL, W2 (128,128), b2 (128)|NULL) are packed once
 * per weight update into the kernel's LDS image by mp_cfconv_pack_f32 (mp_cfconv_packed_floats() floats).
 * recv_sorted ascending; perm (nullable) maps sorted position -> original edge (rbf / send are in original
 * order); out (N,128) must be zero on entry.  flags bit0: fast softplus (v_exp/v_log form, |delta| < 2e-7);
 * bit 2 (value 4) / bit 3 (value 8) force the 8-wave / 4-wave workgroup (default: by tile count); bit 4 (value 16,
 * "several forwards in flight"): half as many workgroups, each serving twice the tiles.  Bit 5 needs a workspace (below);
 * these entry points ignore it. */
int mp_cfconv_packed_floats(void);
int mp_cfconv_pack_f32(const float* W1, const float* b1, int B, const float* W2, const float* b2, float* packed,
                       mpStream_t stream);
int mp_cfconv_fused_f32(const float* x, int64_t N, const float* rbf, int B, const float* packed,
                        const int32_t* recv_sorted, const int32_t* send, const int32_t* perm, int64_t M, int flags,
                        float* out_zeroed, mpStream_t stream);
/* Same with GaussBasisLayer (kgcnn/layers/geom.py:567-571) expanded in registers from the edge distance. */
int mp_cfconv_gauss_fused_f32(const float* x, int64_t N, const float* dist, int bins, float distance, float sigma,
                              float offset, const float* packed, const int32_t* recv_sorted, const int32_t* send,
                              const int32_t* perm, int64_t M, int flags, float* out_zeroed, mpStream_t stream);

/* The same two entry points with a caller workspace, which flags bit 5 (value 32) needs: DETERMINISTIC mode.  The partial
 * sums of every tile's first and last segment (the ones that may continue in a neighbouring 32-edge tile) are then not
 * added to `out` with float atomics but parked in the workspace and added per receiver, in edge order, by a second small
 * kernel: bit-identical results from run to run also for receivers with more than 32 incoming edges (the default mode can
 * differ there in the last bit, float atomics arrive in any order).  Costs one extra launch and 1 KB of workspace per tile;
 * without bit 5 the workspace is ignored (NULL allowed). */
int mp_cfconv_det_workspace_bytes(int64_t M, size_t* bytes_out_host);
int mp_cfconv_fused_ws_f32(const float* x, int64_t N, const float* rbf, int B, const float* packed,
                           const int32_t* recv_sorted, const int32_t* send, const int32_t* perm, int64_t M, int flags,
                           float* out_zeroed, void* ws, size_t ws_bytes, mpStream_t stream);
int mp_cfconv_gauss_fused_ws_f32(const float* x, int64_t N, const float* dist, int bins, float distance, float sigma,
                                 float offset, const float* packed, const int32_t* recv_sorted, const int32_t* send,
                                 const int32_t* perm, int64_t M, int flags, float* out_zeroed, void* ws, size_t ws_bytes,
                                 mpStream_t stream);

/* Inference route of the Gauss variant: the filter w(d) = Dense(Dense(gauss(d))) of a block is a function of the block's
 * weights and of the edge distance alone, so it is tabulated once per weight update and the kernel interpolates it
 * (six-point Lagrange on a power-of-two grid; no per-edge MLP).  Row j of the table holds the 128 filter values at the
 * knot v_lo + (j - 2) / inv_h of v = d - offset, evaluated in double precision and rounded to float once; v is clamped
 * to [v_lo, v_end], beyond which the filter is constant to 2.3e-11 of a unit weight.
 *   mp_cfconv_filter_table_layout  host only: domain v_lo = max(-offset, -7 sigma) .. distance (bins-1)/bins + 7 sigma,
 *                                  spacing 2^-log2_inv_h; MP_EINVAL if the table would exceed MP_FILTER_TABLE_MAX_ROWS.
 *   mp_cfconv_filter_table_f32     fills table (layout->rows x 128 floats) and check2: [0] the largest |interpolant -
 *                                  double filter| over the quarter, half and three-quarter points of every interval and
 *                                  four points beyond the ends, the interpolant evaluated with the kernel's arithmetic;
 *                                  [1] the largest |filter| there.  The caller decides from check2 whether to use the table.
 *   mp_cfconv_table_f32            the forward kernel (same tiles, segment rule, flags bits 4 and 5 and workspace as
 *                                  mp_cfconv_gauss_fused_ws_f32); waves per workgroup 4, 8, 16 or 0 = by tile count. */
#define MP_FILTER_TABLE_MAX_ROWS 256
typedef struct mp_filter_table_layout {
  float v_lo, v_end, inv_h;   /* domain of v = d - offset, 1 / spacing (a power of two) */
  int32_t n_int, rows;        /* intervals; rows = n_int + 5, padded to even */
} mp_filter_table_layout;
int mp_cfconv_filter_table_layout(int bins, float distance, float sigma, float offset, int log2_inv_h,
                                  mp_filter_table_layout* layout_out_host);
int mp_cfconv_filter_table_f32(const float* W1, const float* b1, int B, const float* W2, const float* b2, float distance,
                               float sigma, float offset, const mp_filter_table_layout* layout_host, float* table,
                               float* check2, mpStream_t stream);
int mp_cfconv_table_f32(const float* x, int64_t N, const float* dist, float offset, const float* table,
                        const mp_filter_table_layout* layout_host, const int32_t* recv_sorted, const int32_t* send,
                        const int32_t* perm, int64_t M, int flags, int waves, float* out_zeroed, void* ws, size_t ws_bytes,
                        mpStream_t stream);

/* Reverse pass of SchNetCFconv for forces (kgcnn/model/force.py:159-177 through schnet_conv.py:73-79, geom.py:567-571).
 * dE/dx_j is the forward kernel itself with the two index columns swapped (g_out in place of x, the sender-sorted list in
 * place of the receiver-sorted one).  mp_cfconv_gauss_dist_grad_f32 is the other half: per edge (original order)
 *   g_d[e] (+)= sum_h (v_e W2^T)_h * ssp'(g(d_e) W1 + b1)_h * (g'(d_e) W1)_h ,  v_e = g_out[recv[e]] * x[send[e]]
 * with the weights in the image of mp_cfconv_bwd_pack_f32 (mp_cfconv_bwd_packed_floats() floats: W1 | b1 as the forward
 * packs them, W2 re-ordered for the A operand).  Same FP32 MFMA tiles as the forward (three chains per 32-edge tile). */
int mp_cfconv_bwd_packed_floats(void);
int mp_cfconv_bwd_pack_f32(const float* W1, const float* b1, int B, const float* W2, float* packed, mpStream_t stream);
int mp_cfconv_gauss_dist_grad_f32(const float* x, const float* g_out, int64_t N, const float* dist, int bins,
                                  float distance, float sigma, float offset, const float* packed_bwd, const int32_t* recv,
                                  const int32_t* send, int64_t M, int accumulate, float* g_d, mpStream_t stream);

/* Diagnostic build of mp_cfconv_gauss_fused_f32 (20 bins, fast softplus): adds per-phase shader-cycle sums into
 * diag8 (8 x uint64, caller-zeroed): [0] weight staging, [1] tile setup + Gauss basis, [2] GEMM1, [3] softplus +
 * sender-row loads issued, [4] GEMM2, [5] multiply + slab write, [6] slab read, [7] segmented sum + stores/atomics.
 * Shares only: the stamps fence the schedule. */
int mp_cfconv_gauss_diag_f32(const float* x, int64_t N, const float* dist, int bins, float distance, float sigma,
                             float offset, const float* packed, const int32_t* recv_sorted, const int32_t* send,
                             const int32_t* perm, int64_t M, float* out_zeroed, unsigned long long* diag8,
                             mpStream_t stream);

/* ---------------------------------------------------------------- recurrent / edge-network pieces -------- */
/* One Keras LSTM step from the zero state, as PoolingSet2Set runs it (kgcnn/layers/pool/set2set.py:190: a stateless LSTM
 * layer called on a length-1 sequence): z (R,4U) = x kernel + bias in Keras gate order [i | f | c | o];
 * out (R,U) = rec(z_o) * act(rec(z_i) * act(z_c))  (h0 = c0 = 0: the forget gate and the recurrent kernel drop out). */
int mp_lstm_zero_state_f32(const float* z, int64_t R, int64_t U, int act, int rec_act, float* out, mpStream_t stream);
/* Keras GRUCell combine, reset_after = True (kgcnn/layers/conv/mpnn_conv.py:193 GRUUpdate): mx (R,3U) = x kernel + b_in,
 * mh (R,3U) = h recurrent_kernel + b_rec, gate order [z | r | h]:
 * zg = rec(mx_z + mh_z), rg = rec(mx_r + mh_r), hh = act(mx_h + rg * mh_h), out = zg * h + (1 - zg) * hh. */
int mp_gru_combine_f32(const float* mx, const float* mh, const float* h, int64_t R, int64_t U, int act, int rec_act,
                       float* out, mpStream_t stream);
/* Reverse of mp_gru_combine_f32 for the upstream gradient g (R,U): d_mx (R,3U), d_mh (R,3U) and d_h (R,U), each
 * nullable (at least one given).  The gates are recomputed from mx, mh and h in the forward's order; elementwise, no
 * reduction: equal bits on every run. */
int mp_gru_combine_grad_f32(const float* mx, const float* mh, const float* h, const float* g, int64_t R, int64_t U,
                            int act, int rec_act, float* d_mx, float* d_mh, float* d_h, mpStream_t stream);
/* MatMulMessages, kgcnn/layers/conv/mpnn_conv.py:111 (tf.keras.backend.batch_dot): out[m] = mat[m] (Ro,C) . vec[m] (C). */
int mp_batched_matvec_f32(const float* mat, const float* vec, int64_t M, int64_t Ro, int64_t C, float* out,
                          mpStream_t stream);

/* ---------------------------------------------------------------- fused PaiNN path (+ reverse pass) ------ */
/* Stage 0 of kgcnn/literature/PAiNN.py:100-119 in one launch: OptionalInputEmbedding (z0 (N,128)), EquivariantInitialize
 * with a constant (v0 (N,3,128) = v_init), mp_index_prepare_i64 for K = 2 (recv, send, flag word incl. both sortedness
 * bits), NodePosition -> EdgeDirectionNormalized (rij (M,3), geom.py:331-378) -> NodeDistanceEuclidean (dist (M)) ->
 * BesselBasisLayer (rbf (M,B), geom.py:772-785) and, if rbfd != NULL, d rbf / d dist (M,B) for the reverse pass;
 * cos_cutoff > 0 adds CosCutOffEnvelope (env (M), geom.py:831-837) and its derivative envd (nullable). */
int mp_painn_stage0_f32(const void* numbers /* float32, or int64 if numbers_i64 */, int numbers_i64, int64_t N,
                        const float* emb, int vocab, float v_init, float* z0, float* v0,
                        const int64_t* idx, int64_t M, const int64_t* node_splits, const int64_t* edge_splits, int64_t G,
                        const float* xyz, const float* frequencies, int num_radial, float bessel_cutoff,
                        int envelope_exponent, float cos_cutoff, int32_t* recv, int32_t* send, int32_t* flags, float* dist,
                        float* rij, float* rbf, float* rbfd, float* env, float* envd, mpStream_t stream);
/* PAiNNconv.call edge side, kgcnn/layers/conv/painn_conv.py:99-113, fused (F = units = 128, conv_pool = sum):
 * w = rbf Ww + bw [* env]; sw = s[send] * w; ds[i] = sum sw1; dv[i] = sum (sw2 (x) v[send] + sw3 (x) r_ij) over the edges
 * of receiver i in edge order (CSR ptr / perm as mp_segment_reduce_csr_f32).  s (N,3F) = phi(dense1(z)), v (N,3,F),
 * rbf (M,B<=32), env (M)|NULL, rij (M,3), Ww (B,3F), bw (3F)|NULL; writes ds (N,F), dv (N,3,F) incl. zero rows.
 * z_in != NULL fuses the residual adds of PAiNN.py:126-127: ds := z_in + ds, dv := v + dv.  dv must not alias v.
 * Two waves per receiver, four edges in flight per wave, packed FP32 arithmetic. */
int mp_painn_message_f32(const float* s, const float* v, int64_t N, const float* rbf, int B, const float* env,
                         const float* rij, const float* Ww, const float* bw, const int32_t* ptr, const int32_t* perm,
                         const int32_t* send, int64_t M, const float* z_in, float* ds, float* dv, mpStream_t stream);
/* The same message step with node TILES staged in LDS and the filter Dense (painn_conv.py:100, w = Dense(3F)(rbf)) on the
 * matrix pipe (FP32-exact bf16-piece split, csrc/mp_painn_fused.hip): for receiver-sorted edge lists (no perm) of batched
 * graphs.  tiles (T,8) int32 = {r_lo, r_hi, s_lo, s_hi, e_lo, e_hi, 0, 0}: receivers [r_lo, r_hi) (at most 62) of ONE graph
 * whose nodes are [s_lo, s_hi) (<= max_rows: the s / v rows staged) and whose edges are [e_lo, e_hi) = [ptr[r_lo],
 * ptr[r_hi]) (<= max_edges); every receiver must appear in exactly one tile.  wimage: mp_painn_filter_pack_f32 of Ww | bw
 * (MP_PAINN_FILTER_IMAGE_BYTES, rebuilt when the weights change).  LDS per workgroup: mp_painn_message_tiles_lds_bytes
 * (<= 160 KB, else MP_EINVAL).  Results as mp_painn_message_f32 (same accumulation order per receiver). */
#define MP_PAINN_FILTER_IMAGE_BYTES 73728
int mp_painn_filter_pack_f32(const float* Ww, const float* bw, int B, void* image, mpStream_t stream);
int mp_painn_message_tiles_lds_bytes(int max_rows, int max_edges, int B, int with_env, size_t* out);
int mp_painn_message_tiles_f32(const float* s, const float* v, int64_t N, const float* rbf, int B, const float* env,
                               const float* rij, const void* wimage, const int32_t* ptr, const int32_t* send, int64_t M,
                               const int32_t* tiles, int ntiles, int max_rows, int max_edges, const float* z_in, float* ds,
                               float* dv, mpStream_t stream);
/* Reverse pass of the message block (painn_conv.py:99-113) for forces: sender-parallel over the CSR of column 1
 * (ptr1 / perm1).  Given g_ds (N,F) and g_dv (N,3,F): g_s (N,3F) = dE/ds, g_v (N,3,F) = g_dv + dE/dv through the
 * messages (nullable), and per edge dE/dd (through the filter: rbfd = d rbf / d d, envelope by the product rule) and
 * dE/dr_ij, written (accumulate = 0) or added (accumulate = 1, later blocks) to g_d (2,M), g_rij (2,M,3): one slice per
 * half of the feature axis (two waves serve a sender), summed by mp_edge_geometry_bwd_f32 (slices = 2). */
int mp_painn_message_bwd_f32(const float* s, const float* v, int64_t N, const float* rbf, const float* rbfd, int B,
                             const float* env, const float* envd, const float* rij, const float* Ww, const float* bw,
                             const int32_t* ptr1, const int32_t* perm1, const int32_t* recv, int64_t M, const float* g_ds,
                             const float* g_dv, float* g_s, float* g_v, float* g_d, float* g_rij, int accumulate,
                             mpStream_t stream);
/* The same reverse step on SENDER tiles staged in LDS with the filter AND its distance derivative on the matrix pipe (A rows
 * [rbf_e | 1] and [rbf'_e | 0] against the forward kernel's packed image `wimage`): any edge order (the tile's basis rows are
 * gathered through perm1), batched graphs.  tiles (T,8) int32 = {j_lo, j_hi, s_lo, s_hi, e_lo, e_hi, 0, 0}: senders
 * [j_lo, j_hi) (at most max_senders <= 62: their s / v rows are staged too) of ONE graph whose nodes are [s_lo, s_hi)
 * (<= max_rows: the g_ds / g_dv rows staged) and whose
 * edges are the sender-order positions [e_lo, e_hi) = [ptr1[j_lo], ptr1[j_hi]) (<= max_edges); every sender in exactly one
 * tile.  g_d (M), g_rij (M,3): ONE slice (mp_edge_geometry_bwd_f32 with slices = 1), summed over the feature axis in a
 * fixed order inside the kernel.  LDS per workgroup: mp_painn_message_bwd_tiles_lds_bytes (<= 160 KB, else MP_EINVAL). */
int mp_painn_message_bwd_tiles_lds_bytes(int max_rows, int max_senders, int max_edges, int B, int with_env, size_t* out);
int mp_painn_message_bwd_tiles_f32(const float* s, const float* v, int64_t N, const float* rbf, const float* rbfd, int B,
                                   const float* env, const float* envd, const float* rij, const void* wimage,
                                   const int32_t* ptr1, const int32_t* perm1, const int32_t* recv, int64_t M,
                                   const int32_t* tiles, int ntiles, int max_rows, int max_senders, int max_edges,
                                   const float* g_ds, const float* g_dv, float* g_s, float* g_v, float* g_d, float* g_rij,
                                   int accumulate, mpStream_t stream);
/* PAiNNUpdate.call (painn_conv.py:201-214) after the projection uv (3N,2F) = v [Wu | Wv] (rows (n,k)) in ONE launch
 * (csrc/mp_chain.hip): the element-wise steps
 *   pre:  c (N,2F) = [z | EuclideanNorm_k(v_v)], prod (N,F) = ScalarProduct_k(v_u, v_v);
 *   post: z2 = z + prod a_sv + a_ss, v2 = v + a_vv (x) v_u  with a (N,3F) = [a_vv | a_sv | a_ss] (+ PAiNN.py:131-132)
 * as prologue / epilogue of the two-layer chain a = Dense(Dense(c, act)) (W1 (256,128), W2 (128,384) as mp_chain_pack_f32
 * images).  save_pre keeps c Wd + bd; c_out / prod_out / a_out (any may be NULL) receive what the reverse pass reads. */
int mp_painn_update_fused_f32(const float* z, const float* v, const float* uv, int64_t N, const float* W1_packed,
                              const float* b1, int act1, float alpha1, float* save_pre, const float* W2_packed,
                              const float* b2, float* c_out, float* prod_out, float* a_out, float* z2, float* v2,
                              mpStream_t stream);
/* ... and its reverse in one launch: g_a (N,3F), g_prod (N,F) from g_z2, g_v2 (reverse of post) as the prologue,
 * g_z = g_z2 + g_c[:, :F] and g_uv (3N,2F) (reverse of pre) as the epilogue of the chain against the transposed
 * kernels (W1T (384,128) = Wa^T, W2T (128,256) = Wd^T as mp_chain_pack_f32 images; grad_pre = the saved c Wd + bd).
 * g_v2 == NULL: no gradient reaches v'' (the last block of an energy model, whose readout sees z only). */
int mp_painn_update_fused_bwd_f32(const float* g_z2, const float* g_v2, const float* uv, const float* prod, const float* a,
                                  const float* c, int64_t N, const float* W1T_packed, int act1, float alpha1,
                                  const float* grad_pre, const float* W2T_packed, float* g_z, float* g_uv,
                                  mpStream_t stream);
/* Reverse of NodePosition -> EdgeDirectionNormalized / NodeDistanceEuclidean (PAiNN.py:116-118; Schnet.py:116-117 with
 * g_rij = 0): g_xyz[n] = scale * (sum_{recv(e)=n} t_e - sum_{send(e)=n} t_e), t_e = g_d r_ij + (g_rij - (g_rij.r_ij) r_ij)/d,
 * g_d (slices,M) and g_rij (slices,M,3) being partial sums that are added first,
 * over the receiver CSR (ptr0/perm0) and the sender CSR (ptr1/perm1); scale = -1 yields the physical force
 * (kgcnn/model/force.py:188-189). */
int mp_edge_geometry_bwd_f32(const float* g_d, const float* g_rij, int slices, const float* rij, const float* dist,
                             const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                             int64_t N, int64_t M, float scale, float* g_xyz, mpStream_t stream);

/* Node-side chains of kgcnn/literature/Schnet.py:110-133 / schnet_conv.py:159-165 (F = 128, embedding width 64):
 * node_in:     n = Embedding(Z) W0 + b0 ; x = n Wx
 * node_update: n += ssp(agg W2 + b2) W3 + b3 ; x = n Wx_next ; agg := 0
 * node_last:   n' = n + ssp(agg W2 + b2) W3 + b3 ; h = ssp(ssp(n' Wl0 + bl0) Wl1 + bl1) (N,64) ; agg := 0
 * readout:     out[g] = ssp(sum_{nodes of g} h W_o0 + b_o0) W_o1 + b_o1   (PoolingNodes(sum) + MLP([64,1]));
 *              W_o0 == NULL: out[g] = sum_{nodes of g} (h W_o1 + b_o1)  (last_mlp ending in Dense(1, linear), then
 *              PoolingNodes(sum), use_output_mlp=False: the fork's force_schnet.py configuration)
 * The embedding width is 64 or 128; flags bit 8 (256): `numbers` holds int64 node numbers (the fork's scripts declare
 * int64 inputs) instead of float32.
 * flags bit0: fast softplus as in mp_cfconv_fused_f32; bit1: every weight-matrix pointer is an
 * mp_schnet_node_pack_f32 image of the Keras kernel instead of the kernel itself (biases stay plain): the image stores,
 * per wave and lane, the registers of four consecutive k-steps as one float4, so a workgroup loads its weight slices
 * with 16-B instead of strided 4-B reads.  mp_schnet_node_in_f32, mp_schnet_stage0_f32, mp_schnet_node_update_f32 and
 * mp_schnet_node_last_f32 (and their _save_ forms) are built for images only: they REQUIRE bit 1 and return MP_EINVAL
 * without it, before any device work.  mp_schnet_node_residual_f32 alone reads the Keras kernels themselves. */
int mp_schnet_node_pack_f32(const float* W, int K, int U, float* packed /* K*U floats */, mpStream_t stream);
/* The same slice order with every element as three bf16 pieces (hi + mid + lo = the FP32 value exactly): flags bit 6
 * (value 64) makes the node kernels of the FORWARD run their GEMMs on the bf16 matrix pipe as an exact
 * FP32 emulation (six products per k block, FP32 accumulate: the error of the FP32 matrix instructions at 2.67x their
 * rate).  K % 32 == 0; the image holds K*U*3/2 floats.
 * flags bit 9 (value 512, bf16-piece build): "several launch sequences share the GPU" - a launch with 256 or more 16-node
 * tiles runs on half the CUs (128 persistent workgroups), leaving the others to the kernels of the other sequences. */
int mp_schnet_node_pack_bf16_f32(const float* W, int K, int U, float* packed /* K*U*3/2 floats */, mpStream_t stream);
/* SchNetInteraction.call's node side alone (schnet_conv.py:162-164), out of place, for the layer API:
 * n_out = n_in + Dense(lin)(Dense(ssp)(agg)); agg is left untouched. */
int mp_schnet_node_residual_f32(const float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                                const float* b3, const float* n_in, float* n_out, int flags, mpStream_t stream);
int mp_schnet_node_in_f32(const float* numbers, int64_t N, const float* emb, int vocab, int emb_dim, const float* W0,
                          const float* b0, const float* Wx, float* n_out, float* x_out, int flags, mpStream_t stream);
/* mp_schnet_node_in_f32 and mp_edge_prepare_i64_f32 in ONE launch (disjoint workgroups): they are independent and at
 * QM9 batch sizes each alone occupies less than half of the chip; falls back to the two launches for large batches. */
int mp_schnet_stage0_f32(const float* numbers, int64_t N, const float* emb, int vocab, int emb_dim, const float* W0,
                         const float* b0, const float* Wx, float* n_out, float* x_out, const int64_t* idx, int64_t M,
                         const int64_t* node_splits, const int64_t* edge_splits, int64_t G, const float* xyz,
                         int32_t* recv, int32_t* send, float* dist, int32_t* flags, int flags_arg, mpStream_t stream);
/* The node-input chain as a table: n and x of mp_schnet_node_in_f32 are functions of the node number alone, so the chain
 * runs once per weight update on the numbers 0 .. vocab-1, -1 (same build: flags bits 0, 1 - required -, 6 as the forward)
 * and fills n_table / x_table, (vocab + 1, 128) each: row r < vocab = the chain's rows for a node with number r, row
 * vocab = its rows for a number outside 0 .. vocab-1 (zero embedding row: b0 resp. b0 Wx).  Bit-identical to the chain by
 * construction.  numbers_ws: (vocab + 1) floats of scratch.  vocab + 1 <= MP_SCHNET_TABLE_MAX_ROWS (both tables: 2 MB, half
 * of one XCD's L2); larger vocabularies keep the chain. */
#define MP_SCHNET_TABLE_MAX_ROWS 2048
int mp_schnet_embed_table_f32(const float* emb, int vocab, int emb_dim, const float* W0, const float* b0,
                              const float* Wx, float* numbers_ws, float* n_table, float* x_table, int flags,
                              mpStream_t stream);
/* mp_schnet_node_in_f32 / mp_schnet_stage0_f32 with the chain replaced by a row gather from the tables: per node the number
 * is read (float32, or int64 with flags bit 8; cast and range rule of the chain) and row r of n_table / x_table is copied
 * to n_out / x_out.  No LDS, no barrier, 256-thread workgroups.  The stage-0 form runs the edge preparation on further
 * workgroups of the same launch (at most 128) and falls back to two launches for large batches as mp_schnet_stage0_f32 does. */
int mp_schnet_node_in_table_f32(const float* numbers, int64_t N, int vocab, const float* n_table, const float* x_table,
                                float* n_out, float* x_out, int flags, mpStream_t stream);
int mp_schnet_stage0_table_f32(const float* numbers, int64_t N, int vocab, const float* n_table, const float* x_table,
                               float* n_out, float* x_out, const int64_t* idx, int64_t M, const int64_t* node_splits,
                               const int64_t* edge_splits, int64_t G, const float* xyz, int32_t* recv, int32_t* send,
                               float* dist, int32_t* flags, int flags_arg, mpStream_t stream);
int mp_schnet_node_update_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                              const float* b3, float* n_inout, const float* Wx_next, float* x_out, int flags,
                              mpStream_t stream);
int mp_schnet_node_last_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3, const float* b3,
                            const float* n_in, const float* Wl0, const float* bl0, const float* Wl1, const float* bl1,
                            float* h_out, int flags, mpStream_t stream);
int mp_schnet_readout_f32(const float* h, const int64_t* node_splits, int64_t G, const float* Wo0, const float* bo0,
                          const float* Wo1, const float* bo1, float* out, mpStream_t stream);

/* ---------------------------------------------------------------- on-GPU SetRange (next: SURVEY 8f.2) ---- */
/* SetRange.call, kgcnn/graph/preprocessor.py:288-314 via define_adjacency_from_distance (kgcnn/graph/adj.py:537-593),
 * exclusive mode, no self loops, for a whole ragged batch of coordinates xyz (N,3): pass 1 counts the edges of every
 * receiving atom and scans them (node_ptr (N+1) int32 = receiver CSR, edge_splits (G+1) int64); the caller reads
 * M = node_ptr[N] to size the outputs; pass 2 writes the (M,2) int64 sample indices in row-major (i,j) order and,
 * optionally, int32 receiver / sender ids and the edge distances (range_attributes).  max_distance < 0 or
 * max_neighbours < 0 disables that criterion. */
int mp_radius_graph_workspace_bytes(int64_t N, size_t* bytes_out_host);
int mp_radius_graph_count_f32(const float* xyz, const int64_t* node_splits, int64_t G, int64_t N, float max_distance,
                              int max_neighbours, int32_t* node_ptr, int64_t* edge_splits, void* ws, size_t ws_bytes,
                              mpStream_t stream);
int mp_radius_graph_fill_f32(const float* xyz, const int64_t* node_splits, int64_t G, int64_t N, float max_distance,
                             int max_neighbours, const int32_t* node_ptr, int64_t M, int64_t* idx_out, int32_t* recv,
                             int32_t* send, float* dist, mpStream_t stream);

/* ---------------------------------------------------------------- on-GPU SetAngle ------------------------ */
/* SetAngle.call, kgcnn/graph/preprocessor.py:354-368 via get_angle_indices / get_angle (kgcnn/graph/adj.py:300-415),
 * allow_self_edges=False, for a whole ragged batch of edge lists.  edge_cols (2,M): the shifted, clamped int32 columns
 * of the edge list's index plan; ptr (N+1) / perm (M, or NULL when the column is sorted): the plan's CSR over column
 * pos_fix.  pos_k is the position of k in edge_pairing, pos_fix the other one, pos_ij = 0 if the pairing names i,
 * else 1.  Partners of edge n = (i, j): the edges m != n with idx[m, pos_fix] == idx[n, pos_ij], without those equal to
 * (i, j) / (j, i) unless allow_multi_edges / allow_reverse_edges.  Order: by n, then m ascending.
 * Pass 1 counts the partners of every edge and scans them in int64: off (M+1) = first output row of every edge,
 * angle_splits (G+1) int64; the caller reads A = off[M] to size the outputs.  Pass 2 writes, each pointer nullable:
 * triples (A,3) int64 node ids (i, j, k) local to the graph, pairs (A,2) int64 edge ids (n, m) local to the graph's
 * edge list, triple_cols (3,A) / pair_cols (2,A) int32 shifted ids (the index-plan columns of the triples against the
 * node partition and of the pairs against the edge partition), theta (A) = atan2(|v1 x v2|, v1 . v2) with
 * v1 = x_i - x_j, v2 = x_j - x_k, and the column-0 CSRs triple_ptr (N+1; needs edge_ptr0, the edge list's column-0
 * CSR, and is meaningful when that column is sorted) and pair_ptr (M+1).  A >= 2^31 is MP_EINVAL.  M == 0 or G == 0
 * returns MP_OK without touching the device. */
int mp_angle_list_workspace_bytes(int64_t M, size_t* bytes_out_host);
int mp_angle_list_count_i32(const int32_t* edge_cols, int64_t M, int64_t N, const int32_t* ptr, const int32_t* perm,
                            const int64_t* edge_splits, int64_t G, int pos_fix, int pos_ij, int allow_multi_edges,
                            int allow_reverse_edges, int64_t* off, int64_t* angle_splits, void* ws, size_t ws_bytes,
                            mpStream_t stream);
int mp_angle_list_fill_f32(const int32_t* edge_cols, int64_t M, int64_t N, const int32_t* ptr, const int32_t* perm,
                           const int64_t* node_splits, const int64_t* edge_splits, int64_t G, int pos_fix, int pos_ij,
                           int pos_k, int allow_multi_edges, int allow_reverse_edges, const int64_t* off, int64_t A,
                           const float* xyz, int64_t* triples, int64_t* pairs, int32_t* triple_cols,
                           int32_t* pair_cols, float* theta, const int32_t* edge_ptr0, int32_t* triple_ptr,
                           int32_t* pair_ptr, mpStream_t stream);

/* ---------------------------------------------------------------- periodic cells ------------------------- */
/* ShiftPeriodicLattice.call, kgcnn/layers/geom.py:100-123: out[e] = pos[e] + ((n0 a0 + n1 a1) + n2 a2) with
 * n = image[e] (M,3) int64 and a_k the rows of lattice[g(e)] (G,3,3), g(e) from the edge row_splits (G+1); the
 * reference's reduce_sum order, no contraction.  M == 0 returns MP_OK without touching the device.
 *
 * SetRangePeriodic.call, kgcnn/graph/preprocessor.py:413-441 via range_neighbour_lattice (kgcnn/graph/geom.py:172-368),
 * exclusive mode, no self loops, for a ragged batch of coordinates xyz (N,3) with one cell lattice (G,3,3) per graph
 * (lattice vectors in rows).  Receiver i is connected to every (sender j, image n) with |(x_j + n L) - x_i| <=
 * max_distance in float32 (the shift as above), except (j = i, n = 0); per receiver in the order (distance, sender,
 * image lexicographic), cut after max_neighbours (< 0: no cut); receivers in node order.  Pass 1 writes node_ptr (N+1)
 * int32 = receiver CSR, edge_splits (G+1) int64 and the flag word (zeroed first, then mp_periodic_flag bits; a receiver
 * that raised one counts no edge); the caller reads M = node_ptr[N] and the flag word to size the outputs.  Pass 2
 * writes the (M,2) int64 sample indices (i, j), the (M,3) int64 images and, each nullable, the int32 receiver / sender
 * ids and the distances (range_attributes).  max_distance must be finite and >= 0.  As in mp_radius_graph_*, node_ptr is
 * int32: the caller keeps N x degree below 2^31 (2^31 edges are 50 GB of outputs). */
#define MP_PERIODIC_MAX_HITS 1024           /* neighbours inside the cutoff per receiver, before the max_neighbours cut */
#define MP_PERIODIC_MAX_IMAGE 511           /* |n_k| of an image index */
#define MP_PERIODIC_MAX_CANDIDATES 1048576  /* (sender, image) candidates of the image boxes per receiver */
enum mp_periodic_flag { MP_PERIODIC_FLAG_CAPACITY = 1, MP_PERIODIC_FLAG_IMAGE_RANGE = 2, MP_PERIODIC_FLAG_SINGULAR = 4 };
int mp_lattice_shift_f32(const float* pos, const int64_t* image, const float* lattice, const int64_t* edge_splits,
                         int64_t G, int64_t M, float* out, mpStream_t stream);
int mp_radius_graph_periodic_workspace_bytes(int64_t N, size_t* bytes_out_host);
int mp_radius_graph_periodic_count_f32(const float* xyz, const int64_t* node_splits, const float* lattice, int64_t G,
                                       int64_t N, float max_distance, int max_neighbours, int32_t* node_ptr,
                                       int64_t* edge_splits, int32_t* flags, void* ws, size_t ws_bytes,
                                       mpStream_t stream);
int mp_radius_graph_periodic_fill_f32(const float* xyz, const int64_t* node_splits, const float* lattice, int64_t G,
                                      int64_t N, float max_distance, int max_neighbours, const int32_t* node_ptr,
                                      int64_t M, int64_t* idx_out, int64_t* image_out, int32_t* recv, int32_t* send,
                                      float* dist, mpStream_t stream);

/* ---------------------------------------------------------------- backward helpers (forces) -------------- */
/* EnergyForceModel, kgcnn/model/force.py:159-186: F = -dE/dx needs one reverse pass.  Gather-backward is
 * mp_segment_reduce_csr_f32 over the CSR of the gathered column, segment-sum-backward is mp_gather_rows_f32 by the
 * receiver ids, Dense-backward is mp_dense_f32 with the transposed kernel; these are the remaining derivatives. */
int mp_activation_grad_f32(int act, float act_alpha, const float* pre, const float* gy, int64_t n, float* out,
                           mpStream_t stream);                       /* out = gy * act'(pre) */
int mp_sum_axis_f32(const float* x, int64_t R, int64_t D1, int64_t D2, int axis /* 1 or 2 */, float* out,
                    mpStream_t stream);                              /* un-broadcast of mp_binary_f32 operands */
int mp_euclidean_norm_grad_f32(const float* x, const float* gy, int64_t R, int64_t D, int64_t C, int flags, float* gx,
                               mpStream_t stream);                   /* geom.py:181-193 */
int mp_bessel_basis_grad_f32(const float* d, int64_t M, const float* frequencies, int num_radial, float cutoff,
                             int envelope_exponent, const float* gy, float* gd, mpStream_t stream); /* geom.py:772-785 */
int mp_gauss_basis_grad_f32(const float* d, int64_t M, int bins, float distance, float sigma, float offset,
                            const float* gy, float* gd, mpStream_t stream);                         /* geom.py:567-571 */
int mp_cos_cutoff_grad_f32(const float* d, int64_t n, float cutoff, const float* gy, float* gd, mpStream_t stream);

/* ---------------------------------------------------------------- second derivatives (training on forces) - */
/* A loss on F = -dE/dx (the fork's force_schnet.py:163-205, kgcnn/model/force.py:159-186 under model.fit) runs the
 * reverse pass a second time, backwards.  The linear steps of the first-order pass reverse into forward kernels (gather
 * <-> segment sum, Dense GEMM <-> wgrad); these reverse the elementwise derivatives above (csrc/mp_backward2.hip).
 * For y = gy * f'(x) and an upstream h on y: gy_bar = h f'(x), x_bar = h gy f''(x).  Either output may be NULL.
 *
 * mp_activation_grad2_f32: reverse of mp_activation_grad_f32 (modules.py:15-90, activ.py:15), every act code.
 * mp_gauss_basis_grad2_f32: reverse of mp_gauss_basis_grad_f32 (geom.py:567-571); gy, gy_bar are (M, bins), d, h,
 *   d_bar (M).  d_bar = h sum_k gy_k phi_k''(d), phi'' = (4 gamma^2 u^2 - 2 gamma) phi; gy_bar_k = h phi_k'(d).
 * mp_euclidean_norm_grad2_f32: reverse of mp_euclidean_norm_grad_f32 (geom.py:181-193) on the same (R, D, C) view for
 *   the plain norm f = sqrt(s) (flags: add_eps 2, no_nan 4; invert / square_norm return MP_EINVAL): gy_bar (R, C) =
 *   (h . x) / f, x_bar = gy (h / f - (h . x) x / f^3); zero where s <= 0 (the first-order zero sub-gradient). */
int mp_activation_grad2_f32(int act, float act_alpha, const float* pre, const float* gy, const float* h,
                            float* pre_bar, float* gy_bar, int64_t n, mpStream_t stream);
int mp_gauss_basis_grad2_f32(const float* d, int64_t M, int bins, float distance, float sigma, float offset,
                             const float* gy, const float* h, float* d_bar, float* gy_bar, mpStream_t stream);
int mp_euclidean_norm_grad2_f32(const float* x, const float* gy, const float* h, int64_t R, int64_t D, int64_t C,
                                int flags, float* x_bar, float* gy_bar, mpStream_t stream);

/* The whole fused forward (kgcnn/literature/Schnet.py:104-148 with receiver-sorted edges) as ONE call: stage 0,
 * depth x (cfconv + node update), last node chain, readout, launched in sequence on `stream` from a descriptor of the
 * bound batch slot.  Equivalent to replaying a captured HIP graph of the same eight launches, without the capture:
 * the entry for batches whose shapes change from call to call.  flags: bit0 fast softplus, bit1 node-side
 * weight pointers (W0, Wx, W2, W3, Wl0, Wl1) are mp_schnet_node_pack_f32 images, bits 2-4 as mp_cfconv_fused_f32. */
#define MP_SCHNET_MAX_DEPTH 8
typedef struct mp_schnet_forward_desc {
  int64_t N, M, G;
  int32_t depth, vocab, flags, bins;
  float g_distance, g_sigma, g_offset;
  int32_t emb_dim;                 /* embedding width: 64 (0 = 64) or 128 */
  const float* numbers;            /* (N) node numbers: float32, or int64 with flags bit 8 */
  const float* xyz;                /* (N,3) */
  const int64_t* idx;              /* (M,2) sample indices */
  const int64_t* node_splits;      /* (G+1) */
  const int64_t* edge_splits;      /* (G+1) */
  const float* embedding;          /* (vocab,64) */
  const float* W0;                 /* (64,128) */
  const float* b0;
  const float* Wx[MP_SCHNET_MAX_DEPTH];      /* interaction i: dense1 (128,128), no bias */
  const float* packed[MP_SCHNET_MAX_DEPTH];  /* interaction i: mp_cfconv_pack_f32 image */
  const float* W2[MP_SCHNET_MAX_DEPTH];
  const float* b2[MP_SCHNET_MAX_DEPTH];
  const float* W3[MP_SCHNET_MAX_DEPTH];
  const float* b3[MP_SCHNET_MAX_DEPTH];
  const float* Wl0; const float* bl0; const float* Wl1; const float* bl1;   /* last_mlp */
  const float* Wo0; const float* bo0; const float* Wo1; const float* bo1;   /* output_mlp; Wo0 == NULL: linear head Wo1 */
  int32_t* recv; int32_t* send; float* dist; int32_t* flags_word;           /* (M) work buffers, flag word */
  float* n; float* x; float* agg; float* h; float* out;                     /* (N,128) x3 [agg zeroed], (N,64), (G,1) */
  const float* n_table; const float* x_table;   /* mp_schnet_embed_table_f32 tables; NULL: stage 0 runs the chain */
  /* interaction i: mp_cfconv_filter_table_f32 table; [0] == NULL: every block runs the MFMA kernel from packed[i] */
  const float* filter_table[MP_SCHNET_MAX_DEPTH];
  mp_filter_table_layout filter_layout;
} mp_schnet_forward_desc;
int mp_schnet_forward_launch(const mp_schnet_forward_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- launch groups ------------------------------ */
/* Disjoint union of k resident ragged batches in one launch (the device-side form of concatenating what two
 * MemoryGraphList.tensor() calls produce, kgcnn/data/base.py:203-239): node numbers (float32, or int64 with z_is_i64),
 * coordinates (N,3), edge sample indices (M,2) int64 - unchanged, kgcnn/layers/base.py:27 - and the two row-split arrays,
 * rebased.  Outputs sized for the sums; node_splits / edge_splits get sum(G) + 1 entries.  Lets one launch sequence of the
 * fused forward serve several independent batches (gcnn_keras_amd/fused.py::SchnetFusedRoute.call_group). */
#define MP_CONCAT_MAX 8
typedef struct mp_batch_src {
  const void* z; const float* xyz; const int64_t* idx; const int64_t* node_splits; const int64_t* edge_splits;
  int64_t N, M, G;
} mp_batch_src;
typedef struct mp_concat_desc {
  int32_t k, z_is_i64;
  mp_batch_src src[MP_CONCAT_MAX];
  void* z; float* xyz; int64_t* idx; int64_t* node_splits; int64_t* edge_splits;
} mp_concat_desc;
int mp_concat_batches(const mp_concat_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- batches of a resident data set ------------ */
/* tf.gather(ragged, ids) for up to MP_TAKE_MAX ragged tensors that share their graph axis (G graphs), in one call and
 * without a host read-back: item i receives the rebased dst_splits (B + 1 entries) and the rows of graphs take[0],
 * take[1], ... back to back (bit-exact copy; per-graph edge indices are sample indices, kgcnn/layers/base.py:27, and stay
 * as they are).  take == NULL means the contiguous range first .. first + B - 1.  row_bytes is a multiple of 4; dst_rows
 * is the number of rows dst_values holds (the host knows it from its copy of the splits) and nothing is written past it.
 * An id outside [0, G) is clamped and MP_FLAG_OOB is ORed into *flags.  The scan behind dst_splits walks B in passes of
 * MP_TAKE_SCAN_WIDTH entries; any B is correct.  B == 0 returns MP_OK without a launch. */
#define MP_TAKE_MAX 8
#define MP_TAKE_SCAN_WIDTH 1024
typedef struct mp_take_item {
  const void* src_values; const int64_t* src_splits; int64_t row_bytes;
  void* dst_values; int64_t* dst_splits; int64_t dst_rows;
} mp_take_item;
typedef struct mp_take_desc {
  int32_t k, reserved;
  int64_t G, B, first;
  const int64_t* take;
  int32_t* flags;
  mp_take_item item[MP_TAKE_MAX];
} mp_take_desc;
int mp_ragged_take(const mp_take_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- fused GCN forward -------------------------- */
/* The forward of kgcnn.literature.GCN.make_model (kgcnn/literature/GCN.py:95-109) in 1 + depth launches on 16-node
 * tiles, each launch = one producer of the tile followed by up to three Keras Dense layers on it:
 *   input mode (x != NULL):      t = x (N,K) W_in (K,units_in) + b_in           GCN.py:97  Dense(units, linear)
 *   aggregate mode (x == NULL):  t_i = agg_act( sum_{e: recv(e) = i} weight[e] * h[send[e]] )
 *                                kgcnn/layers/conv/gcn_conv.py:87-90: GatherNodesOutgoing, PoolingWeightedLocalEdges
 *                                (sum, normalize_by_weights=False), Activation; receivers through the CSR `ptr` (N+1)
 *                                over the receiver-sorted edge order, `perm` (nullable) = position -> edge for a list
 *                                that is not sorted (tf.argsort(stable=True), kgcnn/layers/pooling.py:66)
 *   then  t <- act_l(t W_l + b_l)  for l < n_layers (gcn_conv.py:86 lay_dense of the next layer, or GraphMLP,
 *   GCN.py:107), softmax_last: Keras softmax over the last layer's units.  out (N, units of the last layer; units_in
 *   if n_layers == 0).  units_in in {32, 64, 128}, layer widths 1..128.  Sums run in a fixed order: deterministic. */
typedef struct mp_gcn_layer {
  const float* W;   /* (K_l, units) Keras kernel */
  const float* b;   /* (units) or NULL */
  int32_t units, act;
  float alpha;
} mp_gcn_layer;
typedef struct mp_gcn_tile_desc {
  int64_t N;
  const float* x; int64_t K; const float* W_in; const float* b_in;                      /* input mode */
  const float* h; const int32_t* ptr; const int32_t* perm; const int32_t* send;         /* aggregate mode */
  const float* weight; int64_t M; int32_t agg_act; float agg_alpha;
  int32_t units_in, n_layers;
  mp_gcn_layer layer[3];
  int32_t softmax_last;
  float* out;
  const int32_t* tile_start;  /* aggregate mode, nullable: (n_tiles + 1) first node of every tile - strictly increasing,   */
  int64_t n_tiles;            /* tile_start[0] = 0, tile_start[n_tiles] = N, at most 16 nodes per tile (device array; lets */
                              /* the caller cut hub-heavy node ranges into several tiles); NULL: 16 consecutive nodes      */
} mp_gcn_tile_desc;
int mp_gcn_tile_f32(const mp_gcn_tile_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- Dense chains on 16-row tiles ------------ */
/* One or two Keras Dense layers back to back (kgcnn/layers/modules.py:74-87; PAiNNconv / PAiNNUpdate's
 * Dense(units, act) -> Dense(3 units), kgcnn/layers/conv/painn_conv.py:60-62,187-189, and their reverse forms) in one
 * launch, weights in registers, the 128-wide intermediate in LDS - the latency-bound regime of molecular batches:
 *   m = x W1 + b1 ; [save_pre <- m] ; m = act1(m)        or, with grad_pre:  m = (x W1 + b1) * act1'(grad_pre)
 *   out = m W2 + b2 + addend                              W2_packed null: out = m + addend (U1 columns)
 * K1 in {128,256,384}; two stages: U1 = 128, U2 in {128,256,384}; one stage: U1 in {128,256,384}.  W*_packed are
 * mp_chain_pack_f32 images of the Keras kernels (K, U).  addend may alias out.  mp_chain_supported: 1 if built. */
int mp_chain_supported(int K1, int U1, int U2);
int mp_chain_pack_f32(const float* W, int K, int U, float* packed, mpStream_t stream);
int mp_dense_chain_f32(const float* x, int64_t R, int K1, const float* W1_packed, const float* b1, int U1, int act1,
                       float alpha1, float* save_pre, const float* grad_pre, const float* W2_packed, const float* b2,
                       int U2, const float* addend, float* out, mpStream_t stream);

/* Graph readout in one launch: PoolingNodes(sum) over x (N,K) (kgcnn/layers/pooling.py:215-218) followed by the
 * two-layer output MLP Dense(H, act0) -> Dense(1, linear) (kgcnn/literature/PAiNN.py:146-147): out (G,1).  g_x (nullable,
 * (N,K)): also the reverse of this readout, dE_g/dx_n = W0 (W1 * act0'(pre_g)) written to every node row of graph g
 * (what tape.gradient yields there, kgcnn/model/force.py:159-177).  K, H in {64, 128}. */
int mp_pool_mlp2_f32(const float* x, const int64_t* node_splits, int64_t G, int K, const float* W0, const float* b0, int H,
                     int act0, float alpha0, const float* W1, const float* b1, float* out, float* g_x, mpStream_t stream);

/* ---------------------------------------------------------------- SchNet energy + forces ------------------- */
/* Replaces, for a SchNet energy model, kgcnn/model/force.py:159-201 (GradientTape around the energy model, force =
 * -dE/dx) with a forward that keeps the activation derivatives and a hand-written reverse pass.
 *
 * SAVE variants of the forward node chains: as mp_schnet_node_update_f32 / mp_schnet_node_last_f32 / mp_schnet_readout_f32
 * and additionally store sigmoid(pre-activation) of every shifted softplus on the chain (d2 (N,128), dl0 (N,128),
 * dl1 (N,64)) resp. dE_g/d pooled_g (G,64) of the MLP head.  Null outputs = the plain entry.  Packed images only. */
int mp_schnet_node_update_save_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                                   const float* b3, float* n_inout, const float* Wx_next, float* x_out, float* d2_out,
                                   int flags, mpStream_t stream);
int mp_schnet_node_last_save_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                                 const float* b3, const float* n_in, const float* Wl0, const float* bl0,
                                 const float* Wl1, const float* bl1, float* h_out, float* d2_out, float* dl0_out,
                                 float* dl1_out, int flags, mpStream_t stream);
int mp_schnet_readout_grad_f32(const float* h, const int64_t* node_splits, int64_t G, const float* Wo0,
                               const float* bo0, const float* Wo1, const float* bo1, float* out, float* g_pool_out,
                               mpStream_t stream);
/* Reverse node chains on 16-node tiles; every W*T is the mp_schnet_node_pack_f32 image of the TRANSPOSED Keras kernel.
 * head : g_n = ((gh[row] * dl1) Wl1T * dl0) Wl0T ; g_agg = ((g_n W3T) * d2) W2T     gh_row null: gh is one 64-row
 * block: g_n += g_x WxT (g_x rows re-zeroed)     ; g_agg = ((g_n W3T) * d2) W2T */
int mp_schnet_bwd_head_f32(const float* gh, const int32_t* gh_row, const float* dl1, int64_t N, const float* Wl1T,
                           const float* dl0, const float* Wl0T, const float* W3T, const float* d2, const float* W2T,
                           float* g_n, float* g_agg, mpStream_t stream);
int mp_schnet_bwd_block_f32(float* g_x, int64_t N, const float* WxT, float* g_n, const float* W3T, const float* d2,
                            const float* W2T, float* g_agg, mpStream_t stream);
/* out (N,3) = scale * dE/dx from dE/dd (M): sum over the edges touching a node of g_d (x_n - x_other) / d, over the
 * receiver-side and sender-side CSR of the index plan (perm null: that column is sorted).  scale -1: physical force. */
int mp_schnet_force_from_gd_f32(const float* g_d, const float* xyz, const float* dist, const int32_t* recv,
                                const int32_t* send, const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1,
                                const int32_t* perm1, int64_t N, int64_t M, float scale, float* out, mpStream_t stream);
/* The whole energy + force pass of a bound batch slot in one call (the ~32 launches for depth 6, in sequence on
 * `stream`; capturable into a HIP graph): forward as mp_schnet_forward_launch with the SAVE chains (fwd.x unused: the
 * sender features of every block are kept in xs), then head chain, per block distance gradient + swapped-column cfconv
 * + block chain, then the force kernel.  fwd.flags bit 1 (packed node images) is required. */
typedef struct mp_schnet_force_desc {
  mp_schnet_forward_desc fwd;
  float* xs;                       /* (depth, N, 128) sender features x_i of every block */
  float* d2;                       /* (depth, N, 128) */
  float* dl0; float* dl1;          /* (N,128), (N,64) */
  float* g_pool;                   /* (G,64)  MLP head only */
  const int32_t* node_graph;       /* (N) graph of each node, MLP head only */
  const float* W3T[MP_SCHNET_MAX_DEPTH];
  const float* W2T[MP_SCHNET_MAX_DEPTH];
  const float* WxT[MP_SCHNET_MAX_DEPTH];           /* [0] unused */
  const float* packed_bwd[MP_SCHNET_MAX_DEPTH];    /* mp_cfconv_bwd_pack_f32 images */
  const float* Wl0T; const float* Wl1T;
  const int32_t* seg0; const int32_t* perm0;       /* receiver column sorted + its permutation (null: already sorted) */
  const int32_t* seg1; const int32_t* perm1;       /* sender column sorted + its permutation */
  const int32_t* ptr0; const int32_t* ptr1;        /* (N+1) CSR offsets of both columns */
  float* g_n; float* g_agg; float* g_x; float* g_d;   /* (N,128) x3 [g_x zeroed], (M) */
  float* force;                    /* (N,3) out */
  float force_scale;               /* -1: physical force, +1: dE/dx */
} mp_schnet_force_desc;
int mp_schnet_force_launch(const mp_schnet_force_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- host batch packer ---------------------- */
/* The data-format side of the path.  Host pointers only; nothing here launches a kernel.
 *
 * mp_pack_rows_host = kgcnn.data.utils.ragged_tensor_from_nested_numpy (kgcnn/data/utils.py:129-157:
 * np.concatenate(list, axis=0, dtype) + row lengths), as called per property by MemoryGraphList.tensor
 * (kgcnn/data/base.py:203-239): rows_host[g] points to counts_host[g] rows of row_elems elements of src_kind; they
 * are concatenated (converted to dst_kind: f64<->f32, i32<->i64, i32/i64->f32) into dst_host, and the int64
 * row_splits (G+1) are written.  Multi-threaded over contiguous graph ranges (threads <= 1: caller's thread). */
int mp_pack_rows_host(const void* const* rows_host, const int64_t* counts_host, int64_t G, int64_t row_elems,
                      int src_kind, int dst_kind, void* dst_host, int64_t* splits_out_host, int threads);

/* Edge indices of a batch: concatenates the per-graph (m_g, K) sample index lists (idx_kind MP_DT_I64 | MP_DT_I32)
 * into the API's int64 (M,K) tensor and, in the same pass, produces what mp_index_prepare_i64 +
 * mp_csr_from_sorted_i32 would compute on the device for this batch: shifted int32 columns cols[k*M + e]
 * (kgcnn/ops/partition.py:140-155), the MP_FLAG_* word, and - if csr_ptr_out_host is given and column 0 is sorted -
 * the CSR offsets ptr[0..N] (zeros otherwise).  Also writes both row_splits (G+1 each). */
int mp_pack_edge_index_host(const void* const* idx_rows_host, int idx_kind, const int64_t* edge_counts_host,
                            const int64_t* node_counts_host, int64_t G, int K, int64_t* idx_out_host,
                            int64_t* edge_splits_out_host, int64_t* node_splits_out_host, int32_t* cols_out_host,
                            int32_t* csr_ptr_out_host, int32_t* flags_out_host, int threads);

/* Staging memory for the packer (pinned = hipHostMalloc: needs a device; 0 = aligned malloc) and the asynchronous
 * host-to-device copy that hands a packed tensor to the engine on the caller's stream. */
int mp_host_alloc(size_t bytes, int pinned, void** out_host);
int mp_host_free(void* p, int pinned);
int mp_memcpy_h2d_async(void* dst_device, const void* src_host, size_t bytes, mpStream_t stream);

/* ---------------------------------------------------------------- HDNNP2nd: symmetry functions ------------ */
/* Atom-centred symmetry functions (csrc/mp_acsf.hip), Behler's HDNNP2nd (kgcnn/literature/HDNNP2nd.py:154-242).
 * xyz (N,3); z (N) int64 atomic numbers; cols = the index plan's shifted int32 columns (K, M) of the pair list (K = 2,
 * (i, j)) or the triplet list (K = 3, (i, j, k)); ptrc / permc = CSR offsets (N+1) and stable-sort permutation
 * (nullable when column c is sorted) of index column c.  out / g / g_bar are (N, nrel*nfun): out[i, rel*nfun + m].
 * params: (nrel, nfun, P) or, with ncenter > 0, the target-set form (ncenter, nrel, nfun, P) indexed by the receiver's
 * element slot; P = 3 (eta, rs, rc) for G2, 4 (eta, zeta, lambda, rc) for G4.  rmap (31): atomic number -> element
 * slot; pmap (31*31): (z_j, z_k) -> G4 relation; -1 = no entry.  An element without an entry contributes nothing as a
 * neighbour (G2) or as a pair (G4), and a receiver without one gets a zero row from a target-set table: the
 * reference's out-of-range gather of the parameters gives zeros on a GPU and its out-of-range scatter is dropped.
 * Atomic numbers outside [0, 31) count as unmapped.  nrel*nfun <= 2048.
 *
 * mp_acsf_g2_f32: acsf_conv.py:158-210, exp(-eta (r_ij - rs)^2) fc(r_ij), fc = 0.5 (cos(pi clip(r, -rc, rc) / rc) + 1),
 *   summed into the relation of z_j.
 * mp_acsf_g4_f32: acsf_conv.py:419-494, 2^(1-zeta) (1 + lambda cos_ijk)^zeta exp(-eta (r_ij^2 + r_ik^2 + r_jk^2))
 *   fc_ij fc_ik fc_jk (/ multiplicity when it is not 0), summed into the relation of (z_j, z_k); powf semantics.
 * mp_acsf_g*_jvp_f32: forward mode, g_bar[i, rel, m] = sum over i's pairs / triplets of dG_m/dx . (h_i, h_j[, h_k]),
 *   h (N,3): the second-order piece that training through forces needs (d/dbase of base^zeta = zeta base^(zeta-1)).
 * mp_acsf_g*_grad_f32: reverse mode, dx (N,3) = d(sum g . G)/dx; per-entry endpoint partials in ws
 *   (mp_acsf_grad_ws_bytes), added per node over the CSR of every index column: deterministic, no float atomics.
 * All are receiver-parallel over the CSR of column 0; N = 0 needs no device. */
int mp_acsf_grad_ws_bytes(int64_t M, int K, size_t* bytes_out_host);
int mp_acsf_g2_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0,
                   const int32_t* perm0, const int32_t* rmap, const float* params, int nrel, int nfun, int ncenter,
                   float* out, mpStream_t stream);
int mp_acsf_g4_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0,
                   const int32_t* perm0, const int32_t* rmap, const int32_t* pmap, const float* params, int nrel,
                   int nfun, int ncenter, float multiplicity, float* out, mpStream_t stream);
int mp_acsf_g2_jvp_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                       const int32_t* ptr0, const int32_t* perm0, const int32_t* rmap, const float* params, int nrel,
                       int nfun, int ncenter, const float* h, float* g_bar, mpStream_t stream);
int mp_acsf_g4_jvp_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                       const int32_t* ptr0, const int32_t* perm0, const int32_t* rmap, const int32_t* pmap,
                       const float* params, int nrel, int nfun, int ncenter, float multiplicity, const float* h,
                       float* g_bar, mpStream_t stream);
int mp_acsf_g2_grad_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                        const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                        const int32_t* rmap, const float* params, int nrel, int nfun, int ncenter, const float* g,
                        float* ws, size_t ws_bytes, float* dx, mpStream_t stream);
int mp_acsf_g4_grad_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                        const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                        const int32_t* ptr2, const int32_t* perm2, const int32_t* rmap, const int32_t* pmap,
                        const float* params, int nrel, int nfun, int ncenter, float multiplicity, const float* g,
                        float* ws, size_t ws_bytes, float* dx, mpStream_t stream);

/* RelationalDense (csrc/mp_relational.hip, kgcnn/layers/relational.py:219-238 without num_bases / num_blocks).
 * W (nrel, K, U): one kernel per relation; b (U) shared; rel (R) int64; a relation outside [0, nrel) uses a zero
 * kernel (TF-GPU gather), i.e. its row is act(b).  mode 0: y (R,U) = act(x (R,K) W[rel] + b), pre_out (R,U) nullable
 * keeps the pre-activation.  mode 1 (transposed, the reverse pass): y (R,K) = (x (R,U) * act'(pre)) W[rel]^T, pre
 * nullable (no factor), no bias.  FP32, one launch for every relation, no host read-back (graph-capturable).
 * mp_relational_dense_wgrad_f32: dW[q] (K,U) = sum over the rows of relation q of x^T g, rows grouped by a stable sort
 * on the device and added in row order; db (U) = sum_r g[r]; either output nullable; deterministic. */
int mp_relational_dense_f32(const float* x, int64_t R, int64_t K, const int64_t* rel, int64_t nrel, const float* W,
                            const float* b, int64_t U, int act, float act_alpha, int mode, const float* pre,
                            float* pre_out, float* y, mpStream_t stream);
int mp_relational_dense_wgrad_ws_bytes(int64_t R, int64_t nrel, size_t* bytes_out_host);
int mp_relational_dense_wgrad_f32(const float* x, int64_t R, int64_t K, const int64_t* rel, int64_t nrel,
                                  const float* g, int64_t U, float* dW, float* db, void* ws, size_t ws_bytes,
                                  mpStream_t stream);

/* ---------------------------------------------------------------- HDNNP4th: charge equilibration ---------- */
/* CENT charges and Gaussian-charge electrostatics (csrc/mp_cent.hip), Ko et al.'s fourth-generation HDNNP
 * (kgcnn/literature/HDNNP4th.py:25-189).  xyz (N,3); z (N) int64 atomic numbers; node_splits (G+1) int64 row splits of
 * the molecules; sigma / hardness: per-atomic-number tables of ntab entries (the reference's 97, Z = 0..96); an atomic
 * number outside [0, ntab) reads 0 (the reference's out-of-range gather on a GPU).
 *
 * mp_cent_charge_f32: hdnnp_conv.py:148-258, per molecule the bordered system [[A, 1], [1^T, 0]] [Q; lambda] =
 *   [chi; Qtot] over ALL atom pairs of the molecule: A_ii = J[z_i] + 1 / (sigma_i sqrt(pi)), A_ij = erf(r_ij / (sqrt(2)
 *   gamma_ij)) / r_ij with gamma_ij = sqrt(sigma_i^2 + sigma_j^2) (0 where divide_no_nan gives 0); right-hand side +chi
 *   as the reference.  qtot (G).  One wave per molecule, the matrix in LDS, Cholesky + Schur complement in FP64.  At most
 *   MP_CENT_MAX_ATOMS atoms per molecule (the caller rejects larger ones; the kernel writes NaN for them), a molecule
 *   whose factorisation meets a non-positive pivot gets NaN charges, a 0-atom molecule produces nothing.
 * mp_cent_charge_grad_f32: its reverse for an upstream gQ (N), given the forward's charges q: w = A^-1 gQ - mu A^-1 1,
 *   mu = 1^T A^-1 gQ / 1^T A^-1 1; chi_bar = w, x_bar_i = -sum_{j != i} (w_i Q_j + w_j Q_i) f'(r_ij) (x_i - x_j) / r_ij.
 *   Refactors A (no workspace); either output nullable.
 * mp_gauss_energy_f32: hdnnp_conv.py:391-428, energy (G) = sum over the molecule's range_indices (cols = the index plan's
 *   shifted int32 columns (2, M), edge_splits (G+1)) of q_i q_j f(r_ij) / multiplicity (no division when it is 0) + sum
 *   over its atoms of divide_no_nan(q_i^2, sigma_i) / (2 sqrt(pi)).
 * mp_gauss_energy_grad_f32: its reverse for an upstream g_energy (G): q_bar (N), x_bar (N,3), per atom over the CSR
 *   (ptrc / permc, permc nullable when column c is sorted) of both index columns in list order; either output nullable.
 * Deterministic (fixed per-molecule reduction order, no float atomics); N = 0 or G = 0 needs no device. */
#define MP_CENT_MAX_ATOMS 128
int mp_cent_charge_f32(const float* xyz, const int64_t* z, const int64_t* node_splits, int64_t G, int64_t N,
                       const float* chi, const float* qtot, const float* sigma, const float* hardness, int ntab,
                       float* q, mpStream_t stream);
int mp_cent_charge_grad_f32(const float* xyz, const int64_t* z, const int64_t* node_splits, int64_t G, int64_t N,
                            const float* q, const float* gq, const float* sigma, const float* hardness, int ntab,
                            float* chi_bar, float* x_bar, mpStream_t stream);
int mp_gauss_energy_f32(const float* xyz, const int64_t* z, const float* q, const int64_t* node_splits, int64_t G,
                        int64_t N, const int32_t* cols, int64_t M, const int64_t* edge_splits, const float* sigma,
                        int ntab, float multiplicity, float* energy, mpStream_t stream);
int mp_gauss_energy_grad_f32(const float* xyz, const int64_t* z, const float* q, const int64_t* node_splits, int64_t G,
                             int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0, const int32_t* perm0,
                             const int32_t* ptr1, const int32_t* perm1, const float* sigma, int ntab,
                             float multiplicity, const float* g_energy, float* q_bar, float* x_bar,
                             mpStream_t stream);

/* ---------------------------------------------------------------- DimeNet++: angles, basis, triplet step -- */
/* DimeNet++ (csrc/mp_dimenet.hip, kgcnn/literature/DimeNetPP.py:23-183).  Angle pairs (n, m) index EDGES: cols = the
 * index plan's shifted int32 columns (2, T) of the angle list against the edge partition; ptrc / permc = CSR offsets
 * (E+1) and stable-sort permutation (nullable when column c is sorted) of angle column c.  Sums over triplets run in
 * list order and reductions in a fixed order (deterministic, no float atomics); E = 0 or T = 0 needs no device.
 *
 * mp_vector_angle_f32: VectorAngle (kgcnn/layers/geom.py:382-446), theta (T) = atan2(|v1 x v2|, v1 . v2) row by row.
 * mp_vector_angle_grad_f32: its reverse for an upstream g (T); g1 / g2 (T,3), either nullable.  Collinear rows (|v1 x
 *   v2| = 0) get a zero gradient (the reference's tf.norm gradient is NaN there).
 * mp_edge_angle_f32: EdgeAngle (geom.py:450-510), theta[t] = angle(scale[0:3] * v[n_t], scale[3:6] * v[m_t]), v (E,3),
 *   scale (6) nullable (= ones): vector_scale.
 * mp_edge_angle_grad_f32: its reverse, v_bar (E,3): per-triplet partials in ws (mp_edge_angle_grad_ws_bytes), added
 *   per edge over the CSR of both angle columns in list order.
 * mp_spherical_basis_f32: SphericalBasisLayer (kgcnn/layers/conv/dimenet_conv.py:380-463) on distances d (E) and angles
 *   theta (T): rbf_env (E, L*R) = env(d/c) * norm[l,k] j_l(zeros[l,k] d/c) (j_l by the reference's upward recursion,
 *   kgcnn/ops/polynom.py:50-86), sbf (T, L*R) = rbf_env[m_t] * Y_l0(theta_t) (Legendre sum, polynom.py:117-147).
 *   tables (float32): zeros (L,R) | norm (L,R) | Legendre coefficients (L, L/2+1) of x^(l-2i) | sqrt((2l+1)/4pi) (L).
 *   1 <= L <= MP_SBF_MAX_SPHERICAL, 1 <= R <= MP_SBF_MAX_RADIAL; envelope_exponent in [1, 32].
 * mp_spherical_basis_grad_f32: its reverse for an upstream g (T, L*R): d_bar (E) over the CSR of angle column 1 (j_l' =
 *   j_{l-1} - (l+1)/x j_l and the envelope's derivative), theta_bar (T) (-sin theta P_l'(cos theta)); either nullable;
 *   rbf_env = the forward's.
 * mp_dimenet_triplet_f32: the triplet step of DimNetInteractionPPBlock (dimenet_conv.py:186-197), out (E, int_emb)
 *   = sum_{t: A[t,0] = n} xdown[A[t,1]] * ((sbf_t W1) W2): W1 (nsbf, basis_emb), W2 (basis_emb, int_emb), no bias; one
 *   launch, receiver-parallel over the CSR of column 0, no triplet-sized intermediate in memory; an edge without
 *   triplets gets a zero row.  Fused sizes only: int_emb 64, basis_emb 8, nsbf <= 64 (else MP_EINVAL).
 * mp_dimenet_triplet_grad_f32: its reverse for an upstream g (E, int_emb), sender-ordered over the CSR of column 1:
 *   xdown_bar (E, int_emb) and sbf_bar (T, nsbf), either nullable (the weights are frozen: no weight gradients). */
#define MP_SBF_MAX_SPHERICAL 16
#define MP_SBF_MAX_RADIAL 64
int mp_vector_angle_f32(const float* v1, const float* v2, int64_t T, float* theta, mpStream_t stream);
int mp_vector_angle_grad_f32(const float* v1, const float* v2, int64_t T, const float* g, float* g1, float* g2,
                             mpStream_t stream);
int mp_edge_angle_f32(const float* v, int64_t E, const int32_t* cols, int64_t T, const float* scale, float* theta,
                      mpStream_t stream);
int mp_edge_angle_grad_ws_bytes(int64_t T, size_t* bytes_out_host);
int mp_edge_angle_grad_f32(const float* v, int64_t E, const int32_t* cols, int64_t T, const int32_t* ptr0,
                           const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1, const float* scale,
                           const float* g, float* ws, size_t ws_bytes, float* v_bar, mpStream_t stream);
int mp_spherical_basis_f32(const float* d, int64_t E, const float* theta, const int32_t* cols, int64_t T,
                           const float* tables, int num_spherical, int num_radial, float cutoff, int envelope_exponent,
                           float* rbf_env, float* sbf, mpStream_t stream);
int mp_spherical_basis_grad_f32(const float* d, int64_t E, const float* theta, const int32_t* cols, int64_t T,
                                const int32_t* ptr1, const int32_t* perm1, const float* tables, int num_spherical,
                                int num_radial, float cutoff, int envelope_exponent, const float* rbf_env,
                                const float* g, float* d_bar, float* theta_bar, mpStream_t stream);
int mp_dimenet_triplet_f32(const float* xdown, int64_t E, const float* sbf, int nsbf, const int32_t* cols, int64_t T,
                           const int32_t* ptr0, const int32_t* perm0, const float* W1, int basis_emb, const float* W2,
                           int int_emb, float* out, mpStream_t stream);
int mp_dimenet_triplet_grad_f32(const float* xdown, int64_t E, const float* sbf, int nsbf, const int32_t* cols,
                                int64_t T, const int32_t* ptr1, const int32_t* perm1, const float* W1, int basis_emb,
                                const float* W2, int int_emb, const float* g, float* xdown_bar, float* sbf_bar,
                                mpStream_t stream);

/* ---------------------------------------------------------------- EGNN: position encoding, fused edge step -- */
/* EGNN (csrc/mp_egnn.hip, kgcnn/literature/EGNN.py:23-208).
 *
 * mp_position_encoding_f32: PositionEncodingBasisLayer (kgcnn/layers/geom.py:596-713) on x (M): out (M, 2 dim_half) =
 *   [sin(x s_k) | cos(x s_k)], or sin / cos interleaved per k; scales (dim_half) = 2 pi exp(-log(num_mult) k /
 *   (dim_half - 1) - log(wave_length_min)), built on the host in float32.  Accurate sincosf.
 * mp_position_encoding_grad_f32: its reverse for an upstream g (M, 2 dim_half): x_bar (M) = sum_k s_k (g_sin cos - g_cos
 *   sin), k ascending.
 * mp_egnn_edge_f32: the edge step of one EGNN block without edge attributes (EGNN.py:155-174) in one launch plus a
 *   finishing pass: out (N, 128) = sum_{e: cols[0][e] = r} att_e m_e with m_e = act2(act1(Pa[cols[0][e]] +
 *   Pb[cols[1][e]] + enc_e Wc + b1) W2 + b2), att_e = act_att(m_e . w_att + b_att) (w_att null: att_e = 1).
 *   Pa, Pb (N, 128) = h W_a, h W_b, the node-side projections by the first two row blocks of the first Dense kernel; Wc
 *   its remaining rows (2 dim_half, 128) with enc_e the position encoding of x[e], or (1, 128) with enc_e = x[e] when
 *   dim_half = 0; cols = the index plan's shifted int32 columns (2, E); ptr0 (N+1) / perm0 (nullable) = CSR and stable
 *   sort of column 0.  b1, b2, b_att nullable.  ws: mp_egnn_edge_ws_bytes(E).  z1_save / z2_save (E, 128), both
 *   nullable: the two pre-activations in list order, kept for the reverse.  Sums run per receiver in list order, a
 *   receiver cut by a tile boundary through per-tile partials added in tile order: deterministic, no float atomics.
 *   Fused sizes only: width 128, 2 dim_half <= 64 (else MP_EINVAL).  N = 0 needs no device; E = 0 gives zeros.
 * mp_egnn_edge_grad_f32: its reverse for an upstream g (N, 128) from the saved z1 / z2: z1_bar (E, 128), the gradient
 *   of the first layer's pre-activation per edge (its sums over the CSRs of columns 0 / 1 give Pa_bar / Pb_bar), and x_bar (E),
 *   nullable.  The weights are frozen: no weight gradients. */
int mp_position_encoding_f32(const float* x, int64_t M, const float* scales, int dim_half, int interleave, float* out,
                             mpStream_t stream);
int mp_position_encoding_grad_f32(const float* x, int64_t M, const float* scales, int dim_half, int interleave,
                                  const float* g, float* x_bar, mpStream_t stream);
int mp_egnn_edge_ws_bytes(int64_t E, size_t* bytes_out_host);
int mp_egnn_edge_f32(const float* Pa, const float* Pb, int64_t N, const float* x, const int32_t* cols, int64_t E,
                     const int32_t* ptr0, const int32_t* perm0, const float* scales, int dim_half, int interleave,
                     const float* Wc, const float* b1, int act1, const float* W2, const float* b2, int act2,
                     const float* w_att, const float* b_att, int act_att, float alpha, float* ws, size_t ws_bytes,
                     float* z1_save, float* z2_save, float* out, mpStream_t stream);
int mp_egnn_edge_grad_f32(const float* g, int64_t N, const float* x, const int32_t* cols, int64_t E, const float* z1,
                          const float* z2, const float* scales, int dim_half, int interleave, const float* Wc, int act1,
                          const float* W2, int act2, const float* w_att, const float* b_att, int act_att, float alpha,
                          float* z1_bar, float* x_bar, mpStream_t stream);

/* ---------------------------------------------------------------- CGCNN: crystal geometry, batch norm, gate step -- */
/* CGCNN (csrc/mp_cgcnn.hip, csrc/mp_lattice.hip; kgcnn/literature/CGCNN.py:22-189).
 *
 * mp_frac_to_real_f32: FracToRealCoordinates.call (kgcnn/layers/geom.py:1048-1052), the einsum 'ij,ikj->ik' as
 *   written: out[e][k] = (f_0 A[k][0] + f_1 A[k][1]) + f_2 A[k][2] with f = frac[e] (M,3) and A = lattice[g(e)]
 *   (G,3,3), g(e) from the input's own row_splits (G+1); fixed order, no contraction.  That is A f, not the f A of the
 *   reference's docstring.  transposed != 0: the reverse with respect to frac, out[e][j] = (f_0 A[0][j] + f_1 A[1][j])
 *   + f_2 A[2][j].  M == 0 returns MP_OK without touching the device.
 * mp_batchnorm_infer_f32: GraphBatchNormalization.call outside training (kgcnn/layers/norm.py:206-216 = Keras
 *   BatchNormalization with the moving statistics) on x (R, C), last axis: inv = (1 / sqrt(moving_variance + epsilon))
 *   * gamma, out = x * inv + (beta - moving_mean * inv); gamma / beta (C) nullable (scale / center off).  The vectors
 *   are read in place on every call.  moving_mean == NULL (then beta must be NULL): the input reverse, out = x * inv.
 * mp_cgcnn_gate_f32: CGCNNLayer.call (kgcnn/layers/conv/cgcnn_conv.py:67-111 through MessagePassingBase.call,
 *   kgcnn/layers/message.py:81-104) for units = 64 and sum pooling, in one launch plus a node-sized update pass:
 *     z_s[e] = Pa_s[cols[0][e]] + Pb_s[cols[1][e]] + edges[e] Wc_s + b_s      (likewise z_f)
 *     m_e = act_s(BN_s(z_s)) * sigmoid(BN_f(z_f)),  u_r = sum_{e: cols[0][e] = r} m_e,  out_r = act_out(h_r + BN_out(u_r)).
 *   Pa_* , Pb_* (N, 64) = h Wa_*, h Wb_*: the node-side products by the first two 64-row blocks of the s / f Dense
 *   kernels; Wc_* (D, 64) their remaining rows, 1 <= D <= 64 (else MP_EINVAL); edges (E, D); b_* (64) nullable; cols =
 *   the index plan's shifted int32 columns (2, E); ptr0 (N+1) / perm0 (nullable) = CSR and stable sort of column 0.
 *   bn_host: NULL (no batch normalisation) or a HOST array of 12 device pointers {gamma, beta, moving_mean,
 *   moving_variance} x {s, f, out}; a triple whose moving_mean and moving_variance are NULL is off, gamma / beta are
 *   nullable; eps_host: HOST array of the three epsilons (NULL with bn_host).  BN as in mp_batchnorm_infer_f32: a node
 *   without edges gets act_out(h + beta - mean * inv).  ws: mp_cgcnn_gate_ws_bytes(E).  Sums run per receiver in list
 *   order, a receiver cut by a tile boundary through per-tile partials added in tile order: deterministic, no float
 *   atomics.  No reverse: the weights and inputs are frozen.  N = 0 needs no device; out must not alias h. */
int mp_frac_to_real_f32(const float* frac, const float* lattice, const int64_t* row_splits, int64_t G, int64_t M,
                        int transposed, float* out, mpStream_t stream);
int mp_batchnorm_infer_f32(const float* x, int64_t R, int64_t C, const float* gamma, const float* beta,
                           const float* moving_mean, const float* moving_variance, float epsilon, float* out,
                           mpStream_t stream);
int mp_cgcnn_gate_ws_bytes(int64_t E, size_t* bytes_out_host);
int mp_cgcnn_gate_f32(const float* h, const float* Pa_s, const float* Pa_f, const float* Pb_s, const float* Pb_f,
                      int64_t N, const float* edges, int D, const int32_t* cols, int64_t E, const int32_t* ptr0,
                      const int32_t* perm0, const float* Wc_s, const float* Wc_f, const float* b_s, const float* b_f,
                      const float* const* bn_host, const float* eps_host, int act_s, int act_out, float alpha, float* ws,
                      size_t ws_bytes, float* out, mpStream_t stream);

/* ---------------------------------------------------------------- GAT / GATv2: fused multi-head attention --------- */
/* csrc/mp_gat.hip.  One attention block = H heads over the same [nodes, edges, edge_index]; replaces, per head, the three
 * gathers, the (M, 2F + D) concatenation, the Dense layers on it (AttentionHeadGAT.call, kgcnn/layers/conv/gat_conv.py:
 * 103-114; AttentionHeadGATV2.call, :200-214; MultiHeadGATV2Layer.call, :233-323) and PoolingLocalEdgesAttention
 * (kgcnn/layers/pooling.py:464-546: segment softmax, kgcnn/ops/segment.py:5-24, and the weighted segment sum).
 *
 * mp_gat_logits_f32: the logits of heads [head0, head0 + H), 1 <= H <= MP_GAT_MAX_HEADS, units U in {32, 64}, written
 *   to logits[e * logit_heads + head0 + h] in EDGE order; r = cols[0][e], s = cols[1][e], g_e = edges[e] (E, D):
 *     MP_GAT_V2:  logit = a_h . act(P_h[r] + Q_h[s] + g_e Wc_h + b_h);  P_h, Q_h (N, U), Wc_h (D, U), b_h (U) nullable
 *                 (b_host NULL: no head has a bias), a_h (U); 0 <= D <= 64 (else MP_EINVAL).
 *     MP_GAT_V1:  logit = act(p_h[r] + q_h[s] + g_e . Wc_h);  Wc_h (D); pq (N, H, 4), 16-byte aligned, from
 *                 mp_gat_node_scores_f32 with the same H heads; P_host / Q_host / b_host / a_host are not read.  The
 *                 four floats and the edge product are added in float64 and rounded once.
 *   (MP_GAT_V2 does not read pq; its dot product with a_h runs in column order on a float64 accumulator.)
 *   *_host are HOST arrays of H device pointers (copied into the kernel argument); with D = 0 edges and Wc_host are not
 *   read.  cols = the index plan's shifted int32 columns (2, E); perm0 (nullable) = the stable sort of column 0: the
 *   tiles walk receiver-sorted positions so that the gathered P rows repeat (the CSR offsets are not needed here).  An
 *   edge with an index outside [0, N) is skipped: its logit is not written.  E = 0 needs no device.
 * mp_gat_node_scores_f32: the node-side scalars of GAT: with a_h = lay_alpha.kernel (2U + D), p_h[n] = Wn_h[n] . a_h[:U]
 *   and q_h[n] = Wn_h[n] . a_h[U:2U], summed in float64 in column order and stored as pq[n][h] = {p, p - (float)p, q,
 *   q - (float)q}: a logit of a few hundred keeps the absolute accuracy its softmax weight needs.  Wn_host / a_host:
 *   HOST arrays of H device pointers; pq (N, H, 4) floats, 16-byte aligned.  N = 0 needs no device.
 * mp_gat_attend_f32: out[r, head0 + h, :] = sum_e softmax_e(logit_e) Wn_h[cols[1][e]] over the edges of receiver r,
 *   [ptr0[r], ptr0[r + 1]) through perm0, the segment maximum subtracted before the exponential; Wn_host: HOST array
 *   of H device pointers (N, U); logits as written above; out (N, logit_heads, U), every row of the H heads written, a
 *   receiver without edges gets zeros.  One wave per (receiver, head); all sums in an order fixed by the list order and
 *   the lane layout: no atomics, two runs give equal bits.  N = 0 needs no device.
 * Forward only: the weights and inputs are frozen (training takes the layer sequence). */
enum mp_gat_mode { MP_GAT_V1 = 0, MP_GAT_V2 = 1 };
#define MP_GAT_MAX_HEADS 8
int mp_gat_node_scores_f32(int H, int U, const float* const* Wn_host, const float* const* a_host, int64_t N, float* pq,
                           mpStream_t stream);
int mp_gat_logits_f32(int mode, int H, int U, const float* const* P_host, const float* const* Q_host, const float* pq,
                      const float* const* Wc_host, const float* const* b_host, const float* const* a_host, int64_t N,
                      const float* edges, int D, const int32_t* cols, int64_t E, const int32_t* perm0, int act, float alpha,
                      float* logits, int64_t logit_heads, int64_t head0, mpStream_t stream);
int mp_gat_attend_f32(int H, int U, const float* const* Wn_host, int64_t N, const float* logits, int64_t logit_heads,
                      int64_t head0, const int32_t* cols, int64_t E, const int32_t* ptr0, const int32_t* perm0, float* out,
                      mpStream_t stream);

/* ---------------------------------------------------------------- MEGNet: fused edge step of one block ------------- */
/* MEGNet (csrc/mp_megnet.hip; kgcnn/literature/Megnet.py:24-373).
 *
 * mp_megnet_edge_f32: the edge update of one MEGnetBlock and its pool into the receivers
 *   (kgcnn/layers/conv/megnet_conv.py:96-111) in one launch plus a node-sized finishing pass:
 *     z1[e]   = Pa[cols[0][e]] + Pb[cols[1][e]] + edges[e] Wc + Pu[g(e)]                      (64 wide)
 *     e'[e]   = act(act(z1[e]) W1 + b1) W2 + b2                                                (64 -> 32 -> 32)
 *     pool[r] = mean or sum over {e : cols[0][e] = r} of e'[e]; a receiver without edges gets 0.
 *   Pa, Pb (N, 64) = v W_e[0:Fn], v W_e[Fn:2Fn] and Pu (G, 64) = u W_e[2Fn+Fe:] + b0: the node-side and state-side
 *   products by row blocks of the first edge Dense kernel W_e (2Fn + Fe + Fu, 64), its bias folded into Pu; Wc (Fe, 64)
 *   = W_e[2Fn:2Fn+Fe]; W1 (64, 32), W2 (32, 32) row-major; b1, b2 (32) nullable.  edges (E, Fe); edge_splits = the edge
 *   tensor's int64 row_splits (G+1), from which g(e) is looked up; cols = the index plan's shifted int32 columns
 *   (2, E); ptr0 (N+1) / perm0 (nullable) = CSR and stable sort of column 0.  Served: Fn = Fe = Fu = 32 and units0 /
 *   units1 / units2 = 64 / 32 / 32, act any activation code (mp_dense_f32's epilogue function), pool_op MP_SUM or
 *   MP_MEAN; anything else MP_EINVAL.  edges_out (E, 32) in list order, pool_out (N, 32); ws:
 *   mp_megnet_edge_ws_bytes(E).  Sums run per receiver in list order, a receiver cut by a tile boundary through
 *   per-tile partials added in tile order: deterministic, no float atomics.  No reverse: weights and inputs are
 *   frozen.  N = 0 needs no device; E = 0 zeroes pool_out. */
int mp_megnet_edge_ws_bytes(int64_t E, size_t* bytes_out_host);
int mp_megnet_edge_f32(const float* Pa, const float* Pb, int64_t N, const float* Pu, const int64_t* edge_splits,
                       int64_t G, const float* edges, int Fn, int Fe, int Fu, const int32_t* cols, int64_t E,
                       const int32_t* ptr0, const int32_t* perm0, const float* Wc, const float* W1, const float* b1,
                       const float* W2, const float* b2, int units0, int units1, int units2, int act, float alpha,
                       int pool_op, float* ws, size_t ws_bytes, float* edges_out, float* pool_out, mpStream_t stream);

/* ---------------------------------------------------------------- CMPNN: communicate round, ragged GRU readout ----- */
/* CMPNN (csrc/mp_cmpnn.hip, csrc/mp_recurrent.hip; kgcnn/literature/CMPNN.py:23-174).
 *
 * mp_cmpnn_boost_f32: the node booster of one round (CMPNN.py:131-135: two PoolingLocalEdges, LazyMultiply, LazyAdd;
 *   :148-150 for the last step) in one walk of every receiver's CSR segment:
 *     m[n] = pool_{e in [ptr[n], ptr[n+1])} he[e] * max_e he[e],   out[n] = m_only ? m[n] : h[n] + m[n].
 *   he (M, F), h and out (N, F), F a multiple of 4, 16-byte aligned; ptr (N+1) / perm (nullable) = CSR and stable sort of
 *   the receiver column (as mp_segment_reduce_csr_f32: edge order, the first row initialises both accumulators, a
 *   receiver without edges gives 0 for both, so out = h); pool_op MP_SUM or MP_MEAN.  h is not read with m_only.  Every
 *   operation is the layer sequence's, in its order: equal bits.
 * mp_directed_edge_update_f32: the edge update of one round (CMPNN.py:138-143: GatherNodesOutgoing,
 *   DMPNNGatherEdgesPairs, LazySubtract, Dense, LazyAdd, Activation; kgcnn/layers/conv/dmpnn_conv.py:39-46):
 *     out[e] = act2(act1((h[send[e]] - he[rev[e]]) W + b) + he0[e]),   he[rev[e]] := 0 where rev[e] < 0.
 *   h (N, F); he, he0, out (E, F); W (F, F) row-major, b (F) nullable; send (E) = the index plan's shifted sender
 *   column, rev (E) = the batch position of the reverse edge or a negative number.  A tiled FP32-MFMA GEMM (tile of
 *   MP_CMPNN_EDGE_TILE edges x 64 columns) whose A tile is formed while it is staged.  F a multiple of 4, 16-byte aligned
 *   operands.  send outside [0, N) and rev >= E are clamped and OR MP_FLAG_OOB into *flags (nullable).  out must not
 *   overlap he (MP_EINVAL): other tiles gather he[rev] while a tile is written; the caller alternates two buffers.
 * mp_gru_ragged_last_f32: ks.layers.GRU (reset_after = True) over each graph's node sequence, the state after the last
 *   node (CMPNN.py:157), in one launch.  mx (n_nodes, 3U) = x W + b_in for every node (mp_dense_f32), row_splits (G+1)
 *   int64, R (U, 3U) the recurrent kernel, b_rec (3U) nullable, gates [z | r | h], the combine of mp_gru_combine_f32.
 *   out (G, U); a graph without nodes gets the zero state.  U a multiple of 4, at most MP_GRU_RAGGED_MAX_UNITS.  A
 *   workgroup carries 16 graphs to the longest of them.
 * All three: no float atomics, equal bits on every run and stream, no host read-back; forward only. */
#define MP_CMPNN_EDGE_TILE 64
#define MP_GRU_RAGGED_MAX_UNITS 512
int mp_cmpnn_boost_f32(const float* h, const float* he, int64_t M, int64_t F, const int32_t* ptr, const int32_t* perm,
                       int64_t N, int pool_op, int m_only, float* out, mpStream_t stream);
int mp_directed_edge_update_f32(const float* h, int64_t N, const float* he, const float* he0, int64_t E, int64_t F,
                                const int32_t* send, const int32_t* rev, const float* W, const float* b, int act1,
                                int act2, float alpha, float* out, int32_t* flags, mpStream_t stream);
int mp_gru_ragged_last_f32(const float* mx, int64_t n_nodes, const int64_t* row_splits, int64_t G, const float* R,
                           const float* b_rec, int64_t U, int act, int rec_act, float* out, mpStream_t stream);

/* ---------------------------------------------------------------- DMPNN: reverse of the directed edge update -------- */
/* What the tape computes for one round of kgcnn/literature/DMPNN.py:136-140 (DMPNNPPoolingEdgesDirected,
 * kgcnn/layers/conv/dmpnn_conv.py:83-87; the shared Dense, kgcnn/layers/modules.py:15-90; LazyAdd; Activation) when
 * the round ran as  R = segment sum of h at the receiver,  y = mp_directed_edge_update_f32(h := R, he := h, he0 := h0)
 * with act1 = linear.  csrc/mp_dmpnn.hip, csrc/mp_wgrad.hip.
 *
 * mp_directed_edge_update_grad_f32: the reverse of Activation, LazyAdd and Dense's input side in one launch,
 *     p[e] = g[e] * act2'(y[e]),   q[e] = p[e] W^T.
 *   g, y (the forward output), p, q (E, F); W (F, F) row-major.  act2 is MP_ACT_LINEAR (y is not read, may be NULL) or
 *   MP_ACT_RELU (the derivative is taken from the output: the product g * (y > 0), the bits of the layer sequence);
 *   anything else MP_EINVAL.  p is the gradient of he0 and of the pre-activation, q the gradient of the difference
 *   h[send] - he[rev].  The forward kernel's tiling: MP_CMPNN_EDGE_TILE edges x 64 columns of q per workgroup, FP32 MFMA,
 *   the A tile formed while it is staged, W read by rows; the column tile 0 writes p.  F a multiple of 4, 16-byte aligned
 *   operands; p and q must not overlap g or y.  E = 0 returns MP_OK without a launch.
 * mp_directed_edge_wgrad_f32: the weight side of Dense,
 *     dW (F, F) = sum_e d[e]^T p[e],  db (F, nullable) = sum_e p[e],  d[e] = h[send[e]] - he[rev[e]]  (0 where rev[e] < 0)
 *   with d formed while a row slab is staged and never written.  h (N, F); he, p (E, F).  mp_dense_wgrad_f32's row split,
 *   slabs and in-order reduction as they stand (ws from mp_directed_edge_wgrad_ws_bytes, a function of E and F only).
 *   send outside [0, N) and rev >= E are clamped and OR MP_FLAG_OOB into *flags (nullable).  E = 0 writes zeros.
 * mp_directed_edge_hgrad_f32: the last line of the reverse, the adjoint of the receiver sum (a gather at the receiver)
 *   minus the adjoint of DMPNNGatherEdgesPairs (dmpnn_conv.py:39-46),
 *     out[e] = rbar[recv[e]] - sum_{j in [rev_ptr[e], rev_ptr[e+1])} q[rev_perm[j]],
 *   rbar (N, F) = the segment sum of q over the sender CSR; rev_ptr (E+2) / rev_perm (E, nullable) = CSR and stable sort
 *   of rev with the edges that have no reverse moved to the extra segment E: right for any rev, an involution or not.
 *   Rows are added in CSR order.  recv outside [0, N) is clamped and flagged.
 * All three: no float atomics, equal bits on every run and stream, no host read-back. */
int mp_directed_edge_update_grad_f32(const float* g, const float* y, int64_t E, int64_t F, const float* W, int act2,
                                     float* p, float* q, mpStream_t stream);
int mp_directed_edge_wgrad_ws_bytes(int64_t E, int64_t F, size_t* bytes_out_host);
int mp_directed_edge_wgrad_f32(const float* h, int64_t N, const float* he, int64_t E, int64_t F, const int32_t* send,
                               const int32_t* rev, const float* p, float* dw, float* db, void* ws, size_t ws_bytes,
                               int32_t* flags, mpStream_t stream);
int mp_directed_edge_hgrad_f32(const float* rbar, int64_t N, const float* q, int64_t E, int64_t F, const int32_t* recv,
                               const int32_t* rev_ptr, const int32_t* rev_perm, float* out, int32_t* flags,
                               mpStream_t stream);

/* ---------------------------------------------------------------- RGCN / GNNFilm: fused relational message step ---- */
/* csrc/mp_rgcn.hip.  One block of kgcnn/literature/RGCN.py:96-103 (GatherNodesOutgoing, Dense, RelationalDense,
 * LazyMultiply, PoolingLocalMessages, LazyAdd, Activation) or of kgcnn/literature/GNNFilm.py:93-102
 * (GatherNodesSelection, three RelationalDense, LazyMultiply, LazyAdd, PoolingLocalMessages, Activation) in one launch,
 * for a LINEAR message RelationalDense: the sum over a receiver's edges is taken in front of the per-relation product.
 *   MP_RELCONV_RGCN:  out[i] = act( sum_q A_iq W[q] + s_i b + act0(nodes[i] W0 + b0) ),
 *                     A_iq = sum_{e -> i, rel[e] = q} weights[e] nodes[send e],  s_i = sum_{e -> i} weights[e]
 *   MP_RELCONV_FILM:  out[i] = act( sum_q [ g_iq * (A_iq W[q] + c_iq b) + c_iq t_iq ] ),  A unweighted, c_iq its edge count,
 *                     g_iq = act_m(nodes[i] Wg[q] + bg),  t_iq = act_m(nodes[i] Wt[q] + bt)
 * nodes (N, K); cols = the index plan's shifted int32 columns (2, E), receiver first; ptr0 (N+1) / perm0 (nullable) =
 * CSR and stable sort of the receiver column; rel (E) int64; weights (E) nullable (ones; RGCN only); W, Wg, Wt
 * (R, K, U) effective kernels; W0 (K, U); every bias (U) nullable; out (N, U), every row written: a receiver without
 * edges gets act(act0(n W0 + b0)) (RGCN) or act(0) (FiLM).  A relation outside [0, R) uses a zero kernel as
 * mp_relational_dense_f32 does (RGCN: the edge adds weights[e] b; FiLM: b * act_m(bg) + act_m(bt)); a position whose
 * edge id or sender is out of range is skipped.  K and U each in {32, 64, 128}, 1 <= R <= MP_RELCONV_MAX_RELATIONS
 * (MP_EINVAL otherwise).  One workgroup owns 16 consecutive receivers and all of their positions, staged 256 at a time;
 * the relations present are dealt to its four waves, whose sums are added in wave order: no workspace, no float atomics,
 * a fixed summation order (per wave: chunk ascending, relation ascending, list order within), equal bits on every run.
 * FP32.  N = 0 needs no device; E = 0 writes the no-edge rows.  Forward only. */
enum mp_relconv_mode { MP_RELCONV_RGCN = 0, MP_RELCONV_FILM = 1 };
#define MP_RELCONV_MAX_RELATIONS 64
int mp_relational_conv_f32(int mode, const float* nodes, int64_t N, int64_t K, const int32_t* cols, int64_t E,
                           const int32_t* ptr0, const int32_t* perm0, const int64_t* rel, const float* weights,
                           int64_t R, const float* W, const float* b, int64_t U, const float* W0, const float* b0,
                           int act0, const float* Wg, const float* bg, const float* Wt, const float* bt, int act_m,
                           int act, float alpha, float* out, mpStream_t stream);

/* ---------------------------------------------------------------- AttentiveFP: edge head, attentive readout --------- */
/* csrc/mp_attentivefp.hip, which states the algebra (kgcnn/layers/conv/attentivefp_conv.py:75-107, 196-220).
 *
 * mp_afp_edge_f32: the per-edge part of AttentiveHeadFP with use_edge_features, over receiver-sorted positions p
 *   (edge e = perm0[p], r = cols[0][e], s = cols[1][e], g_e = edges[e] (E, D)):
 *     hidden = act(X[s] + g_e W2e + b2),  msg[p] = hidden Wl + bl,  logit[p] = a . act(P[r] + hidden Wae + ba)
 *   X, P (N, U) node-side products; W2e (D, U), Wl, Wae (U, U) row-block views of the layers' kernels, read in place;
 *   every bias (U) nullable; a (U).  logit (E) and msg (E, U) are written in POSITION order; a position whose edge id,
 *   receiver or sender is out of range gets zeros.  U in {32, 64}, 1 <= D <= 64 (MP_EINVAL otherwise).  E = 0 needs no
 *   device.
 * mp_afp_attend_f32: out[r] = act_context(sum_p softmax_p(logit[p]) msg[p]) over the positions [ptr0[r], ptr0[r + 1]),
 *   the segment maximum subtracted before the exponential; out (N, U), every row written, a receiver without edges gets
 *   act_context(0).  One wave per receiver, the sweeps of mp_gat_attend_f32.  N = 0 needs no device.
 * mp_afp_readout_f32: PoolingNodesAttentive.call behind its Dense (wn = n Wl + bl), the loop over `depth` inside one
 *   launch: h_g = pool_op (MP_SUM / MP_MEAN) of the graph's rows of n (n_nodes, U); per iteration
 *   a_i = act(w . [h_g || n_i] + b), cont_g = act_context(sum_i softmax_i(a_i) wn_i), h_g = GRUCell(cont_g, h_g) with
 *   K, R (U, 3U), b_in, b_rec (3U) nullable, gates [z | r | h], the combine of mp_gru_combine_f32.  w (2U), b (1)
 *   nullable; node_term: workspace of n_nodes doubles; out (G, U); a graph without nodes runs the recurrence on
 *   cont = act_context(0).  U a multiple of 4, at most MP_AFP_READOUT_MAX_UNITS; depth >= 0.  A workgroup carries 16
 *   graphs.  G = 0 needs no device.
 * All three: no float atomics, equal bits on every run and stream, no host read-back; forward only. */
#define MP_AFP_READOUT_MAX_UNITS 256
int mp_afp_edge_f32(int U, const float* X, const float* P, int64_t N, const float* edges, int D, const float* W2e,
                    const float* b2, const float* Wl, const float* bl, const float* Wae, const float* ba, const float* a,
                    const int32_t* cols, int64_t E, const int32_t* perm0, int act, float alpha, float* logit, float* msg,
                    mpStream_t stream);
int mp_afp_attend_f32(int U, const float* msg, const float* logit, int64_t N, const int32_t* cols, int64_t E,
                      const int32_t* ptr0, const int32_t* perm0, int act_context, float alpha, float* out,
                      mpStream_t stream);
int mp_afp_readout_f32(const float* n, const float* wn, int64_t n_nodes, const int64_t* row_splits, int64_t G, int U,
                       int depth, int pool_op, const float* w, const float* b, const float* K, const float* R,
                       const float* b_in, const float* b_rec, int act, float alpha, int act_context, int gru_act,
                       int rec_act, double* node_term, float* out, mpStream_t stream);

/* ---------------------------------------------------------------- extensive energy / force label scaler ------------
 * kgcnn/data/transform/scaler/mol.py:38-98 (_ExtensiveMolecularScalerBase._fit / _predict) and
 * kgcnn/data/transform/scaler/force.py:164-222 (EnergyForceExtensiveLabelScaler.transform / inverse_transform): a ridge
 * regression of the molecular energies (G, S) on the per-molecule element counts, the population standard deviation of
 * the residual, and the transform itself.  Everything floating-point is FP64 with a fixed summation order (rows in chunks
 * of MP_SCALER_CHUNK_ROWS, slabs added in chunk order): the same bits on every run and stream, no float atomics.
 * K, the number of species present, stays on the device (selection[95]); buffers are sized for K = 95.  number_kind:
 * MP_DT_F32 (cast as Keras casts: truncation), MP_DT_I32 or MP_DT_I64.  y / energy kinds: MP_DT_F32 or MP_DT_F64.
 *
 * mp_scaler_species_count: mol.py:55-67.  counts (G, 95) int32 = per-graph histogram of the atomic numbers (one wave per
 *   graph, integer LDS atomics), mask (95) int32 = 1 where any graph holds the number, selection (96) int32 = the numbers
 *   present in ascending order, -1 behind them, selection[95] = K.  A number outside [0, 95) is not counted and ORs
 *   MP_FLAG_OOB into *flags (the caller zeroes the word).  N = node_splits[G]; splits are clamped to [0, N].
 * mp_scaler_fit_ws_bytes: workspace of the two calls below for G graphs and S states.
 * mp_scaler_normal_f64: Ridge.fit's normal equations.  A (K, K) = X^T W X + alpha I and b (K, S) = X^T W y with X the
 *   count columns selection[0..K), W = diag(sample_weight (G) or 1); fit_intercept centres X and y by their weighted
 *   means first (sklearn's _preprocess_data), which land in mean (K + S) (zeros otherwise).  Buffers: A 95*95, b 95*S,
 *   mean 95+S doubles.
 * mp_scaler_solve_f64: one workgroup, Cholesky of A in FP64 LDS, forward and back substitution for the S right-hand
 *   sides.  coef (95, S): rows [0, K) in selection order, zeros behind; intercept (S) = y_mean - x_mean . coef or 0;
 *   table (95, S) = coef scattered by atomic number, 0 for absent numbers.  *status = 0, or 1 + the column of a
 *   non-positive pivot (then coef, table and intercept are NaN); the host raises ValueError.
 * mp_scaler_residual_std_f64: mol.py:69-73.  scale (S) = sqrt(mean((d - mean(d))^2)) of d = y - (X coef + intercept),
 *   two passes; ones when standardize = 0.
 * mp_scaler_apply: force.py:164-178 (inverse = 0) and :207-222 (inverse = 1) in one launch, one wave per graph.  The
 *   graph's offset (S) = intercept + sum over its atoms of table[Z], straight from the ragged numbers.  Forward:
 *   energy_out = (energy_in - offset) / scale, force_out = force_in / scale; inverse: energy_in * scale + offset,
 *   force_in * scale.  Energies (G, S), forces (N, 3 * S) float32 (that is (N, 3) for S = 1 and (N, 3, S) otherwise),
 *   offset_out (G, S) FP64; energy_in, force_in and offset_out are each nullable.  An atomic number with present[Z] = 0
 *   contributes 0 (the reference's behaviour, which prints a warning) and ORs MP_FLAG_UNKNOWN_SPECIES into *flags, one
 *   outside [0, 95) contributes 0 and ORs MP_FLAG_OOB.  Outputs may alias their inputs. */
#define MP_SCALER_MAX_NUMBER 95
#define MP_SCALER_CHUNK_ROWS 256
#define MP_SCALER_MAX_STATES 32
int mp_scaler_species_count(const void* numbers, int number_kind, const int64_t* node_splits, int64_t G, int64_t N,
                            int32_t* counts, int32_t* mask, int32_t* selection, int32_t* flags, mpStream_t stream);
int mp_scaler_fit_ws_bytes(int64_t G, int S, size_t* bytes_out_host);
int mp_scaler_normal_f64(const int32_t* counts, const int32_t* selection, int64_t G, const void* y, int y_kind, int S,
                         const double* sample_weight, double alpha, int fit_intercept, double* A, double* b,
                         double* mean, void* ws, size_t ws_bytes, mpStream_t stream);
int mp_scaler_solve_f64(const double* A, const double* b, const double* mean, const int32_t* selection, int S,
                        int fit_intercept, double* coef, double* intercept, double* table, int32_t* status,
                        mpStream_t stream);
int mp_scaler_residual_std_f64(const int32_t* counts, const int32_t* selection, int64_t G, const void* y, int y_kind,
                               int S, const double* coef, const double* intercept, int standardize, double* scale,
                               void* ws, size_t ws_bytes, mpStream_t stream);
int mp_scaler_apply(const void* numbers, int number_kind, const int64_t* node_splits, int64_t G, int64_t N, int S,
                    int inverse, const double* table, const int32_t* present, const double* intercept,
                    const double* scale, const void* energy_in, int energy_in_kind, void* energy_out,
                    int energy_out_kind, const float* force_in, float* force_out, double* offset_out, int32_t* flags,
                    mpStream_t stream);

/* ---------------------------------------------------------------- MEGAN: fused importance readout and its reverse --- */
/* csrc/mp_megan.hip.  The tail of kgcnn/literature/MEGAN.py:274-308 behind the last attention layer: the sum of the
 * layers' attention logits and its sigmoid (edge importances), the two mean pools over the index columns and their
 * average (PoolingLocalEdges pooling_index 0 and 1, LazyAverage), the sigmoid of the node-importance Dense chain and
 * the multiply (node importances), and the K weighted graph pools with their concatenation.  K channels, 1 <= K <=
 * MP_MEGAN_MAX_CHANNELS; all float32; no atomics, every sum in an order fixed by the inputs (equal bits on every run
 * and stream); no host read-back, no scratch.
 *
 * mp_megan_edge_importance_f32: ei[e,k] = sigmoid(sum_l logits_l[e,k]) over L (M, K) tensors, 1 <= L <=
 *   MP_MEGAN_MAX_LAYERS, summed in layer order; logits_host is a HOST array of L device pointers (copied into the
 *   kernel argument, as mp_gat_logits_f32's groups).  ei (M, K).  M = 0 returns MP_OK without a launch.
 * mp_megan_readout_f32: with ptr0 / perm0 and ptr1 / perm1 the CSR offsets (N + 1) and stable sorts (M, nullable = the
 *   column is sorted) of index columns 0 and 1,
 *     p[n,k]  = 0.5 (mean of ei[e,k] over list 0 of n + mean of ei[e,k] over list 1 of n), lists walked in list order,
 *               an empty list gives 0;
 *     ni[n,k] = sigmoid(z[n,k]) p[n,k],   z (N, K) the linear output of the last node-importance Dense;
 *     out[b, k W + f] = pool_op (MP_SUM / MP_MEAN) over the nodes [splits[b], splits[b+1]) in node order of
 *               ni[n,k] x[n,f];   x (N, W), W a multiple of 4 up to MP_MEGAN_MAX_WIDTH, x and out 16-byte aligned.
 *   Writes ni (N, K), out (G, K W) (every row: a graph without nodes gets zeros; the host trims trailing empty graphs)
 *   and, when non-null, p (N, K) for the reverse.  One wave per graph, tiles of MP_MEGAN_NODE_TILE nodes; x is read
 *   once.  G = 0 returns MP_OK without a launch.
 * mp_megan_readout_grad_f32: the reverse of the readout for g_out (G, K W) and a nullable g_ni (N, K), with
 *   s = 1 (MP_SUM) or 1 / nodes of the graph (MP_MEAN):
 *     x_bar[n,f] = s sum_k ni[n,k] g_out[b, k W + f],      t[n,k] = g_ni[n,k] + s sum_f x[n,f] g_out[b, k W + f],
 *     z_bar[n,k] = t p sigma(z) (1 - sigma(z)),            q[n,k] = t sigma(z)      (the gradient of p).
 *   ni is recomputed from z and p.  One wave per node.  N = 0 returns MP_OK without a launch.
 * mp_megan_edge_importance_grad_f32: per edge, with r = cols[0][e], s = cols[1][e] (the index plan's shifted columns,
 *   (2, M)) and deg0 / deg1 the list lengths from the two CSR offsets,
 *     ei_bar = g_ei[e,k] (nullable) + 0.5 q[r,k] / deg0[r] + 0.5 q[s,k] / deg1[s],    s_bar = ei_bar ei (1 - ei):
 *   a gather, not the adjoint scatter.  s_bar (M, K) is the gradient of every layer's logits.  An index outside [0, N)
 *   contributes nothing.  M = 0 returns MP_OK without a launch. */
#define MP_MEGAN_MAX_CHANNELS 8
#define MP_MEGAN_MAX_LAYERS 8
#define MP_MEGAN_MAX_WIDTH 512
#define MP_MEGAN_NODE_TILE 64
int mp_megan_edge_importance_f32(int L, const float* const* logits_host, int64_t M, int K, float* ei, mpStream_t stream);
int mp_megan_readout_f32(const float* ei, int64_t M, int K, const int32_t* ptr0, const int32_t* perm0,
                         const int32_t* ptr1, const int32_t* perm1, const float* z, const float* x, int64_t N, int64_t W,
                         const int64_t* splits, int64_t G, int pool_op, float* p, float* ni, float* out,
                         mpStream_t stream);
int mp_megan_readout_grad_f32(const float* g_out, const float* g_ni, const float* x, const float* z, const float* p,
                              int64_t N, int K, int64_t W, const int64_t* splits, int64_t G, int pool_op, float* x_bar,
                              float* z_bar, float* q, mpStream_t stream);
int mp_megan_edge_importance_grad_f32(const float* g_ei, const float* q, const float* ei, const int32_t* cols,
                                      const int32_t* ptr0, const int32_t* ptr1, int64_t N, int64_t M, int K, float* s_bar,
                                      mpStream_t stream);

/* ---------------------------------------------------------------- MAT: all-pairs molecule attention on ragged rows --- */
/* csrc/mp_mat.hip.  One or several attention heads of kgcnn/layers/conv/mat_conv.py:137-178 (MATAttentionHead) without
 * the padded (batch, Nmax, Nmax, units) tensors, the masks, the dense distance matrix (MATDistanceMatrix) and the dense
 * adjacency (CastEdgeIndicesToDenseAdjacency): every atom attends to every atom of its molecule.  Rows are the atoms of
 * the batch; C = H * U channels, head h owns columns [h U, (h+1) U); mol(i) = the rows [node_splits[g], node_splits[g+1])
 * of i's molecule; d2(i,j) = (dx^2 + dy^2) + dz^2 of xyz[i] - xyz[j]:
 *     att_c(i,j) = softmax over j in mol(i) of q[i,c] sqrt(U) k[j,c]                 (per channel c)
 *     dist(i,j)  = MP_MAT_TRAFO_EXP: exp(-d2);  MP_MAT_TRAFO_SOFTMAX: softmax over j in mol(i) of d2;  MP_MAT_TRAFO_NONE: d2
 *     y[i,c] = lambda_attention sum_j att_c(i,j) v[j,c] + lambda_distance sum_j dist(i,j) v[j,c]
 *            + lambda_adjacency (sum over edges e with receiver i of w[e] v[send[e], c] + (add_identity ? v[i,c] : 0))
 *   q, k, v: (N, C) row-major with leading dimensions ldq, ldk, ldv >= C in floats (column blocks of one packed (N, 3C)
 *   product pass without copies); xyz (N, 3); ptr0 (N + 1) / perm0 (M, nullable = the receiver column is sorted): the index
 *   plan's receiver CSR, walked in list order; send (M) the shifted sender column; w (M) one weight per edge.  Duplicate
 *   edges add, self loops count.  A sender outside [0, N) is clamped and MP_FLAG_OOB is raised in *flags (nullable).
 *   The maximum under every exponential is exact (min / max of k per channel and molecule; row maximum of d2): scores
 *   of any size stay finite, q = 0 gives the uniform distribution, a molecule of one atom att = 1.
 *   One workgroup per (molecule, MP_MAT_RECV_TILE receivers), senders streamed through LDS MP_MAT_SEND_TILE at a time: no
 *   cap on the molecule size, molecules without atoms are skipped.  Any U >= 1.  Every row of a molecule is written, also
 *   without edges.  No atomics on data, sums in an order fixed by the inputs: equal bits on every call and stream.
 *   N = 0 or G = 0 returns MP_OK without a launch.
 * Without Wm: out (N, C) = y;  E, merge and h are ignored (h must be null).
 * With Wm (the merge epilogue; y is never written): out (N, E) = h (N, E, nullable) + y @ Wm for MP_MAT_MERGE_CONCAT,
 *   Wm (C, E);  = h + (sum over heads of y[:, h U : (h+1) U]) @ Wm for MP_MAT_MERGE_SUM, Wm (U, E).  Served:
 *   U a multiple of 4 (the product walks the channels four at a time and a group must not straddle two heads),
 *   C <= MP_MAT_EPILOGUE_MAX_CHANNELS and 1 <= E <= MP_MAT_EPILOGUE_MAX_WIDTH; anything else is MP_EINVAL.  out must not
 *   alias q, k or v. */
#define MP_MAT_RECV_TILE 16
#define MP_MAT_SEND_TILE 64
#define MP_MAT_TRAFO_NONE 0
#define MP_MAT_TRAFO_EXP 1
#define MP_MAT_TRAFO_SOFTMAX 2
#define MP_MAT_MERGE_CONCAT 0
#define MP_MAT_MERGE_SUM 1
#define MP_MAT_EPILOGUE_MAX_CHANNELS 256
#define MP_MAT_EPILOGUE_MAX_WIDTH 256
int mp_mat_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, int64_t N,
                         int H, int U, const float* xyz, const int64_t* node_splits, int64_t G, const int32_t* ptr0,
                         const int32_t* perm0, const int32_t* send, const float* w, int64_t M, int trafo,
                         float lambda_attention, float lambda_distance, float lambda_adjacency, int add_identity,
                         const float* Wm, int64_t E, int merge, const float* h, float* out, int32_t* flags,
                         mpStream_t stream);

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
#endif /* MPENGINE_H */
