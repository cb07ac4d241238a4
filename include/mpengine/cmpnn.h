/*
 * mpengine/cmpnn.h - CMPNN.
 * Defined in csrc/: mp_cmpnn.hip, mp_recurrent.hip (mp_gru_ragged_last_f32).
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_CMPNN_H
#define MPENGINE_CMPNN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_CMPNN_H */
