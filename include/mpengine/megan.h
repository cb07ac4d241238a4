/*
 * mpengine/megan.h - MEGAN.
 * Defined in csrc/: mp_megan.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_MEGAN_H
#define MPENGINE_MEGAN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_MEGAN_H */
