/*
 * mpengine/gat.h - GAT / GATv2.
 * Defined in csrc/: mp_gat.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_GAT_H
#define MPENGINE_GAT_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_GAT_H */
