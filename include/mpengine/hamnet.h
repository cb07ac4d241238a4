/*
 * mpengine/hamnet.h - HamNet.
 * Defined in csrc/: mp_hamnet.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_HAMNET_H
#define MPENGINE_HAMNET_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- HamNet: dynamic message step, fingerprint -------- */
/* csrc/mp_hamnet.hip, which states the algebra (kgcnn/layers/conv/hamnet_conv.py:508-528 HamNaiveDynMessage.call,
 * :194-207 HamNetGlobalReadoutAttend.call, :358-368 HamNetFingerprintGenerator.call).
 *
 * mp_hamnet_edge_f32 replaces the three gathers, both LazySubtract, both LazyConcatenate, dense_align and dense_e
 *   (hamnet_conv.py:512-526) behind the node-side products, over receiver-sorted positions p (edge e = perm0[p],
 *   u = cols[0][e] the receiver, v = cols[1][e], d_e = [p_v - p_u || q_v - q_u] formed per edge from the rows of p, q
 *   (N, C)):
 *     logit[p] = w_align[:2C] . d_e + w_align[2C:] . he_e + b_align      float64 accumulator, rounded once
 *     me[e]    = act(A[u] + d_e Wd + B[v] + b_e)                         only when me is not null
 *   A, B (N, UE) = h W_e[:F], h W_e[F + 2C:]; Wd (2C, UE) = rows F .. F + 2C of dense_e.kernel, read in place; he (E, D);
 *   w_align (2C + D); b_align (1), b_e (UE) nullable.  logit (E) is written in POSITION order, me (E, UE) in EDGE order;
 *   they are the only edge-sized tensors written.  With me null, A, B, Wd and b_e are not read.  A position whose edge
 *   id, receiver or sender is out of range gets a zero logit.  1 <= C <= 8; D, UE multiples of 4 up to 256; the feature
 *   rows 16-byte aligned (MP_EINVAL otherwise).  E = 0 needs no device.
 * mp_hamnet_attend_f32 replaces dense_attend's gather, pool_attention and final_activ (hamnet_conv.py:518-523):
 *   out[r] = act_last(sum_p softmax_p(logit[p]) T[v_p]) over the positions [ptr0[r], ptr0[r + 1]), T (N, U) =
 *   act(h W_att + b), the segment maximum subtracted before every exponential; out (N, U), every row written, a receiver
 *   without edges gets act_last(0).  One wave per receiver, the sweeps of mp_afp_attend_f32 at a run-time width: U a
 *   multiple of 4 up to 256.  N = 0 needs no device.
 * mp_hamnet_fingerprint_f32: HamNetFingerprintGenerator.call (hamnet_conv.py:358-368) behind its Dense launches
 *   (M = act(h W_v2m + b) (n_nodes, U), T_i = act(h W_att,i + b_i) (n_nodes, UA)), the loop over `depth` inside one launch:
 *   s_g = pool_op (MP_SUM / MP_MEAN) of the graph's rows of M; per iteration i  a_n = w_i . [s_g || h_n] + b_i (float64,
 *   rounded once), m_g = act_attend(sum_n softmax_n(a_n) T_i[n]), s_g = act(GRUCell_i(m_g, s_g)) with K_i (UA, 3U), R_i
 *   (U, 3U), b_in_i, b_rec_i (3U) nullable, gates [z | r | h], the combine of mp_gru_combine_f32.  h (n_nodes, F); w_i
 *   (U + F); b_i (1) nullable.  The `*_host` arguments are HOST arrays of `depth` device pointers, copied into the
 *   kernel argument (as mp_gat_logits_f32's); b_host, b_in_host, b_rec_host may be null or hold nulls.  node_term:
 *   workspace of n_nodes doubles; out (G, U); a graph without nodes starts from 0 and runs the recurrence on
 *   act_attend(0).  F, U, UA multiples of 4 up to 256, 0 <= depth <= MP_HAMNET_MAX_DEPTH.  A workgroup carries 16 graphs.
 *   G = 0 needs no device.
 * All three: no float atomics, equal bits on every run and stream, no host read-back; forward only. */
#define MP_HAMNET_MAX_DEPTH 8
#define MP_HAMNET_MAX_WIDTH 256
#define MP_HAMNET_MAX_COORDS 8
int mp_hamnet_edge_f32(const float* A, const float* B, int64_t N, int UE, const float* p, const float* q, int C,
                       const float* he, int D, const float* w_align, const float* b_align, const float* Wd,
                       const float* b_e, const int32_t* cols, int64_t E, const int32_t* perm0, int act, float alpha,
                       float* logit, float* me, mpStream_t stream);
int mp_hamnet_attend_f32(int U, const float* T, const float* logit, int64_t N, const int32_t* cols, int64_t E,
                         const int32_t* ptr0, const int32_t* perm0, int act_last, float alpha, float* out,
                         mpStream_t stream);
int mp_hamnet_fingerprint_f32(const float* h, const float* M, int64_t n_nodes, const int64_t* row_splits, int64_t G,
                              int F, int U, int UA, int depth, int pool_op, const float* const* T_host,
                              const float* const* w_host, const float* const* b_host, const float* const* K_host,
                              const float* const* R_host, const float* const* b_in_host,
                              const float* const* b_rec_host, int act, float alpha, int act_attend, int gru_act,
                              int rec_act, double* node_term, float* out, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_HAMNET_H */
