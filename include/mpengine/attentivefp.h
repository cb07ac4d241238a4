/*
 * mpengine/attentivefp.h - AttentiveFP.
 * Defined in csrc/: mp_attentivefp.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_ATTENTIVEFP_H
#define MPENGINE_ATTENTIVEFP_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_ATTENTIVEFP_H */
