/*
 * mpengine/recurrent.h - LSTM / GRU steps, batched matrix-vector product.
 * Defined in csrc/: mp_recurrent.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_RECURRENT_H
#define MPENGINE_RECURRENT_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_RECURRENT_H */
