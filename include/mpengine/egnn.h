/*
 * mpengine/egnn.h - EGNN.
 * Defined in csrc/: mp_egnn.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_EGNN_H
#define MPENGINE_EGNN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_EGNN_H */
