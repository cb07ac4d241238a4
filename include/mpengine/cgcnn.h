/*
 * mpengine/cgcnn.h - CGCNN.
 * Defined in csrc/: mp_cgcnn.hip, mp_lattice.hip (mp_frac_to_real_f32).
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_CGCNN_H
#define MPENGINE_CGCNN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_CGCNN_H */
