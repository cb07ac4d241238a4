/*
 * mpengine/dimenet.h - DimeNet++.
 * Defined in csrc/: mp_dimenet.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_DIMENET_H
#define MPENGINE_DIMENET_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_DIMENET_H */
