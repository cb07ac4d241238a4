/*
 * mpengine/backward.h - first and second derivatives of the elementwise steps.
 * Defined in csrc/: mp_backward.hip, mp_backward2.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_BACKWARD_H
#define MPENGINE_BACKWARD_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_BACKWARD_H */
