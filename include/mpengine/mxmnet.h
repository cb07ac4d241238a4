/*
 * mpengine/mxmnet.h - MXMNet: the multiplex edge message with its two epilogues, the triplet pool, and their reverses.
 * Defined in csrc/: mp_mxmnet.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_MXMNET_H
#define MPENGINE_MXMNET_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- MXMNet: multiplex edge message ------------------- */
/* The message of MXMGlobalMP.propagate (kgcnn/layers/conv/mxmnet_conv.py:38-53: gather both ends, concatenate with the
 * edge attributes, Dense with activation, a bias-free Dense on the attributes, their product, the pool and the add), and
 * of MXMLocalMP's mlp_kj x lin_rbf1 (:139-144) and mlp_ji_1 (:150).  The Dense on [x_i || x_j || a] is linear in its three
 * row blocks, so per edge e = (i_e, j_e), with cols (2, E) int32 = column 0 | column 1 of the index plan:
 *     z_e = Pa[i_e] + Pb[j_e] + a_e Wc + b,    y_e = act(z_e) * (a_e Wl)        (no Wl: y_e = act(z_e)).
 * Pa = x W[0:F], Pb = x W[F:2F] (N, W) are node-sized Dense launches of the caller, Wc (Ka, W) = W[2F:2F+Ka] and
 * Wl (Ka, W) row-major, b (W) nullable.
 *
 * mp_mxm_edge_f32, two epilogues:
 *   out != NULL (pool): out (N, W) = base + red over {e : i_e = r} of y_e, red the sum (MP_SUM) or mean (MP_MEAN) over the
 *     sorted positions [ptr0[r], ptr0[r+1]) in list order (position p is edge perm0[p], or p with perm0 NULL); base (N, W)
 *     nullable; a receiver without edges gets base, or 0.  Nothing edge-sized is written.  ws: (tiles, 2, W) floats
 *     (mp_mxm_edge_ws_bytes) for receivers cut by a tile boundary, added in tile order by a node-sized finishing kernel.
 *   y != NULL (edge): y (E, W) in list order; ptr0, perm0, base, ws are not read.
 *   Exactly one of out and y is given.  z_save (E, W), l_save (E, W), both nullable, receive z_e and a_e Wl in list order
 *   for the reverse (l_save needs Wl).
 *   One workgroup of 2 W threads walks tiles of 32 positions; a_e [Wc | Wl] runs on v_mfma_f32_32x32x2_f32 with the wave's
 *   32 columns of both kernels resident in registers, the gathered rows are added in the accumulator layout, W threads
 *   add the tile's rows per receiver in list order (csrc/mp_edge_tile.h).  No float atomics: equal bits on every run and
 *   stream.  W in {32, 64, 128}, 1 <= Ka <= 128, act an MP_ACT_* code, anything else MP_EINVAL.  Both ends of
 *   every edge must lie in [0, N) (the index plan validates them); the kernels follow no index outside that range and
 *   give such an edge a zero row.
 * mp_mxm_edge_grad_f32: the reverse from z_save and l_save.  g is the upstream of out (N, W) with pooled != 0 (MP_MEAN
 *   divides by the receiver's count ptr0[r+1] - ptr0[r]) or of y (E, W) with pooled == 0 (pool_op, ptr0 not read):
 *     z_bar[e] = g_e * l_e * act'(z_e)   (E, W) list order,      l_bar[e] = g_e * act(z_e),
 *     a_bar (E, Ka) = z_bar Wc^T + l_bar Wl^T  on the matrix pipe; nullable, then only z_bar is written.
 *   Pa_bar / Pb_bar are mp_segment_reduce_csr_f32 sums of z_bar over the CSRs of columns 0 / 1 (the caller).
 * All: N = 0 or (edge epilogue / reverse) E = 0 returns MP_OK without touching the device; N and E are indexed with
 * 32 bits (N < 2^31 - 1, E < 2^31 - 32). */
int mp_mxm_edge_ws_bytes(int64_t E, int W, size_t* bytes_out_host);
int mp_mxm_edge_f32(const float* Pa, const float* Pb, int64_t N, int W, const float* a, int Ka, const float* Wc,
                    const float* Wl, const float* b, const int32_t* cols, int64_t E, const int32_t* ptr0,
                    const int32_t* perm0, int act, float alpha, int pool_op, const float* base, float* ws, size_t ws_bytes,
                    float* z_save, float* l_save, float* out, float* y, mpStream_t stream);
int mp_mxm_edge_grad_f32(const float* g, int pooled, int64_t N, int W, int Ka, const float* Wc, const float* Wl,
                         const int32_t* cols, int64_t E, const int32_t* ptr0, int act, float alpha, int pool_op,
                         const float* z_save, const float* l_save, float* z_bar, float* a_bar, mpStream_t stream);

/* ---------------------------------------------------------------- MXMNet: triplet pool ------------------------------ */
/* The triplet step of MXMLocalMP (kgcnn/layers/conv/mxmnet_conv.py:145-148 and :158-161: GatherNodesOutgoing by angle
 * column 1, LazyMultiply with the mlp_sbf output, PoolingLocalMessages into angle column 0) in one pass:
 *     out[n] (E, W) = red over {t : A[t,0] = n} of x[A[t,1]] * s[t],
 * x (E, W) edge messages, s (T, W), cols (2, T) int32 = angle column 0 | column 1, ptr0 (E+1) / perm0 (nullable) the CSR of
 * column 0 over sorted positions, red the sum (MP_SUM) or mean (MP_MEAN), in list order; an edge without triplets gets a
 * zero row.  One thread per (edge, column); nothing triplet-sized is written; any W >= 1.  A triplet whose column 1 lies
 * outside [0, E) adds an exact 0.
 * mp_mxm_triplet_grad_f32: x_bar[m] (E, W) = sum over {t : A[t,1] = m} of g[A[t,0]] * s[t] (x 1/count of A[t,0] for
 *   MP_MEAN) over the CSR ptr1 / perm1 of column 1 in list order; s_bar[t] (T, W) = g[A[t,0]] * x[A[t,1]] likewise scaled.
 *   Either output nullable; ptr0 gives the counts of the mean.
 * E = 0 returns MP_OK without touching the device; T = 0 zeroes out / x_bar. */
int mp_mxm_triplet_f32(const float* x, int64_t E, int W, const float* s, const int32_t* cols, int64_t T,
                       const int32_t* ptr0, const int32_t* perm0, int pool_op, float* out, mpStream_t stream);
int mp_mxm_triplet_grad_f32(const float* x, int64_t E, int W, const float* s, const int32_t* cols, int64_t T,
                            const int32_t* ptr0, const int32_t* ptr1, const int32_t* perm1, int pool_op, const float* g,
                            float* x_bar, float* s_bar, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_MXMNET_H */
