/*
 * mpengine/dmpnn.h - DMPNN.
 * Defined in csrc/: mp_dmpnn.hip, mp_wgrad.hip (mp_directed_edge_wgrad_*).
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_DMPNN_H
#define MPENGINE_DMPNN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- DMPNN: reverse of the directed edge update -------- */
/* What the tape computes for one round of kgcnn/literature/DMPNN.py:136-140 (DMPNNPPoolingEdgesDirected,
 * kgcnn/layers/conv/dmpnn_conv.py:83-87; the shared Dense, kgcnn/layers/modules.py:15-90; LazyAdd; Activation) when
 * the round ran as  R = segment sum of h at the receiver,  y = mp_directed_edge_update_f32(h := R, he := h, he0 := h0)
 * with act1 = linear.  csrc/mp_dmpnn.hip, csrc/mp_wgrad.hip.
 *
 * mp_directed_edge_update_grad_f32: the reverse of Activation, LazyAdd and Dense's input side in one launch,
 *     p[e] = g[e] * act2'(y[e]),   q[e] = p[e] W^T.
 *   g, y (the forward output), p, q (E, F); W (F, F) row-major.  act2 is MP_ACT_LINEAR (y is not read, may be NULL) or
 *   MP_ACT_RELU (the derivative is taken from the output: the product g * (y > 0), the bits of the layer sequence);
 *   anything else MP_EINVAL.  p is the gradient of he0 and of the pre-activation, q the gradient of the difference
 *   h[send] - he[rev].  The forward kernel's tiling: MP_CMPNN_EDGE_TILE edges x 64 columns of q per workgroup, FP32 MFMA,
 *   the A tile formed while it is staged, W read by rows; the column tile 0 writes p.  F a multiple of 4, 16-byte aligned
 *   operands; p and q must not overlap g or y.  E = 0 returns MP_OK without a launch.
 * mp_directed_edge_wgrad_f32: the weight side of Dense,
 *     dW (F, F) = sum_e d[e]^T p[e],  db (F, nullable) = sum_e p[e],  d[e] = h[send[e]] - he[rev[e]]  (0 where rev[e] < 0)
 *   with d formed while a row slab is staged and never written.  h (N, F); he, p (E, F).  mp_dense_wgrad_f32's row split,
 *   slabs and in-order reduction as they stand (ws from mp_directed_edge_wgrad_ws_bytes, a function of E and F only).
 *   send outside [0, N) and rev >= E are clamped and OR MP_FLAG_OOB into *flags (nullable).  E = 0 writes zeros.
 * mp_directed_edge_hgrad_f32: the last line of the reverse, the adjoint of the receiver sum (a gather at the receiver)
 *   minus the adjoint of DMPNNGatherEdgesPairs (dmpnn_conv.py:39-46),
 *     out[e] = rbar[recv[e]] - sum_{j in [rev_ptr[e], rev_ptr[e+1])} q[rev_perm[j]],
 *   rbar (N, F) = the segment sum of q over the sender CSR; rev_ptr (E+2) / rev_perm (E, nullable) = CSR and stable sort
 *   of rev with the edges that have no reverse moved to the extra segment E: right for any rev, an involution or not.
 *   Rows are added in CSR order.  recv outside [0, N) is clamped and flagged.
 * All three: no float atomics, equal bits on every run and stream, no host read-back. */
int mp_directed_edge_update_grad_f32(const float* g, const float* y, int64_t E, int64_t F, const float* W, int act2,
                                     float* p, float* q, mpStream_t stream);
int mp_directed_edge_wgrad_ws_bytes(int64_t E, int64_t F, size_t* bytes_out_host);
int mp_directed_edge_wgrad_f32(const float* h, int64_t N, const float* he, int64_t E, int64_t F, const int32_t* send,
                               const int32_t* rev, const float* p, float* dw, float* db, void* ws, size_t ws_bytes,
                               int32_t* flags, mpStream_t stream);
int mp_directed_edge_hgrad_f32(const float* rbar, int64_t N, const float* q, int64_t E, int64_t F, const int32_t* recv,
                               const int32_t* rev_ptr, const int32_t* rev_perm, float* out, int32_t* flags,
                               mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_DMPNN_H */
