/*
 * mpengine/painn.h - the fused PaiNN path and its reverse pass.
 * Defined in csrc/: mp_painn_fused.hip, mp_chain.hip (mp_painn_update_fused_*).
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_PAINN_H
#define MPENGINE_PAINN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- fused PaiNN path (+ reverse pass) ------ */
/* Stage 0 of kgcnn/literature/PAiNN.py:100-119 in one launch: OptionalInputEmbedding (z0 (N,128)), EquivariantInitialize
 * with a constant (v0 (N,3,128) = v_init), mp_index_prepare_i64 for K = 2 (recv, send, flag word incl. both sortedness
 * bits), NodePosition -> EdgeDirectionNormalized (rij (M,3), geom.py:331-378) -> NodeDistanceEuclidean (dist (M)) ->
 * BesselBasisLayer (rbf (M,B), geom.py:772-785) and, if rbfd != NULL, d rbf / d dist (M,B) for the reverse pass;
 * cos_cutoff > 0 adds CosCutOffEnvelope (env (M), geom.py:831-837) and its derivative envd (nullable). */
int mp_painn_stage0_f32(const void* numbers /* float32, or int64 if numbers_i64 */, int numbers_i64, int64_t N,
                        const float* emb, int vocab, float v_init, float* z0, float* v0,
                        const int64_t* idx, int64_t M, const int64_t* node_splits, const int64_t* edge_splits, int64_t G,
                        const float* xyz, const float* frequencies, int num_radial, float bessel_cutoff,
                        int envelope_exponent, float cos_cutoff, int32_t* recv, int32_t* send, int32_t* flags, float* dist,
                        float* rij, float* rbf, float* rbfd, float* env, float* envd, mpStream_t stream);
/* PAiNNconv.call edge side, kgcnn/layers/conv/painn_conv.py:99-113, fused (F = units = 128, conv_pool = sum):
 * w = rbf Ww + bw [* env]; sw = s[send] * w; ds[i] = sum sw1; dv[i] = sum (sw2 (x) v[send] + sw3 (x) r_ij) over the edges
 * of receiver i in edge order (CSR ptr / perm as mp_segment_reduce_csr_f32).  s (N,3F) = phi(dense1(z)), v (N,3,F),
 * rbf (M,B<=32), env (M)|NULL, rij (M,3), Ww (B,3F), bw (3F)|NULL; writes ds (N,F), dv (N,3,F) incl. zero rows.
 * z_in != NULL fuses the residual adds of PAiNN.py:126-127: ds := z_in + ds, dv := v + dv.  dv must not alias v.
 * Two waves per receiver, four edges in flight per wave, packed FP32 arithmetic. */
int mp_painn_message_f32(const float* s, const float* v, int64_t N, const float* rbf, int B, const float* env,
                         const float* rij, const float* Ww, const float* bw, const int32_t* ptr, const int32_t* perm,
                         const int32_t* send, int64_t M, const float* z_in, float* ds, float* dv, mpStream_t stream);
/* The same message step with node TILES staged in LDS and the filter Dense (painn_conv.py:100, w = Dense(3F)(rbf)) on the
 * matrix pipe (FP32-exact bf16-piece split, csrc/mp_painn_fused.hip): for receiver-sorted edge lists (no perm) of batched
 * graphs.  tiles (T,8) int32 = {r_lo, r_hi, s_lo, s_hi, e_lo, e_hi, 0, 0}: receivers [r_lo, r_hi) (at most 62) of ONE graph
 * whose nodes are [s_lo, s_hi) (<= max_rows: the s / v rows staged) and whose edges are [e_lo, e_hi) = [ptr[r_lo],
 * ptr[r_hi]) (<= max_edges); every receiver must appear in exactly one tile.  wimage: mp_painn_filter_pack_f32 of Ww | bw
 * (MP_PAINN_FILTER_IMAGE_BYTES, rebuilt when the weights change).  LDS per workgroup: mp_painn_message_tiles_lds_bytes
 * (<= 160 KB, else MP_EINVAL).  Results as mp_painn_message_f32 (same accumulation order per receiver). */
#define MP_PAINN_FILTER_IMAGE_BYTES 73728
int mp_painn_filter_pack_f32(const float* Ww, const float* bw, int B, void* image, mpStream_t stream);
int mp_painn_message_tiles_lds_bytes(int max_rows, int max_edges, int B, int with_env, size_t* out);
int mp_painn_message_tiles_f32(const float* s, const float* v, int64_t N, const float* rbf, int B, const float* env,
                               const float* rij, const void* wimage, const int32_t* ptr, const int32_t* send, int64_t M,
                               const int32_t* tiles, int ntiles, int max_rows, int max_edges, const float* z_in, float* ds,
                               float* dv, mpStream_t stream);
/* Reverse pass of the message block (painn_conv.py:99-113) for forces: sender-parallel over the CSR of column 1
 * (ptr1 / perm1).  Given g_ds (N,F) and g_dv (N,3,F): g_s (N,3F) = dE/ds, g_v (N,3,F) = g_dv + dE/dv through the
 * messages (nullable), and per edge dE/dd (through the filter: rbfd = d rbf / d d, envelope by the product rule) and
 * dE/dr_ij, written (accumulate = 0) or added (accumulate = 1, later blocks) to g_d (2,M), g_rij (2,M,3): one slice per
 * half of the feature axis (two waves serve a sender), summed by mp_edge_geometry_bwd_f32 (slices = 2). */
int mp_painn_message_bwd_f32(const float* s, const float* v, int64_t N, const float* rbf, const float* rbfd, int B,
                             const float* env, const float* envd, const float* rij, const float* Ww, const float* bw,
                             const int32_t* ptr1, const int32_t* perm1, const int32_t* recv, int64_t M, const float* g_ds,
                             const float* g_dv, float* g_s, float* g_v, float* g_d, float* g_rij, int accumulate,
                             mpStream_t stream);
/* The same reverse step on SENDER tiles staged in LDS with the filter AND its distance derivative on the matrix pipe (A rows
 * [rbf_e | 1] and [rbf'_e | 0] against the forward kernel's packed image `wimage`): any edge order (the tile's basis rows are
 * gathered through perm1), batched graphs.  tiles (T,8) int32 = {j_lo, j_hi, s_lo, s_hi, e_lo, e_hi, 0, 0}: senders
 * [j_lo, j_hi) (at most max_senders <= 62: their s / v rows are staged too) of ONE graph whose nodes are [s_lo, s_hi)
 * (<= max_rows: the g_ds / g_dv rows staged) and whose
 * edges are the sender-order positions [e_lo, e_hi) = [ptr1[j_lo], ptr1[j_hi]) (<= max_edges); every sender in exactly one
 * tile.  g_d (M), g_rij (M,3): ONE slice (mp_edge_geometry_bwd_f32 with slices = 1), summed over the feature axis in a
 * fixed order inside the kernel.  LDS per workgroup: mp_painn_message_bwd_tiles_lds_bytes (<= 160 KB, else MP_EINVAL). */
int mp_painn_message_bwd_tiles_lds_bytes(int max_rows, int max_senders, int max_edges, int B, int with_env, size_t* out);
int mp_painn_message_bwd_tiles_f32(const float* s, const float* v, int64_t N, const float* rbf, const float* rbfd, int B,
                                   const float* env, const float* envd, const float* rij, const void* wimage,
                                   const int32_t* ptr1, const int32_t* perm1, const int32_t* recv, int64_t M,
                                   const int32_t* tiles, int ntiles, int max_rows, int max_senders, int max_edges,
                                   const float* g_ds, const float* g_dv, float* g_s, float* g_v, float* g_d, float* g_rij,
                                   int accumulate, mpStream_t stream);
/* PAiNNUpdate.call (painn_conv.py:201-214) after the projection uv (3N,2F) = v [Wu | Wv] (rows (n,k)) in ONE launch
 * (csrc/mp_chain.hip): the element-wise steps
 *   pre:  c (N,2F) = [z | EuclideanNorm_k(v_v)], prod (N,F) = ScalarProduct_k(v_u, v_v);
 *   post: z2 = z + prod a_sv + a_ss, v2 = v + a_vv (x) v_u  with a (N,3F) = [a_vv | a_sv | a_ss] (+ PAiNN.py:131-132)
 * as prologue / epilogue of the two-layer chain a = Dense(Dense(c, act)) (W1 (256,128), W2 (128,384) as mp_chain_pack_f32
 * images).  save_pre keeps c Wd + bd; c_out / prod_out / a_out (any may be NULL) receive what the reverse pass reads. */
int mp_painn_update_fused_f32(const float* z, const float* v, const float* uv, int64_t N, const float* W1_packed,
                              const float* b1, int act1, float alpha1, float* save_pre, const float* W2_packed,
                              const float* b2, float* c_out, float* prod_out, float* a_out, float* z2, float* v2,
                              mpStream_t stream);
/* ... and its reverse in one launch: g_a (N,3F), g_prod (N,F) from g_z2, g_v2 (reverse of post) as the prologue,
 * g_z = g_z2 + g_c[:, :F] and g_uv (3N,2F) (reverse of pre) as the epilogue of the chain against the transposed
 * kernels (W1T (384,128) = Wa^T, W2T (128,256) = Wd^T as mp_chain_pack_f32 images; grad_pre = the saved c Wd + bd).
 * g_v2 == NULL: no gradient reaches v'' (the last block of an energy model, whose readout sees z only). */
int mp_painn_update_fused_bwd_f32(const float* g_z2, const float* g_v2, const float* uv, const float* prod, const float* a,
                                  const float* c, int64_t N, const float* W1T_packed, int act1, float alpha1,
                                  const float* grad_pre, const float* W2T_packed, float* g_z, float* g_uv,
                                  mpStream_t stream);
/* Reverse of NodePosition -> EdgeDirectionNormalized / NodeDistanceEuclidean (PAiNN.py:116-118; Schnet.py:116-117 with
 * g_rij = 0): g_xyz[n] = scale * (sum_{recv(e)=n} t_e - sum_{send(e)=n} t_e), t_e = g_d r_ij + (g_rij - (g_rij.r_ij) r_ij)/d,
 * g_d (slices,M) and g_rij (slices,M,3) being partial sums that are added first,
 * over the receiver CSR (ptr0/perm0) and the sender CSR (ptr1/perm1); scale = -1 yields the physical force
 * (kgcnn/model/force.py:188-189). */
int mp_edge_geometry_bwd_f32(const float* g_d, const float* g_rij, int slices, const float* rij, const float* dist,
                             const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                             int64_t N, int64_t M, float scale, float* g_xyz, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_PAINN_H */
