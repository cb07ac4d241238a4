/*
 * mpengine/wgrad.h - parameter gradients.
 * Defined in csrc/: mp_wgrad.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_WGRAD_H
#define MPENGINE_WGRAD_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- parameter gradients (training) ------- */
/* What the Keras tape computes for the weights under model.fit (kgcnn/layers/modules.py:15-90 Dense, :526-534
 * Embedding; training/train_qm.py:164-166, training/train_citation.py:102-110).  csrc/mp_wgrad.hip.
 *
 * mp_dense_wgrad_f32: dW (K,U) = x^T g and, if db is not NULL, db (U) = sum_r g[r], over the R rows of x (R,K) and
 * g (R,U); FP32 MFMA with the row index as the reduction dimension.  The rows are cut into chunks (a function of R, K, U
 * only) whose partial products land in ws (mp_dense_wgrad_ws_bytes; 0 bytes when one chunk suffices) and are added in
 * chunk order by a second launch: deterministic, no atomics.  R = 0 writes zeros. */
int mp_dense_wgrad_ws_bytes(int64_t R, int64_t K, int64_t U, size_t* bytes_out_host);
int mp_dense_wgrad_f32(const float* x, int64_t R, int64_t K, const float* g, int64_t U, float* dw, float* db, void* ws,
                       size_t ws_bytes, mpStream_t stream);
/* Embedding table gradient: table_grad[t] (vocab,dim) = sum over i with int32(numbers[i]) = t of g[i] (N,dim), added in
 * node order for each t (stable sort by type + CSR + mp_segment_reduce_csr_f32); numbers outside [0, vocab) - zero
 * rows in mp_embedding_f32 - contribute nothing.  N = 0 writes zeros.  ws from mp_embedding_grad_ws_bytes. */
int mp_embedding_grad_ws_bytes(int64_t N, int64_t vocab, size_t* bytes_out_host);
int mp_embedding_grad_f32(const float* numbers, int64_t N, const float* g, int64_t vocab, int64_t dim, void* ws,
                          size_t ws_bytes, float* table_grad, mpStream_t stream);
/* Reverse of mp_softmax_rows_f32 from its output y: out (R,C) = y * (g - rowsum(g * y)). */
int mp_softmax_rows_grad_f32(const float* y, const float* g, int64_t R, int64_t C, float* out, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_WGRAD_H */
