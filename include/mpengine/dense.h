/*
 * mpengine/dense.h - Dense, activations, layer normalisation, broadcasting and column-block ops.
 * Defined in csrc/: mp_dense.hip, mp_elementwise.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_DENSE_H
#define MPENGINE_DENSE_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- dense / elementwise -------------------- */
/* Keras Dense on flat values, kgcnn/layers/modules.py:85: out = act(x @ W + b); x (R,K), W (K,U) row-major
 * ("kernel" layout), b (U) nullable.  FP32 MFMA (v_mfma_f32_32x32x2_f32), k-ordered fma chain. */
int mp_dense_f32(const float* x, int64_t R, int64_t K, const float* W, const float* b, int64_t U, int act,
                 float act_alpha, float* out, mpStream_t stream);

/* Dense with a fused prologue / epilogue, for chains of Dense layers and their reverse pass (PAiNNconv / PAiNNUpdate,
 * kgcnn/layers/conv/painn_conv.py:98-99, 206-207; EnergyForceModel's tape, kgcnn/model/force.py:159-177):
 * in_mode 0: as mp_dense_f32; 1: x := in_act(x) while staging (x is a saved pre-activation); 2: x := x * in_act'(in_pre)
 * (in_pre (R,K): the reverse pass through an activation, fused into the GEMM with the transposed kernel).
 * Epilogue, in this order: out_pre (R,U) nullable receives the pre-activation x W + b; the result act(x W + b) is
 * multiplied by in_act'(grad_pre) if grad_pre (R,U) is given (the activation derivative applied where the upstream
 * gradient is produced); addend (R,U) nullable, may alias out, is added last. */
int mp_dense_ex_f32(const float* x, int64_t R, int64_t K, const float* W, const float* b, int64_t U, int act,
                    float act_alpha, int in_mode, int in_act, float in_alpha, const float* in_pre, const float* addend,
                    float* out_pre, const float* grad_pre, float* out, mpStream_t stream);

/* mp_dense_f32 for few output tiles and a long contraction (GCN's first layer, kgcnn/literature/GCN.py:95:
 * (2708,1433) x (1433,64) = 43 tiles of 64x64 for 256 CUs): the k range is cut into `splits` slices computed by separate
 * workgroups into the workspace (splits * R * U floats), a second kernel adds the slices in order and applies bias and
 * activation - deterministic, no atomics. */
int mp_dense_splitk_workspace_bytes(int64_t R, int64_t U, int splits, size_t* bytes_out_host);
int mp_dense_splitk_f32(const float* x, int64_t R, int64_t K, const float* W, const float* b, int64_t U, int act,
                        float act_alpha, int splits, void* ws, size_t ws_bytes, float* out, mpStream_t stream);

int mp_activation_f32(int act, float act_alpha, const float* x, int64_t n, float* out, mpStream_t stream);
int mp_softmax_rows_f32(const float* x, int64_t R, int64_t C, float* out, mpStream_t stream);

/* GraphLayerNormalization over the last axis of the values (kgcnn/layers/norm.py:8-110 = Keras LayerNormalization):
 * out = (x - mean_row) * rsqrt(var_row + epsilon) * gamma + beta, biased variance; gamma / beta (C) nullable. */
int mp_layer_norm_f32(const float* x, int64_t R, int64_t C, const float* gamma, const float* beta, float epsilon,
                      float* out, mpStream_t stream);

/* Broadcasting binary op on (R, D1, D2) views: operand strides in elements, 0 = broadcast
 * (LazyAdd/LazySubtract/LazyMultiply of kgcnn/layers/modules.py:187-301, incl. PaiNN's (M,1,F)*(M,3,F)). */
int mp_binary_f32(int op, const float* a, const int64_t* a_strides_host, const float* b, const int64_t* b_strides_host,
                  int64_t R, int64_t D1, int64_t D2, float* out, mpStream_t stream);

/* Strided 2-D column-block copy: dst[r*dst_ld + dst_off + c] = src[r*src_ld + src_off + c], c < C
 * (LazyConcatenate modules.py:305-364 and SplitEmbedding painn_conv.py:329-340 on values). */
int mp_copy_cols_f32(const float* src, int64_t src_ld, int64_t src_off, float* dst, int64_t dst_ld, int64_t dst_off,
                     int64_t R, int64_t C, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_DENSE_H */
