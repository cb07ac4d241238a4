/*
 * mpengine/chain.h - Dense chains on 16-row tiles, pooled MLP readout.
 * Defined in csrc/: mp_chain.hip, mp_readout.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_CHAIN_H
#define MPENGINE_CHAIN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- Dense chains on 16-row tiles ------------ */
/* One or two Keras Dense layers back to back (kgcnn/layers/modules.py:74-87; PAiNNconv / PAiNNUpdate's
 * Dense(units, act) -> Dense(3 units), kgcnn/layers/conv/painn_conv.py:60-62,187-189, and their reverse forms) in one
 * launch, weights in registers, the 128-wide intermediate in LDS - the latency-bound regime of molecular batches:
 *   m = x W1 + b1 ; [save_pre <- m] ; m = act1(m)        or, with grad_pre:  m = (x W1 + b1) * act1'(grad_pre)
 *   out = m W2 + b2 + addend                              W2_packed null: out = m + addend (U1 columns)
 * K1 in {128,256,384}; two stages: U1 = 128, U2 in {128,256,384}; one stage: U1 in {128,256,384}.  W*_packed are
 * mp_chain_pack_f32 images of the Keras kernels (K, U).  addend may alias out.  mp_chain_supported: 1 if built. */
int mp_chain_supported(int K1, int U1, int U2);
int mp_chain_pack_f32(const float* W, int K, int U, float* packed, mpStream_t stream);
int mp_dense_chain_f32(const float* x, int64_t R, int K1, const float* W1_packed, const float* b1, int U1, int act1,
                       float alpha1, float* save_pre, const float* grad_pre, const float* W2_packed, const float* b2,
                       int U2, const float* addend, float* out, mpStream_t stream);

/* Graph readout in one launch: PoolingNodes(sum) over x (N,K) (kgcnn/layers/pooling.py:215-218) followed by the
 * two-layer output MLP Dense(H, act0) -> Dense(1, linear) (kgcnn/literature/PAiNN.py:146-147): out (G,1).  g_x (nullable,
 * (N,K)): also the reverse of this readout, dE_g/dx_n = W0 (W1 * act0'(pre_g)) written to every node row of graph g
 * (what tape.gradient yields there, kgcnn/model/force.py:159-177).  K, H in {64, 128}. */
int mp_pool_mlp2_f32(const float* x, const int64_t* node_splits, int64_t G, int K, const float* W0, const float* b0, int H,
                     int act0, float alpha0, const float* W1, const float* b1, float* out, float* g_x, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_CHAIN_H */
