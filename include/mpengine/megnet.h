/*
 * mpengine/megnet.h - MEGNet.
 * Defined in csrc/: mp_megnet.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_MEGNET_H
#define MPENGINE_MEGNET_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- MEGNet: fused edge step of one block ------------- */
/* MEGNet (csrc/mp_megnet.hip; kgcnn/literature/Megnet.py:24-373).
 *
 * mp_megnet_edge_f32: the edge update of one MEGnetBlock and its pool into the receivers
 *   (kgcnn/layers/conv/megnet_conv.py:96-111) in one launch plus a node-sized finishing pass:
 *     z1[e]   = Pa[cols[0][e]] + Pb[cols[1][e]] + edges[e] Wc + Pu[g(e)]                      (64 wide)
 *     e'[e]   = act(act(z1[e]) W1 + b1) W2 + b2                                                (64 -> 32 -> 32)
 *     pool[r] = mean or sum over {e : cols[0][e] = r} of e'[e]; a receiver without edges gets 0.
 *   Pa, Pb (N, 64) = v W_e[0:Fn], v W_e[Fn:2Fn] and Pu (G, 64) = u W_e[2Fn+Fe:] + b0: the node-side and state-side
 *   products by row blocks of the first edge Dense kernel W_e (2Fn + Fe + Fu, 64), its bias folded into Pu; Wc (Fe, 64)
 *   = W_e[2Fn:2Fn+Fe]; W1 (64, 32), W2 (32, 32) row-major; b1, b2 (32) nullable.  edges (E, Fe); edge_splits = the edge
 *   tensor's int64 row_splits (G+1), from which g(e) is looked up; cols = the index plan's shifted int32 columns
 *   (2, E); ptr0 (N+1) / perm0 (nullable) = CSR and stable sort of column 0.  Served: Fn = Fe = Fu = 32 and units0 /
 *   units1 / units2 = 64 / 32 / 32, act any activation code (mp_dense_f32's epilogue function), pool_op MP_SUM or
 *   MP_MEAN; anything else MP_EINVAL.  edges_out (E, 32) in list order, pool_out (N, 32); ws:
 *   mp_megnet_edge_ws_bytes(E).  Sums run per receiver in list order, a receiver cut by a tile boundary through
 *   per-tile partials added in tile order: deterministic, no float atomics.  No reverse: weights and inputs are
 *   frozen.  N = 0 needs no device; E = 0 zeroes pool_out. */
int mp_megnet_edge_ws_bytes(int64_t E, size_t* bytes_out_host);
int mp_megnet_edge_f32(const float* Pa, const float* Pb, int64_t N, const float* Pu, const int64_t* edge_splits,
                       int64_t G, const float* edges, int Fn, int Fe, int Fu, const int32_t* cols, int64_t E,
                       const int32_t* ptr0, const int32_t* perm0, const float* Wc, const float* W1, const float* b1,
                       const float* W2, const float* b2, int units0, int units1, int units2, int act, float alpha,
                       int pool_op, float* ws, size_t ws_bytes, float* edges_out, float* pool_out, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_MEGNET_H */
