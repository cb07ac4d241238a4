/*
 * mpengine/mat.h - MAT.
 * Defined in csrc/: mp_mat.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_MAT_H
#define MPENGINE_MAT_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- MAT: all-pairs molecule attention on ragged rows --- */
/* csrc/mp_mat.hip.  One or several attention heads of kgcnn/layers/conv/mat_conv.py:137-178 (MATAttentionHead) without
 * the padded (batch, Nmax, Nmax, units) tensors, the masks, the dense distance matrix (MATDistanceMatrix) and the dense
 * adjacency (CastEdgeIndicesToDenseAdjacency): every atom attends to every atom of its molecule.  Rows are the atoms of
 * the batch; C = H * U channels, head h owns columns [h U, (h+1) U); mol(i) = the rows [node_splits[g], node_splits[g+1])
 * of i's molecule; d2(i,j) = (dx^2 + dy^2) + dz^2 of xyz[i] - xyz[j]:
 *     att_c(i,j) = softmax over j in mol(i) of q[i,c] sqrt(U) k[j,c]                 (per channel c)
 *     dist(i,j)  = MP_MAT_TRAFO_EXP: exp(-d2);  MP_MAT_TRAFO_SOFTMAX: softmax over j in mol(i) of d2;  MP_MAT_TRAFO_NONE: d2
 *     y[i,c] = lambda_attention sum_j att_c(i,j) v[j,c] + lambda_distance sum_j dist(i,j) v[j,c]
 *            + lambda_adjacency (sum over edges e with receiver i of w[e] v[send[e], c] + (add_identity ? v[i,c] : 0))
 *   q, k, v: (N, C) row-major with leading dimensions ldq, ldk, ldv >= C in floats (column blocks of one packed (N, 3C)
 *   product pass without copies); xyz (N, 3); ptr0 (N + 1) / perm0 (M, nullable = the receiver column is sorted): the index
 *   plan's receiver CSR, walked in list order; send (M) the shifted sender column; w (M) one weight per edge.  Duplicate
 *   edges add, self loops count.  A sender outside [0, N) is clamped and MP_FLAG_OOB is raised in *flags (nullable).
 *   The maximum under every exponential is exact (min / max of k per channel and molecule; row maximum of d2): scores
 *   of any size stay finite, q = 0 gives the uniform distribution, a molecule of one atom att = 1.
 *   One workgroup per (molecule, MP_MAT_RECV_TILE receivers), senders streamed through LDS MP_MAT_SEND_TILE at a time: no
 *   cap on the molecule size, molecules without atoms are skipped.  Any U >= 1.  Every row of a molecule is written, also
 *   without edges.  No atomics on data, sums in an order fixed by the inputs: equal bits on every call and stream.
 *   N = 0 or G = 0 returns MP_OK without a launch.
 * Without Wm: out (N, C) = y;  E, merge and h are ignored (h must be null).
 * With Wm (the merge epilogue; y is never written): out (N, E) = h (N, E, nullable) + y @ Wm for MP_MAT_MERGE_CONCAT,
 *   Wm (C, E);  = h + (sum over heads of y[:, h U : (h+1) U]) @ Wm for MP_MAT_MERGE_SUM, Wm (U, E).  Served:
 *   U a multiple of 4 (the product walks the channels four at a time and a group must not straddle two heads),
 *   C <= MP_MAT_EPILOGUE_MAX_CHANNELS and 1 <= E <= MP_MAT_EPILOGUE_MAX_WIDTH; anything else is MP_EINVAL.  out must not
 *   alias q, k or v. */
#define MP_MAT_RECV_TILE 16
#define MP_MAT_SEND_TILE 64
#define MP_MAT_TRAFO_NONE 0
#define MP_MAT_TRAFO_EXP 1
#define MP_MAT_TRAFO_SOFTMAX 2
#define MP_MAT_MERGE_CONCAT 0
#define MP_MAT_MERGE_SUM 1
#define MP_MAT_EPILOGUE_MAX_CHANNELS 256
#define MP_MAT_EPILOGUE_MAX_WIDTH 256
int mp_mat_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, int64_t N,
                         int H, int U, const float* xyz, const int64_t* node_splits, int64_t G, const int32_t* ptr0,
                         const int32_t* perm0, const int32_t* send, const float* w, int64_t M, int trafo,
                         float lambda_attention, float lambda_distance, float lambda_adjacency, int add_identity,
                         const float* Wm, int64_t E, int merge, const float* h, float* out, int32_t* flags,
                         mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_MAT_H */
