/*
 * mpengine/rgcn.h - RGCN / GNNFilm.
 * Defined in csrc/: mp_rgcn.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_RGCN_H
#define MPENGINE_RGCN_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- RGCN / GNNFilm: fused relational message step ---- */
/* csrc/mp_rgcn.hip.  One block of kgcnn/literature/RGCN.py:96-103 (GatherNodesOutgoing, Dense, RelationalDense,
 * LazyMultiply, PoolingLocalMessages, LazyAdd, Activation) or of kgcnn/literature/GNNFilm.py:93-102
 * (GatherNodesSelection, three RelationalDense, LazyMultiply, LazyAdd, PoolingLocalMessages, Activation) in one launch,
 * for a LINEAR message RelationalDense: the sum over a receiver's edges is taken in front of the per-relation product.
 *   MP_RELCONV_RGCN:  out[i] = act( sum_q A_iq W[q] + s_i b + act0(nodes[i] W0 + b0) ),
 *                     A_iq = sum_{e -> i, rel[e] = q} weights[e] nodes[send e],  s_i = sum_{e -> i} weights[e]
 *   MP_RELCONV_FILM:  out[i] = act( sum_q [ g_iq * (A_iq W[q] + c_iq b) + c_iq t_iq ] ),  A unweighted, c_iq its edge count,
 *                     g_iq = act_m(nodes[i] Wg[q] + bg),  t_iq = act_m(nodes[i] Wt[q] + bt)
 * nodes (N, K); cols = the index plan's shifted int32 columns (2, E), receiver first; ptr0 (N+1) / perm0 (nullable) =
 * CSR and stable sort of the receiver column; rel (E) int64; weights (E) nullable (ones; RGCN only); W, Wg, Wt
 * (R, K, U) effective kernels; W0 (K, U); every bias (U) nullable; out (N, U), every row written: a receiver without
 * edges gets act(act0(n W0 + b0)) (RGCN) or act(0) (FiLM).  A relation outside [0, R) uses a zero kernel as
 * mp_relational_dense_f32 does (RGCN: the edge adds weights[e] b; FiLM: b * act_m(bg) + act_m(bt)); a position whose
 * edge id or sender is out of range is skipped.  K and U each in {32, 64, 128}, 1 <= R <= MP_RELCONV_MAX_RELATIONS
 * (MP_EINVAL otherwise).  One workgroup owns 16 consecutive receivers and all of their positions, staged 256 at a time;
 * the relations present are dealt to its four waves, whose sums are added in wave order: no workspace, no float atomics,
 * a fixed summation order (per wave: chunk ascending, relation ascending, list order within), equal bits on every run.
 * FP32.  N = 0 needs no device; E = 0 writes the no-edge rows.  Forward only. */
enum mp_relconv_mode { MP_RELCONV_RGCN = 0, MP_RELCONV_FILM = 1 };
#define MP_RELCONV_MAX_RELATIONS 64
int mp_relational_conv_f32(int mode, const float* nodes, int64_t N, int64_t K, const int32_t* cols, int64_t E,
                           const int32_t* ptr0, const int32_t* perm0, const int64_t* rel, const float* weights,
                           int64_t R, const float* W, const float* b, int64_t U, const float* W0, const float* b0,
                           int act0, const float* Wg, const float* bg, const float* Wt, const float* bt, int act_m,
                           int act, float alpha, float* out, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_RGCN_H */
