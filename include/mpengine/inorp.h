/*
 * mpengine/inorp.h - INorp (Interaction Networks): the folded edge step of one block and its reverse.
 * Defined in csrc/: mp_inorp.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_INORP_H
#define MPENGINE_INORP_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- INorp: folded edge step ---------------------------- */
/* One block of kgcnn/literature/INorp.py:117-127 with a two-layer edge MLP Dense(H1, act) -> Dense(H2, linear):
 *     eu[e]  = act([n[send e] || n[recv e] || edges[e]] W1 + b1) W2 + b2,    nu[r] = pool over {e : recv e = r} of eu[e].
 * The second layer is linear, so it commutes with the pool:
 *     nu[r] = (pool_e act(z1[e])) W2 + c[r] b2,   c = the edge count of r for a sum, [count > 0] for a mean,
 * and the first layer is linear in its three column blocks:
 *     z1[e] = Pj[send e] + Pi[recv e] + edges[e] Wc,   Pj = n W1[0:F],  Pi = n W1[F:2F] + b1,  Wc = W1[2F:2F+Fe].
 * The two node-sized products and the (N, H1) x (H1, H2) product are mp_dense_f32 launches of the caller.
 *
 * mp_inorp_edge_f32: out (N, H1),
 *     h[p] = act((Pj[send] + Pi[recv]) + edges[e] Wc)  at sorted position p (edge e = perm0[p], or p when perm0 is NULL),
 *     out[r] = sum (MP_SUM) or mean (MP_MEAN) of h over the positions [ptr0[r], ptr0[r+1]) in list order; exactly 0 for
 *     a receiver without edges.
 *   Pj, Pi (N, H1); edges (E, Fe); Wc (Fe, H1) row-major; cols (2, E) int32 receivers | senders (the index plan);
 *   ptr0 (N+1) the receivers' CSR over sorted positions.  H1 in {16, 32, 64, 128}, 1 <= Fe <= 64 (the staged rows are
 *   zero-padded to the matrix instruction's k step of 4), act an MP_ACT_* code, anything else MP_EINVAL.
 *   One 256-thread workgroup walks tiles of 32 positions: the edge rows and both gathered rows of a tile are requested
 *   together, edges Wc runs on v_mfma_f32_16x16x4_f32 with Wc resident in registers, H1 threads add the tile's rows per
 *   receiver in list order.  A receiver cut by a tile boundary leaves partial sums in ws (tiles, 2, H1) floats
 *   (mp_inorp_edge_ws_bytes), which a node-sized finishing kernel adds in tile order.  No float atomics: equal bits on
 *   every run and stream.  An edge whose sender lies outside [0, N) is skipped wherever it stands in its receiver's
 *   range: it adds an exact 0 and still counts in the mean's divisor, the range's length; a receiver all of whose
 *   edges are skipped gets 0.  An edge whose receiver lies outside [0, N) is skipped too and must lie in no range of ptr0.
 * mp_inorp_edge_grad_f32: the reverse, with z1 recomputed in the forward's operation order (nothing edge-sized is saved),
 *     gz[e]    = g[recv e] (/ count of recv e for MP_MEAN) * act'(z1[e])     (E, H1), at the edge's LIST position e,
 *     pi_bar[r] = sum of gz over the positions of r, the same walk                (N, H1);
 *   g (N, H1) is the upstream of out.  act' is mp_activation_grad_f32's (relu: 0 at an exact 0).  The rows of skipped
 *   edges are written as zeros.  The same workspace size.
 * All: N = 0 returns MP_OK without touching the device, E = 0 zeroes out / pi_bar; N and E are indexed with 32 bits
 * (N < 2^31 - 1, E < 2^31 - 32), more is MP_EINVAL, as is a workspace shorter than mp_inorp_edge_ws_bytes reports. */
int mp_inorp_edge_ws_bytes(int64_t E, int H1, size_t* bytes_out_host);
int mp_inorp_edge_f32(const float* Pj, const float* Pi, int64_t N, int H1, const float* edges, int Fe, const float* Wc,
                      const int32_t* cols, int64_t E, const int32_t* ptr0, const int32_t* perm0, int act, float alpha,
                      int pool_op, float* ws, size_t ws_bytes, float* out, mpStream_t stream);
int mp_inorp_edge_grad_f32(const float* Pj, const float* Pi, int64_t N, int H1, const float* edges, int Fe,
                           const float* Wc, const int32_t* cols, int64_t E, const int32_t* ptr0, const int32_t* perm0,
                           int act, float alpha, int pool_op, const float* g, float* ws, size_t ws_bytes, float* gz,
                           float* pi_bar, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_INORP_H */
