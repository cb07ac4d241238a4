/*
 * mpengine/schnet.h - the fused SchNet convolution: edge preparation, cfconv, filter tables, distance gradient.
 * Defined in csrc/: mp_index.hip (mp_edge_prepare_i64_f32), mp_cfconv.hip, mp_cfconv_bwd.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_SCHNET_H
#define MPENGINE_SCHNET_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- fused SchNet path --------------------- */
/* mp_index_prepare_i64 for K = 2 fused with NodePosition -> LazySubtract -> EuclideanNorm
 * (kgcnn/literature/Schnet.py:116-117): recv (M), send (M) shifted int32 ids, dist (M) nullable = ||x_i - x_j||,
 * flags as mp_index_prepare_i64 (column 0 sortedness only). */
int mp_edge_prepare_i64_f32(const int64_t* idx, int64_t M, const int64_t* node_splits, const int64_t* edge_splits,
                            int64_t G, int64_t N, const float* xyz, int32_t* recv, int32_t* send, float* dist,
                            int32_t* flags, mpStream_t stream);

/* SchNetCFconv.call, kgcnn/layers/conv/schnet_conv.py:73-79, fused (F = units = 128, cfconv_pool = sum,
 * activation = shifted_softplus): out[i] += sum_{e: recv[e]=i} x[send[e]] * (ssp(rbf[e] W1 + b1) W2 + b2).
 * The filter-MLP weights (Keras layouts W1 (B,128), b1 (128)|NULL, W2 (128,128), b2 (128)|NULL) are packed once
 * per weight update into the kernel's LDS image by mp_cfconv_pack_f32 (mp_cfconv_packed_floats() floats).
 * recv_sorted ascending; perm (nullable) maps sorted position -> original edge (rbf / send are in original
 * order); out (N,128) must be zero on entry.  flags bit0: fast softplus (v_exp/v_log form, |delta| < 2e-7);
 * bit 2 (value 4) / bit 3 (value 8) force the 8-wave / 4-wave workgroup (default: by tile count); bit 4 (value 16,
 * "several forwards in flight"): half as many workgroups, each serving twice the tiles.  Bit 5 needs a workspace (below);
 * these entry points ignore it. */
int mp_cfconv_packed_floats(void);
int mp_cfconv_pack_f32(const float* W1, const float* b1, int B, const float* W2, const float* b2, float* packed,
                       mpStream_t stream);
int mp_cfconv_fused_f32(const float* x, int64_t N, const float* rbf, int B, const float* packed,
                        const int32_t* recv_sorted, const int32_t* send, const int32_t* perm, int64_t M, int flags,
                        float* out_zeroed, mpStream_t stream);
/* Same with GaussBasisLayer (kgcnn/layers/geom.py:567-571) expanded in registers from the edge distance. */
int mp_cfconv_gauss_fused_f32(const float* x, int64_t N, const float* dist, int bins, float distance, float sigma,
                              float offset, const float* packed, const int32_t* recv_sorted, const int32_t* send,
                              const int32_t* perm, int64_t M, int flags, float* out_zeroed, mpStream_t stream);

/* The same two entry points with a caller workspace, which flags bit 5 (value 32) needs: DETERMINISTIC mode.  The partial
 * sums of every tile's first and last segment (the ones that may continue in a neighbouring 32-edge tile) are then not
 * added to `out` with float atomics but parked in the workspace and added per receiver, in edge order, by a second small
 * kernel: bit-identical results from run to run also for receivers with more than 32 incoming edges (the default mode can
 * differ there in the last bit, float atomics arrive in any order).  Costs one extra launch and 1 KB of workspace per tile;
 * without bit 5 the workspace is ignored (NULL allowed). */
int mp_cfconv_det_workspace_bytes(int64_t M, size_t* bytes_out_host);
int mp_cfconv_fused_ws_f32(const float* x, int64_t N, const float* rbf, int B, const float* packed,
                           const int32_t* recv_sorted, const int32_t* send, const int32_t* perm, int64_t M, int flags,
                           float* out_zeroed, void* ws, size_t ws_bytes, mpStream_t stream);
int mp_cfconv_gauss_fused_ws_f32(const float* x, int64_t N, const float* dist, int bins, float distance, float sigma,
                                 float offset, const float* packed, const int32_t* recv_sorted, const int32_t* send,
                                 const int32_t* perm, int64_t M, int flags, float* out_zeroed, void* ws, size_t ws_bytes,
                                 mpStream_t stream);

/* Inference route of the Gauss variant: the filter w(d) = Dense(Dense(gauss(d))) of a block is a function of the block's
 * weights and of the edge distance alone, so it is tabulated once per weight update and the kernel interpolates it
 * (six-point Lagrange on a power-of-two grid; no per-edge MLP).  Row j of the table holds the 128 filter values at the
 * knot v_lo + (j - 2) / inv_h of v = d - offset, evaluated in double precision and rounded to float once; v is clamped
 * to [v_lo, v_end], beyond which the filter is constant to 2.3e-11 of a unit weight.
 *   mp_cfconv_filter_table_layout  host only: domain v_lo = max(-offset, -7 sigma) .. distance (bins-1)/bins + 7 sigma,
 *                                  spacing 2^-log2_inv_h; MP_EINVAL if the table would exceed MP_FILTER_TABLE_MAX_ROWS.
 *   mp_cfconv_filter_table_f32     fills table (layout->rows x 128 floats) and check2: [0] the largest |interpolant -
 *                                  double filter| over the quarter, half and three-quarter points of every interval and
 *                                  four points beyond the ends, the interpolant evaluated with the kernel's arithmetic;
 *                                  [1] the largest |filter| there.  The caller decides from check2 whether to use the table.
 *   mp_cfconv_table_f32            the forward kernel (same tiles, segment rule, flags bits 4 and 5 and workspace as
 *                                  mp_cfconv_gauss_fused_ws_f32); waves per workgroup 4, 8, 16 or 0 = by tile count. */
#define MP_FILTER_TABLE_MAX_ROWS 256
typedef struct mp_filter_table_layout {
  float v_lo, v_end, inv_h;   /* domain of v = d - offset, 1 / spacing (a power of two) */
  int32_t n_int, rows;        /* intervals; rows = n_int + 5, padded to even */
} mp_filter_table_layout;
int mp_cfconv_filter_table_layout(int bins, float distance, float sigma, float offset, int log2_inv_h,
                                  mp_filter_table_layout* layout_out_host);
int mp_cfconv_filter_table_f32(const float* W1, const float* b1, int B, const float* W2, const float* b2, float distance,
                               float sigma, float offset, const mp_filter_table_layout* layout_host, float* table,
                               float* check2, mpStream_t stream);
int mp_cfconv_table_f32(const float* x, int64_t N, const float* dist, float offset, const float* table,
                        const mp_filter_table_layout* layout_host, const int32_t* recv_sorted, const int32_t* send,
                        const int32_t* perm, int64_t M, int flags, int waves, float* out_zeroed, void* ws, size_t ws_bytes,
                        mpStream_t stream);

/* Reverse pass of SchNetCFconv for forces (kgcnn/model/force.py:159-177 through schnet_conv.py:73-79, geom.py:567-571).
 * dE/dx_j is the forward kernel itself with the two index columns swapped (g_out in place of x, the sender-sorted list in
 * place of the receiver-sorted one).  mp_cfconv_gauss_dist_grad_f32 is the other half: per edge (original order)
 *   g_d[e] (+)= sum_h (v_e W2^T)_h * ssp'(g(d_e) W1 + b1)_h * (g'(d_e) W1)_h ,  v_e = g_out[recv[e]] * x[send[e]]
 * with the weights in the image of mp_cfconv_bwd_pack_f32 (mp_cfconv_bwd_packed_floats() floats: W1 | b1 as the forward
 * packs them, W2 re-ordered for the A operand).  Same FP32 MFMA tiles as the forward (three chains per 32-edge tile). */
int mp_cfconv_bwd_packed_floats(void);
int mp_cfconv_bwd_pack_f32(const float* W1, const float* b1, int B, const float* W2, float* packed, mpStream_t stream);
int mp_cfconv_gauss_dist_grad_f32(const float* x, const float* g_out, int64_t N, const float* dist, int bins,
                                  float distance, float sigma, float offset, const float* packed_bwd, const int32_t* recv,
                                  const int32_t* send, int64_t M, int accumulate, float* g_d, mpStream_t stream);

/* Diagnostic build of mp_cfconv_gauss_fused_f32 (20 bins, fast softplus): adds per-phase shader-cycle sums into
 * diag8 (8 x uint64, caller-zeroed): [0] weight staging, [1] tile setup + Gauss basis, [2] GEMM1, [3] softplus +
 * sender-row loads issued, [4] GEMM2, [5] multiply + slab write, [6] slab read, [7] segmented sum + stores/atomics.
 * Shares only: the stamps fence the schedule. */
int mp_cfconv_gauss_diag_f32(const float* x, int64_t N, const float* dist, int bins, float distance, float sigma,
                             float offset, const float* packed, const int32_t* recv_sorted, const int32_t* send,
                             const int32_t* perm, int64_t M, float* out_zeroed, unsigned long long* diag8,
                             mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_SCHNET_H */
