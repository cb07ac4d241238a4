/*
 * mpengine/schnet_model.h - SchNet node chains, embedding tables, the one-call forward, energy and forces.
 * Defined in csrc/: mp_schnet_node.hip, mp_schnet_table.hip, mp_schnet_forward.hip, mp_schnet_bwd.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_SCHNET_MODEL_H
#define MPENGINE_SCHNET_MODEL_H

#include "core.h"
#include "schnet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Node-side chains of kgcnn/literature/Schnet.py:110-133 / schnet_conv.py:159-165 (F = 128, embedding width 64):
 * node_in:     n = Embedding(Z) W0 + b0 ; x = n Wx
 * node_update: n += ssp(agg W2 + b2) W3 + b3 ; x = n Wx_next ; agg := 0
 * node_last:   n' = n + ssp(agg W2 + b2) W3 + b3 ; h = ssp(ssp(n' Wl0 + bl0) Wl1 + bl1) (N,64) ; agg := 0
 * readout:     out[g] = ssp(sum_{nodes of g} h W_o0 + b_o0) W_o1 + b_o1   (PoolingNodes(sum) + MLP([64,1]));
 *              W_o0 == NULL: out[g] = sum_{nodes of g} (h W_o1 + b_o1)  (last_mlp ending in Dense(1, linear), then
 *              PoolingNodes(sum), use_output_mlp=False: the fork's force_schnet.py configuration)
 * The embedding width is 64 or 128; flags bit 8 (256): `numbers` holds int64 node numbers (the fork's scripts declare
 * int64 inputs) instead of float32.
 * flags bit0: fast softplus as in mp_cfconv_fused_f32; bit1: every weight-matrix pointer is an
 * mp_schnet_node_pack_f32 image of the Keras kernel instead of the kernel itself (biases stay plain): the image stores,
 * per wave and lane, the registers of four consecutive k-steps as one float4, so a workgroup loads its weight slices
 * with 16-B instead of strided 4-B reads.  mp_schnet_node_in_f32, mp_schnet_stage0_f32, mp_schnet_node_update_f32 and
 * mp_schnet_node_last_f32 (and their _save_ forms) are built for images only: they REQUIRE bit 1 and return MP_EINVAL
 * without it, before any device work.  mp_schnet_node_residual_f32 alone reads the Keras kernels themselves. */
int mp_schnet_node_pack_f32(const float* W, int K, int U, float* packed /* K*U floats */, mpStream_t stream);
/* The same slice order with every element as three bf16 pieces (hi + mid + lo = the FP32 value exactly): flags bit 6
 * (value 64) makes the node kernels of the FORWARD run their GEMMs on the bf16 matrix pipe as an exact
 * FP32 emulation (six products per k block, FP32 accumulate: the error of the FP32 matrix instructions at 2.67x their
 * rate).  K % 32 == 0; the image holds K*U*3/2 floats.
 * flags bit 9 (value 512, bf16-piece build): "several launch sequences share the GPU" - a launch with 256 or more 16-node
 * tiles runs on half the CUs (128 persistent workgroups), leaving the others to the kernels of the other sequences. */
int mp_schnet_node_pack_bf16_f32(const float* W, int K, int U, float* packed /* K*U*3/2 floats */, mpStream_t stream);
/* SchNetInteraction.call's node side alone (schnet_conv.py:162-164), out of place, for the layer API:
 * n_out = n_in + Dense(lin)(Dense(ssp)(agg)); agg is left untouched. */
int mp_schnet_node_residual_f32(const float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                                const float* b3, const float* n_in, float* n_out, int flags, mpStream_t stream);
int mp_schnet_node_in_f32(const float* numbers, int64_t N, const float* emb, int vocab, int emb_dim, const float* W0,
                          const float* b0, const float* Wx, float* n_out, float* x_out, int flags, mpStream_t stream);
/* mp_schnet_node_in_f32 and mp_edge_prepare_i64_f32 in ONE launch (disjoint workgroups): they are independent and at
 * QM9 batch sizes each alone occupies less than half of the chip; falls back to the two launches for large batches. */
int mp_schnet_stage0_f32(const float* numbers, int64_t N, const float* emb, int vocab, int emb_dim, const float* W0,
                         const float* b0, const float* Wx, float* n_out, float* x_out, const int64_t* idx, int64_t M,
                         const int64_t* node_splits, const int64_t* edge_splits, int64_t G, const float* xyz,
                         int32_t* recv, int32_t* send, float* dist, int32_t* flags, int flags_arg, mpStream_t stream);
/* The node-input chain as a table: n and x of mp_schnet_node_in_f32 are functions of the node number alone, so the chain
 * runs once per weight update on the numbers 0 .. vocab-1, -1 (same build: flags bits 0, 1 - required -, 6 as the forward)
 * and fills n_table / x_table, (vocab + 1, 128) each: row r < vocab = the chain's rows for a node with number r, row
 * vocab = its rows for a number outside 0 .. vocab-1 (zero embedding row: b0 resp. b0 Wx).  Bit-identical to the chain by
 * construction.  numbers_ws: (vocab + 1) floats of scratch.  vocab + 1 <= MP_SCHNET_TABLE_MAX_ROWS (both tables: 2 MB, half
 * of one XCD's L2); larger vocabularies keep the chain. */
#define MP_SCHNET_TABLE_MAX_ROWS 2048
int mp_schnet_embed_table_f32(const float* emb, int vocab, int emb_dim, const float* W0, const float* b0,
                              const float* Wx, float* numbers_ws, float* n_table, float* x_table, int flags,
                              mpStream_t stream);
/* mp_schnet_node_in_f32 / mp_schnet_stage0_f32 with the chain replaced by a row gather from the tables: per node the number
 * is read (float32, or int64 with flags bit 8; cast and range rule of the chain) and row r of n_table / x_table is copied
 * to n_out / x_out.  No LDS, no barrier, 256-thread workgroups.  The stage-0 form runs the edge preparation on further
 * workgroups of the same launch (at most 128) and falls back to two launches for large batches as mp_schnet_stage0_f32 does. */
int mp_schnet_node_in_table_f32(const float* numbers, int64_t N, int vocab, const float* n_table, const float* x_table,
                                float* n_out, float* x_out, int flags, mpStream_t stream);
int mp_schnet_stage0_table_f32(const float* numbers, int64_t N, int vocab, const float* n_table, const float* x_table,
                               float* n_out, float* x_out, const int64_t* idx, int64_t M, const int64_t* node_splits,
                               const int64_t* edge_splits, int64_t G, const float* xyz, int32_t* recv, int32_t* send,
                               float* dist, int32_t* flags, int flags_arg, mpStream_t stream);
int mp_schnet_node_update_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                              const float* b3, float* n_inout, const float* Wx_next, float* x_out, int flags,
                              mpStream_t stream);
int mp_schnet_node_last_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3, const float* b3,
                            const float* n_in, const float* Wl0, const float* bl0, const float* Wl1, const float* bl1,
                            float* h_out, int flags, mpStream_t stream);
int mp_schnet_readout_f32(const float* h, const int64_t* node_splits, int64_t G, const float* Wo0, const float* bo0,
                          const float* Wo1, const float* bo1, float* out, mpStream_t stream);

/* The whole fused forward (kgcnn/literature/Schnet.py:104-148 with receiver-sorted edges) as ONE call: stage 0,
 * depth x (cfconv + node update), last node chain, readout, launched in sequence on `stream` from a descriptor of the
 * bound batch slot.  Equivalent to replaying a captured HIP graph of the same eight launches, without the capture:
 * the entry for batches whose shapes change from call to call.  flags: bit0 fast softplus, bit1 node-side
 * weight pointers (W0, Wx, W2, W3, Wl0, Wl1) are mp_schnet_node_pack_f32 images, bits 2-4 as mp_cfconv_fused_f32. */
#define MP_SCHNET_MAX_DEPTH 8
typedef struct mp_schnet_forward_desc {
  int64_t N, M, G;
  int32_t depth, vocab, flags, bins;
  float g_distance, g_sigma, g_offset;
  int32_t emb_dim;                 /* embedding width: 64 (0 = 64) or 128 */
  const float* numbers;            /* (N) node numbers: float32, or int64 with flags bit 8 */
  const float* xyz;                /* (N,3) */
  const int64_t* idx;              /* (M,2) sample indices */
  const int64_t* node_splits;      /* (G+1) */
  const int64_t* edge_splits;      /* (G+1) */
  const float* embedding;          /* (vocab,64) */
  const float* W0;                 /* (64,128) */
  const float* b0;
  const float* Wx[MP_SCHNET_MAX_DEPTH];      /* interaction i: dense1 (128,128), no bias */
  const float* packed[MP_SCHNET_MAX_DEPTH];  /* interaction i: mp_cfconv_pack_f32 image */
  const float* W2[MP_SCHNET_MAX_DEPTH];
  const float* b2[MP_SCHNET_MAX_DEPTH];
  const float* W3[MP_SCHNET_MAX_DEPTH];
  const float* b3[MP_SCHNET_MAX_DEPTH];
  const float* Wl0; const float* bl0; const float* Wl1; const float* bl1;   /* last_mlp */
  const float* Wo0; const float* bo0; const float* Wo1; const float* bo1;   /* output_mlp; Wo0 == NULL: linear head Wo1 */
  int32_t* recv; int32_t* send; float* dist; int32_t* flags_word;           /* (M) work buffers, flag word */
  float* n; float* x; float* agg; float* h; float* out;                     /* (N,128) x3 [agg zeroed], (N,64), (G,1) */
  const float* n_table; const float* x_table;   /* mp_schnet_embed_table_f32 tables; NULL: stage 0 runs the chain */
  /* interaction i: mp_cfconv_filter_table_f32 table; [0] == NULL: every block runs the MFMA kernel from packed[i] */
  const float* filter_table[MP_SCHNET_MAX_DEPTH];
  mp_filter_table_layout filter_layout;
} mp_schnet_forward_desc;
int mp_schnet_forward_launch(const mp_schnet_forward_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- SchNet energy + forces ------------------- */
/* Replaces, for a SchNet energy model, kgcnn/model/force.py:159-201 (GradientTape around the energy model, force =
 * -dE/dx) with a forward that keeps the activation derivatives and a hand-written reverse pass.
 *
 * SAVE variants of the forward node chains: as mp_schnet_node_update_f32 / mp_schnet_node_last_f32 / mp_schnet_readout_f32
 * and additionally store sigmoid(pre-activation) of every shifted softplus on the chain (d2 (N,128), dl0 (N,128),
 * dl1 (N,64)) resp. dE_g/d pooled_g (G,64) of the MLP head.  Null outputs = the plain entry.  Packed images only. */
int mp_schnet_node_update_save_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                                   const float* b3, float* n_inout, const float* Wx_next, float* x_out, float* d2_out,
                                   int flags, mpStream_t stream);
int mp_schnet_node_last_save_f32(float* agg, int64_t N, const float* W2, const float* b2, const float* W3,
                                 const float* b3, const float* n_in, const float* Wl0, const float* bl0,
                                 const float* Wl1, const float* bl1, float* h_out, float* d2_out, float* dl0_out,
                                 float* dl1_out, int flags, mpStream_t stream);
int mp_schnet_readout_grad_f32(const float* h, const int64_t* node_splits, int64_t G, const float* Wo0,
                               const float* bo0, const float* Wo1, const float* bo1, float* out, float* g_pool_out,
                               mpStream_t stream);
/* Reverse node chains on 16-node tiles; every W*T is the mp_schnet_node_pack_f32 image of the TRANSPOSED Keras kernel.
 * head : g_n = ((gh[row] * dl1) Wl1T * dl0) Wl0T ; g_agg = ((g_n W3T) * d2) W2T     gh_row null: gh is one 64-row
 * block: g_n += g_x WxT (g_x rows re-zeroed)     ; g_agg = ((g_n W3T) * d2) W2T */
int mp_schnet_bwd_head_f32(const float* gh, const int32_t* gh_row, const float* dl1, int64_t N, const float* Wl1T,
                           const float* dl0, const float* Wl0T, const float* W3T, const float* d2, const float* W2T,
                           float* g_n, float* g_agg, mpStream_t stream);
int mp_schnet_bwd_block_f32(float* g_x, int64_t N, const float* WxT, float* g_n, const float* W3T, const float* d2,
                            const float* W2T, float* g_agg, mpStream_t stream);
/* out (N,3) = scale * dE/dx from dE/dd (M): sum over the edges touching a node of g_d (x_n - x_other) / d, over the
 * receiver-side and sender-side CSR of the index plan (perm null: that column is sorted).  scale -1: physical force. */
int mp_schnet_force_from_gd_f32(const float* g_d, const float* xyz, const float* dist, const int32_t* recv,
                                const int32_t* send, const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1,
                                const int32_t* perm1, int64_t N, int64_t M, float scale, float* out, mpStream_t stream);
/* The whole energy + force pass of a bound batch slot in one call (the ~32 launches for depth 6, in sequence on
 * `stream`; capturable into a HIP graph): forward as mp_schnet_forward_launch with the SAVE chains (fwd.x unused: the
 * sender features of every block are kept in xs), then head chain, per block distance gradient + swapped-column cfconv
 * + block chain, then the force kernel.  fwd.flags bit 1 (packed node images) is required. */
typedef struct mp_schnet_force_desc {
  mp_schnet_forward_desc fwd;
  float* xs;                       /* (depth, N, 128) sender features x_i of every block */
  float* d2;                       /* (depth, N, 128) */
  float* dl0; float* dl1;          /* (N,128), (N,64) */
  float* g_pool;                   /* (G,64)  MLP head only */
  const int32_t* node_graph;       /* (N) graph of each node, MLP head only */
  const float* W3T[MP_SCHNET_MAX_DEPTH];
  const float* W2T[MP_SCHNET_MAX_DEPTH];
  const float* WxT[MP_SCHNET_MAX_DEPTH];           /* [0] unused */
  const float* packed_bwd[MP_SCHNET_MAX_DEPTH];    /* mp_cfconv_bwd_pack_f32 images */
  const float* Wl0T; const float* Wl1T;
  const int32_t* seg0; const int32_t* perm0;       /* receiver column sorted + its permutation (null: already sorted) */
  const int32_t* seg1; const int32_t* perm1;       /* sender column sorted + its permutation */
  const int32_t* ptr0; const int32_t* ptr1;        /* (N+1) CSR offsets of both columns */
  float* g_n; float* g_agg; float* g_x; float* g_d;   /* (N,128) x3 [g_x zeroed], (M) */
  float* force;                    /* (N,3) out */
  float force_scale;               /* -1: physical force, +1: dE/dx */
} mp_schnet_force_desc;
int mp_schnet_force_launch(const mp_schnet_force_desc* desc_host, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_SCHNET_MODEL_H */
