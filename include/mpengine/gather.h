/*
 * mpengine/gather.h - row gathers, repeat, embedding lookup.
 * Defined in csrc/: mp_gather.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_GATHER_H
#define MPENGINE_GATHER_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- gather --------------------------------- */
/* tf.gather(node, idx[:, col], axis=0) of kgcnn/layers/gather.py:83,228 on prepared int32 columns:
 * out[(e*ncols + c)*row_elems + f] = x[cols[colsel[c]*M + e]*row_elems + f]; ncols=2, colsel={0,1} gives the
 * GatherNodes concat layout [x_i || x_j] (gather.py:88-90).  Bit-exact copy. */
int mp_gather_rows_f32(const float* x, int64_t N, int64_t row_elems, const int32_t* cols, int64_t M, int ncols,
                       const int32_t* colsel_host, float* out, mpStream_t stream);

/* Same, straight from the API's int64 sample indices with the shift fused (no prepared columns). */
int mp_gather_rows_i64_f32(const float* x, int64_t N, int64_t row_elems, const int64_t* idx, int64_t M, int K,
                           int col /* -1: all K columns, concat layout */, const int64_t* node_splits,
                           const int64_t* edge_splits, int64_t G, float* out, mpStream_t stream);

/* GatherState, kgcnn/layers/gather.py:363-369: out = repeat(state, row_lengths(splits), axis=0). */
int mp_repeat_rows_f32(const float* state, const int64_t* splits, int64_t G, int64_t row_elems, int64_t N, float* out,
                       mpStream_t stream);

/* Embedding lookup of float node numbers (cast to int32 like Keras Embedding; kgcnn/layers/modules.py:526-528). */
int mp_embedding_f32(const float* table, int64_t vocab, int64_t dim, const float* numbers, int64_t N, float* out,
                     int32_t* flags, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_GATHER_H */
