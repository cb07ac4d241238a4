/*
 * mpengine/batching.h - launch groups, batches of a resident data set, the host batch packer.
 * Defined in csrc/: mp_concat.hip, mp_take.hip, mp_pack.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_BATCHING_H
#define MPENGINE_BATCHING_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- launch groups ------------------------------ */
/* Disjoint union of k resident ragged batches in one launch (the device-side form of concatenating what two
 * MemoryGraphList.tensor() calls produce, kgcnn/data/base.py:203-239): node numbers (float32, or int64 with z_is_i64),
 * coordinates (N,3), edge sample indices (M,2) int64 - unchanged, kgcnn/layers/base.py:27 - and the two row-split arrays,
 * rebased.  Outputs sized for the sums; node_splits / edge_splits get sum(G) + 1 entries.  Lets one launch sequence of the
 * fused forward serve several independent batches (gcnn_keras_amd/fused.py::SchnetFusedRoute.call_group). */
#define MP_CONCAT_MAX 8
typedef struct mp_batch_src {
  const void* z; const float* xyz; const int64_t* idx; const int64_t* node_splits; const int64_t* edge_splits;
  int64_t N, M, G;
} mp_batch_src;
typedef struct mp_concat_desc {
  int32_t k, z_is_i64;
  mp_batch_src src[MP_CONCAT_MAX];
  void* z; float* xyz; int64_t* idx; int64_t* node_splits; int64_t* edge_splits;
} mp_concat_desc;
int mp_concat_batches(const mp_concat_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- batches of a resident data set ------------ */
/* tf.gather(ragged, ids) for up to MP_TAKE_MAX ragged tensors that share their graph axis (G graphs), in one call and
 * without a host read-back: item i receives the rebased dst_splits (B + 1 entries) and the rows of graphs take[0],
 * take[1], ... back to back (bit-exact copy; per-graph edge indices are sample indices, kgcnn/layers/base.py:27, and stay
 * as they are).  take == NULL means the contiguous range first .. first + B - 1.  row_bytes is a multiple of 4; dst_rows
 * is the number of rows dst_values holds (the host knows it from its copy of the splits) and nothing is written past it.
 * An id outside [0, G) is clamped and MP_FLAG_OOB is ORed into *flags.  The scan behind dst_splits walks B in passes of
 * MP_TAKE_SCAN_WIDTH entries; any B is correct.  B == 0 returns MP_OK without a launch. */
#define MP_TAKE_MAX 8
#define MP_TAKE_SCAN_WIDTH 1024
typedef struct mp_take_item {
  const void* src_values; const int64_t* src_splits; int64_t row_bytes;
  void* dst_values; int64_t* dst_splits; int64_t dst_rows;
} mp_take_item;
typedef struct mp_take_desc {
  int32_t k, reserved;
  int64_t G, B, first;
  const int64_t* take;
  int32_t* flags;
  mp_take_item item[MP_TAKE_MAX];
} mp_take_desc;
int mp_ragged_take(const mp_take_desc* desc_host, mpStream_t stream);

/* ---------------------------------------------------------------- host batch packer ---------------------- */
/* The data-format side of the path.  Host pointers only; nothing here launches a kernel.
 *
 * mp_pack_rows_host = kgcnn.data.utils.ragged_tensor_from_nested_numpy (kgcnn/data/utils.py:129-157:
 * np.concatenate(list, axis=0, dtype) + row lengths), as called per property by MemoryGraphList.tensor
 * (kgcnn/data/base.py:203-239): rows_host[g] points to counts_host[g] rows of row_elems elements of src_kind; they
 * are concatenated (converted to dst_kind: f64<->f32, i32<->i64, i32/i64->f32) into dst_host, and the int64
 * row_splits (G+1) are written.  Multi-threaded over contiguous graph ranges (threads <= 1: caller's thread). */
int mp_pack_rows_host(const void* const* rows_host, const int64_t* counts_host, int64_t G, int64_t row_elems,
                      int src_kind, int dst_kind, void* dst_host, int64_t* splits_out_host, int threads);

/* Edge indices of a batch: concatenates the per-graph (m_g, K) sample index lists (idx_kind MP_DT_I64 | MP_DT_I32)
 * into the API's int64 (M,K) tensor and, in the same pass, produces what mp_index_prepare_i64 +
 * mp_csr_from_sorted_i32 would compute on the device for this batch: shifted int32 columns cols[k*M + e]
 * (kgcnn/ops/partition.py:140-155), the MP_FLAG_* word, and - if csr_ptr_out_host is given and column 0 is sorted -
 * the CSR offsets ptr[0..N] (zeros otherwise).  Also writes both row_splits (G+1 each). */
int mp_pack_edge_index_host(const void* const* idx_rows_host, int idx_kind, const int64_t* edge_counts_host,
                            const int64_t* node_counts_host, int64_t G, int K, int64_t* idx_out_host,
                            int64_t* edge_splits_out_host, int64_t* node_splits_out_host, int32_t* cols_out_host,
                            int32_t* csr_ptr_out_host, int32_t* flags_out_host, int threads);

/* Staging memory for the packer (pinned = hipHostMalloc: needs a device; 0 = aligned malloc) and the asynchronous
 * host-to-device copy that hands a packed tensor to the engine on the caller's stream. */
int mp_host_alloc(size_t bytes, int pinned, void** out_host);
int mp_host_free(void* p, int pinned);
int mp_memcpy_h2d_async(void* dst_device, const void* src_host, size_t bytes, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_BATCHING_H */
