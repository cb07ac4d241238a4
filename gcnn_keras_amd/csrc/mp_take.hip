// tf.gather(ragged, ids) for up to MP_TAKE_MAX ragged tensors that share their graph axis, in ONE C call and without a
// host read-back: the batch `perm[a:b]` of a resident data set (what MemoryGraphList.tensor() returned once) assembled on
// the device, so that a shuffled epoch (kgcnn/training/train_qm.py:159-166: model.fit(..., shuffle=True)) is not fed by
// the host packer.  Per-graph "sample" edge indices are copied unchanged (kgcnn/layers/base.py:27); only the row splits
// are rebased.
//
// Two launches on the caller's stream:
//   1. take_splits_kernel   one workgroup per item: row length of graph take[b] (clamped into [0, G), MP_FLAG_OOB raised
//                           otherwise), exclusive scan over the B lengths -> dst_splits.  The workgroup walks B in passes of
//                           MP_TAKE_SCAN_WIDTH entries and carries the running total from pass to pass: any B.
//   2. take_copy_kernel     parallel over the destination: a thread owns one 16-byte unit of dst_values, finds the batch
//                           graph of its first byte by binary search in dst_splits (mp_owner_of) and reads from
//                           src_splits[take[b]].  The unit moves as one 16-byte access when it lies inside one graph and
//                           its source address is 16-byte aligned too; otherwise as four 4-byte words, each looked up on
//                           its own (a unit of 4-byte rows can span several graphs; (N, 3) coordinates start most graphs
//                           off a 16-byte boundary).  Every offset is 64-bit; nothing is written past dst_rows rows.
#include "mp_common.h"
#include "../../include/mpengine/batching.h"

namespace {

constexpr int kScanWidth = MP_TAKE_SCAN_WIDTH;  // threads of the scan workgroup = entries per pass
constexpr int kScanWaves = kScanWidth / 64;

struct TakeArgs {
  mp_take_desc d;
  int32_t vec_ok[MP_TAKE_MAX];  // dst_values is 16-byte aligned: the unit grid coincides with 16-byte addresses
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// graph id of batch entry b, clamped into [0, G); `oob` is raised when it had to be clamped
__device__ __forceinline__ int64_t take_id(const mp_take_desc& d, int64_t b, bool* oob) {
  int64_t id = d.take ? d.take[b] : d.first + b;
  if (id < 0 || id >= d.G) {
    if (oob) *oob = true;
    id = id < 0 ? 0 : d.G - 1;
  }
  return id;
}

__global__ __launch_bounds__(kScanWidth) void take_splits_kernel(TakeArgs a) {
  __shared__ int64_t wave_total[kScanWaves];
  __shared__ int64_t carry_s;
  const mp_take_item& it = a.d.item[blockIdx.x];
  const int64_t B = a.d.B;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    carry_s = 0;
    it.dst_splits[0] = 0;
  }
  __syncthreads();
  int local_flags = 0;
  for (int64_t base = 0; base < B; base += kScanWidth) {  // block-uniform trip count
    const int64_t b = base + threadIdx.x;
    int64_t len = 0;
    if (b < B) {
      bool oob = false;
      const int64_t id = take_id(a.d, b, &oob);
      if (oob) local_flags |= MP_FLAG_OOB;
      len = it.src_splits[id + 1] - it.src_splits[id];
      if (len < 0) len = 0;  // splits that do not ascend: never a negative length
    }
    int64_t incl = len;  // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int64_t before = carry_s;
    for (int w = 0; w < wave; ++w) before += wave_total[w];
    if (b < B) it.dst_splits[b + 1] = before + incl;
    __syncthreads();  // everyone has read carry_s and wave_total
    if (threadIdx.x == kScanWidth - 1) carry_s = before + incl;  // read again only behind the next pass's first barrier
  }
  if (blockIdx.x == 0) mp_publish_flags(a.d.flags, local_flags);  // the ids are the same for every item
}

__global__ __launch_bounds__(256) void take_copy_kernel(TakeArgs a) {
  const mp_take_item& it = a.d.item[blockIdx.y];
  const int64_t B = a.d.B, rb = it.row_bytes;
  const int64_t* __restrict__ ds = it.dst_splits;
  const int64_t* __restrict__ ss = it.src_splits;
  int64_t rows = ds[B];
  if (rows > it.dst_rows) rows = it.dst_rows;  // never past the destination the caller sized
  const int64_t total = rows * rb;             // bytes, a multiple of 4
  const char* src = static_cast<const char*>(it.src_values);
  char* dst = static_cast<char*>(it.dst_values);
  const bool vec_ok = a.vec_ok[blockIdx.y] != 0;
  const int64_t units = (total + 15) >> 4;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; u < units; u += stride) {
    const int64_t o = u << 4;                        // first destination byte of the unit (o < total)
    int64_t b = mp_owner_of(ds, B, o / rb);          // ds[b] <= row < ds[b + 1]
    int64_t d0 = ds[b] * rb, d1 = ds[b + 1] * rb;    // destination bytes of graph b
    int64_t s0 = ss[take_id(a.d, b, nullptr)] * rb;  // source byte of its first row
    if (vec_ok && o + 16 <= d1 && o + 16 <= total) {
      const char* p = src + s0 + (o - d0);
      if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<u32x4*>(dst + o) = *reinterpret_cast<const u32x4*>(p);
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t w = o + 4 * j;
      if (w >= total) break;
      if (w >= d1) {  // next non-empty graph: w < total = ds[B] * rb at the most, so b stays below B
        do { ++b; } while (ds[b + 1] * rb <= w);
        d0 = ds[b] * rb;
        d1 = ds[b + 1] * rb;
        s0 = ss[take_id(a.d, b, nullptr)] * rb;
      }
      *reinterpret_cast<uint32_t*>(dst + w) = *reinterpret_cast<const uint32_t*>(src + s0 + (w - d0));
    }
  }
}

}  // namespace

extern "C" int mp_ragged_take(const mp_take_desc* d, mpStream_t stream) {
  MP_REQUIRE(d != nullptr && d->k >= 1 && d->k <= MP_TAKE_MAX, "mp_ragged_take: 1..%d items", MP_TAKE_MAX);
  MP_REQUIRE(d->B >= 0 && d->G >= 0, "mp_ragged_take: negative size");
  if (d->B == 0) return MP_OK;
  MP_REQUIRE(d->G >= 1, "mp_ragged_take: %lld graphs asked of an empty data set", static_cast<long long>(d->B));
  MP_REQUIRE(d->flags != nullptr, "mp_ragged_take: null flag word");
  TakeArgs a{};
  a.d = *d;
  int64_t max_units = 0;
  for (int i = 0; i < d->k; ++i) {
    const mp_take_item& it = d->item[i];
    MP_REQUIRE(it.src_splits && it.dst_splits, "mp_ragged_take: null row splits in item %d", i);
    MP_REQUIRE(it.row_bytes >= 4 && it.row_bytes % 4 == 0, "mp_ragged_take: row_bytes of item %d is no multiple of 4", i);
    MP_REQUIRE(it.dst_rows >= 0 && it.dst_rows <= INT64_MAX / it.row_bytes, "mp_ragged_take: bad dst_rows in item %d", i);
    MP_REQUIRE(it.dst_rows == 0 || (it.src_values && it.dst_values), "mp_ragged_take: null values in item %d", i);
    MP_REQUIRE((reinterpret_cast<uintptr_t>(it.src_values) & 3) == 0 && (reinterpret_cast<uintptr_t>(it.dst_values) & 3) == 0,
               "mp_ragged_take: values of item %d are not 4-byte aligned", i);
    a.vec_ok[i] = mp::aligned16(it.dst_values) ? 1 : 0;
    const int64_t units = (it.dst_rows * it.row_bytes + 15) / 16;
    if (units > max_units) max_units = units;
  }
  hipStream_t s = mp::as_stream(stream);
  take_splits_kernel<<<d->k, kScanWidth, 0, s>>>(a);
  int rc = mp::check_launch("mp_ragged_take (splits)");
  if (rc != MP_OK || max_units == 0) return rc;
  take_copy_kernel<<<dim3(mp::grid_for(max_units), d->k), 256, 0, s>>>(a);
  return mp::check_launch("mp_ragged_take (copy)");
}
