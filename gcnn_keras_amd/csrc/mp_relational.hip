// RelationalDense of HDNNP2nd's RelationalMLP (kgcnn/layers/relational.py:219-238, without num_bases / num_blocks):
//
//   mp_relational_dense_f32        mode 0: y (R,U) = act(x (R,K) W[rel[r]] + b), pre_out keeps x W[rel] + b
//                                  mode 1 (transposed): y (R,K) = (x (R,U) * act'(pre)) W[rel]^T  (pre nullable: no factor)
//   mp_relational_dense_wgrad_f32  dW[q] = x_q^T g_q over the rows of relation q, db = sum_r g[r]
//
// W is (nrel, K, U) row-major, one Keras kernel per relation; the bias is shared by all relations (relational.py:235-236).
// A relation outside [0, nrel) uses a zero kernel (TF-GPU gather: zeros), so its row is act(b) and it has no kernel
// gradient.  FP32, fma chains in k order (the precision class of mp_dense_f32).
//
// The forward serves every relation in one launch: a thread owns one output element and reads its relation's kernel
// column through L2 (the fork's 30 x 640 x 35 kernels are 2.7 MB).  The weight gradient groups the rows by relation on
// the device - Keras' int32 cast, stable radix sort, CSR offsets, as mp_embedding_grad_f32 does - and adds each
// relation's rows in row order: the same bits every run and on every stream.  Nothing is read back to the host, so a
// captured HIP graph replays every call.
#include "mp_common.h"
#include "../../include/mpengine/hdnnp.h"
#include "../../include/mpengine/index.h"

namespace {


__device__ __forceinline__ int64_t rel_of(const int64_t* rel, int64_t r, int64_t nrel) {
  const int64_t v = rel[r];
  return (v >= 0 && v < nrel) ? v : -1;
}

__global__ void rel_dense_kernel(const float* __restrict__ x, int64_t R, int64_t K, const int64_t* __restrict__ rel,
                                 int64_t nrel, const float* __restrict__ W, const float* __restrict__ b, int64_t U,
                                 int act, float alpha, float* __restrict__ pre_out, float* __restrict__ y) {
  const int64_t total = R * U, stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = t / U, u = t - r * U;
    const int64_t q = rel_of(rel, r, nrel);
    float acc = 0.0f;
    if (q >= 0) {
      const float* xr = x + r * K;
      const float* w = W + q * K * U + u;
      for (int64_t k = 0; k < K; ++k) acc = fmaf(xr[k], w[k * U], acc);
    }
    if (b) acc += b[u];
    if (pre_out) pre_out[t] = acc;
    y[t] = mp_apply_act(act, alpha, acc);
  }
}

__global__ void rel_dense_t_kernel(const float* __restrict__ g, int64_t R, int64_t K, const int64_t* __restrict__ rel,
                                   int64_t nrel, const float* __restrict__ W, int64_t U, int act, float alpha,
                                   const float* __restrict__ pre, float* __restrict__ y) {
  const int64_t total = R * K, stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = t / K, k = t - r * K;
    const int64_t q = rel_of(rel, r, nrel);
    float acc = 0.0f;
    if (q >= 0) {
      const float* gr = g + r * U;
      const float* w = W + (q * K + k) * U;
      for (int64_t u = 0; u < U; ++u) {
        float gv = gr[u];
        if (pre) gv *= mp_act_grad(act, alpha, pre[r * U + u]);
        acc = fmaf(gv, w[u], acc);
      }
    }
    y[t] = acc;
  }
}

// Keras' int32 cast of the relation ids; out-of-range ids go to the bucket nrel, which no kernel gradient reads
__global__ void rel_ids_kernel(const int64_t* __restrict__ rel, int64_t R, int64_t nrel, int32_t* __restrict__ ids) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < R; r += stride) {
    const int64_t v = rel[r];
    ids[r] = static_cast<int32_t>((v >= 0 && v < nrel) ? v : nrel);
  }
}

// dW[q,k,u] = sum over the rows of relation q, in row order, of x[r,k] g[r,u]
__global__ void rel_wgrad_kernel(const float* __restrict__ x, int64_t K, const float* __restrict__ g, int64_t U,
                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ perm, int64_t nrel,
                                 float* __restrict__ dW) {
  const int64_t total = nrel * K * U, stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t q = t / (K * U), rem = t - q * K * U;
    const int64_t k = rem / U, u = rem - k * U;
    float acc = 0.0f;
    for (int32_t p = ptr[q]; p < ptr[q + 1]; ++p) {
      const int64_t r = perm[p];
      acc = fmaf(x[r * K + k], g[r * U + u], acc);
    }
    dW[t] = acc;
  }
}

// db[u] = sum_r g[r,u]: one workgroup per column, a fixed row stride per thread and a fixed tree over the workgroup
__global__ __launch_bounds__(256) void col_sum_kernel(const float* __restrict__ g, int64_t R, int64_t U,
                                                      float* __restrict__ db) {
  __shared__ float part[256];
  const int64_t u = blockIdx.x;
  float acc = 0.0f;
  for (int64_t r = threadIdx.x; r < R; r += 256) acc += g[r * U + u];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[u] = part[0];
}

}  // namespace

extern "C" {

int mp_relational_dense_f32(const float* x, int64_t R, int64_t K, const int64_t* rel, int64_t nrel, const float* W,
                            const float* b, int64_t U, int act, float act_alpha, int mode, const float* pre,
                            float* pre_out, float* y, mpStream_t stream) {
  MP_REQUIRE(R >= 0 && K >= 1 && U >= 1 && nrel >= 1 && (mode == 0 || mode == 1) && act >= MP_ACT_LINEAR &&
             act <= MP_ACT_LAST, "mp_relational_dense_f32: bad arguments");
  MP_REQUIRE(mode == 0 || (!b && !pre_out), "mp_relational_dense_f32: the transposed mode takes no bias / pre_out");
  if (R == 0) return MP_OK;
  MP_REQUIRE(x && rel && W && y, "mp_relational_dense_f32: null pointer");
  hipStream_t s = mp::as_stream(stream);
  if (mode == 0) {
    rel_dense_kernel<<<mp::grid_for(R * U), 256, 0, s>>>(x, R, K, rel, nrel, W, b, U, act, act_alpha, pre_out, y);
  } else {
    rel_dense_t_kernel<<<mp::grid_for(R * K), 256, 0, s>>>(x, R, K, rel, nrel, W, U, act, act_alpha, pre, y);
  }
  return mp::check_launch("mp_relational_dense_f32");
}

int mp_relational_dense_wgrad_ws_bytes(int64_t R, int64_t nrel, size_t* bytes_out_host) {
  MP_REQUIRE(R >= 0 && nrel >= 1 && bytes_out_host, "mp_relational_dense_wgrad_ws_bytes: bad arguments");
  size_t sort = 0;
  int rc = mp_sort_workspace_bytes(R, &sort);
  if (rc != MP_OK) return rc;
  const size_t n = static_cast<size_t>(R > 0 ? R : 1);
  *bytes_out_host = 3 * mp::align256(sizeof(int32_t) * n) + mp::align256(sizeof(int32_t) * static_cast<size_t>(nrel + 2)) + sort;
  return MP_OK;
}

int mp_relational_dense_wgrad_f32(const float* x, int64_t R, int64_t K, const int64_t* rel, int64_t nrel,
                                  const float* g, int64_t U, float* dW, float* db, void* ws, size_t ws_bytes,
                                  mpStream_t stream) {
  MP_REQUIRE(R >= 0 && K >= 1 && U >= 1 && nrel >= 1, "mp_relational_dense_wgrad_f32: bad sizes");
  MP_REQUIRE(dW || db, "mp_relational_dense_wgrad_f32: no output");
  hipStream_t s = mp::as_stream(stream);
  if (R == 0) {
    if (dW) MP_HIP(hipMemsetAsync(dW, 0, sizeof(float) * static_cast<size_t>(nrel * K * U), s));
    if (db) MP_HIP(hipMemsetAsync(db, 0, sizeof(float) * static_cast<size_t>(U), s));
    return MP_OK;
  }
  MP_REQUIRE(g && (!dW || (x && rel && ws)), "mp_relational_dense_wgrad_f32: null pointer");
  if (db) {
    col_sum_kernel<<<static_cast<unsigned>(U), 256, 0, s>>>(g, R, U, db);
    int rc = mp::check_launch("mp_relational_dense_wgrad_f32 (db)");
    if (rc != MP_OK) return rc;
  }
  if (!dW) return MP_OK;
  size_t need = 0;
  int rc = mp_relational_dense_wgrad_ws_bytes(R, nrel, &need);
  if (rc != MP_OK) return rc;
  MP_REQUIRE(ws_bytes >= need, "mp_relational_dense_wgrad_f32: workspace %zu < %zu bytes", ws_bytes, need);
  char* p = static_cast<char*>(ws);
  const size_t nb = mp::align256(sizeof(int32_t) * static_cast<size_t>(R));
  int32_t* ids = reinterpret_cast<int32_t*>(p);
  int32_t* ids_sorted = reinterpret_cast<int32_t*>(p + nb);
  int32_t* perm = reinterpret_cast<int32_t*>(p + 2 * nb);
  int32_t* ptr = reinterpret_cast<int32_t*>(p + 3 * nb);
  const size_t head = 3 * nb + mp::align256(sizeof(int32_t) * static_cast<size_t>(nrel + 2));
  rel_ids_kernel<<<mp::grid_for(R), 256, 0, s>>>(rel, R, nrel, ids);
  rc = mp::check_launch("mp_relational_dense_wgrad_f32 (ids)");
  if (rc != MP_OK) return rc;
  rc = mp_sort_segments_i32(ids, R, ids_sorted, perm, p + head, ws_bytes - head, stream);
  if (rc != MP_OK) return rc;
  rc = mp_csr_from_sorted_i32(ids_sorted, R, nrel + 1, ptr, stream);
  if (rc != MP_OK) return rc;
  rel_wgrad_kernel<<<mp::grid_for(nrel * K * U), 256, 0, s>>>(x, K, g, U, ptr, perm, nrel, dW);
  return mp::check_launch("mp_relational_dense_wgrad_f32");
}

}  // extern "C"
