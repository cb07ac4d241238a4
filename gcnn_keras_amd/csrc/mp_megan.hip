// MEGAN (kgcnn/literature/MEGAN.py:251-327): the importance readout behind the last attention layer, and its reverse.
//
// As a layer sequence the tail is: L logit tensors concatenated and summed, a sigmoid (the edge importances ei), two
// mean pools of ei (one per index column) and their average p, the node-importance Dense chain with linear output z,
// a sigmoid and a multiply (the node importances ni), then per channel k a column slice, a broadcast multiply into an
// (N, W) temporary and a graph pool, and a concatenation: about 3K + 8 launches and K node-sized temporaries.  Here:
//
//   mp_megan_edge_importance_f32       ei[e,k] = sigmoid(sum_l logits_l[e,k]),  summed in layer order
//   mp_megan_readout_f32               p[n,k]  = 0.5 (mean_{e: idx[e,0]=n} ei[e,k] + mean_{e: idx[e,1]=n} ei[e,k])
//                                      ni[n,k] = sigmoid(z[n,k]) p[n,k]
//                                      out[b, kW+f] = pool_{n in graph b} ni[n,k] x[n,f]        (sum or mean)
//   mp_megan_readout_grad_f32          x_bar[n,f] = s sum_k ni[n,k] g_out[b,kW+f]
//                                      t[n,k]  = g_ni[n,k] + s sum_f x[n,f] g_out[b,kW+f]       (s = 1 or 1/nodes)
//                                      z_bar   = t p sigma(z)(1 - sigma(z)),   q = t sigma(z)
//   mp_megan_edge_importance_grad_f32  ei_bar[e,k] = g_ei[e,k] + 0.5 q[idx[e,0],k]/deg0 + 0.5 q[idx[e,1],k]/deg1
//                                      s_bar = ei_bar ei (1 - ei)            (the gradient of every layer's logits)
//
// The readout is one wave per graph.  Per tile of 64 nodes, lane j owns node j: it walks the node's two CSR lists in
// list order, reading the K adjacent importances of every edge, and keeps ni[n, 0..K) in registers.  Then the wave
// walks the tile's nodes in node order: every lane owns up to two 16-byte column chunks of x (W <= 512) and K
// accumulators per chunk, ni[n,k] comes to all lanes by a wave shuffle.  x is read once, coalesced, and no LDS, barrier or
// atomic is used: every sum runs in an order fixed by the lists and the node order.
// The reverse of the readout is one wave per node (K dot products over W, reduced by the xor butterfly); the reverse of
// the edge importances is a gather per (edge, channel), not the adjoint scatter, because the mean pools' adjoints
// broadcast a node value to the edges of its list.
#include "mp_common.h"
#include "../../include/mpengine/megan.h"

namespace {

constexpr int MAXK = MP_MEGAN_MAX_CHANNELS;
constexpr int MAXL = MP_MEGAN_MAX_LAYERS;
constexpr int TILE = MP_MEGAN_NODE_TILE;   // nodes per tile = lanes of a wave
static_assert(TILE == 64, "a lane owns a node of the tile");

struct LogitPtrs {
  const float* l[MAXL];
};

__global__ __launch_bounds__(256) void megan_edge_importance_kernel(LogitPtrs lp, int L, int64_t total,
                                                                    float* __restrict__ ei) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
    float s = lp.l[0][i];
#pragma unroll
    for (int l = 1; l < MAXL; ++l)
      if (l < L) s += lp.l[l][i];
    ei[i] = mp_sigmoid(s);
  }
}

// sum of ei rows over the list [ptr[n], ptr[n+1]) in list order, divided by its length; an empty list gives 0
template <int K>
__device__ __forceinline__ void list_mean(const float* __restrict__ ei, int64_t M, const int32_t* __restrict__ ptr,
                                          const int32_t* __restrict__ perm, int64_t n, float (&mean)[K]) {
  int64_t a = ptr[n], b = ptr[n + 1];
  a = a < 0 ? 0 : (a > M ? M : a);
  b = b < a ? a : (b > M ? M : b);
  float s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0f;
  for (int64_t j = a; j < b; ++j) {
    int64_t e = perm ? static_cast<int64_t>(perm[j]) : j;
    e = e < 0 ? 0 : (e >= M ? M - 1 : e);
    const float* row = ei + e * K;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += row[k];
  }
  const float cnt = static_cast<float>(b - a);
#pragma unroll
  for (int k = 0; k < K; ++k) mean[k] = b > a ? s[k] / cnt : 0.0f;
}

struct ReadoutArgs {
  const float* ei;       // (M, K)
  const int32_t* ptr0;   // (N + 1) CSR of index column 0
  const int32_t* perm0;  // (M) nullable
  const int32_t* ptr1;   // (N + 1) CSR of index column 1
  const int32_t* perm1;  // (M) nullable
  const float* z;        // (N, K)
  const float* x;        // (N, W)
  const int64_t* splits; // (G + 1)
  float* p;              // (N, K) nullable
  float* ni;             // (N, K)
  float* out;            // (G, K * W)
  int M, N, G;           // 32 bits each (checked on the host): the kernel is short of scalar registers, not of range
  int W, mean;
};

// NC: 16-byte column chunks per lane, W <= 256 * NC.  K is a template argument: with the channel loops unrolled over a
// run-time K the kernel runs out of scalar registers (the compiler spills them), and a small K keeps few accumulators.
template <int NC, int K>
__global__ __launch_bounds__(256) void megan_readout_kernel(ReadoutArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int W = a.W;
  const int chunks = W >> 2;
  for (int64_t b = wave; b < a.G; b += waves) {
    int64_t n0 = a.splits[b], n1 = a.splits[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    float4 acc[NC][K];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int k = 0; k < K; ++k) acc[c][k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int64_t t0 = n0; t0 < n1; t0 += TILE) {
      const int rows = static_cast<int>(n1 - t0 < TILE ? n1 - t0 : TILE);
      // node side: lane j owns node t0 + j
      float w[K];
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = 0.0f;
      if (lane < rows) {
        const int64_t n = t0 + lane;
        float m0[K], m1[K];
        list_mean<K>(a.ei, a.M, a.ptr0, a.perm0, n, m0);
        list_mean<K>(a.ei, a.M, a.ptr1, a.perm1, n, m1);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float pk = 0.5f * (m1[k] + m0[k]);
          w[k] = mp_sigmoid(a.z[n * K + k]) * pk;
          if (a.p != nullptr) a.p[n * K + k] = pk;
          a.ni[n * K + k] = w[k];
        }
      }
      // graph side: the tile's nodes in node order
      for (int j = 0; j < rows; ++j) {
        const float* xr = a.x + (t0 + j) * W;
        float wj[K];
#pragma unroll
        for (int k = 0; k < K; ++k) wj[k] = __shfl(w[k], j, 64);   // a vector register each: K scalars would spill
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int ch = lane + 64 * c;
          if (ch < chunks) {
            const float4 v = *reinterpret_cast<const float4*>(xr + 4 * ch);
#pragma unroll
            for (int k = 0; k < K; ++k) {
              acc[c][k].x += wj[k] * v.x;
              acc[c][k].y += wj[k] * v.y;
              acc[c][k].z += wj[k] * v.z;
              acc[c][k].w += wj[k] * v.w;
            }
          }
        }
      }
    }
    const float den = a.mean != 0 && n1 > n0 ? static_cast<float>(n1 - n0) : 1.0f;   // x / 1 is x
    float* orow = a.out + b * (static_cast<int64_t>(K) * W);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int ch = lane + 64 * c;
      if (ch < chunks) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float4 v = acc[c][k];
          *reinterpret_cast<float4*>(orow + static_cast<int64_t>(k) * W + 4 * ch) =
              make_float4(v.x / den, v.y / den, v.z / den, v.w / den);
        }
      }
    }
  }
}

struct ReadoutGradArgs {
  const float* g_out;    // (G, K * W)
  const float* g_ni;     // (N, K) nullable
  const float* x;        // (N, W)
  const float* z;        // (N, K)
  const float* p;        // (N, K)
  const int64_t* splits; // (G + 1)
  float* x_bar;          // (N, W)
  float* z_bar;          // (N, K)
  float* q;              // (N, K)
  int64_t N, G;
  int K, W, mean;
};

__global__ __launch_bounds__(256) void megan_readout_grad_kernel(ReadoutGradArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int K = a.K, W = a.W;
  const int chunks = W >> 2;
  for (int64_t n = wave; n < a.N; n += waves) {
    const int64_t b = mp_owner_of(a.splits, a.G, n);
    const int64_t cnt = a.splits[b + 1] - a.splits[b];
    const float s = a.mean != 0 && cnt > 0 ? 1.0f / static_cast<float>(cnt) : 1.0f;
    const float* go = a.g_out + b * (static_cast<int64_t>(K) * W);
    const float* xr = a.x + n * W;
    float sg[MAXK], w[MAXK], dot[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      sg[k] = k < K ? mp_sigmoid(a.z[n * K + k]) : 0.0f;
      w[k] = k < K ? sg[k] * a.p[n * K + k] : 0.0f;
      dot[k] = 0.0f;
    }
    for (int ch = lane; ch < chunks; ch += 64) {
      const float4 v = *reinterpret_cast<const float4*>(xr + 4 * ch);
      float4 xb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        if (k < K) {
          const float4 g = *reinterpret_cast<const float4*>(go + static_cast<int64_t>(k) * W + 4 * ch);
          dot[k] += v.x * g.x + v.y * g.y + v.z * g.z + v.w * g.w;
          xb.x += w[k] * g.x;
          xb.y += w[k] * g.y;
          xb.z += w[k] * g.z;
          xb.w += w[k] * g.w;
        }
      }
      *reinterpret_cast<float4*>(a.x_bar + n * W + 4 * ch) = make_float4(s * xb.x, s * xb.y, s * xb.z, s * xb.w);
    }
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k < K) dot[k] = mp_wave_sum(dot[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        if (k < K) {
          const float t = (a.g_ni != nullptr ? a.g_ni[n * K + k] : 0.0f) + s * dot[k];
          a.z_bar[n * K + k] = t * a.p[n * K + k] * sg[k] * (1.0f - sg[k]);
          a.q[n * K + k] = t * sg[k];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void megan_edge_importance_grad_kernel(
    const float* __restrict__ g_ei, const float* __restrict__ q, const float* __restrict__ ei,
    const int32_t* __restrict__ cols, const int32_t* __restrict__ ptr0, const int32_t* __restrict__ ptr1, int64_t N,
    int64_t M, int K, float* __restrict__ s_bar) {
  const int64_t total = M * K;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t e = i / K;
    const int k = static_cast<int>(i - e * K);
    const int64_t r = cols[e], s = cols[M + e];
    float bar = g_ei != nullptr ? g_ei[i] : 0.0f;
    if (r >= 0 && r < N) {   // an edge with an index out of range lies in no list
      const int32_t d = ptr0[r + 1] - ptr0[r];
      bar += 0.5f * q[r * K + k] / static_cast<float>(d > 0 ? d : 1);
    }
    if (s >= 0 && s < N) {
      const int32_t d = ptr1[s + 1] - ptr1[s];
      bar += 0.5f * q[s * K + k] / static_cast<float>(d > 0 ? d : 1);
    }
    const float v = ei[i];
    s_bar[i] = bar * v * (1.0f - v);
  }
}

bool sizes_ok(int64_t N, int64_t M, int K) {
  return N >= 0 && M >= 0 && N < (int64_t{1} << 31) - 1 && M * K < (int64_t{1} << 31);
}

}  // namespace

extern "C" {

int mp_megan_edge_importance_f32(int L, const float* const* logits_host, int64_t M, int K, float* ei, mpStream_t stream) {
  const char* what = "mp_megan_edge_importance_f32";
  MP_REQUIRE(L >= 1 && L <= MAXL, "%s: 1 to %d logit tensors, got %d", what, MAXL, L);
  MP_REQUIRE(K >= 1 && K <= MAXK, "%s: 1 to %d channels, got %d", what, MAXK, K);
  MP_REQUIRE(sizes_ok(0, M, K), "%s: bad sizes M=%lld", what, (long long)M);
  if (M == 0) return MP_OK;
  MP_REQUIRE(logits_host && ei, "%s: null pointer", what);
  LogitPtrs lp{};
  for (int l = 0; l < L; ++l) {
    lp.l[l] = logits_host[l];
    MP_REQUIRE(lp.l[l], "%s: null pointer in layer %d", what, l);
  }
  megan_edge_importance_kernel<<<mp::grid_for(M * K), 256, 0, mp::as_stream(stream)>>>(lp, L, M * K, ei);
  return mp::check_launch(what);
}

int mp_megan_readout_f32(const float* ei, int64_t M, int K, const int32_t* ptr0, const int32_t* perm0,
                         const int32_t* ptr1, const int32_t* perm1, const float* z, const float* x, int64_t N, int64_t W,
                         const int64_t* splits, int64_t G, int pool_op, float* p, float* ni, float* out,
                         mpStream_t stream) {
  const char* what = "mp_megan_readout_f32";
  MP_REQUIRE(K >= 1 && K <= MAXK, "%s: 1 to %d channels, got %d", what, MAXK, K);
  MP_REQUIRE(W >= 4 && W % 4 == 0 && W <= MP_MEGAN_MAX_WIDTH, "%s: W must be a multiple of 4 up to %d, got %lld", what,
             MP_MEGAN_MAX_WIDTH, (long long)W);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: the graph pool is MP_SUM or MP_MEAN, got %d", what, pool_op);
  MP_REQUIRE(sizes_ok(N, M, K) && G >= 0 && G < (int64_t{1} << 31), "%s: bad sizes N=%lld M=%lld G=%lld", what,
             (long long)N, (long long)M, (long long)G);
  if (G == 0) return MP_OK;
  MP_REQUIRE(splits && out, "%s: null pointer", what);
  MP_REQUIRE(N == 0 || (ptr0 && ptr1 && z && x && ni), "%s: null pointer", what);
  MP_REQUIRE(M == 0 || ei, "%s: null pointer", what);
  MP_REQUIRE(mp::aligned16(x) && mp::aligned16(out), "%s: x and out must be 16-byte aligned", what);
  ReadoutArgs a{};
  a.ei = ei; a.ptr0 = ptr0; a.perm0 = perm0; a.ptr1 = ptr1; a.perm1 = perm1; a.z = z; a.x = x; a.splits = splits;
  a.p = p; a.ni = ni; a.out = out;
  a.M = static_cast<int>(M); a.N = static_cast<int>(N); a.G = static_cast<int>(G);
  a.W = static_cast<int>(W); a.mean = pool_op == MP_MEAN ? 1 : 0;
  const unsigned grid = mp::grid_for(G * 64);
  const hipStream_t st = mp::as_stream(stream);
#define MP_MEGAN_READOUT(KK)                                                   \
  case KK:                                                                     \
    if (W <= 256) megan_readout_kernel<1, KK><<<grid, 256, 0, st>>>(a);        \
    else megan_readout_kernel<2, KK><<<grid, 256, 0, st>>>(a);                 \
    break;
  switch (K) {
    MP_MEGAN_READOUT(1) MP_MEGAN_READOUT(2) MP_MEGAN_READOUT(3) MP_MEGAN_READOUT(4)
    MP_MEGAN_READOUT(5) MP_MEGAN_READOUT(6) MP_MEGAN_READOUT(7) MP_MEGAN_READOUT(8)
  }
#undef MP_MEGAN_READOUT
  return mp::check_launch(what);
}

int mp_megan_readout_grad_f32(const float* g_out, const float* g_ni, const float* x, const float* z, const float* p,
                              int64_t N, int K, int64_t W, const int64_t* splits, int64_t G, int pool_op, float* x_bar,
                              float* z_bar, float* q, mpStream_t stream) {
  const char* what = "mp_megan_readout_grad_f32";
  MP_REQUIRE(K >= 1 && K <= MAXK, "%s: 1 to %d channels, got %d", what, MAXK, K);
  MP_REQUIRE(W >= 4 && W % 4 == 0 && W <= MP_MEGAN_MAX_WIDTH, "%s: W must be a multiple of 4 up to %d, got %lld", what,
             MP_MEGAN_MAX_WIDTH, (long long)W);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: the graph pool is MP_SUM or MP_MEAN, got %d", what, pool_op);
  MP_REQUIRE(sizes_ok(N, 0, K) && G >= 0 && G < (int64_t{1} << 31), "%s: bad sizes N=%lld G=%lld", what, (long long)N,
             (long long)G);
  if (N == 0) return MP_OK;
  MP_REQUIRE(G > 0, "%s: %lld nodes and no graph", what, (long long)N);
  MP_REQUIRE(g_out && x && z && p && splits && x_bar && z_bar && q, "%s: null pointer", what);
  MP_REQUIRE(mp::aligned16(g_out) && mp::aligned16(x) && mp::aligned16(x_bar), "%s: g_out, x and x_bar must be 16-byte aligned",
             what);
  ReadoutGradArgs a{};
  a.g_out = g_out; a.g_ni = g_ni; a.x = x; a.z = z; a.p = p; a.splits = splits; a.x_bar = x_bar; a.z_bar = z_bar; a.q = q;
  a.N = N; a.G = G; a.K = K; a.W = static_cast<int>(W); a.mean = pool_op == MP_MEAN ? 1 : 0;
  megan_readout_grad_kernel<<<mp::grid_for(N * 64), 256, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch(what);
}

int mp_megan_edge_importance_grad_f32(const float* g_ei, const float* q, const float* ei, const int32_t* cols,
                                      const int32_t* ptr0, const int32_t* ptr1, int64_t N, int64_t M, int K, float* s_bar,
                                      mpStream_t stream) {
  const char* what = "mp_megan_edge_importance_grad_f32";
  MP_REQUIRE(K >= 1 && K <= MAXK, "%s: 1 to %d channels, got %d", what, MAXK, K);
  MP_REQUIRE(sizes_ok(N, M, K), "%s: bad sizes N=%lld M=%lld", what, (long long)N, (long long)M);
  if (M == 0) return MP_OK;
  MP_REQUIRE(q && ei && cols && ptr0 && ptr1 && s_bar, "%s: null pointer", what);
  MP_REQUIRE(N > 0, "%s: %lld edges and no node", what, (long long)M);
  megan_edge_importance_grad_kernel<<<mp::grid_for(M * K), 256, 0, mp::as_stream(stream)>>>(g_ei, q, ei, cols, ptr0, ptr1,
                                                                                          N, M, K, s_bar);
  return mp::check_launch(what);
}

}  // extern "C"
