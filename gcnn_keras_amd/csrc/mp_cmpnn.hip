// CMPNN (kgcnn/literature/CMPNN.py:126-150): one communicate round in two launches.
//
// mp_cmpnn_boost_f32 - the node booster (CMPNN.py:131-135, :148-150):
//   h'[n] = h[n] + pool(he)[n] * max(he)[n],  pool = sum or mean over {e : recv e = n}
// One work item owns (receiver, 16-byte feature chunk) and walks the receiver's CSR segment ONCE, folding every row into a
// sum and a max accumulator - the two PoolingLocalEdges of the layer sequence read the edge states twice.  The walk is the
// one of csrc/mp_segment.hip (rows fetched eight or sixteen at a time, folded in edge order, the first row initialises both
// accumulators, a receiver without edges gives 0 for both, unsorted lists through the plan's permutation), and with
// -ffp-contract=off every operation is the one PoolingLocalEdges / LazyMultiply / LazyAdd perform, in their order: the
// result has the bits of the layer sequence.
//
// mp_directed_edge_update_f32 - the edge update (CMPNN.py:138-143; the same directed update as DMPNN's):
//   out[e] = act2(act1((h'[send e] - he[rev e]) W + b) + he0[e]),   he[rev e] := 0 where rev e < 0
// The tiled FP32-MFMA GEMM of csrc/mp_dense.hip (64 x 64 output tile per 256-thread workgroup, 2 x 2 waves of one 32 x 32
// accumulator, k slabs of 64 staged through LDS, the next slab's loads issued in front of the current slab's MFMAs) with
// three changes: the A tile is formed while it is staged, from the sender's row minus the reverse edge's row (the row
// indices of a thread's four A rows are read once, in front of the k loop); the residual he0 is added in the epilogue; two
// activations are applied there.  W (F x F, 360 KB at F = 300) is streamed slab by slab like mp_dense's.  The gather, the
// pair gather, its mask product, the difference, the Dense output, the residual sum and the activation - seven edge-sized
// tensors - are never written.  `out` must not alias `he`: other tiles gather he[rev] while this one writes.
#include <type_traits>

#include "mp_common.h"
#include "../../include/mpengine/cmpnn.h"

namespace {

using floatx16 = __attribute__((ext_vector_type(16))) float;

// ------------------------------------------------------------------------------------------------ node booster
template <bool PERM>
__global__ __launch_bounds__(256) void cmpnn_boost_kernel(const float* __restrict__ h, const float* __restrict__ he,
                                                          int64_t M, int64_t F, const int32_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ perm, int64_t N, int mean,
                                                          int m_only, float* __restrict__ out) {
  const int64_t chunks = F / 4;
  const int64_t total = N * chunks;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t c = t % chunks;
    const int64_t n = t / chunks;
    int64_t a = static_cast<int64_t>(ptr[n]);
    int64_t b = static_cast<int64_t>(ptr[n + 1]);
    a = a < 0 ? 0 : (a > M ? M : a);
    b = b < a ? a : (b > M ? M : b);
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* base = he + c * 4;
    // as segment_reduce_csr_kernel: unconditional phases (tail slots repeat the segment's last row and are masked in the
    // fold), so the UB index loads and then the UB row loads are in flight together
    auto fold = [&](int64_t e0, auto ub_tag) {
      constexpr int UB = decltype(ub_tag)::value;
      float4 v[UB];
      int64_t rr[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int64_t ec = e0 + u < b ? e0 + u : b - 1;
        int64_t r = PERM ? static_cast<int64_t>(perm[ec]) : ec;
        rr[u] = r < 0 ? 0 : (r >= M ? M - 1 : r);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) v[u] = *reinterpret_cast<const float4*>(base + rr[u] * F);
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        if (e0 + u < b) {
          const float w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
          if (e0 + u == a) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { sum[i] = w[i]; mx[i] = w[i]; }
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { sum[i] += w[i]; mx[i] = fmaxf(mx[i], w[i]); }
          }
        }
      }
    };
    int64_t e0 = a;
    for (; b - e0 >= 16; e0 += 16) fold(e0, std::integral_constant<int, 16>());
    for (; e0 < b; e0 += 8) fold(e0, std::integral_constant<int, 8>());
    if (mean && b > a) {
      const float cnt = static_cast<float>(b - a);
#pragma unroll
      for (int i = 0; i < 4; ++i) sum[i] = sum[i] / cnt;
    }
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = sum[i] * mx[i];
    if (!m_only) {
      const float4 hv = *reinterpret_cast<const float4*>(h + n * F + c * 4);
      r[0] = hv.x + r[0]; r[1] = hv.y + r[1]; r[2] = hv.z + r[2]; r[3] = hv.w + r[3];
    }
    *reinterpret_cast<float4*>(out + n * F + c * 4) = make_float4(r[0], r[1], r[2], r[3]);
  }
}

// ------------------------------------------------------------------------------------------------ edge update
constexpr int BM = 64, BN = 64, BK = 64;   // BM = the edge tile (MP_CMPNN_EDGE_TILE)
constexpr int A_LD = BK + 1;
static_assert(BM == MP_CMPNN_EDGE_TILE, "the header names the edge tile");

__global__ __launch_bounds__(256) void directed_edge_update_kernel(
    const float* __restrict__ h, int N, const float* __restrict__ he, const float* __restrict__ he0, int E, int F,
    const int32_t* __restrict__ send, const int32_t* __restrict__ rev, const float* __restrict__ W,
    const float* __restrict__ bias, int act1, int act2, float alpha, float* __restrict__ out,
    int32_t* __restrict__ flags) {
  __shared__ __align__(16) float As[BM * A_LD];
  __shared__ __align__(16) float Bs[BK * BN];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int row0 = static_cast<int>(blockIdx.x) * BM;
  const int col0 = static_cast<int>(blockIdx.y) * BN;

  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;

  constexpr int NV = (BM * BK) / (256 * 4);   // float4 per thread and tile (A and B tiles have the same size)
  // the thread's A rows are the same in every k slab: sender and reverse position once, clamped into their tensors
  // (an index out of range is clamped and flagged, never followed)
  size_t srow[NV], rrow[NV];
  bool has_rev[NV];
  int local_flags = 0;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int ar = (tid + i * 256) / (BK / 4);
    const int e = row0 + ar < E ? row0 + ar : E - 1;
    int s = send[e], r = rev[e];
    if (s < 0 || s >= N) { local_flags |= MP_FLAG_OOB; s = s < 0 ? 0 : N - 1; }
    if (r >= E) { local_flags |= MP_FLAG_OOB; r = E - 1; }
    has_rev[i] = r >= 0;
    srow[i] = static_cast<size_t>(s) * F;
    rrow[i] = static_cast<size_t>(r < 0 ? 0 : r) * F;
  }
  if (flags != nullptr && blockIdx.y == 0) mp_publish_flags(flags, local_flags);

  float4 ra4[NV], rr4[NV], rb4[NV];
  // every load is unconditional, from an address clamped into the operand; what lies outside is zeroed at the LDS store
  // (csrc/mp_dense.hip: a guarded load costs a branch and a full wait per load)
  auto load_tile = [&](int k0) {
    const int k_last = F - 4, c_last = F - 4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      int gk = k0 + (idx % (BK / 4)) * 4;
      gk = gk < F ? gk : k_last;
      ra4[i] = *reinterpret_cast<const float4*>(h + srow[i] + gk);
      rr4[i] = *reinterpret_cast<const float4*>(he + rrow[i] + gk);
      int gk2 = k0 + idx / (BN / 4), gc = col0 + (idx % (BN / 4)) * 4;
      gk2 = gk2 < F ? gk2 : F - 1;
      gc = gc < F ? gc : c_last;
      rb4[i] = *reinterpret_cast<const float4*>(W + static_cast<size_t>(gk2) * F + gc);
    }
  };
  auto store_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      const int ar = idx / (BK / 4), ac = (idx % (BK / 4)) * 4;
      const bool ok = (row0 + ar) < E && (k0 + ac) < F;
      const float4 x = ra4[i];
      const float4 y = has_rev[i] ? rr4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      float* d = As + ar * A_LD + ac;
      d[0] = ok ? x.x - y.x : 0.0f;
      d[1] = ok ? x.y - y.y : 0.0f;
      d[2] = ok ? x.z - y.z : 0.0f;
      d[3] = ok ? x.w - y.w : 0.0f;
      const bool okb = (k0 + idx / (BN / 4)) < F && (col0 + (idx % (BN / 4)) * 4) < F;
      *reinterpret_cast<float4*>(Bs + idx * 4) = okb ? rb4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  const int ktiles = (F + BK - 1) / BK;
  load_tile(0);
  for (int t = 0; t < ktiles; ++t) {
    store_tile(t * BK);
    __syncthreads();
    if (t + 1 < ktiles) load_tile((t + 1) * BK);
    const int left = F - t * BK;
    const int steps = left >= BK ? BK / 2 : (left + 1) / 2;   // k pairs that hold data
    const float* a_ptr = As + (wr * 32 + (lane & 31)) * A_LD + (lane >> 5);
    const float* b_ptr = Bs + (lane >> 5) * BN + wc * 32 + (lane & 31);
    if (steps == BK / 2) {
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_ptr[kk * 2], b_ptr[kk * 2 * BN], acc, 0, 0, 0);
    } else {   // last, partial k slab (zero padded)
      for (int kk = 0; kk < steps; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_ptr[kk * 2], b_ptr[kk * 2 * BN], acc, 0, 0, 0);
    }
    __syncthreads();
  }

  const int col = col0 + wc * 32 + (lane & 31);
  if (col < F) {
    const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row < E) {
        const size_t at = static_cast<size_t>(row) * F + col;
        float v = mp_apply_act(act1, alpha, acc[r] + bv);   // Dense(**edge_dense)
        v = v + he0[at];                                     // LazyAdd([he, he0])
        out[at] = mp_apply_act(act2, alpha, v);              // Activation(**edge_activation)
      }
    }
  }
}

bool overlap(const float* a, const float* b, size_t n) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), len = n * sizeof(float);
  return x < y + len && y < x + len;
}

}  // namespace

extern "C" {

int mp_cmpnn_boost_f32(const float* h, const float* he, int64_t M, int64_t F, const int32_t* ptr, const int32_t* perm,
                       int64_t N, int pool_op, int m_only, float* out, mpStream_t stream) {
  const char* what = "mp_cmpnn_boost_f32";
  MP_REQUIRE(M >= 0 && N >= 0 && F >= 4 && F % 4 == 0, "%s: bad sizes M=%lld N=%lld F=%lld (F a multiple of 4)", what,
             (long long)M, (long long)N, (long long)F);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: pooling is sum or mean, got op %d", what, pool_op);
  if (N == 0) return MP_OK;
  MP_REQUIRE(ptr && out && (m_only || h) && (M == 0 || he), "%s: null pointer", what);
  MP_REQUIRE(mp::aligned16(he) && mp::aligned16(out) && mp::aligned16(h), "%s: operands must be 16-byte aligned", what);
  const unsigned grid = mp::grid_for(N * (F / 4));
  hipStream_t s = mp::as_stream(stream);
  const int mean = pool_op == MP_MEAN ? 1 : 0;
  if (perm) cmpnn_boost_kernel<true><<<grid, 256, 0, s>>>(h, he, M, F, ptr, perm, N, mean, m_only ? 1 : 0, out);
  else cmpnn_boost_kernel<false><<<grid, 256, 0, s>>>(h, he, M, F, ptr, perm, N, mean, m_only ? 1 : 0, out);
  return mp::check_launch(what);
}

int mp_directed_edge_update_f32(const float* h, int64_t N, const float* he, const float* he0, int64_t E, int64_t F,
                                const int32_t* send, const int32_t* rev, const float* W, const float* b, int act1,
                                int act2, float alpha, float* out, int32_t* flags, mpStream_t stream) {
  const char* what = "mp_directed_edge_update_f32";
  MP_REQUIRE(N >= 0 && E >= 0 && F >= 4 && F % 4 == 0, "%s: bad sizes N=%lld E=%lld F=%lld (F a multiple of 4)", what,
             (long long)N, (long long)E, (long long)F);
  MP_REQUIRE(N < (int64_t{1} << 31) - 1 && E < (int64_t{1} << 31) - BM && F <= (1 << 20),
             "%s: nodes and edges are indexed with 32 bits", what);
  MP_REQUIRE(act1 >= MP_ACT_LINEAR && act1 <= MP_ACT_LAST && act2 >= MP_ACT_LINEAR && act2 <= MP_ACT_LAST,
             "%s: unknown activation %d / %d", what, act1, act2);
  if (E == 0) return MP_OK;
  MP_REQUIRE(h && he && he0 && send && rev && W && out, "%s: null pointer", what);
  MP_REQUIRE(N > 0, "%s: %lld edges and no node", what, (long long)E);
  const size_t n = static_cast<size_t>(E) * static_cast<size_t>(F);
  MP_REQUIRE(!overlap(out, he, n), "%s: out must not alias he (other tiles gather he[rev] while a tile is written)", what);
  MP_REQUIRE(mp::aligned16(h) && mp::aligned16(he) && mp::aligned16(W), "%s: operands must be 16-byte aligned", what);
  const int64_t gx = mp::ceil_div(E, BM), gy = mp::ceil_div(F, BN);
  MP_REQUIRE(gy <= 65535, "%s: grid too large", what);
  dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
  directed_edge_update_kernel<<<grid, 256, 0, mp::as_stream(stream)>>>(
      h, static_cast<int>(N), he, he0, static_cast<int>(E), static_cast<int>(F), send, rev, W, b, act1, act2, alpha, out,
      flags);
  return mp::check_launch(what);
}

}  // extern "C"
