// DMPNN (kgcnn/literature/DMPNN.py:136-142): the reverse of the directed edge update of csrc/mp_cmpnn.hip,
//   y[e] = act2(act1((R[send e] - h[rev e]) W + b) + h0[e]),   act1 = linear, act2 in {linear, relu}.
//
// mp_directed_edge_update_grad_f32 - what the tape computes through Activation, LazyAdd and Dense (kgcnn/layers/
// modules.py:15-90):
//   p[e] = g[e] * act2'(y[e])      the gradient of h0 and of the pre-activation (relu: taken from the output, y > 0)
//   q[e] = p[e] W^T                the gradient of the difference d[e] = R[send e] - h[rev e]
// The forward kernel's tiling run the other way: a 64-edge x 64-column tile of q per 256-thread workgroup, 2 x 2 waves of
// one 32 x 32 accumulator, k slabs of 64 staged through LDS, the next slab's loads issued in front of the current slab's
// MFMAs, every load unconditional from a clamped address.  The A tile is formed while it is staged (g and y are loaded,
// g * act2'(y) is stored); the workgroups of column tile 0 walk every k slab of their rows and write p out on the way.
// B is W read by rows: q's column j contracts row j of W, so the B tile is staged row-major like the A tile and read
// with the A tile's pattern.  The Activation gradient, the LazyAdd fan-out and the Dense input gradient - two edge-sized
// tensors and three launches of the layer sequence - are one launch.
//
// mp_directed_edge_hgrad_f32 - the last line of the reverse:
//   h_bar[e] = R_bar[recv e] - sum over e' with rev e' = e of q[e']
// The first term is the adjoint of the receiver sum R (a gather at the receiver), the second the adjoint of the pair
// gather as a segment sum over the CSR of rev (edges without a reverse lie in the extra segment E, which nobody reads):
// right for any rev, an involution or not.  One work item owns (edge, 16-byte chunk); rows are added in CSR order.
#include "mp_common.h"
#include "../../include/mpengine/cmpnn.h"
#include "../../include/mpengine/dmpnn.h"

namespace {

using floatx16 = __attribute__((ext_vector_type(16))) float;

constexpr int BM = 64, BN = 64, BK = 64;   // BM = the edge tile (MP_CMPNN_EDGE_TILE)
constexpr int T_LD = BK + 1;               // both tiles are row-major over k: the MFMA reads walk rows 1 bank apart
static_assert(BM == MP_CMPNN_EDGE_TILE, "the header names the edge tile");

__device__ __forceinline__ float4 mask_grad(float4 g, float4 y, bool relu) {
  // g * (y > 0), the product itself: the bits of the layer sequence's derivative kernel
  if (!relu) return g;
  return make_float4(g.x * (y.x > 0.0f ? 1.0f : 0.0f), g.y * (y.y > 0.0f ? 1.0f : 0.0f),
                     g.z * (y.z > 0.0f ? 1.0f : 0.0f), g.w * (y.w > 0.0f ? 1.0f : 0.0f));
}

__global__ __launch_bounds__(256) void directed_edge_update_grad_kernel(
    const float* __restrict__ g, const float* __restrict__ y, int E, int F, const float* __restrict__ W, int relu,
    float* __restrict__ p, float* __restrict__ q) {
  __shared__ __align__(16) float As[BM * T_LD];
  __shared__ __align__(16) float Bs[BN * T_LD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int row0 = static_cast<int>(blockIdx.x) * BM;
  const int col0 = static_cast<int>(blockIdx.y) * BN;
  const bool write_p = blockIdx.y == 0;

  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;

  constexpr int NV = (BM * BK) / (256 * 4);   // float4 per thread and tile (A and B tiles have the same size)
  // a thread's tile rows are the same in every k slab: the edge row of g / y / p and the row of W, clamped
  size_t arow[NV], brow[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int r = (tid + i * 256) / (BK / 4);
    arow[i] = static_cast<size_t>(row0 + r < E ? row0 + r : E - 1) * F;
    brow[i] = static_cast<size_t>(col0 + r < F ? col0 + r : F - 1) * F;
  }

  float4 rg4[NV], ry4[NV], rb4[NV];
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int gk = k0 + ((tid + i * 256) % (BK / 4)) * 4;
      gk = gk < F ? gk : F - 4;
      rg4[i] = *reinterpret_cast<const float4*>(g + arow[i] + gk);
      ry4[i] = relu ? *reinterpret_cast<const float4*>(y + arow[i] + gk) : make_float4(0.f, 0.f, 0.f, 0.f);
      rb4[i] = *reinterpret_cast<const float4*>(W + brow[i] + gk);
    }
  };
  auto store_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      const int r = idx / (BK / 4), c = (idx % (BK / 4)) * 4;
      const bool k_ok = (k0 + c) < F;
      const bool ok = (row0 + r) < E && k_ok;
      const float4 v = mask_grad(rg4[i], ry4[i], relu != 0);
      if (write_p && ok) *reinterpret_cast<float4*>(p + arow[i] + k0 + c) = v;
      float* a = As + r * T_LD + c;
      a[0] = ok ? v.x : 0.0f;
      a[1] = ok ? v.y : 0.0f;
      a[2] = ok ? v.z : 0.0f;
      a[3] = ok ? v.w : 0.0f;
      const bool okb = (col0 + r) < F && k_ok;
      const float4 w = rb4[i];
      float* b = Bs + r * T_LD + c;
      b[0] = okb ? w.x : 0.0f;
      b[1] = okb ? w.y : 0.0f;
      b[2] = okb ? w.z : 0.0f;
      b[3] = okb ? w.w : 0.0f;
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
    // A[row = lane & 31][k = lane >> 5] and B[k = lane >> 5][col = lane & 31] = W[col0 + col][k0 + k]
    const float* a_ptr = As + (wr * 32 + (lane & 31)) * T_LD + (lane >> 5);
    const float* b_ptr = Bs + (wc * 32 + (lane & 31)) * T_LD + (lane >> 5);
    if (steps == BK / 2) {
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_ptr[kk * 2], b_ptr[kk * 2], acc, 0, 0, 0);
    } else {   // last, partial k slab (zero padded)
      for (int kk = 0; kk < steps; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_ptr[kk * 2], b_ptr[kk * 2], acc, 0, 0, 0);
    }
    __syncthreads();
  }

  const int col = col0 + wc * 32 + (lane & 31);
  if (col < F) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row < E) q[static_cast<size_t>(row) * F + col] = acc[r];
    }
  }
}

__global__ __launch_bounds__(256) void directed_edge_hgrad_kernel(
    const float* __restrict__ rbar, int64_t N, const float* __restrict__ q, int64_t E, int64_t F,
    const int32_t* __restrict__ recv, const int32_t* __restrict__ ptr, const int32_t* __restrict__ perm,
    float* __restrict__ out, int32_t* __restrict__ flags) {
  const int64_t chunks = F / 4;
  const int64_t total = E * chunks;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  int local_flags = 0;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t c = t % chunks;
    const int64_t e = t / chunks;
    int64_t n = recv[e];
    if (n < 0 || n >= N) { local_flags |= MP_FLAG_OOB; n = n < 0 ? 0 : N - 1; }
    int64_t a = ptr[e], b = ptr[e + 1];
    a = a < 0 ? 0 : (a > E ? E : a);
    b = b < a ? a : (b > E ? E : b);
    const float4 rv = *reinterpret_cast<const float4*>(rbar + n * F + c * 4);
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t j = a; j < b; ++j) {
      int64_t r = perm ? static_cast<int64_t>(perm[j]) : j;
      r = r < 0 ? 0 : (r >= E ? E - 1 : r);
      const float4 v = *reinterpret_cast<const float4*>(q + r * F + c * 4);
      s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
    }
    *reinterpret_cast<float4*>(out + e * F + c * 4) = make_float4(rv.x - s[0], rv.y - s[1], rv.z - s[2], rv.w - s[3]);
  }
  if (flags != nullptr) mp_publish_flags(flags, local_flags);
}

}  // namespace

extern "C" {

int mp_directed_edge_update_grad_f32(const float* g, const float* y, int64_t E, int64_t F, const float* W, int act2,
                                     float* p, float* q, mpStream_t stream) {
  const char* what = "mp_directed_edge_update_grad_f32";
  MP_REQUIRE(E >= 0 && F >= 4 && F % 4 == 0, "%s: bad sizes E=%lld F=%lld (F a multiple of 4)", what, (long long)E,
             (long long)F);
  MP_REQUIRE(E < (int64_t{1} << 31) - BM && F <= (1 << 20), "%s: edges are indexed with 32 bits", what);
  MP_REQUIRE(act2 == MP_ACT_LINEAR || act2 == MP_ACT_RELU,
             "%s: the derivative is taken from the output for linear and relu, got activation %d", what, act2);
  if (E == 0) return MP_OK;
  const bool relu = act2 == MP_ACT_RELU;
  MP_REQUIRE(g && W && p && q && (y || !relu), "%s: null pointer", what);
  MP_REQUIRE(mp::aligned16(g) && mp::aligned16(y) && mp::aligned16(W) && mp::aligned16(p),
             "%s: operands must be 16-byte aligned", what);
  const int64_t gx = mp::ceil_div(E, BM), gy = mp::ceil_div(F, BN);
  MP_REQUIRE(gy <= 65535, "%s: grid too large", what);
  dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
  directed_edge_update_grad_kernel<<<grid, 256, 0, mp::as_stream(stream)>>>(g, y, static_cast<int>(E),
                                                                            static_cast<int>(F), W, relu ? 1 : 0, p, q);
  return mp::check_launch(what);
}

int mp_directed_edge_hgrad_f32(const float* rbar, int64_t N, const float* q, int64_t E, int64_t F, const int32_t* recv,
                               const int32_t* rev_ptr, const int32_t* rev_perm, float* out, int32_t* flags,
                               mpStream_t stream) {
  const char* what = "mp_directed_edge_hgrad_f32";
  MP_REQUIRE(N >= 0 && E >= 0 && F >= 4 && F % 4 == 0, "%s: bad sizes N=%lld E=%lld F=%lld (F a multiple of 4)", what,
             (long long)N, (long long)E, (long long)F);
  if (E == 0) return MP_OK;
  MP_REQUIRE(rbar && q && recv && rev_ptr && out, "%s: null pointer", what);
  MP_REQUIRE(N > 0, "%s: %lld edges and no node", what, (long long)E);
  MP_REQUIRE(mp::aligned16(rbar) && mp::aligned16(q) && mp::aligned16(out), "%s: operands must be 16-byte aligned", what);
  directed_edge_hgrad_kernel<<<mp::grid_for(E * (F / 4)), 256, 0, mp::as_stream(stream)>>>(rbar, N, q, E, F, recv, rev_ptr,
                                                                                          rev_perm, out, flags);
  return mp::check_launch(what);
}

}  // extern "C"
