// MXMNet (kgcnn/layers/conv/mxmnet_conv.py:11-192): the multiplex edge message with its two epilogues, the triplet pool
// of the local message passing, and their reverses.
//
// Edge message, one launch (plus a node-sized finishing pass for the pool epilogue):
//   z_e = Pa[i_e] + Pb[j_e] + a_e Wc + b,   y_e = act(z_e) * (a_e Wl)   (no gate without Wl),
//   pool: out[r] = base[r] + sum / mean over {e : i_e = r} of y_e;   edge: y (E, W) in list order.
// Pa = x W_a and Pb = x W_b are made on the node side by two Dense launches on row blocks of the Dense kernel (in place:
// no repacked copy that could go stale under graph replay).  One workgroup of W / 32 waves walks tiles of 32 positions
// (receiver-sorted for the pool, list order for the edge epilogue):
//   phase 0  indices of the tile                                                                            -> LDS
//   phase 1  the tile's attribute rows, transposed and zero-padded to the k bucket                          -> aT[k][e]
//   phase 2  a [Wc | Wl] on the matrix pipe: v_mfma_f32_32x32x2_f32, positions = rows, wave w owns columns [32w, 32w+32)
//            of both kernels, resident in 2 x KP/2 registers per lane for the whole kernel; the two gathered rows of
//            every position are requested before the products and added in the accumulator layout
//   phase 3  bias, activation, gate -> y (edge) or the edge-major tile in LDS (pool); z and the gate saved on a tape
//   phase 4  pool: per-receiver sums in list order by W threads, the walk of csrc/mp_edge_tile.h; mxm_edge_finish_kernel
//            writes the receivers cut by a tile boundary, divides for the mean, adds base and fills receivers without
//            edges.  No atomics: two runs give equal bits.
//
// Reverse: per tile of 32 edges in list order, from the saved z and gate: z_bar = g_e * l * act'(z), l_bar = g_e * act(z),
// and a_bar = [z_bar | l_bar] [Wc | Wl]^T on the matrix pipe (wave w owns attribute columns [32w, 32w+32)).  The sums of
// z_bar into Pa_bar / Pb_bar run on the segment-sum kernel over the two CSRs (host side), in list order.
//
// Triplet pool: out[n] = sum / mean over {t : A[t,0] = n} of x[A[t,1]] * s[t], one thread per (edge, column) over the CSR
// of angle column 0 in list order.  mp_gather_segment_reduce_csr_f32 (csrc/mp_segment.hip) gathers and reduces, but
// its multiplicand is one scalar per position; here it is a row of s, so the step has a kernel of its own.
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/mxmnet.h"

namespace {

constexpr int TE = mp_tile::TE;   // positions per tile
constexpr int HS = TE + 1;        // row stride of the transposed tiles
constexpr int MAXK = 128;         // widest attribute row

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------- edge message
struct EdgeArgs {
  const float* Pa;       // (N, W), gathered by column 0
  const float* Pb;       // (N, W), gathered by column 1
  const float* a;        // (E, Ka)
  const float* Wc;       // (Ka, W)
  const float* Wl;       // (Ka, W) nullable: no gate
  const float* b;        // (W) nullable
  const int32_t* col0;   // (2, E) column 0 | column 1
  const int32_t* ptr0;   // (N+1) CSR of column 0 over sorted positions (pool)
  const int32_t* perm0;  // (E) sorted position -> edge, nullable (pool)
  const float* g;        // reverse: (N, W) or (E, W)
  const float* z;        // reverse: (E, W)
  const float* l;        // reverse: (E, W), with Wl
  float* out;            // pool: (N, W)
  float* y;              // edge: (E, W)
  float* bnd;            // pool: (tiles, 2, W)
  float* z_save;         // nullable
  float* l_save;         // nullable
  float* z_bar;          // reverse: (E, W)
  float* a_bar;          // reverse: (E, Ka) nullable
  int N, E, Ka;          // N, E below 2^31 (checked on the host)
  int act, pooled, mean;
  float alpha;
};

// row of accumulator element i in lane `lane` of a 32x32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int i, int lane) { return 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3); }

template <int W, int KP>
__global__ __launch_bounds__(2 * W) void mxm_edge_fwd_kernel(EdgeArgs a) {
  constexpr int NT = 2 * W;        // threads: one wave per 32 output columns
  constexpr int MS = W + 1;        // row stride of the edge-major tile
  __shared__ float aT[KP * HS];
  __shared__ float yL[TE * MS];
  __shared__ int recvL[TE], sndL[TE], eidL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int col = 32 * wave + (lane & 31);
  const int Ka = a.Ka;
  const bool gate = a.Wl != nullptr;
  const bool pool = a.out != nullptr;

  float wv[KP / 2], wg[KP / 2];
#pragma unroll
  for (int s = 0; s < KP / 2; ++s) {
    const int k = 2 * s + (lane >> 5);
    wv[s] = k < Ka ? a.Wc[(size_t)k * W + col] : 0.0f;
    wg[s] = (gate && k < Ka) ? a.Wl[(size_t)k * W + col] : 0.0f;
  }
  const float bias = a.b ? a.b[col] : 0.0f;

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's walk is done with the tiles in LDS
    // phase 0
    if (t < TE) {
      const mp_tile::Pos p = mp_tile::load_pos(a.col0, pool ? a.perm0 : nullptr, a.N, a.E, p0, t, nv);
      recvL[t] = p.r; sndL[t] = p.s; eidL[t] = p.e;
    }
    __syncthreads();
    // phase 1: (position, k) with k fastest: rows are read along k, the transposed store has stride HS
    for (int i = t; i < TE * KP; i += NT) {
      const int e = i / KP, k = i - e * KP;
      float v = 0.0f;
      if (k < Ka && recvL[e] >= 0) v = a.a[(size_t)eidL[e] * Ka + k];
      aT[k * HS + e] = v;
    }
    // the gathered rows of this lane's 16 positions, in flight under the products (skipped rows read row 0)
    float pa[16], pb[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = acc_row(i, lane);
      const int r = recvL[e] < 0 ? 0 : recvL[e];
      pa[i] = a.Pa[(size_t)r * W + col];
      pb[i] = a.Pb[(size_t)sndL[e] * W + col];
    }
    __syncthreads();
    // phase 2
    f32x16 accv, accg;
#pragma unroll
    for (int i = 0; i < 16; ++i) { accv[i] = 0.0f; accg[i] = 0.0f; }
    {
      const float* ap = aT + (lane >> 5) * HS + (lane & 31);
#pragma unroll
      for (int s = 0; s < KP / 2; ++s) accv = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * HS], wv[s], accv, 0, 0, 0);
      if (gate) {
#pragma unroll
        for (int s = 0; s < KP / 2; ++s) accg = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * HS], wg[s], accg, 0, 0, 0);
      }
    }
    // phase 3
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = acc_row(i, lane);
      const bool valid = recvL[e] >= 0;
      const float z = ((pa[i] + pb[i]) + accv[i]) + bias;
      float v = mp_apply_act(a.act, a.alpha, z);
      if (gate) v *= accg[i];
      if (!valid) v = 0.0f;
      if (e < nv) {
        const size_t at = (size_t)eidL[e] * W + col;
        if (a.z_save && valid) a.z_save[at] = z;
        if (a.l_save && gate && valid) a.l_save[at] = accg[i];
        if (!pool) a.y[at] = v;
      }
      if (pool) yL[e * MS + col] = v;
    }
    if (!pool) continue;
    __syncthreads();
    // phase 4
    if (t < W) mp_tile::walk<W>(recvL, nv, a.ptr0, a.out, a.bnd, tile, t, [=](int e) { return yL[e * MS + t]; });
  }
}

// Receivers cut by a tile boundary: their slots in tile order; the mean's division; base; receivers without edges.
template <int W>
__global__ void mxm_edge_finish_kernel(const int32_t* __restrict__ ptr0, int64_t N, const float* __restrict__ bnd,
                                       const float* __restrict__ base, int mean, float* __restrict__ out) {
  const int64_t total = N * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / W;
    const int col = static_cast<int>(i - r * W);
    const int64_t s0 = ptr0[r], s1 = ptr0[r + 1];
    if (s1 <= s0) { out[i] = base ? base[i] : 0.0f; continue; }
    float sum;
    if (!mp_tile::cut_sum<W>(bnd, s0, s1, col, &sum)) sum = out[i];
    if (mean) sum = sum / static_cast<float>(s1 - s0);
    out[i] = base ? sum + base[i] : sum;
  }
}

template <int W>
__global__ __launch_bounds__(256) void mxm_edge_bwd_kernel(EdgeArgs a) {
  __shared__ float dT[2 * W * HS];   // [z_bar | l_bar], transposed
  __shared__ int recvL[TE];
  __shared__ float scaleL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int Ka = a.Ka;
  const bool gate = a.Wl != nullptr;
  const bool want_a = a.a_bar != nullptr;
  const int j = 32 * wave + (lane & 31);   // this lane's attribute column

  // B[k][j] = [Wc | Wl]^T: Wc[j][k] for k < W, Wl[j][k - W] behind it
  float wc[W / 2], wl[W / 2];
#pragma unroll
  for (int s = 0; s < W / 2; ++s) {
    const int k = 2 * s + (lane >> 5);
    wc[s] = (want_a && j < Ka) ? a.Wc[(size_t)j * W + k] : 0.0f;
    wl[s] = (want_a && gate && j < Ka) ? a.Wl[(size_t)j * W + k] : 0.0f;
  }

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();
    if (t < TE) {
      int r = -1;
      float sc = 1.0f;
      if (t < nv) {
        r = a.col0[p0 + t];
        const int s = a.col0[a.E + p0 + t];
        if (r < 0 || r >= a.N || s < 0 || s >= a.N) r = -1;
        if (r >= 0 && a.pooled && a.mean) {
          const int c = a.ptr0[r + 1] - a.ptr0[r];
          sc = 1.0f / static_cast<float>(c > 0 ? c : 1);
        }
      }
      recvL[t] = r; scaleL[t] = sc;
    }
    __syncthreads();
    for (int i = t; i < TE * W; i += 256) {
      const int e = i / W, k = i - e * W;
      float zb = 0.0f, lb = 0.0f;
      const int r = recvL[e];
      if (r >= 0) {
        const size_t at = (size_t)(p0 + e) * W + k;
        const float ge = a.pooled ? a.g[(size_t)r * W + k] * scaleL[e] : a.g[at];
        const float z = a.z[at];
        const float d = ge * mp_act_grad(a.act, a.alpha, z);
        if (gate) {
          zb = d * a.l[at];
          lb = ge * mp_apply_act(a.act, a.alpha, z);
        } else {
          zb = d;
        }
      }
      if (e < nv) a.z_bar[(size_t)(p0 + e) * W + k] = zb;
      dT[k * HS + e] = zb;
      dT[(W + k) * HS + e] = lb;
    }
    if (!want_a) continue;
    __syncthreads();
    if (32 * wave < Ka) {   // wave-uniform
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
      const float* ap = dT + (lane >> 5) * HS + (lane & 31);
#pragma unroll
      for (int s = 0; s < W / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * HS], wc[s], acc, 0, 0, 0);
      if (gate) {
        const float* lp = ap + W * HS;
#pragma unroll
        for (int s = 0; s < W / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lp[2 * s * HS], wl[s], acc, 0, 0, 0);
      }
      if (j < Ka) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int e = acc_row(i, lane);
          if (e < nv) a.a_bar[(size_t)(p0 + e) * Ka + j] = acc[i];
        }
      }
    }
  }
}

unsigned edge_grid(int64_t E) {
  const int64_t tiles = mp_tile::tiles_of(E);
  return static_cast<unsigned>(tiles < 1024 ? tiles : 1024);
}

template <int W>
void launch_fwd(const EdgeArgs& a, hipStream_t stream) {
  const unsigned grid = edge_grid(a.E);
  if (a.Ka <= 32) mxm_edge_fwd_kernel<W, 32><<<grid, 2 * W, 0, stream>>>(a);
  else if (a.Ka <= 64) mxm_edge_fwd_kernel<W, 64><<<grid, 2 * W, 0, stream>>>(a);
  else mxm_edge_fwd_kernel<W, MAXK><<<grid, 2 * W, 0, stream>>>(a);
}

int check_edge(const char* what, int64_t N, int64_t E, int W, int Ka, int act, int pool_op, bool pooled) {
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(W == 32 || W == 64 || W == 128, "%s: width %d is not one of 32, 64, 128", what, W);
  MP_REQUIRE(Ka >= 1 && Ka <= MAXK, "%s: attribute width %d is not in 1..%d", what, Ka, MAXK);
  MP_REQUIRE(act >= MP_ACT_LINEAR && act <= MP_ACT_LAST, "%s: unknown activation code %d", what, act);
  MP_REQUIRE(!pooled || pool_op == MP_SUM || pool_op == MP_MEAN, "%s: pooling %d is not MP_SUM or MP_MEAN", what, pool_op);
  return MP_OK;
}

// ---------------------------------------------------------------------------------------------- triplet pool
__global__ void mxm_triplet_fwd_kernel(const float* __restrict__ x, int64_t E, int W, const float* __restrict__ s,
                                       const int32_t* __restrict__ cols, int64_t T, const int32_t* __restrict__ ptr0,
                                       const int32_t* __restrict__ perm0, int mean, float* __restrict__ out) {
  const int64_t total = E * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / W;
    const int col = static_cast<int>(i - n * W);
    const int s0 = ptr0[n], s1 = ptr0[n + 1];
    float acc = 0.0f;
    for (int p = s0; p < s1; ++p) {
      const int64_t tr = perm0 ? perm0[p] : p;
      if (tr < 0 || tr >= T) continue;
      const int64_t m = cols[T + tr];
      if (m < 0 || m >= E) continue;
      acc += x[m * W + col] * s[tr * W + col];
    }
    if (mean && s1 > s0) acc = acc / static_cast<float>(s1 - s0);
    out[i] = acc;
  }
}

__device__ __forceinline__ float triplet_scale(const int32_t* ptr0, int64_t n, int mean) {
  if (!mean) return 1.0f;
  const int c = ptr0[n + 1] - ptr0[n];
  return 1.0f / static_cast<float>(c > 0 ? c : 1);
}

__global__ void mxm_triplet_xbar_kernel(int64_t E, int W, const float* __restrict__ s, const int32_t* __restrict__ cols,
                                        int64_t T, const int32_t* __restrict__ ptr0, const int32_t* __restrict__ ptr1,
                                        const int32_t* __restrict__ perm1, int mean, const float* __restrict__ g,
                                        float* __restrict__ x_bar) {
  const int64_t total = E * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / W;
    const int col = static_cast<int>(i - m * W);
    const int s0 = ptr1[m], s1 = ptr1[m + 1];
    float acc = 0.0f;
    for (int p = s0; p < s1; ++p) {
      const int64_t tr = perm1 ? perm1[p] : p;
      if (tr < 0 || tr >= T) continue;
      const int64_t n = cols[tr];
      if (n < 0 || n >= E) continue;
      acc += (g[n * W + col] * triplet_scale(ptr0, n, mean)) * s[tr * W + col];
    }
    x_bar[i] = acc;
  }
}

__global__ void mxm_triplet_sbar_kernel(const float* __restrict__ x, int64_t E, int W, const int32_t* __restrict__ cols,
                                        int64_t T, const int32_t* __restrict__ ptr0, int mean,
                                        const float* __restrict__ g, float* __restrict__ s_bar) {
  const int64_t total = T * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tr = i / W;
    const int col = static_cast<int>(i - tr * W);
    const int64_t n = cols[tr], m = cols[T + tr];
    float v = 0.0f;
    if (n >= 0 && n < E && m >= 0 && m < E) v = (g[n * W + col] * triplet_scale(ptr0, n, mean)) * x[m * W + col];
    s_bar[i] = v;
  }
}

int check_triplet(const char* what, int64_t E, int W, int64_t T, int pool_op) {
  MP_REQUIRE(E >= 0 && T >= 0 && E < (int64_t(1) << 31) - 1 && T < (int64_t(1) << 31) - 1 && W >= 1, "%s: bad sizes", what);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: pooling %d is not MP_SUM or MP_MEAN", what, pool_op);
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_mxm_edge_ws_bytes(int64_t E, int W, size_t* bytes_out_host) {
  MP_REQUIRE(E >= 0 && bytes_out_host, "mp_mxm_edge_ws_bytes: bad arguments");
  MP_REQUIRE(W == 32 || W == 64 || W == 128, "mp_mxm_edge_ws_bytes: width %d is not one of 32, 64, 128", W);
  *bytes_out_host = mp_tile::ws_bytes(E, W);
  return MP_OK;
}

int mp_mxm_edge_f32(const float* Pa, const float* Pb, int64_t N, int W, const float* a, int Ka, const float* Wc,
                    const float* Wl, const float* b, const int32_t* cols, int64_t E, const int32_t* ptr0,
                    const int32_t* perm0, int act, float alpha, int pool_op, const float* base, float* ws, size_t ws_bytes,
                    float* z_save, float* l_save, float* out, float* y, mpStream_t stream) {
  const char* what = "mp_mxm_edge_f32";
  const bool pooled = out != nullptr;
  int rc = check_edge(what, N, E, W, Ka, act, pool_op, pooled);
  if (rc != MP_OK) return rc;
  MP_REQUIRE((out != nullptr) != (y != nullptr), "%s: exactly one of out (pool) and y (edge) is given", what);
  MP_REQUIRE(!l_save || Wl, "%s: l_save without Wl", what);
  if (N == 0 || (!pooled && E == 0)) return MP_OK;
  hipStream_t st = mp::as_stream(stream);
  if (pooled) MP_REQUIRE(ptr0, "%s: null pointer", what);
  if (E > 0) {
    MP_REQUIRE(Pa && Pb && a && Wc && cols, "%s: null pointer", what);
    if (pooled) {
      const size_t need = mp_tile::ws_bytes(E, W);
      MP_REQUIRE(ws && ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", what, ws ? ws_bytes : (size_t)0, need);
    }
    EdgeArgs k{};
    k.Pa = Pa; k.Pb = Pb; k.a = a; k.Wc = Wc; k.Wl = Wl; k.b = b; k.col0 = cols; k.ptr0 = ptr0; k.perm0 = perm0;
    k.out = out; k.y = y; k.bnd = ws; k.z_save = z_save; k.l_save = l_save; k.N = static_cast<int>(N);
    k.E = static_cast<int>(E); k.Ka = Ka; k.act = act; k.alpha = alpha;
    if (W == 32) launch_fwd<32>(k, st);
    else if (W == 64) launch_fwd<64>(k, st);
    else launch_fwd<128>(k, st);
    rc = mp::check_launch(what);
    if (rc != MP_OK || !pooled) return rc;
  }
  const int mean = pool_op == MP_MEAN ? 1 : 0;
  const unsigned grid = mp::grid_for(N * W);
  if (W == 32) mxm_edge_finish_kernel<32><<<grid, 256, 0, st>>>(ptr0, N, ws, base, mean, out);
  else if (W == 64) mxm_edge_finish_kernel<64><<<grid, 256, 0, st>>>(ptr0, N, ws, base, mean, out);
  else mxm_edge_finish_kernel<128><<<grid, 256, 0, st>>>(ptr0, N, ws, base, mean, out);
  return mp::check_launch("mp_mxm_edge_f32 (finish)");
}

int mp_mxm_edge_grad_f32(const float* g, int pooled, int64_t N, int W, int Ka, const float* Wc, const float* Wl,
                         const int32_t* cols, int64_t E, const int32_t* ptr0, int act, float alpha, int pool_op,
                         const float* z_save, const float* l_save, float* z_bar, float* a_bar, mpStream_t stream) {
  const char* what = "mp_mxm_edge_grad_f32";
  int rc = check_edge(what, N, E, W, Ka, act, pool_op, pooled != 0);
  if (rc != MP_OK || N == 0 || E == 0) return rc;
  MP_REQUIRE(g && cols && z_save && z_bar && (!Wl || l_save) && (!a_bar || Wc), "%s: null pointer", what);
  MP_REQUIRE(!(pooled && pool_op == MP_MEAN) || ptr0, "%s: null pointer", what);
  EdgeArgs k{};
  k.g = g; k.z = z_save; k.l = l_save; k.Wc = Wc; k.Wl = Wl; k.col0 = cols; k.ptr0 = ptr0; k.z_bar = z_bar;
  k.a_bar = a_bar; k.N = static_cast<int>(N); k.E = static_cast<int>(E); k.Ka = Ka; k.act = act; k.alpha = alpha;
  k.pooled = pooled ? 1 : 0; k.mean = pool_op == MP_MEAN ? 1 : 0;
  hipStream_t st = mp::as_stream(stream);
  const unsigned grid = edge_grid(E);
  if (W == 32) mxm_edge_bwd_kernel<32><<<grid, 256, 0, st>>>(k);
  else if (W == 64) mxm_edge_bwd_kernel<64><<<grid, 256, 0, st>>>(k);
  else mxm_edge_bwd_kernel<128><<<grid, 256, 0, st>>>(k);
  return mp::check_launch(what);
}

int mp_mxm_triplet_f32(const float* x, int64_t E, int W, const float* s, const int32_t* cols, int64_t T,
                       const int32_t* ptr0, const int32_t* perm0, int pool_op, float* out, mpStream_t stream) {
  const char* what = "mp_mxm_triplet_f32";
  int rc = check_triplet(what, E, W, T, pool_op);
  if (rc != MP_OK || E == 0) return rc;
  MP_REQUIRE(ptr0 && out && (T == 0 || (x && s && cols)), "%s: null pointer", what);
  mxm_triplet_fwd_kernel<<<mp::grid_for(E * W), 256, 0, mp::as_stream(stream)>>>(x, E, W, s, cols, T, ptr0, perm0,
                                                                                  pool_op == MP_MEAN ? 1 : 0, out);
  return mp::check_launch(what);
}

int mp_mxm_triplet_grad_f32(const float* x, int64_t E, int W, const float* s, const int32_t* cols, int64_t T,
                            const int32_t* ptr0, const int32_t* ptr1, const int32_t* perm1, int pool_op, const float* g,
                            float* x_bar, float* s_bar, mpStream_t stream) {
  const char* what = "mp_mxm_triplet_grad_f32";
  int rc = check_triplet(what, E, W, T, pool_op);
  if (rc != MP_OK || E == 0) return rc;
  const int mean = pool_op == MP_MEAN ? 1 : 0;
  MP_REQUIRE(g && ptr0 && (T == 0 || cols), "%s: null pointer", what);
  hipStream_t st = mp::as_stream(stream);
  if (x_bar) {
    MP_REQUIRE(ptr1 && (T == 0 || s), "%s: null pointer", what);
    mxm_triplet_xbar_kernel<<<mp::grid_for(E * W), 256, 0, st>>>(E, W, s, cols, T, ptr0, ptr1, perm1, mean, g, x_bar);
    rc = mp::check_launch(what);
    if (rc != MP_OK) return rc;
  }
  if (s_bar && T > 0) {
    MP_REQUIRE(x, "%s: null pointer", what);
    mxm_triplet_sbar_kernel<<<mp::grid_for(T * W), 256, 0, st>>>(x, E, W, cols, T, ptr0, mean, g, s_bar);
    rc = mp::check_launch(what);
  }
  return rc;
}

}  // extern "C"
