// INorp (kgcnn/literature/INorp.py:117-127): the folded edge step of one block and its reverse.  With a two-layer edge MLP
// Dense(H1, act) -> Dense(H2, linear) the second layer commutes with the pool, and the first is linear in the column blocks
// of [n[send] || n[recv] || edges], so the per-edge work is
//   h[p]   = act((Pj[send] + Pi[recv]) + edges[e] Wc)                  Pj = n W1[0:F], Pi = n W1[F:2F] + b1, Wc = W1[2F:]
//   out[r] = sum or mean of h over the sorted positions of receiver r, in list order; 0 for a receiver without edges
// and the (N, H1) result goes through the second Dense on the nodes.  No edge-sized tensor is written.
// Built as megnet_edge_kernel is: one workgroup (4 waves) walks tiles of 32 receiver-sorted positions:
//   phase 0  receiver, sender and edge id of each position                                                         -> LDS
//   phase 1  the edge rows X (32 x Fe, zero-padded to a multiple of 4 columns) and the gathered rows of Pj and Pi are all
//            requested before the first is waited for; X goes to LDS
//   phase 2  X Wc on the matrix pipe (v_mfma_f32_16x16x4_f32), the slabs of Wc a wave needs resident in registers for the
//            whole kernel; the gathered rows are added behind it, the activation applied                          -> LDS
//   phase 3  per-receiver sums in list order by H1 threads (one per column): the walk of csrc/mp_edge_tile.h, which states
//            the rule for receivers cut by a tile boundary.  No atomics: two runs give equal bits.
// The 16 x 16 output blocks of a tile (2 row blocks x H1/16 column blocks) are dealt to the waves so that a wave keeps as
// few slabs of Wc as possible: H1 = 128 two column blocks and both row blocks per wave, 64 one and both, 32 one block per
// wave, 16 one block for each of the first two waves.
// The reverse runs the same phases with GRAD set: z1 is recomputed in the same operation order, phase 2 writes
// gz = g[recv] (/ count) * act'(z1) at the edge's list position and into LDS, and phase 3 sums gz per receiver (Pi_bar).
// A position whose SENDER lies outside [0, N) keeps its receiver in the walk and adds an exact 0 (okL), so the receiver's
// other edges stay in one segment and a receiver all of whose edges are skipped is stored as 0; a position whose RECEIVER
// lies outside belongs to no segment of ptr0 (r = -1).
// inorp_finish_kernel then takes every node's sum (direct, or the cut receiver's slots in tile order), zeroes the
// receivers without edges and divides by the edge count for the forward's mean.
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/inorp.h"

namespace {

constexpr int TE = mp_tile::TE;   // positions per tile
constexpr int FE_MAX = 64;        // widest edge row
constexpr int KS_MAX = FE_MAX / 4;   // k steps of the 16x16x4 product
constexpr int XS = FE_MAX + 1;    // row stride of the staged edge rows in LDS

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct EdgeArgs {
  const float* Pj;        // (N, H1), gathered by the sender
  const float* Pi;        // (N, H1), gathered by the receiver, first-layer bias folded in
  const float* x;         // (E, Fe) edge features
  const float* Wc;        // (Fe, H1)
  const float* g;         // (N, H1) upstream of out (reverse only)
  const int32_t* col0;    // (2, E) receivers | senders
  const int32_t* ptr0;    // (N+1) CSR of col0 over sorted positions
  const int32_t* perm0;   // (E) sorted position -> edge, nullable
  float* out;             // (N, H1): sums of the receivers that lie inside one tile (reverse: Pi_bar)
  float* bnd;             // (tiles, 2, H1)
  float* gz;              // (E, H1) (reverse only)
  int N, E;               // below 2^31 (checked on the host)
  int Fe;
  int act;
  int mean;
  float alpha;
};

template <int H1, bool GRAD>
__global__ __launch_bounds__(256, 2) void inorp_edge_kernel(EdgeArgs a) {
  constexpr int CB = H1 / 16;                  // column blocks of the tile's output
  constexpr int NCB = CB >= 4 ? CB / 4 : 1;    // column blocks a wave owns
  constexpr int NRB = CB >= 4 ? 2 : 1;         // row blocks a wave owns
  constexpr int HS = H1 + 1;
  __shared__ float xL[TE * XS];
  __shared__ float hL[TE * HS];
  __shared__ int recvL[TE], sndL[TE], eidL[TE], okL[TE], rawL[TE], cntL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lc = lane & 15, kq = lane >> 4;
  const bool active = CB >= 2 || wave < 2;                       // H1 = 16 has two blocks only
  const int cbase = CB >= 4 ? wave * NCB : (CB == 2 ? wave >> 1 : 0);
  const int rbase = CB >= 4 ? 0 : wave & 1;
  const int ks = (a.Fe + 3) >> 2, fp = 4 * ks;                  // k steps, padded edge width

  // B operands: step s reads row 4s + (lane >> 4) of the wave's columns; rows behind Fe are zero
  float wc[NCB][KS_MAX];
#pragma unroll
  for (int j = 0; j < NCB; ++j) {
#pragma unroll
    for (int s = 0; s < KS_MAX; ++s) {
      const int k = 4 * s + kq;
      wc[j][s] = (active && k < a.Fe) ? a.Wc[(size_t)k * H1 + 16 * (cbase + j) + lc] : 0.0f;
    }
  }

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's walk is done with the tiles in LDS
    // phase 0
    if (t < TE) {
      const mp_tile::Pos p = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p0, t, nv);
      int raw = -1, r = p.r;   // raw: the list position; r: the receiver, kept for a row skipped for its sender alone
      if (t < nv) {
        raw = a.perm0 ? a.perm0[p0 + t] : p0 + t;
        if (raw < 0 || raw >= a.E) raw = -1;
        if (r < 0 && raw >= 0) {
          const int r0 = a.col0[raw];
          if (r0 >= 0 && r0 < a.N) r = r0;
        }
      }
      recvL[t] = r; sndL[t] = p.s; eidL[t] = p.e; okL[t] = p.r >= 0 ? 1 : 0;
      if (GRAD) {
        int cnt = 1;   // the mean's divisor is the segment's length, as in the forward's finishing pass
        if (a.mean && r >= 0) cnt = a.ptr0[r + 1] - a.ptr0[r];
        rawL[t] = raw; cntL[t] = cnt < 1 ? 1 : cnt;   // gz is written at raw also for a skipped edge (zeros)
      }
    }
    __syncthreads();
    // phase 1: every global load of the tile is issued before the first one is waited for
    float xv[TE * FE_MAX / 256];
#pragma unroll
    for (int j = 0; j < TE * FE_MAX / 256; ++j) {
      const int idx = t + 256 * j;
      const int row = idx / fp, c = idx - row * fp;
      xv[j] = (idx < TE * fp && c < a.Fe && okL[row]) ? a.x[(size_t)eidL[row] * a.Fe + c] : 0.0f;
    }
    // the gathered rows (C layout of 16x16x4: col = lane & 15, row = 4 * (lane >> 4) + i)
    float pj[NCB][NRB][4], pi[NCB][NRB][4], gg[NCB][NRB][4];
#pragma unroll
    for (int j = 0; j < NCB; ++j) {
#pragma unroll
      for (int b = 0; b < NRB; ++b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 16 * (rbase + b) + 4 * kq + i;
          const int col = 16 * (cbase + j) + lc;
          const bool ok = active && okL[e];
          pj[j][b][i] = ok ? a.Pj[(size_t)sndL[e] * H1 + col] : 0.0f;
          pi[j][b][i] = ok ? a.Pi[(size_t)recvL[e] * H1 + col] : 0.0f;
          gg[j][b][i] = (GRAD && ok) ? a.g[(size_t)recvL[e] * H1 + col] : 0.0f;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < TE * FE_MAX / 256; ++j) {
      const int idx = t + 256 * j;
      const int row = idx / fp, c = idx - row * fp;
      if (idx < TE * fp) xL[row * XS + c] = xv[j];
    }
    __syncthreads();
    // phase 2
    if (active) {
      f32x4 acc[NCB][NRB];
#pragma unroll
      for (int j = 0; j < NCB; ++j)
#pragma unroll
        for (int b = 0; b < NRB; ++b)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[j][b][i] = 0.0f;
      const float* ap = xL + (16 * rbase + lc) * XS + kq;
#pragma unroll
      for (int s = 0; s < KS_MAX; ++s) {
        if (s < ks) {   // the same for every lane
#pragma unroll
          for (int b = 0; b < NRB; ++b) {
            const float av = ap[16 * b * XS + 4 * s];
#pragma unroll
            for (int j = 0; j < NCB; ++j) acc[j][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wc[j][s], acc[j][b], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NCB; ++j) {
#pragma unroll
        for (int b = 0; b < NRB; ++b) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int e = 16 * (rbase + b) + 4 * kq + i;
            const int col = 16 * (cbase + j) + lc;
            const bool ok = okL[e] != 0;
            const float z = (pj[j][b][i] + pi[j][b][i]) + acc[j][b][i];
            float v = 0.0f;
            if (GRAD) {
              if (ok) {
                const float up = a.mean ? gg[j][b][i] / static_cast<float>(cntL[e]) : gg[j][b][i];
                v = up * mp_act_grad(a.act, a.alpha, z);
              }
              if (rawL[e] >= 0) a.gz[(size_t)rawL[e] * H1 + col] = v;
            } else if (ok) {
              v = mp_apply_act(a.act, a.alpha, z);
            }
            hL[e * HS + col] = v;
          }
        }
      }
    }
    __syncthreads();
    // phase 3
    if (t < H1)
      mp_tile::walk<H1>(recvL, nv, a.ptr0, a.out, a.bnd, tile, t, [=](int e) { return hL[e * HS + t]; });
  }
}

// every node's row: direct, a cut receiver's sum, or 0 without edges; the mean divides by the count.
template <int H1>
__global__ void inorp_finish_kernel(const int32_t* __restrict__ ptr0, int64_t N, const float* __restrict__ bnd, int mean,
                                    float* __restrict__ out) {
  const int64_t total = N * H1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / H1;
    const int col = static_cast<int>(i - r * H1);
    const int64_t s0 = ptr0[r], s1 = ptr0[r + 1];
    float u = 0.0f;
    if (s1 > s0) {
      if (!mp_tile::cut_sum<H1>(bnd, s0, s1, col, &u)) u = out[i];
      if (mean) u = u / static_cast<float>(s1 - s0);
    }
    out[i] = u;
  }
}

template <int H1, bool GRAD>
int launch(const EdgeArgs& a, int64_t N, int64_t E, int finish_mean, const char* what, hipStream_t stream) {
  if (E > 0) {
    const int64_t tiles = mp_tile::tiles_of(E);
    inorp_edge_kernel<H1, GRAD><<<static_cast<unsigned>(tiles < 1024 ? tiles : 1024), 256, 0, stream>>>(a);
    const int rc = mp::check_launch(what);
    if (rc != MP_OK) return rc;
  }
  inorp_finish_kernel<H1><<<mp::grid_for(N * H1), 256, 0, stream>>>(a.ptr0, N, a.bnd, finish_mean, a.out);
  return mp::check_launch(what);
}

template <bool GRAD>
int dispatch(const EdgeArgs& a, int H1, int64_t N, int64_t E, int finish_mean, const char* what, hipStream_t stream) {
  switch (H1) {
    case 16: return launch<16, GRAD>(a, N, E, finish_mean, what, stream);
    case 32: return launch<32, GRAD>(a, N, E, finish_mean, what, stream);
    case 64: return launch<64, GRAD>(a, N, E, finish_mean, what, stream);
    default: return launch<128, GRAD>(a, N, E, finish_mean, what, stream);
  }
}

bool width_ok(int H1) { return H1 == 16 || H1 == 32 || H1 == 64 || H1 == 128; }

// the checks both directions share
int check_args(const char* what, int64_t N, int H1, int Fe, int64_t E, int act, int pool_op) {
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes N = %lld, E = %lld (32-bit indexing)", what,
             static_cast<long long>(N), static_cast<long long>(E));
  MP_REQUIRE(width_ok(H1), "%s: the hidden width is 16, 32, 64 or 128, got %d", what, H1);
  MP_REQUIRE(Fe >= 1 && Fe <= FE_MAX, "%s: the edge width is 1 to %d, got %d", what, FE_MAX, Fe);
  MP_REQUIRE(act >= 0 && act <= MP_ACT_LAST, "%s: unknown activation code %d", what, act);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: pooling is sum or mean, got op %d", what, pool_op);
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_inorp_edge_ws_bytes(int64_t E, int H1, size_t* bytes_out_host) {
  MP_REQUIRE(E >= 0 && bytes_out_host, "mp_inorp_edge_ws_bytes: bad arguments");
  MP_REQUIRE(width_ok(H1), "mp_inorp_edge_ws_bytes: the hidden width is 16, 32, 64 or 128, got %d", H1);
  *bytes_out_host = mp_tile::ws_bytes(E, H1);
  return MP_OK;
}

int mp_inorp_edge_f32(const float* Pj, const float* Pi, int64_t N, int H1, const float* edges, int Fe, const float* Wc,
                      const int32_t* cols, int64_t E, const int32_t* ptr0, const int32_t* perm0, int act, float alpha,
                      int pool_op, float* ws, size_t ws_bytes, float* out, mpStream_t stream) {
  const char* what = "mp_inorp_edge_f32";
  const int rc = check_args(what, N, H1, Fe, E, act, pool_op);
  if (rc != MP_OK) return rc;
  if (N == 0) return MP_OK;
  MP_REQUIRE(ptr0 && out, "%s: null pointer", what);
  if (E > 0) {
    const size_t need = mp_tile::ws_bytes(E, H1);
    MP_REQUIRE(Pj && Pi && edges && Wc && cols && ws, "%s: null pointer", what);
    MP_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", what, ws_bytes, need);
  }
  EdgeArgs a{};
  a.Pj = Pj; a.Pi = Pi; a.x = edges; a.Wc = Wc; a.col0 = cols; a.ptr0 = ptr0; a.perm0 = perm0; a.out = out; a.bnd = ws;
  a.N = static_cast<int>(N); a.E = static_cast<int>(E); a.Fe = Fe; a.act = act; a.alpha = alpha;
  return dispatch<false>(a, H1, N, E, pool_op == MP_MEAN ? 1 : 0, what, mp::as_stream(stream));
}

int mp_inorp_edge_grad_f32(const float* Pj, const float* Pi, int64_t N, int H1, const float* edges, int Fe,
                           const float* Wc, const int32_t* cols, int64_t E, const int32_t* ptr0, const int32_t* perm0,
                           int act, float alpha, int pool_op, const float* g, float* ws, size_t ws_bytes, float* gz,
                           float* pi_bar, mpStream_t stream) {
  const char* what = "mp_inorp_edge_grad_f32";
  const int rc = check_args(what, N, H1, Fe, E, act, pool_op);
  if (rc != MP_OK) return rc;
  if (N == 0) return MP_OK;
  MP_REQUIRE(ptr0 && pi_bar, "%s: null pointer", what);
  if (E > 0) {
    const size_t need = mp_tile::ws_bytes(E, H1);
    MP_REQUIRE(Pj && Pi && edges && Wc && cols && g && ws && gz, "%s: null pointer", what);
    MP_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", what, ws_bytes, need);
  }
  EdgeArgs a{};
  a.Pj = Pj; a.Pi = Pi; a.x = edges; a.Wc = Wc; a.g = g; a.col0 = cols; a.ptr0 = ptr0; a.perm0 = perm0; a.out = pi_bar;
  a.bnd = ws; a.gz = gz; a.N = static_cast<int>(N); a.E = static_cast<int>(E); a.Fe = Fe; a.act = act; a.alpha = alpha;
  a.mean = pool_op == MP_MEAN ? 1 : 0;
  return dispatch<true>(a, H1, N, E, 0, what, mp::as_stream(stream));
}

}  // extern "C"
