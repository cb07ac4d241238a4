// GAT / GATv2 attention (kgcnn/layers/conv/gat_conv.py:103-114, 200-214, 233-323): the logits of H heads over one
// [nodes, edges, edge_index] in one launch and the segment-softmax attention of all of them in a second one.
//
// Logit algebra.  r = receiver (index column 0), s = sender, g_e the edge features of width D (D = 0 without
// use_edge_features), n the node features (N, F), U the units of a head.
//   GATv2 (gat_conv.py:200-214, 233-323):  logit_e = a . act(P[r] + Q[s] + g_e Wc + b)
//       the reference runs Dense(U, act) on the (M, 2F + D) concatenation [n_r, n_s, g_e] and Dense(1) on the result.
//       With Wa = lay_alpha_activation.kernel (2F + D, U):  P = n Wa[:F], Q = n Wa[F:2F] (N, U), Wc = Wa[2F:] (D, U),
//       b its bias, a = lay_alpha.kernel (U).
//   GAT (gat_conv.py:103-114):  logit_e = act(p[r] + q[s] + g_e . c)
//       the reference runs Dense(1, act) on [Wn_r, Wn_s, g_e] with Wn = n Wl + bl.  With a = lay_alpha.kernel
//       (2U + D):  p = Wn a[:U], q = Wn a[U:2U] (N), c = a[2U:] (D).
//       p and q are NOT Dense outputs: a logit is one float of cancelling terms, and the softmax weight inherits its
//       ABSOLUTE error (with logits of +-250 one float32 ulp is 1.5e-5).  Two float32 scalars rounded at that magnitude,
//       added in float32, measured 2.0e-5 on the output rows against the float32 restatement's 5.7e-6.  So
//       gat_node_scores_kernel forms p and q of all heads per node in float64 (2U terms per node and head, node-sized
//       work) and stores each as a float32 value plus its float32 remainder; the edge kernel adds the four floats and the
//       D-term edge product in float64 and rounds once.  Likewise the U-term dot product with `a` of GATv2 (phase 3).
//   both:  out[r] = sum_e softmax_e(logit_e) Wn[s_e] over the edges of receiver r, the maximum of the segment
//       subtracted first (kgcnn/layers/pooling.py:464-546, kgcnn/ops/segment.py:5-24).
// P, Q and Wn are node-side Dense launches on row-block views of the layers' own kernels; the per-edge work is two
// gathered rows plus the D-wide edge product.
//
// gat_logits_v2_kernel<U> is modelled on cgcnn_gate_kernel (csrc/mp_cgcnn.hip): one workgroup (4 waves) walks tiles of
// mp_tile::TE = 32 receiver-sorted positions (mp_tile::load_pos: a row with an index out of range is skipped and its
// logit is not written),
//   phase 0  indices and the edge-feature tile G (32 x D, zero-padded to a multiple of 4 columns)              -> LDS
//   phase 1  G Wc on the matrix pipe (v_mfma_f32_16x16x4_f32): U = 64: wave w owns columns [16w, 16w + 16) of both
//            16-row blocks; U = 32: wave w owns columns [16 (w & 1), +16) of row block w >> 1.  Its D x 16 slab of Wc
//            lives in 16 registers per lane for the whole kernel.  D = 0 skips the product.
//   phase 2  per (edge, column): gathered rows + product + bias, activation                                      -> LDS
//   phase 3  thread e < 32 sums a[c] * hidden[e][c] over c = 0 .. U-1 in column order (float64 accumulator, one rounding)
//            and writes logits[edge][head].
//            No cross-lane reduction, so the order does not depend on the grid.
// HEADS: blockIdx.y is the head.  The alternative - one workgroup keeps a tile's G in LDS and loops over the heads - reads
// G once instead of H times, but has to reload each head's Wc slab (16 registers per lane) for every tile, or hold 8 of
// them; with the head in the grid the slab, bias and `a` are loaded once per workgroup exactly as in the CGCNN kernel,
// and the H workgroups of one tile read the same 32 x D floats of G, which the second to H-th find in cache.
// The per-head pointers travel in a by-value kernel argument (HeadPtrs, at most MP_GAT_MAX_HEADS = 8 heads).
//
// gat_node_scores_kernel: one thread per (node, head): p and q as (value, remainder) pairs, (N, H, 4) floats.
// gat_logits_v1_kernel: one thread per (sorted position, head); no matrix pipe (the edge term is a D-term dot product).
//
// gat_attend_kernel<U>: one WAVE per (receiver, head), receivers' ranges [ptr0[r], ptr0[r + 1]) read through perm0.
//   sweep 1  the maximum: lane l takes positions l, l + 64, ...; butterfly maximum (exact in any order).
//   sweep 2  the sum of exp(logit - max): every lane adds its own positions in list order, then the xor butterfly of
//            mp_wave_sum adds the 64 partials in a fixed order.
//   sweep 3  the weighted rows: the segment in chunks of 64 positions; lane l holds (sender, weight) of position l of the
//            chunk, weight = exp(logit - max) / sum; the 64 lanes are 64 / U position groups x U columns; group k adds
//            positions k, k + 64 / U, ... of every chunk in list order, the groups are added in group order.
// The order of every sum is fixed by the list order and the lane layout alone: no atomics, two runs give equal bits, and
// a receiver of degree 1000 is spread over the wave instead of one lane.  A receiver without (valid) edges gets a zero
// row; every output row is written, so the caller needs no memset.  Output (N, H_total, U): concatenated heads are the
// tensor itself.
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/gat.h"

namespace {

constexpr int TE = mp_tile::TE;
constexpr int MAXD = 64;      // widest edge feature
constexpr int KS = MAXD / 4;  // MFMA steps at the widest edge feature
constexpr int GS = MAXD + 1;  // row stride of the edge-feature tile
constexpr int MAXH = MP_GAT_MAX_HEADS;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct HeadPtrs {
  const float* P[MAXH];   // GATv2: (N, U) by the receiver
  const float* Q[MAXH];   // GATv2: (N, U) by the sender
  const float* Wc[MAXH];  // GATv2: (D, U);                 GAT: c (D)
  const float* b[MAXH];   // GATv2: (U) nullable
  const float* a[MAXH];   // GATv2: (U)
};

struct LogitArgs {
  HeadPtrs hp;
  const float* g;        // (E, D) edge features
  const float* pq;       // GAT: (N, H, 4) = p, its remainder, q, its remainder
  const int32_t* col0;   // (2, E) receivers | senders
  const int32_t* perm0;  // (E) sorted position -> edge, nullable
  float* logits;         // (E, Hs) in edge order
  int N, E, D;           // N, E below 2^31 (checked on the host)
  int Hs, h0;            // row stride of logits and the first head's column
  int act;
  float alpha;
};

template <int U>
__global__ __launch_bounds__(256) void gat_logits_v2_kernel(LogitArgs a) {
  constexpr int HS = U + 1;          // row stride of the hidden tile
  constexpr int RB = U == 64 ? 2 : 1;  // 16-row blocks per wave
  __shared__ float gL[TE * GS];
  __shared__ float hL[TE * HS];
  __shared__ int recvL[TE], sndL[TE], eidL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int head = blockIdx.y;
  const int D = a.D;
  const int col = (U == 64 ? 16 * wave : 16 * (wave & 1)) + (lane & 15), kq = lane >> 4;
  const int rb0 = U == 64 ? 0 : (wave >> 1);
  const float* __restrict__ Pp = a.hp.P[head];
  const float* __restrict__ Qp = a.hp.Q[head];
  const float* __restrict__ Wc = a.hp.Wc[head];
  const float* __restrict__ av = a.hp.a[head];

  // B operand of step s: rows 4s + (lane >> 4), the wave's 16 columns; rows past D are zero
  float wc[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + kq;
    wc[s] = k < D ? Wc[(size_t)k * U + col] : 0.0f;
  }
  const float bias = a.hp.b[head] ? a.hp.b[head][col] : 0.0f;

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's phase 3 is done with the tiles in LDS
    // phase 0
    if (t < TE) {
      const mp_tile::Pos p = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p0, t, nv);
      recvL[t] = p.r; sndL[t] = p.s; eidL[t] = p.e;
    }
    __syncthreads();
    if (D > 0) {
      for (int i = t; i < TE * MAXD; i += 256) {
        const int e = i >> 6, k = i & (MAXD - 1);
        gL[e * GS + k] = (k < D && recvL[e] >= 0) ? a.g[(size_t)eidL[e] * D + k] : 0.0f;
      }
      __syncthreads();
    }
    // phase 1
    f32x4 acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[rb][i] = 0.0f;
    {
      const float* ap = gL + (16 * rb0 + (lane & 15)) * GS + kq;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if (4 * s < D) {   // wave-uniform
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[16 * rb * GS + 4 * s], wc[s], acc[rb], 0, 0, 0);
        }
      }
    }
    // phase 2: C layout of 16x16x4: col = lane & 15, row = 4 * (lane >> 4) + i
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = 16 * (rb0 + rb) + 4 * kq + i;
        const int r = recvL[e];
        float hid = 0.0f;
        if (r >= 0) {
          const float z = ((Pp[(size_t)r * U + col] + Qp[(size_t)sndL[e] * U + col]) + acc[rb][i]) + bias;
          hid = mp_apply_act(a.act, a.alpha, z);
        }
        hL[e * HS + col] = hid;
      }
    }
    __syncthreads();
    // phase 3
    if (t < TE && recvL[t] >= 0) {
      double sum = 0.0;
      for (int c = 0; c < U; ++c) sum += (double)hL[t * HS + c] * (double)av[c];
      a.logits[(size_t)eidL[t] * a.Hs + a.h0 + head] = static_cast<float>(sum);
    }
  }
}

struct ScoreArgs {
  const float* Wn[MAXH];  // (N, U)
  const float* a[MAXH];   // (2U + D): the first 2U entries are read
  float* pq;              // (N, H, 4)
  int N, H, U;
};

__global__ __launch_bounds__(256) void gat_node_scores_kernel(ScoreArgs a) {
  const int64_t total = (int64_t)a.N * a.H;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = static_cast<int>(i / a.H), head = static_cast<int>(i - (int64_t)n * a.H);
    const float* __restrict__ w = a.Wn[head] + (size_t)n * a.U;
    const float* __restrict__ av = a.a[head];
    double p = 0.0, q = 0.0;
    for (int c = 0; c < a.U; ++c) {
      p += (double)w[c] * (double)av[c];
      q += (double)w[c] * (double)av[a.U + c];
    }
    const float ph = static_cast<float>(p), qh = static_cast<float>(q);
    reinterpret_cast<float4*>(a.pq)[i] = make_float4(ph, static_cast<float>(p - (double)ph), qh,
                                                     static_cast<float>(q - (double)qh));
  }
}

__global__ __launch_bounds__(256) void gat_logits_v1_kernel(LogitArgs a, int H) {
  const int64_t total = (int64_t)a.E * H;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = static_cast<int>(i / H), head = static_cast<int>(i - (int64_t)p * H);
    const mp_tile::Pos pos = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p, 0, 1);
    if (pos.r < 0) continue;
    const float4 pr = reinterpret_cast<const float4*>(a.pq)[(size_t)pos.r * H + head];
    const float4 qs = reinterpret_cast<const float4*>(a.pq)[(size_t)pos.s * H + head];
    double z = ((double)pr.x + (double)pr.y) + ((double)qs.z + (double)qs.w);
    if (a.D > 0) {
      const float* __restrict__ c = a.hp.Wc[head];
      const float* __restrict__ g = a.g + (size_t)pos.e * a.D;
      double dot = 0.0;
      for (int k = 0; k < a.D; ++k) dot += (double)g[k] * (double)c[k];
      z += dot;
    }
    a.logits[(size_t)pos.e * a.Hs + a.h0 + head] = mp_apply_act(a.act, a.alpha, static_cast<float>(z));
  }
}

struct AttendArgs {
  const float* Wn[MAXH];  // (N, U) messages of every head, gathered by the sender
  const float* logits;    // (E, Hs)
  const int32_t* col0;    // (2, E)
  const int32_t* ptr0;    // (N + 1)
  const int32_t* perm0;   // nullable
  float* out;             // (N, Hs, U)
  int N, E, H, Hs, h0;
};

// position p of a receiver's range -> (edge, sender); false: a row the logits kernels skip (mp_tile::load_pos)
__device__ __forceinline__ bool attend_pos(const AttendArgs& a, int p, int* e_out, int* s_out) {
  const mp_tile::Pos pos = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p, 0, 1);
  *e_out = pos.e;
  *s_out = pos.s;
  return pos.r >= 0;
}

template <int U>
__global__ __launch_bounds__(256) void gat_attend_kernel(AttendArgs a) {
  constexpr int G = 64 / U;   // position groups of the wave in sweep 3
  const int lane = threadIdx.x & 63;
  const int64_t items = (int64_t)a.N * a.H;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int col = lane % U, grp = lane / U;
  for (int64_t item = wave0; item < items; item += nwaves) {
    const int r = static_cast<int>(item / a.H), head = static_cast<int>(item - (int64_t)r * a.H);
    int lo = a.ptr0[r], hi = a.ptr0[r + 1];
    lo = lo < 0 ? 0 : (lo > a.E ? a.E : lo);
    hi = hi < lo ? lo : (hi > a.E ? a.E : hi);
    const float* __restrict__ lg = a.logits + a.h0 + head;
    const float* __restrict__ wn = a.Wn[head];
    // sweep 1
    float mx = -INFINITY;
    for (int p = lo + lane; p < hi; p += 64) {
      int e, s;
      if (attend_pos(a, p, &e, &s)) mx = fmaxf(mx, lg[(size_t)e * a.Hs]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    // sweep 2
    float part = 0.0f;
    for (int p = lo + lane; p < hi; p += 64) {
      int e, s;
      if (attend_pos(a, p, &e, &s)) part += expf(lg[(size_t)e * a.Hs] - mx);
    }
    const float sum = mp_wave_sum(part);
    // sweep 3
    float acc = 0.0f;
    for (int c0 = lo; c0 < hi; c0 += 64) {   // wave-uniform bounds
      int snd = 0;
      float w = 0.0f;
      if (c0 + lane < hi) {
        int e;
        if (attend_pos(a, c0 + lane, &e, &snd)) w = expf(lg[(size_t)e * a.Hs] - mx) / sum;
      }
      const int n = hi - c0 < 64 ? hi - c0 : 64;
      for (int j = 0; j < n; j += G) {
        const int src = j + grp;             // positions past n hold w = 0, snd = 0
        const float wj = __shfl(w, src, 64);
        const int sj = __shfl(snd, src, 64);
        if (wj != 0.0f) acc += wj * wn[(size_t)sj * U + col];
      }
    }
    if (G == 2) {
      const float other = __shfl(acc, lane + 32, 64);   // group 0 + group 1
      acc += other;
    }
    if (grp == 0) a.out[((size_t)r * a.Hs + a.h0 + head) * U + col] = acc;
  }
}

}  // namespace

extern "C" {

int mp_gat_node_scores_f32(int H, int U, const float* const* Wn_host, const float* const* a_host, int64_t N, float* pq,
                           mpStream_t stream) {
  const char* what = "mp_gat_node_scores_f32";
  MP_REQUIRE(H >= 1 && H <= MAXH, "%s: 1 to %d heads per launch, got %d", what, MAXH, H);
  MP_REQUIRE(U == 32 || U == 64, "%s: units must be 32 or 64, got %d", what, U);
  MP_REQUIRE(N >= 0 && N < (int64_t(1) << 31) - 1, "%s: bad sizes", what);
  if (N == 0) return MP_OK;
  MP_REQUIRE(Wn_host && a_host && pq && mp::aligned16(pq), "%s: null or unaligned pointer", what);
  ScoreArgs a{};
  for (int h = 0; h < H; ++h) {
    a.Wn[h] = Wn_host[h];
    a.a[h] = a_host[h];
    MP_REQUIRE(a.Wn[h] && a.a[h], "%s: null pointer in head %d", what, h);
  }
  a.pq = pq; a.N = static_cast<int>(N); a.H = H; a.U = U;
  gat_node_scores_kernel<<<mp::grid_for(N * H), 256, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch(what);
}

int mp_gat_logits_f32(int mode, int H, int U, const float* const* P_host, const float* const* Q_host, const float* pq,
                      const float* const* Wc_host, const float* const* b_host, const float* const* a_host, int64_t N,
                      const float* edges, int D, const int32_t* cols, int64_t E, const int32_t* perm0, int act, float alpha,
                      float* logits, int64_t logit_heads, int64_t head0, mpStream_t stream) {
  const char* what = "mp_gat_logits_f32";
  MP_REQUIRE(mode == MP_GAT_V1 || mode == MP_GAT_V2, "%s: mode must be MP_GAT_V1 or MP_GAT_V2, got %d", what, mode);
  MP_REQUIRE(H >= 1 && H <= MAXH, "%s: 1 to %d heads per launch, got %d", what, MAXH, H);
  MP_REQUIRE(U == 32 || U == 64, "%s: units must be 32 or 64, got %d", what, U);
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(D >= 0 && (mode == MP_GAT_V1 || D <= MAXD), "%s: GATv2 takes 0 to %d edge features, got %d", what, MAXD, D);
  MP_REQUIRE(act >= 0 && act <= MP_ACT_LAST, "%s: unknown activation code", what);
  MP_REQUIRE(head0 >= 0 && logit_heads >= head0 + H && logit_heads < (int64_t(1) << 31), "%s: heads [%lld, %lld) do not fit %lld logit columns",
             what, (long long)head0, (long long)(head0 + H), (long long)logit_heads);
  if (E == 0) return MP_OK;
  MP_REQUIRE(cols && logits && (D == 0 || (edges && Wc_host)), "%s: null pointer", what);
  const bool v2 = mode == MP_GAT_V2;
  MP_REQUIRE(v2 ? (P_host && Q_host && a_host) : (pq && mp::aligned16(pq)), "%s: null or unaligned pointer", what);
  LogitArgs a{};
  for (int h = 0; h < H; ++h) {
    a.hp.P[h] = v2 ? P_host[h] : nullptr;
    a.hp.Q[h] = v2 ? Q_host[h] : nullptr;
    a.hp.Wc[h] = D > 0 ? Wc_host[h] : nullptr;
    a.hp.b[h] = v2 && b_host ? b_host[h] : nullptr;
    a.hp.a[h] = v2 ? a_host[h] : nullptr;
    MP_REQUIRE((D == 0 || a.hp.Wc[h]) && (!v2 || (a.hp.P[h] && a.hp.Q[h] && a.hp.a[h])), "%s: null pointer in head %d",
               what, h);
  }
  a.g = edges; a.pq = pq; a.col0 = cols; a.perm0 = perm0; a.logits = logits;
  a.N = static_cast<int>(N); a.E = static_cast<int>(E); a.D = D;
  a.Hs = static_cast<int>(logit_heads); a.h0 = static_cast<int>(head0);
  a.act = act; a.alpha = alpha;
  if (mode == MP_GAT_V1) {
    gat_logits_v1_kernel<<<mp::grid_for(E * H), 256, 0, mp::as_stream(stream)>>>(a, H);
  } else {
    const int64_t tiles = mp_tile::tiles_of(E);
    const dim3 grid(static_cast<unsigned>(tiles < 1024 ? tiles : 1024), static_cast<unsigned>(H));
    if (U == 64) gat_logits_v2_kernel<64><<<grid, 256, 0, mp::as_stream(stream)>>>(a);
    else gat_logits_v2_kernel<32><<<grid, 256, 0, mp::as_stream(stream)>>>(a);
  }
  return mp::check_launch(what);
}

int mp_gat_attend_f32(int H, int U, const float* const* Wn_host, int64_t N, const float* logits, int64_t logit_heads,
                      int64_t head0, const int32_t* cols, int64_t E, const int32_t* ptr0, const int32_t* perm0, float* out,
                      mpStream_t stream) {
  const char* what = "mp_gat_attend_f32";
  MP_REQUIRE(H >= 1 && H <= MAXH, "%s: 1 to %d heads per launch, got %d", what, MAXH, H);
  MP_REQUIRE(U == 32 || U == 64, "%s: units must be 32 or 64, got %d", what, U);
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(head0 >= 0 && logit_heads >= head0 + H && logit_heads < (int64_t(1) << 31), "%s: heads [%lld, %lld) do not fit %lld columns",
             what, (long long)head0, (long long)(head0 + H), (long long)logit_heads);
  if (N == 0) return MP_OK;
  MP_REQUIRE(ptr0 && out, "%s: null pointer", what);
  MP_REQUIRE(E == 0 || (Wn_host && logits && cols), "%s: null pointer", what);
  AttendArgs a{};
  for (int h = 0; h < H; ++h) {
    a.Wn[h] = Wn_host ? Wn_host[h] : nullptr;
    MP_REQUIRE(E == 0 || a.Wn[h], "%s: null pointer in head %d", what, h);
  }
  a.logits = logits; a.col0 = cols; a.ptr0 = ptr0; a.perm0 = perm0; a.out = out;
  a.N = static_cast<int>(N); a.E = static_cast<int>(E); a.H = H;
  a.Hs = static_cast<int>(logit_heads); a.h0 = static_cast<int>(head0);
  const unsigned grid = mp::grid_for(N * H * 64);
  if (U == 64) gat_attend_kernel<64><<<grid, 256, 0, mp::as_stream(stream)>>>(a);
  else gat_attend_kernel<32><<<grid, 256, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch(what);
}

}  // extern "C"
