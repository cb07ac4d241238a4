// EGNN (kgcnn/literature/EGNN.py:23-208): position encoding and the fused edge step of one block, with their reverses.
//
// Position encoding (kgcnn/layers/geom.py:596-713): out[row] = [sin(x s_k) | cos(x s_k)] (or interleaved), accurate
// sincosf (arguments reach several hundred radians: d^2 up to 100 times s_0 = 2 pi).
//
// Fused edge step (EGNN.py:155-174 without edge attributes), one launch plus a small finishing pass:
//   m_i[r] = sum_{e: recv(e) = r} att_e * m_e,   m_e = act2(act1(Pa[recv_e] + Pb[send_e] + enc_e Wc + b1) W2 + b2),
//   att_e = act_att(m_e . w_att + b_att)   (1 without an attention layer).
// Pa = h W_a and Pb = h W_b are made on the node side by two Dense launches on row blocks of the first kernel (in place:
// no repacked copy that could go stale), so the per-edge first layer is two gathered 128-wide rows plus a (<= 64)-wide
// product.  One workgroup (4 waves) walks tiles of 32 receiver-sorted edges:
//   phase 0  indices, the norm output and its encoding (computed here: no (E, 2K) tensor exists)           -> LDS
//   phase 1  first layer per (edge, column), activation, transposed into LDS                                -> h1T[k][e]
//   phase 2  second layer on the matrix pipe: v_mfma_f32_32x32x2_f32, edges = rows, wave w owns output columns
//            [32w, 32w+32); its 128 x 32 slab of W2 lives in 64 registers per lane for the whole kernel
//   phase 3  bias, activation, attention dot (8 lanes per edge, fixed xor tree) and activation             -> LDS
//   phase 4  per-receiver sums in edge order by 128 threads (one per column): the walk of csrc/mp_edge_tile.h, which
//            states the rule for receivers cut by a tile boundary; egnn_edge_finish_kernel writes their sums and zeroes
//            the receivers without edges.  No atomics: two runs give equal bits.
// With z1_save / z2_save given (a forward that will be differentiated) both pre-activations are stored per edge; the
// reverse reads them instead of repeating the gathers, the encoding and the GEMM.
//
// Reverse: per tile of 32 edges (list order), m_e and att_e from z2, the attention's and the second activation's
// derivative, the mirror GEMM with W2^T on the matrix pipe, the first activation's derivative -> z1_bar (E, 128), and
// x_bar (E) through Wc^T and the encoding's derivative.  The sums of z1_bar into Pa_bar / Pb_bar run on the segment-sum kernel
// over the two CSRs (host side), in list order.
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/egnn.h"

namespace {

constexpr int F = 128;        // node / message width of the fused step
constexpr int TE = mp_tile::TE;   // edges per tile
constexpr int MAXC = 64;      // widest encoding (2K)
constexpr int HS = TE + 1;    // row stride of the transposed tiles
constexpr int MS = F + 1;     // row stride of the edge-major tiles
static_assert(TE * MS <= F * HS, "the edge-major tile reuses the transposed tile's LDS");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------- position encoding
__global__ void position_encoding_kernel(const float* __restrict__ x, int64_t M, const float* __restrict__ scales, int K,
                                         int interleave, float* __restrict__ out) {
  const int64_t total = M * K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / K;
    const int k = static_cast<int>(i - row * K);
    float s, c;
    sincosf(x[row] * scales[k], &s, &c);
    float* o = out + row * 2 * K;
    o[interleave ? 2 * k : k] = s;
    o[interleave ? 2 * k + 1 : K + k] = c;
  }
}

__global__ void position_encoding_grad_kernel(const float* __restrict__ x, int64_t M, const float* __restrict__ scales,
                                              int K, int interleave, const float* __restrict__ g,
                                              float* __restrict__ x_bar) {
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < M; row += (int64_t)gridDim.x * blockDim.x) {
    const float xv = x[row];
    const float* gr = g + row * 2 * K;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
      float s, c;
      const float sk = scales[k];
      sincosf(xv * sk, &s, &c);
      acc += sk * (gr[interleave ? 2 * k : k] * c - gr[interleave ? 2 * k + 1 : K + k] * s);
    }
    x_bar[row] = acc;
  }
}

// ---------------------------------------------------------------------------------------------- fused edge step
struct EdgeArgs {
  const float* Pa;       // (N, F) h W_a, gathered by the receiver
  const float* Pb;       // (N, F) h W_b, gathered by the sender
  const float* x;        // (E) norm output
  const int32_t* col0;   // (2, E) receivers | senders
  const int32_t* ptr0;   // (N+1) CSR of col0 over sorted positions
  const int32_t* perm0;  // (E) sorted position -> edge, nullable
  const float* scales;   // (K), null when K == 0
  const float* Wc;       // (C, F), C = 2K or 1
  const float* b1;       // (F) nullable
  const float* W2;       // (F, F)
  const float* b2;       // (F) nullable
  const float* w_att;    // (F) nullable: no attention
  const float* b_att;    // (1) nullable
  const float* g;        // reverse: (N, F) upstream
  const float* z1;       // reverse: (E, F)
  const float* z2;       // reverse: (E, F)
  float* out;            // forward: (N, F)
  float* z1_save;        // forward, nullable
  float* z2_save;        // forward, nullable
  float* bnd;            // forward: (tiles, 2, F)
  float* z1_bar;         // reverse: (E, F)
  float* x_bar;          // reverse: (E) nullable
  int N, E;            // both below 2^31 (checked on the host)
  int K, C, interleave, act1, act2, act_att;
  float alpha;
};

__device__ __forceinline__ int enc_col(int k, int K, int interleave, bool cosine) {
  return interleave ? 2 * k + (cosine ? 1 : 0) : (cosine ? K + k : k);
}

// acc (32 edges x 32 columns of this wave) += A (32 x 128, transposed in LDS as aT[k][e]) x the wave's register slab.
__device__ __forceinline__ void tile_gemm(const float* aT, const float (&wreg)[F / 2], int lane, f32x16& acc) {
  const float* ap = aT + (lane >> 5) * HS + (lane & 31);
#pragma unroll
  for (int s = 0; s < F / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * HS], wreg[s], acc, 0, 0, 0);
}

__global__ __launch_bounds__(256) void egnn_edge_fwd_kernel(EdgeArgs a) {
  __shared__ float h1T[F * HS];
  float* mL = h1T;   // the second layer's output reuses the first layer's tile (TE * MS <= F * HS), after a barrier
  __shared__ float WcL[MAXC * F];
  __shared__ float encL[TE * MAXC];
  __shared__ float b1L[F], b2L[F], waL[F], scL[MAXC];
  __shared__ float xL[TE], attL[TE];
  __shared__ int recvL[TE], sndL[TE];
  __shared__ int eidL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int K = a.K, C = a.C;

  for (int i = t; i < C * F; i += 256) WcL[i] = a.Wc[i];
  if (t < F) {
    b1L[t] = a.b1 ? a.b1[t] : 0.0f;
    b2L[t] = a.b2 ? a.b2[t] : 0.0f;
    waL[t] = a.w_att ? a.w_att[t] : 0.0f;
  }
  if (t < K) scL[t] = a.scales[t];
  const float batt = (a.w_att && a.b_att) ? a.b_att[0] : 0.0f;

  float wreg[F / 2];
#pragma unroll
  for (int s = 0; s < F / 2; ++s) wreg[s] = a.W2[(size_t)(2 * s + (lane >> 5)) * F + 32 * wave + (lane & 31)];

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's walk is done with the tiles in LDS; the weights above are visible
    // phase 0
    if (t < TE) {
      const mp_tile::Pos p = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p0, t, nv);
      float xv = 0.0f;
      if (t < nv) xv = a.x[p.e];   // beside the index loads, not behind them; used for valid rows only
      recvL[t] = p.r; sndL[t] = p.s; eidL[t] = p.e; xL[t] = xv;
    }
    __syncthreads();
    if (K > 0) {
      for (int i = t; i < TE * K; i += 256) {
        const int e = i / K, k = i - e * K;
        float s, c;
        sincosf(xL[e] * scL[k], &s, &c);
        encL[e * MAXC + enc_col(k, K, a.interleave, false)] = s;
        encL[e * MAXC + enc_col(k, K, a.interleave, true)] = c;
      }
    } else if (t < TE) {
      encL[t * MAXC] = xL[t];
    }
    __syncthreads();
    // phase 1
    {
      // 16 edges per thread and one column, in two groups of 8: a group's gathers are issued together, then the
      // encoding's product column by column (c ascending, as a row-by-row loop would add them)
      const int k = t & (F - 1), half = t >> 7;
      constexpr int G = 8;
#pragma unroll 1
      for (int e0 = half; e0 < TE; e0 += 2 * G) {
        float z[G], d[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int e = e0 + 2 * i, r = recvL[e] < 0 ? 0 : recvL[e];   // invalid rows read row 0 and are zeroed below
          z[i] = a.Pa[(size_t)r * F + k] + a.Pb[(size_t)sndL[e] * F + k];
          d[i] = 0.0f;
        }
        for (int c = 0; c < C; ++c) {
          const float w = WcL[c * F + k];
#pragma unroll
          for (int i = 0; i < G; ++i) d[i] += encL[(e0 + 2 * i) * MAXC + c] * w;
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int e = e0 + 2 * i;
          const bool valid = recvL[e] >= 0;
          const float zz = (z[i] + d[i]) + b1L[k];
          if (a.z1_save && valid) a.z1_save[(size_t)eidL[e] * F + k] = zz;
          h1T[k * HS + e] = valid ? mp_apply_act(a.act1, a.alpha, zz) : 0.0f;
        }
      }
    }
    __syncthreads();
    // phase 2 + 3
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    tile_gemm(h1T, wreg, lane, acc);
    __syncthreads();   // every wave has read h1T
    {
      const int col = 32 * wave + (lane & 31);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int e = 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
        const float z = acc[i] + b2L[col];
        if (a.z2_save && recvL[e] >= 0) a.z2_save[(size_t)eidL[e] * F + col] = z;
        mL[e * MS + col] = mp_apply_act(a.act2, a.alpha, z);
      }
    }
    __syncthreads();
    {
      const int e = t >> 3, part = t & 7;
      float d = 0.0f;
      if (a.w_att) {
        for (int c = part * 16; c < part * 16 + 16; ++c) d += mL[e * MS + c] * waL[c];
        d += __shfl_xor(d, 1);
        d += __shfl_xor(d, 2);
        d += __shfl_xor(d, 4);
      }
      if (part == 0) attL[e] = a.w_att ? mp_apply_act(a.act_att, a.alpha, d + batt) : 1.0f;
    }
    __syncthreads();
    // phase 4
    if (t < F)
      mp_tile::walk<F>(recvL, nv, a.ptr0, a.out, a.bnd, tile, t, [=](int e) { return attL[e] * mL[e * MS + t]; });
  }
}

// Receivers whose edges span several tiles: the cut receiver's sum; receivers without edges: zero; the rest stay.
__global__ void egnn_edge_finish_kernel(const int32_t* __restrict__ ptr0, int64_t N, const float* __restrict__ bnd,
                                        float* __restrict__ out) {
  const int64_t total = N * F;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / F;
    const int col = static_cast<int>(i - r * F);
    const int64_t s0 = ptr0[r], s1 = ptr0[r + 1];
    if (s1 <= s0) { out[i] = 0.0f; continue; }
    float sum;
    if (mp_tile::cut_sum<F>(bnd, s0, s1, col, &sum)) out[i] = sum;
  }
}

__global__ __launch_bounds__(256) void egnn_edge_bwd_kernel(EdgeArgs a) {
  __shared__ float dT[F * HS];          // z2_bar, transposed
  float* zL = dT;                       // z1_bar, edge-major: reuses dT after the GEMM (TE * MS <= F * HS)
  __shared__ float WcL[MAXC * MS];
  __shared__ float encbL[TE * MAXC];
  __shared__ float waL[F], scL[MAXC];
  __shared__ float xL[TE], attL[TE], dattL[TE];
  __shared__ int recvL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int K = a.K, C = a.C;
  const bool want_x = a.x_bar != nullptr;

  if (want_x)
    for (int i = t; i < C * F; i += 256) WcL[(i / F) * MS + (i % F)] = a.Wc[i];
  if (t < F) waL[t] = a.w_att ? a.w_att[t] : 0.0f;
  if (t < K) scL[t] = a.scales[t];
  const float batt = (a.w_att && a.b_att) ? a.b_att[0] : 0.0f;

  // B[k][j] = W2^T[k][j] = W2[j][k], j = this wave's 32 columns of h1_bar
  float wreg[F / 2];
#pragma unroll
  for (int s = 0; s < F / 2; ++s) wreg[s] = a.W2[(size_t)(32 * wave + (lane & 31)) * F + 2 * s + (lane >> 5)];

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();
    if (t < TE) {
      int r = -1;
      float xv = 0.0f;
      if (t < nv) {
        r = a.col0[p0 + t];
        xv = a.x[p0 + t];
        if (r < 0 || r >= a.N) r = -1;
      }
      recvL[t] = r; xL[t] = xv;
    }
    __syncthreads();
    // attention and its derivative: d = m . w_att, gm = g[recv] . m
    {
      const int e = t >> 3, part = t & 7;
      const int r = recvL[e];
      float d = 0.0f, gm = 0.0f;
      if (a.w_att && r >= 0) {
        const float* z2 = a.z2 + (size_t)(p0 + e) * F;
        const float* gr = a.g + (size_t)r * F;
#pragma unroll
        for (int c = part * 16; c < part * 16 + 16; ++c) {
          const float m = mp_apply_act(a.act2, a.alpha, z2[c]);
          d += m * waL[c];
          gm += gr[c] * m;
        }
      }
      if (a.w_att) {
        d += __shfl_xor(d, 1);  gm += __shfl_xor(gm, 1);
        d += __shfl_xor(d, 2);  gm += __shfl_xor(gm, 2);
        d += __shfl_xor(d, 4);  gm += __shfl_xor(gm, 4);
      }
      if (part == 0) {
        attL[e] = a.w_att ? mp_apply_act(a.act_att, a.alpha, d + batt) : 1.0f;
        dattL[e] = a.w_att ? gm * mp_act_grad(a.act_att, a.alpha, d + batt) : 0.0f;
      }
    }
    __syncthreads();
    {
      const int k = t & (F - 1);
#pragma unroll
      for (int i = 0; i < TE / 2; ++i) {
        const int e = (t >> 7) + 2 * i;
        float v = 0.0f;
        const int r = recvL[e];
        if (r >= 0) {
          const float z = a.z2[(size_t)(p0 + e) * F + k];
          const float mbar = attL[e] * a.g[(size_t)r * F + k] + dattL[e] * waL[k];
          v = mbar * mp_act_grad(a.act2, a.alpha, z);
        }
        dT[k * HS + e] = v;
      }
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    tile_gemm(dT, wreg, lane, acc);
    __syncthreads();   // every wave has read dT
    {
      const int col = 32 * wave + (lane & 31);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int e = 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
        float v = 0.0f;
        if (e < nv) {
          if (recvL[e] >= 0) v = acc[i] * mp_act_grad(a.act1, a.alpha, a.z1[(size_t)(p0 + e) * F + col]);
          a.z1_bar[(size_t)(p0 + e) * F + col] = v;
        }
        zL[e * MS + col] = v;
      }
    }
    if (!want_x) continue;
    __syncthreads();
    for (int i = t; i < TE * C; i += 256) {
      const int e = i / C, c = i - e * C;
      float d = 0.0f;
      for (int k = 0; k < F; ++k) d += zL[e * MS + k] * WcL[c * MS + k];
      encbL[e * MAXC + c] = d;
    }
    __syncthreads();
    if (t < nv) {
      float xb;
      if (K > 0) {
        xb = 0.0f;
        for (int k = 0; k < K; ++k) {
          float s, c;
          const float sk = scL[k];
          sincosf(xL[t] * sk, &s, &c);
          xb += sk * (encbL[t * MAXC + enc_col(k, K, a.interleave, false)] * c -
                      encbL[t * MAXC + enc_col(k, K, a.interleave, true)] * s);
        }
      } else {
        xb = encbL[t * MAXC];
      }
      a.x_bar[p0 + t] = xb;
    }
  }
}

int check_edge(const char* what, int64_t N, int64_t E, int K, int interleave, int act1, int act2, int act_att) {
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(K >= 0 && 2 * K <= MAXC, "%s: the fused edge step takes an encoding of at most %d columns (dim_half <= %d)",
             what, MAXC, MAXC / 2);
  MP_REQUIRE(interleave == 0 || interleave == 1, "%s: bad interleave flag", what);
  MP_REQUIRE(act1 >= 0 && act2 >= 0 && act_att >= 0 && act1 <= MP_ACT_LAST && act2 <= MP_ACT_LAST && act_att <= MP_ACT_SELU,
             "%s: unknown activation code", what);
  return MP_OK;
}

unsigned edge_grid(int64_t E) {
  const int64_t tiles = mp_tile::tiles_of(E);
  return static_cast<unsigned>(tiles < 512 ? tiles : 512);
}

}  // namespace

extern "C" {

int mp_position_encoding_f32(const float* x, int64_t M, const float* scales, int dim_half, int interleave, float* out,
                             mpStream_t stream) {
  MP_REQUIRE(M >= 0 && dim_half >= 1, "mp_position_encoding_f32: bad sizes");
  if (M == 0) return MP_OK;
  MP_REQUIRE(x && scales && out, "mp_position_encoding_f32: null pointer");
  position_encoding_kernel<<<mp::grid_for(M * dim_half), 256, 0, mp::as_stream(stream)>>>(x, M, scales, dim_half,
                                                                                          interleave ? 1 : 0, out);
  return mp::check_launch("mp_position_encoding_f32");
}

int mp_position_encoding_grad_f32(const float* x, int64_t M, const float* scales, int dim_half, int interleave,
                                  const float* g, float* x_bar, mpStream_t stream) {
  MP_REQUIRE(M >= 0 && dim_half >= 1, "mp_position_encoding_grad_f32: bad sizes");
  if (M == 0) return MP_OK;
  MP_REQUIRE(x && scales && g && x_bar, "mp_position_encoding_grad_f32: null pointer");
  position_encoding_grad_kernel<<<mp::grid_for(M), 256, 0, mp::as_stream(stream)>>>(x, M, scales, dim_half,
                                                                                    interleave ? 1 : 0, g, x_bar);
  return mp::check_launch("mp_position_encoding_grad_f32");
}

int mp_egnn_edge_ws_bytes(int64_t E, size_t* bytes_out_host) {
  MP_REQUIRE(E >= 0 && bytes_out_host, "mp_egnn_edge_ws_bytes: bad arguments");
  *bytes_out_host = mp_tile::ws_bytes(E, F);
  return MP_OK;
}

int mp_egnn_edge_f32(const float* Pa, const float* Pb, int64_t N, const float* x, const int32_t* cols, int64_t E,
                     const int32_t* ptr0, const int32_t* perm0, const float* scales, int dim_half, int interleave,
                     const float* Wc, const float* b1, int act1, const float* W2, const float* b2, int act2,
                     const float* w_att, const float* b_att, int act_att, float alpha, float* ws, size_t ws_bytes,
                     float* z1_save, float* z2_save, float* out, mpStream_t stream) {
  int rc = check_edge("mp_egnn_edge_f32", N, E, dim_half, interleave, act1, act2, act_att);
  if (rc != MP_OK || N == 0) return rc;
  MP_REQUIRE(ptr0 && out, "mp_egnn_edge_f32: null pointer");
  const size_t need = mp_tile::ws_bytes(E, F);
  if (E > 0) {
    MP_REQUIRE(Pa && Pb && x && cols && Wc && W2 && ws && (dim_half == 0 || scales), "mp_egnn_edge_f32: null pointer");
    MP_REQUIRE(ws_bytes >= need, "mp_egnn_edge_f32: workspace of %zu bytes, need %zu", ws_bytes, need);
    EdgeArgs a{};
    a.Pa = Pa; a.Pb = Pb; a.x = x; a.col0 = cols; a.ptr0 = ptr0; a.perm0 = perm0; a.scales = scales; a.Wc = Wc;
    a.b1 = b1; a.W2 = W2; a.b2 = b2; a.w_att = w_att; a.b_att = b_att; a.out = out; a.z1_save = z1_save;
    a.z2_save = z2_save; a.bnd = ws; a.N = static_cast<int>(N); a.E = static_cast<int>(E); a.K = dim_half;
    a.C = dim_half > 0 ? 2 * dim_half : 1;
    a.interleave = interleave; a.act1 = act1; a.act2 = act2; a.act_att = act_att; a.alpha = alpha;
    egnn_edge_fwd_kernel<<<edge_grid(E), 256, 0, mp::as_stream(stream)>>>(a);
    rc = mp::check_launch("mp_egnn_edge_f32");
    if (rc != MP_OK) return rc;
  }
  egnn_edge_finish_kernel<<<mp::grid_for(N * F), 256, 0, mp::as_stream(stream)>>>(ptr0, N, ws, out);
  return mp::check_launch("mp_egnn_edge_f32 (finish)");
}

int mp_egnn_edge_grad_f32(const float* g, int64_t N, const float* x, const int32_t* cols, int64_t E, const float* z1,
                          const float* z2, const float* scales, int dim_half, int interleave, const float* Wc, int act1,
                          const float* W2, int act2, const float* w_att, const float* b_att, int act_att, float alpha,
                          float* z1_bar, float* x_bar, mpStream_t stream) {
  int rc = check_edge("mp_egnn_edge_grad_f32", N, E, dim_half, interleave, act1, act2, act_att);
  if (rc != MP_OK || E == 0) return rc;
  MP_REQUIRE(g && x && cols && z1 && z2 && Wc && W2 && z1_bar && (dim_half == 0 || scales),
             "mp_egnn_edge_grad_f32: null pointer");
  EdgeArgs a{};
  a.g = g; a.x = x; a.col0 = cols; a.z1 = z1; a.z2 = z2; a.scales = scales; a.Wc = Wc; a.W2 = W2;
  a.w_att = w_att; a.b_att = b_att; a.z1_bar = z1_bar; a.x_bar = x_bar; a.N = static_cast<int>(N);
  a.E = static_cast<int>(E); a.K = dim_half;
  a.C = dim_half > 0 ? 2 * dim_half : 1; a.interleave = interleave; a.act1 = act1; a.act2 = act2; a.act_att = act_att;
  a.alpha = alpha;
  egnn_edge_bwd_kernel<<<edge_grid(E), 256, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_egnn_edge_grad_f32");
}

}  // extern "C"
