// Recurrent cells and the edge-network matvec of the NMPN / Set2Set family, as their reference layers use them:
//  * PoolingSet2Set (kgcnn/layers/pool/set2set.py:172-199) calls a STATELESS Keras LSTM on a length-1 sequence in every
//    iteration, i.e. one LSTM step from the zero state: the input GEMM runs on the matrix cores (mp_dense_f32), this file
//    holds the gate arithmetic;
//  * GRUUpdate (kgcnn/layers/conv/mpnn_conv.py:111-210) is one Keras GRUCell step (reset_after = True) on the flat node
//    values: two GEMMs + the combine below;
//  * MatMulMessages (mpnn_conv.py:69-108) is a per-edge matrix-vector product with the (M,F,F) matrices the edge network
//    produced: memory bound on the matrices (16 KB per edge at F = 64), read once with 16-B loads;
//  * the GRU readout of CMPNN (kgcnn/literature/CMPNN.py:157) is a Keras GRU over every graph's node sequence: the input
//    GEMM runs on the matrix cores (mp_dense_f32), the recurrence is one launch of this file.
#include <type_traits>

#include "mp_common.h"
#include "../../include/mpengine/cmpnn.h"
#include "../../include/mpengine/recurrent.h"

namespace {

// Keras LSTM gate order along the 4U axis: input, forget, cell candidate, output.
__global__ void lstm_zero_state_kernel(const float* __restrict__ z, int64_t R, int64_t U, int act, int rec_act,
                                       float* __restrict__ out) {
  const int64_t total = R * U;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = t / U, u = t % U;
    const float* zr = z + r * 4 * U;
    const float i = mp_apply_act(rec_act, 0.0f, zr[u]);
    const float c = i * mp_apply_act(act, 0.0f, zr[2 * U + u]);   // c = f * c0 + i * c~ with c0 = 0
    const float o = mp_apply_act(rec_act, 0.0f, zr[3 * U + u]);
    out[t] = o * mp_apply_act(act, 0.0f, c);
  }
}

// Keras GRUCell, reset_after = True; gate order along the 3U axis: update z, reset r, candidate h.
__global__ void gru_combine_kernel(const float* __restrict__ mx, const float* __restrict__ mh,
                                   const float* __restrict__ h, int64_t R, int64_t U, int act, int rec_act,
                                   float* __restrict__ out) {
  const int64_t total = R * U;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = t / U, u = t % U;
    const float* x = mx + r * 3 * U;
    const float* y = mh + r * 3 * U;
    const float zg = mp_apply_act(rec_act, 0.0f, x[u] + y[u]);
    const float rg = mp_apply_act(rec_act, 0.0f, x[U + u] + y[U + u]);
    const float hh = mp_apply_act(act, 0.0f, x[2 * U + u] + rg * y[2 * U + u]);
    out[t] = zg * h[t] + (1.0f - zg) * hh;
  }
}

// Reverse of gru_combine_kernel for an upstream gradient g (R, U).  The gates are recomputed from mx, mh and h in the
// forward's order (nothing but its three inputs is kept on the tape).  With a_z = mx_z + mh_z, a_r = mx_r + mh_r,
// a_h = mx_h + rg * mh_h:  d_h = g zg;  d a_z = g (h - hh) rec'(a_z);  d a_h = g (1 - zg) act'(a_h);
// d a_r = d a_h mh_h rec'(a_r);  d_mx = [d a_z | d a_r | d a_h],  d_mh = [d a_z | d a_r | d a_h rg].
__global__ void gru_combine_grad_kernel(const float* __restrict__ mx, const float* __restrict__ mh,
                                        const float* __restrict__ h, const float* __restrict__ g, int64_t R, int64_t U,
                                        int act, int rec_act, float* __restrict__ d_mx, float* __restrict__ d_mh,
                                        float* __restrict__ d_h) {
  const int64_t total = R * U;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = t / U, u = t % U;
    const float* x = mx + r * 3 * U;
    const float* y = mh + r * 3 * U;
    const float az = x[u] + y[u], ar = x[U + u] + y[U + u], yh = y[2 * U + u];
    const float zg = mp_apply_act(rec_act, 0.0f, az);
    const float rg = mp_apply_act(rec_act, 0.0f, ar);
    const float ah = x[2 * U + u] + rg * yh;
    const float hh = mp_apply_act(act, 0.0f, ah);
    const float gt = g[t];
    const float daz = gt * (h[t] - hh) * mp_act_grad(rec_act, 0.0f, az);
    const float dah = gt * (1.0f - zg) * mp_act_grad(act, 0.0f, ah);
    const float dar = dah * yh * mp_act_grad(rec_act, 0.0f, ar);
    if (d_h) d_h[t] = gt * zg;
    if (d_mx) {
      float* o = d_mx + r * 3 * U;
      o[u] = daz; o[U + u] = dar; o[2 * U + u] = dah;
    }
    if (d_mh) {
      float* o = d_mh + r * 3 * U;
      o[u] = daz; o[U + u] = dar; o[2 * U + u] = dah * rg;
    }
  }
}

// out[m][r] = sum_c mat[m][r][c] vec[m][c].  LPR = C / 4 lanes share a row (one float4 each), so a wave instruction reads
// 64 / LPR whole rows = 1 KB contiguous; the LPR partial dot products are reduced with log2(LPR) xor shuffles.
template <int LPR>
__global__ __launch_bounds__(256) void batched_matvec_kernel(const float* __restrict__ mat, const float* __restrict__ vec,
                                                             int64_t M, int64_t Ro, float* __restrict__ out) {
  constexpr int C = 4 * LPR;
  constexpr int RPI = 64 / LPR;   // rows per wave instruction
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR, c4 = lane % LPR;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t m = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; m < M; m += nwaves) {
    const float4 v = *reinterpret_cast<const float4*>(vec + m * C + 4 * c4);
    const float* base = mat + m * Ro * C;
    for (int64_t r0 = 0; r0 < Ro; r0 += RPI) {
      const int64_t r = r0 + sub;
      float acc = 0.0f;
      if (r < Ro) {
        const float4 a = *reinterpret_cast<const float4*>(base + r * C + 4 * c4);
        acc = a.x * v.x + a.y * v.y + a.z * v.z + a.w * v.w;
      }
#pragma unroll
      for (int off = LPR / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
      if (c4 == 0 && r < Ro) out[m * Ro + r] = acc;
    }
  }
}

__global__ void batched_matvec_generic_kernel(const float* __restrict__ mat, const float* __restrict__ vec, int64_t M,
                                              int64_t Ro, int64_t C, float* __restrict__ out) {
  const int64_t total = M * Ro;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t m = t / Ro;
    const float* a = mat + t * C;
    const float* v = vec + m * C;
    float acc = 0.0f;
    for (int64_t c = 0; c < C; ++c) acc += a[c] * v[c];
    out[t] = acc;
  }
}

// Keras GRU (reset_after = True) over the node sequence of every graph, state after the last node (the readout of
// kgcnn/literature/CMPNN.py:157).  The whole recurrence is this one launch: the loop over the sequence runs in here.
// A workgroup of 8 waves owns 16 graphs = the rows of one A operand of v_mfma_f32_16x16x4_f32 (4 and 8 graphs per
// workgroup measured the same: DESIGN 3.20); their states live in LDS (row stride = 4 mod 64 floats: the 64 lanes of an A read hit 64 banks).
// Per step wave w takes the 16-column blocks w, w + 8, ... of the state (up to four) and computes the z, r and h blocks of
// `state R` for all of them in ONE pass over k, so the three recurrent pre-activations of one (graph, column) meet in one
// lane and the combine is mp_gru_combine_f32's, in its order.  R (u x 3u, 1.08 MB at u = 300) does not fit a workgroup: its
// slabs are re-read (from L2) in every step, and a step is a chain of such round trips - so the loads of several k steps
// for every block and gate of the wave (GRU_LOADS x 3 = 36) are issued together, in front of their MFMAs: 19 round trips per
// step instead of one per block, gate and k group.  A graph whose sequence has ended keeps its state while the tile runs
// to its longest member; a graph without nodes leaves the zero state.
constexpr int GRU_ROWS = 16;
constexpr int GRU_THREADS = 512;
constexpr int GRU_WAVES = GRU_THREADS / 64;
constexpr int GRU_LOADS = 12;   // k steps x blocks whose three slab loads are in flight together (36 loads)
constexpr int GRU_MAX_UNITS = MP_GRU_RAGGED_MAX_UNITS;
constexpr int GRU_MAX_BLOCKS = (GRU_MAX_UNITS / 16 + GRU_WAVES - 1) / GRU_WAVES;   // column blocks of one wave
constexpr int GRU_MAX_STRIDE = ((GRU_MAX_UNITS + 63) / 64) * 64 + 4;
static_assert(GRU_MAX_BLOCKS == 4, "the step below is instantiated for one to four blocks per wave");

typedef float gru_f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(GRU_THREADS) void gru_ragged_last_kernel(
    const float* __restrict__ mx, int64_t n_nodes, const int64_t* __restrict__ splits, int64_t G,
    const float* __restrict__ R, const float* __restrict__ b_rec, int U, int act, int rec_act,
    float* __restrict__ out) {
  __shared__ float hL[GRU_ROWS * GRU_MAX_STRIDE];
  __shared__ long long startL[GRU_ROWS];
  __shared__ int lenL[GRU_ROWS];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lc = lane & 15, kq = lane >> 4;
  const int S = ((U + 63) / 64) * 64 + 4;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * GRU_ROWS;
  const int U3 = 3 * U;

  if (t < GRU_ROWS) {
    const int64_t g = g0 + t;
    int64_t a = 0, b = 0;
    if (g < G) {
      a = splits[g];
      b = splits[g + 1];
      a = a < 0 ? 0 : (a > n_nodes ? n_nodes : a);
      b = b < a ? a : (b > n_nodes ? n_nodes : b);
    }
    startL[t] = a;
    const int64_t len = b - a;
    lenL[t] = len > 0x7fffffff ? 0x7fffffff : static_cast<int>(len);
  }
  for (int i = t; i < GRU_ROWS * S; i += GRU_THREADS) hL[i] = 0.0f;
  __syncthreads();
  int steps = 0;
#pragma unroll
  for (int r = 0; r < GRU_ROWS; ++r) steps = lenL[r] > steps ? lenL[r] : steps;

  const int blocks = (U + 15) / 16;
  const int my_blocks = wave < blocks ? (blocks - wave + GRU_WAVES - 1) / GRU_WAVES : 0;   // wave-uniform
  const int ksteps = U / 4;
  float hnew[GRU_MAX_BLOCKS][4];

  // phase 1 of a step for a wave with NB blocks: its blocks of `state R` and the combine, in registers (the states in
  // LDS are only read)
  auto advance = [&](int step, auto nb_tag) {
    constexpr int NB = decltype(nb_tag)::value;
    constexpr int GRU_KGROUP = GRU_LOADS / NB;
    int colc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int col = 16 * (wave + j * GRU_WAVES) + lc;
      colc[j] = col < U ? col : U - 1;   // the last block may be partial: work on a column inside, drop the result
    }
    gru_f32x4 az[NB], ar[NB], ah[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) { az[j][i] = 0.0f; ar[j][i] = 0.0f; ah[j][i] = 0.0f; }
    const float* ap = hL + lc * S + kq;
    const float* bp = R + kq * U3;   // offsets into R stay below 3 u^2 < 2^20
    int s = 0;
    for (; s + GRU_KGROUP <= ksteps; s += GRU_KGROUP) {
      float a[GRU_KGROUP], wz[NB][GRU_KGROUP], wr[NB][GRU_KGROUP], wh[NB][GRU_KGROUP];
#pragma unroll
      for (int q = 0; q < GRU_KGROUP; ++q) {
        const float* bs = bp + 4 * (s + q) * U3;
        a[q] = ap[4 * (s + q)];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          wz[j][q] = bs[colc[j]];
          wr[j][q] = bs[U + colc[j]];
          wh[j][q] = bs[2 * U + colc[j]];
        }
      }
#pragma unroll
      for (int q = 0; q < GRU_KGROUP; ++q) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          az[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], wz[j][q], az[j], 0, 0, 0);
          ar[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], wr[j][q], ar[j], 0, 0, 0);
          ah[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], wh[j][q], ah[j], 0, 0, 0);
        }
      }
    }
    for (; s < ksteps; ++s) {
      const float a = ap[4 * s];
      const float* bs = bp + 4 * s * U3;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        az[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[colc[j]], az[j], 0, 0, 0);
        ar[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[U + colc[j]], ar[j], 0, 0, 0);
        ah[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[2 * U + colc[j]], ah[j], 0, 0, 0);
      }
    }
    // the input pre-activations of the lane's (graph, column) pairs, then the combine
    bool live[4];
    size_t xrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * kq + i;
      live[i] = step < lenL[row];
      xrow[i] = static_cast<size_t>(live[i] ? startL[row] + step : 0) * U3;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float xz[4], xr[4], xh[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* xp = mx + xrow[i] + colc[j];
        xz[i] = live[i] ? xp[0] : 0.0f;
        xr[i] = live[i] ? xp[U] : 0.0f;
        xh[i] = live[i] ? xp[2 * U] : 0.0f;
      }
      const float bz = b_rec ? b_rec[colc[j]] : 0.0f, br = b_rec ? b_rec[U + colc[j]] : 0.0f,
                  bh = b_rec ? b_rec[2 * U + colc[j]] : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hold = hL[(4 * kq + i) * S + colc[j]];
        const float zg = mp_apply_act(rec_act, 0.0f, xz[i] + (az[j][i] + bz));
        const float rg = mp_apply_act(rec_act, 0.0f, xr[i] + (ar[j][i] + br));
        const float hh = mp_apply_act(act, 0.0f, xh[i] + rg * (ah[j][i] + bh));
        const float hn = zg * hold + (1.0f - zg) * hh;
        hnew[j][i] = live[i] ? hn : hold;
      }
    }
  };

  for (int step = 0; step < steps; ++step) {
    if (my_blocks == 4) advance(step, std::integral_constant<int, 4>());
    else if (my_blocks == 3) advance(step, std::integral_constant<int, 3>());
    else if (my_blocks == 2) advance(step, std::integral_constant<int, 2>());
    else if (my_blocks == 1) advance(step, std::integral_constant<int, 1>());
    __syncthreads();
    // phase 2: the new states
#pragma unroll
    for (int j = 0; j < GRU_MAX_BLOCKS; ++j) {
      const int col = 16 * (wave + j * GRU_WAVES) + lc;
      if (j < my_blocks && col < U) {
#pragma unroll
        for (int i = 0; i < 4; ++i) hL[(4 * kq + i) * S + col] = hnew[j][i];
      }
    }
    __syncthreads();
  }
  for (int i = t; i < GRU_ROWS * U; i += GRU_THREADS) {
    const int row = i / U, col = i - row * U;
    if (g0 + row < G) out[static_cast<size_t>(g0 + row) * U + col] = hL[row * S + col];
  }
}

}  // namespace

extern "C" {

int mp_gru_ragged_last_f32(const float* mx, int64_t n_nodes, const int64_t* row_splits, int64_t G, const float* R,
                           const float* b_rec, int64_t U, int act, int rec_act, float* out, mpStream_t stream) {
  const char* what = "mp_gru_ragged_last_f32";
  MP_REQUIRE(n_nodes >= 0 && G >= 0, "%s: bad sizes", what);
  MP_REQUIRE(U >= 4 && U % 4 == 0 && U <= GRU_MAX_UNITS, "%s: units must be a multiple of 4, at most %d, got %lld", what,
             GRU_MAX_UNITS, (long long)U);
  MP_REQUIRE(act >= MP_ACT_LINEAR && act <= MP_ACT_LAST && rec_act >= MP_ACT_LINEAR && rec_act <= MP_ACT_LAST,
             "%s: unknown activation", what);
  if (G == 0) return MP_OK;
  MP_REQUIRE(row_splits && R && out && (n_nodes == 0 || mx), "%s: null pointer", what);
  const int64_t grid = mp::ceil_div(G, GRU_ROWS);
  MP_REQUIRE(grid < (int64_t{1} << 31), "%s: grid too large", what);
  gru_ragged_last_kernel<<<static_cast<unsigned>(grid), GRU_THREADS, 0, mp::as_stream(stream)>>>(
      mx, n_nodes, row_splits, G, R, b_rec, static_cast<int>(U), act, rec_act, out);
  return mp::check_launch(what);
}

int mp_lstm_zero_state_f32(const float* z, int64_t R, int64_t U, int act, int rec_act, float* out, mpStream_t stream) {
  MP_REQUIRE(R >= 0 && U >= 1, "mp_lstm_zero_state_f32: bad sizes");
  MP_REQUIRE(act >= MP_ACT_LINEAR && act <= MP_ACT_LAST && rec_act >= MP_ACT_LINEAR && rec_act <= MP_ACT_LAST,
             "mp_lstm_zero_state_f32: unknown activation");
  if (R == 0) return MP_OK;
  MP_REQUIRE(z && out, "mp_lstm_zero_state_f32: null pointer");
  lstm_zero_state_kernel<<<mp::grid_for(R * U), 256, 0, mp::as_stream(stream)>>>(z, R, U, act, rec_act, out);
  return mp::check_launch("mp_lstm_zero_state_f32");
}

int mp_gru_combine_f32(const float* mx, const float* mh, const float* h, int64_t R, int64_t U, int act, int rec_act,
                       float* out, mpStream_t stream) {
  MP_REQUIRE(R >= 0 && U >= 1, "mp_gru_combine_f32: bad sizes");
  MP_REQUIRE(act >= MP_ACT_LINEAR && act <= MP_ACT_LAST && rec_act >= MP_ACT_LINEAR && rec_act <= MP_ACT_LAST,
             "mp_gru_combine_f32: unknown activation");
  if (R == 0) return MP_OK;
  MP_REQUIRE(mx && mh && h && out, "mp_gru_combine_f32: null pointer");
  gru_combine_kernel<<<mp::grid_for(R * U), 256, 0, mp::as_stream(stream)>>>(mx, mh, h, R, U, act, rec_act, out);
  return mp::check_launch("mp_gru_combine_f32");
}

int mp_gru_combine_grad_f32(const float* mx, const float* mh, const float* h, const float* g, int64_t R, int64_t U,
                            int act, int rec_act, float* d_mx, float* d_mh, float* d_h, mpStream_t stream) {
  const char* what = "mp_gru_combine_grad_f32";
  MP_REQUIRE(R >= 0 && U >= 1, "%s: bad sizes", what);
  MP_REQUIRE(act >= MP_ACT_LINEAR && act <= MP_ACT_LAST && rec_act >= MP_ACT_LINEAR && rec_act <= MP_ACT_LAST,
             "%s: unknown activation", what);
  if (R == 0) return MP_OK;
  MP_REQUIRE(mx && mh && h && g, "%s: null pointer", what);
  MP_REQUIRE(d_mx || d_mh || d_h, "%s: no gradient asked for", what);
  gru_combine_grad_kernel<<<mp::grid_for(R * U), 256, 0, mp::as_stream(stream)>>>(mx, mh, h, g, R, U, act, rec_act, d_mx,
                                                                                 d_mh, d_h);
  return mp::check_launch(what);
}

int mp_batched_matvec_f32(const float* mat, const float* vec, int64_t M, int64_t Ro, int64_t C, float* out,
                          mpStream_t stream) {
  MP_REQUIRE(M >= 0 && Ro >= 1 && C >= 1, "mp_batched_matvec_f32: bad sizes");
  if (M == 0) return MP_OK;
  MP_REQUIRE(mat && vec && out, "mp_batched_matvec_f32: null pointer");
  hipStream_t s = mp::as_stream(stream);
  const bool aligned = (reinterpret_cast<uintptr_t>(mat) % 16 == 0) && (reinterpret_cast<uintptr_t>(vec) % 16 == 0);
  const unsigned grid = mp::grid_for(M * 64);
  if (aligned && C == 256) batched_matvec_kernel<64><<<grid, 256, 0, s>>>(mat, vec, M, Ro, out);
  else if (aligned && C == 128) batched_matvec_kernel<32><<<grid, 256, 0, s>>>(mat, vec, M, Ro, out);
  else if (aligned && C == 64) batched_matvec_kernel<16><<<grid, 256, 0, s>>>(mat, vec, M, Ro, out);
  else if (aligned && C == 32) batched_matvec_kernel<8><<<grid, 256, 0, s>>>(mat, vec, M, Ro, out);
  else if (aligned && C == 16) batched_matvec_kernel<4><<<grid, 256, 0, s>>>(mat, vec, M, Ro, out);
  else batched_matvec_generic_kernel<<<mp::grid_for(M * Ro), 256, 0, s>>>(mat, vec, M, Ro, C, out);
  return mp::check_launch("mp_batched_matvec_f32");
}

}  // extern "C"
