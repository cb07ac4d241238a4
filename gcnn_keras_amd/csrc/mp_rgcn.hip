// RGCN and GNNFilm (kgcnn/literature/RGCN.py:96-103, kgcnn/literature/GNNFilm.py:93-102): one block in one launch.
//
// The layer sequence gathers an (M, K) tensor, sends it through RelationalDense (one thread per output element, a scalar
// fma chain over K), multiplies and segment-sums it: four edge-sized round trips per block, GNNFilm three RelationalDense
// calls.  The sum over a receiver's edges commutes with the per-relation product whenever the message RelationalDense is
// linear, so for receiver i
//   MP_RELCONV_RGCN  h_i = sum_q A_iq W_q + s_i b,  A_iq = sum_{e -> i, rel e = q} w_e n_{j(e)},  s_i = sum_{e -> i} w_e
//                    out_i = act(h_i + act0(n_i W0 + b0))
//   MP_RELCONV_FILM  h_i = sum_q [ g_iq * (A_iq W_q + c_iq b) + c_iq t_iq ],  g_iq = act_m(n_i Wg_q + bg),
//                    t_iq = act_m(n_i Wt_q + bt),  c_iq = number of such edges (A unweighted);  out_i = act(h_i)
// and nothing edge-sized is written.
//
// One 256-thread workgroup owns 16 consecutive receivers and walks all of their CSR positions itself, so no receiver is
// cut across workgroups and there is no workspace.  The tile's positions are staged in LDS CHUNK at a time (sender,
// relation, row, weight) together with a 64-bit mask of the relations present in the chunk.  The present relations, in
// ascending order, are dealt to the four waves in turn, and a wave does everything for its relation on its own, without a
// workgroup barrier: it finds the matching positions by ballot, accumulates A_q (16 x K, row stride K + 2, lane = column)
// in list order - a sender row is read only where the relation matches - into its own LDS tile, and runs A_q W_q for all U
// columns on v_mfma_f32_16x16x4_f32, the weight slice read straight from the (R, K, U) kernel (lane: k = 4 s + (lane >> 4),
// column lane & 15, as mp_node_tile.h).  In FiLM mode the wave runs two more products on the tile's own node rows and
// folds g * (. + c b) + c t into its running sum; in RGCN mode every product is added to the running sum.  At the end the
// four waves' sums are added in wave order through LDS; the RGCN self loop is one more product in front of the epilogue.
// (A first form walked the relations one after the other with the whole workgroup, two barriers and the exposed latency
// of the gather and of the weight loads per relation: on 128 QM9-sized graphs with 20 relations it was SLOWER than the
// layer sequence, 160 against 134 us per replayed RGCN forward.)
// A tile with more than CHUNK positions repeats this per chunk (the products are linear in A and c).  The summation order
// is fixed - per wave: chunk ascending, its relations ascending, list order within; then wave order - with no atomics on
// floats: two runs give equal bits.
//
// A relation outside [0, R) uses a zero kernel, as mp_relational_dense_f32 does: in RGCN such an edge adds w_e b (it is
// part of s_i only), in FiLM b * act_m(bg) + act_m(bt).  A position whose edge id or sender is out of range is skipped.
// FP32 throughout; forward only.
#include <type_traits>

#include "mp_common.h"
#include "../../include/mpengine/rgcn.h"

namespace {

using floatx4 = __attribute__((ext_vector_type(4))) float;

constexpr int TILE = 16;      // receivers per workgroup = rows of one MFMA
constexpr int CHUNK = 256;    // positions staged at a time (one per thread)
constexpr int NTHREADS = 256;
constexpr int REL_SKIP = -2;  // staged relation of a skipped position
constexpr int REL_ZERO = -1;  // staged relation of an id outside [0, R): zero kernel

struct RelConvArgs {
  const float* nodes; int N;
  const int32_t* cols; const int32_t* ptr0; const int32_t* perm0; int E;
  const int64_t* rel; const float* weights; int R;
  const float* W; const float* b;
  const float* W0; const float* b0; int act0;
  const float* Wg; const float* bg; const float* Wt; const float* bt; int act_m;
  int act; float alpha;
  float* out;
};

// acc[cb] += X (16 x K, LDS, row stride K + 2) @ Wq[:, col0 + 16 cb + (lane & 15)].  The product is formed on two
// accumulators of its own per column block (even and odd k steps: 2 NCB independent MFMA chains cover the 40-cycle
// dependent latency) and added to acc once: a running sum never becomes one fma chain over relations x K terms, whose
// rounding error grows with its length (measured: 3.4e-6 of a row from float64 with one chain over 64 relations x 128,
// against 6e-7 for the per-edge order).
template <int K, int U, int NCB>
__device__ __forceinline__ void tile_product(const float* __restrict__ Xs, const float* __restrict__ Wq, int col0,
                                             int lane, floatx4 (&acc)[NCB]) {
  const float* xp = Xs + (lane & 15) * (K + 2) + (lane >> 4);
  const float* wp = Wq + (lane >> 4) * U + col0 + (lane & 15);
  floatx4 p0[NCB], p1[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) p0[cb] = p1[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int s = 0; s < K / 4; s += 2) {
    const float a0 = xp[4 * s], a1 = xp[4 * s + 4];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      p0[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wp[4 * s * U + 16 * cb], p0[cb], 0, 0, 0);
      p1[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wp[(4 * s + 4) * U + 16 * cb], p1[cb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] += p0[cb] + p1[cb];
}

// LDS traffic of ONE wave: its earlier writes are visible to its later reads (other lanes' included)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int K, int U, bool FILM>
__global__ __launch_bounds__(NTHREADS) void relational_conv_kernel(const RelConvArgs a) {
  constexpr int LD = K + 2;                       // (2 row + k) mod 32: the A operand reads are conflict-free
  constexpr int NCBT = U / 16;                    // 16-column blocks of the output tile
  constexpr int CG = NCBT < 4 ? NCBT : 4;         // column blocks per product pass of a wave
  constexpr int NCB = U >= 64 ? U / 64 : 1;       // column blocks per wave in the epilogue
  constexpr int KPL = (K + 63) / 64;              // columns of A per lane in the accumulate walk
  constexpr int NSUB = CHUNK / 64;
  // four A_q tiles, one per wave; the same memory carries the waves' partial sums (16 x U each) to the epilogue
  __shared__ float s_buf[cmax(4 * TILE * LD, 4 * TILE * U)];
  __shared__ float Xs[TILE * LD];
  __shared__ int s_send[CHUNK];
  __shared__ int s_rel[CHUNK];
  __shared__ int s_row[CHUNK];
  __shared__ float s_w[CHUNK];
  __shared__ int s_ptr[TILE + 1];
  __shared__ float s_cnt[4][TILE];                // c_iq of the relation a wave works on
  __shared__ float s_tot[TILE];                   // RGCN: s_i ; FiLM: edges with a relation outside [0, R)
  __shared__ unsigned s_mask[2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int node0 = static_cast<int>(blockIdx.x) * TILE;
  const int N = a.N, E = a.E, R = a.R;
  float* As = s_buf + wave * TILE * LD;

  // the tile's CSR ranges, clamped into [0, E] and monotone; rows behind N are empty
  if (tid == 0) {
    int prev = 0;
    for (int r = 0; r <= TILE; ++r) {
      int p = prev;
      if (E > 0 && node0 + r <= N) {
        p = a.ptr0[node0 + r];
        p = p < 0 ? 0 : (p > E ? E : p);
        if (r > 0 && p < prev) p = prev;
      }
      s_ptr[r] = p;
      prev = p;
    }
  }
  if (tid < TILE) s_tot[tid] = 0.0f;
  // the tile's own node rows (zero behind N)
  for (int i = tid; i < TILE * K; i += NTHREADS) {
    const int r = i / K, c = i % K;
    Xs[r * LD + c] = node0 + r < N ? a.nodes[static_cast<size_t>(node0 + r) * K + c] : 0.0f;
  }
  __syncthreads();
  const int p_begin = s_ptr[0], p_end = s_ptr[TILE];

  floatx4 hsum[NCBT];                             // this wave's share of the tile's sum, all U columns
#pragma unroll
  for (int cb = 0; cb < NCBT; ++cb) hsum[cb] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = p_begin; c0 < p_end; c0 += CHUNK) {
    const int c1 = c0 + CHUNK < p_end ? c0 + CHUNK : p_end;
    if (tid < 2) s_mask[tid] = 0u;
    __syncthreads();   // the previous chunk's readers are done; the mask is zero
    {
      int q = REL_SKIP, s = 0, row = 0;
      float w = 0.0f;
      if (c0 + tid < c1) {
        const int p = c0 + tid;
        const int e = a.perm0 ? a.perm0[p] : p;
        for (int r = 1; r < TILE; ++r) row += s_ptr[r] <= p ? 1 : 0;   // the receiver's row: s_ptr[row] <= p < s_ptr[row + 1]
        if (e >= 0 && e < E) {
          s = a.cols[static_cast<size_t>(E) + e];
          if (s >= 0 && s < N) {
            const int64_t q64 = a.rel[e];
            q = (q64 >= 0 && q64 < R) ? static_cast<int>(q64) : REL_ZERO;
            w = (!FILM && a.weights) ? a.weights[e] : 1.0f;
            if (q >= 0) atomicOr(&s_mask[q >> 5], 1u << (q & 31));
          } else {
            s = 0;
          }
        }
      }
      s_send[tid] = s; s_rel[tid] = q; s_row[tid] = row; s_w[tid] = w;   // behind c1: REL_SKIP
    }
    __syncthreads();
    // per row: RGCN the sum of all weights, FiLM the number of zero-kernel edges (list order)
    if (tid < TILE) {
      const int lo = s_ptr[tid] > c0 ? s_ptr[tid] : c0, hi = s_ptr[tid + 1] < c1 ? s_ptr[tid + 1] : c1;
      float t = s_tot[tid];
      for (int p = lo; p < hi; ++p) {
        const int q = s_rel[p - c0];
        if (FILM) { if (q == REL_ZERO) t += 1.0f; }
        else if (q != REL_SKIP) t += s_w[p - c0];
      }
      s_tot[tid] = t;
    }
    const unsigned m0 = s_mask[0], m1 = s_mask[1];
    __syncthreads();   // every wave holds the mask before a fast wave zeroes it for the next chunk

    // the present relations in ascending order, dealt to the four waves in turn; a wave owns its relation's A_q tile
    int turn = 0;
    for (int q = 0; q < R; ++q) {
      if (!(((q < 32 ? m0 : m1) >> (q & 31)) & 1u)) continue;   // uniform over the workgroup
      if (((turn++) & 3) != wave) continue;                    // uniform over the wave
      // A_q: lane = column(s); the wave walks the matching positions in list order (ascending row), one row at a time
#pragma unroll
      for (int r = 0; r < TILE; ++r)
#pragma unroll
        for (int kk = 0; kk < KPL; ++kk)
          if (lane + 64 * kk < K) As[r * LD + lane + 64 * kk] = 0.0f;
      if (lane < TILE) s_cnt[wave][lane] = 0.0f;
      int cur = -1;
      float sum[KPL], cnt = 0.0f;
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) sum[kk] = 0.0f;
      auto flush = [&]() {
        if (cur >= 0) {
#pragma unroll
          for (int kk = 0; kk < KPL; ++kk)
            if (lane + 64 * kk < K) As[cur * LD + lane + 64 * kk] = sum[kk];
          if (lane == 0) s_cnt[wave][cur] = cnt;
        }
      };
      for (int j = 0; j < NSUB && 64 * j < c1 - c0; ++j) {
        unsigned long long m = __ballot(s_rel[64 * j + lane] == q);
        while (m != 0ull) {
          const int p = 64 * j + static_cast<int>(__builtin_ctzll(m));
          m &= m - 1ull;
          // one position for the whole wave: its row, sender and weight live in scalar registers
          const int row = __builtin_amdgcn_readfirstlane(s_row[p]);
          const float w = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_w[p])));
          const float* src = a.nodes + static_cast<size_t>(__builtin_amdgcn_readfirstlane(s_send[p])) * K + lane;
          if (row != cur) {
            flush();
            cur = row; cnt = 0.0f;
#pragma unroll
            for (int kk = 0; kk < KPL; ++kk) sum[kk] = 0.0f;
          }
#pragma unroll
          for (int kk = 0; kk < KPL; ++kk)
            if (lane + 64 * kk < K) sum[kk] += FILM ? src[64 * kk] : w * src[64 * kk];
          cnt += 1.0f;
        }
      }
      flush();
      wave_sync();
      const float* Wq = a.W + static_cast<size_t>(q) * K * U;
      // one pass of CG column blocks; called per constant cg (a loop over cg is not always unrolled, and hsum[cg + cb]
      // has to stay a register)
      auto pass = [&](auto cg_tag) {
        constexpr int cg = decltype(cg_tag)::value;
        if (!FILM) {
          floatx4 (&part)[CG] = *reinterpret_cast<floatx4 (*)[CG]>(&hsum[cg]);
          tile_product<K, U, CG>(As, Wq, 16 * cg, lane, part);
        } else {
          floatx4 pm[CG], pg[CG], pt[CG];
#pragma unroll
          for (int cb = 0; cb < CG; ++cb) pm[cb] = pg[cb] = pt[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
          tile_product<K, U, CG>(As, Wq, 16 * cg, lane, pm);
          tile_product<K, U, CG>(Xs, a.Wg + static_cast<size_t>(q) * K * U, 16 * cg, lane, pg);
          tile_product<K, U, CG>(Xs, a.Wt + static_cast<size_t>(q) * K * U, 16 * cg, lane, pt);
#pragma unroll
          for (int cb = 0; cb < CG; ++cb) {
            const int col = 16 * (cg + cb) + (lane & 15);
            const float bm = a.b ? a.b[col] : 0.0f, bgv = a.bg ? a.bg[col] : 0.0f, btv = a.bt ? a.bt[col] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float c = s_cnt[wave][4 * (lane >> 4) + i];
              if (c > 0.0f) {   // a row without such an edge adds nothing (not even 0 * inf)
                const float g = mp_apply_act(a.act_m, a.alpha, pg[cb][i] + bgv);
                const float t = mp_apply_act(a.act_m, a.alpha, pt[cb][i] + btv);
                hsum[cg + cb][i] += g * (pm[cb][i] + c * bm) + c * t;
              }
            }
          }
        }
      };
      pass(std::integral_constant<int, 0>());
      if constexpr (NCBT > CG) pass(std::integral_constant<int, CG>());
      static_assert(NCBT <= 2 * CG, "U <= 128: at most two passes");
      wave_sync();     // the reads of As and s_cnt are done before the next relation's writes
    }
  }
  __syncthreads();       // every wave is through with its A_q tile; s_tot of the last chunk

  // the four partial sums to LDS (wave w: floats [w * 16 * U, (w + 1) * 16 * U), row-major), added in wave order below
#pragma unroll
  for (int cb = 0; cb < NCBT; ++cb)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      s_buf[(wave * TILE + 4 * (lane >> 4) + i) * U + 16 * cb + (lane & 15)] = hsum[cb][i];
  __syncthreads();

  const int col0 = wave * 16 * NCB;
  if (col0 >= U) return;                          // U = 32: two waves hold the columns
  floatx4 self[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) self[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (!FILM) tile_product<K, U, NCB>(Xs, a.W0, col0, lane, self);
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int col = col0 + 16 * cb + (lane & 15);
    const float bm = a.b ? a.b[col] : 0.0f;
    float extra_b = 0.0f, zero_edge = 0.0f;
    if (FILM) {
      const float bgv = a.bg ? a.bg[col] : 0.0f, btv = a.bt ? a.bt[col] : 0.0f;
      zero_edge = bm * mp_apply_act(a.act_m, a.alpha, bgv) + mp_apply_act(a.act_m, a.alpha, btv);
    } else {
      extra_b = a.b0 ? a.b0[col] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * (lane >> 4) + i;
      if (node0 + row >= N) continue;
      const float t = s_tot[row];
      const float* part = s_buf + row * U + col;
      float v = ((part[0] + part[TILE * U]) + part[2 * TILE * U]) + part[3 * TILE * U];
      if (FILM) {
        if (t > 0.0f) v += t * zero_edge;
      } else {
        v = (v + t * bm) + mp_apply_act(a.act0, a.alpha, self[cb][i] + extra_b);
      }
      a.out[static_cast<size_t>(node0 + row) * U + col] = mp_apply_act(a.act, a.alpha, v);
    }
  }
}

template <int K, int U>
void launch(int mode, unsigned grid, hipStream_t s, const RelConvArgs& a) {
  if (mode == MP_RELCONV_FILM) relational_conv_kernel<K, U, true><<<grid, NTHREADS, 0, s>>>(a);
  else relational_conv_kernel<K, U, false><<<grid, NTHREADS, 0, s>>>(a);
}

template <int K>
bool launch_u(int U, int mode, unsigned grid, hipStream_t s, const RelConvArgs& a) {
  switch (U) {
    case 32: launch<K, 32>(mode, grid, s, a); return true;
    case 64: launch<K, 64>(mode, grid, s, a); return true;
    case 128: launch<K, 128>(mode, grid, s, a); return true;
    default: return false;
  }
}

bool width_ok(int64_t w) { return w == 32 || w == 64 || w == 128; }
bool act_ok(int act) { return act >= MP_ACT_LINEAR && act <= MP_ACT_LAST; }

}  // namespace

extern "C" {

int mp_relational_conv_f32(int mode, const float* nodes, int64_t N, int64_t K, const int32_t* cols, int64_t E,
                           const int32_t* ptr0, const int32_t* perm0, const int64_t* rel, const float* weights,
                           int64_t R, const float* W, const float* b, int64_t U, const float* W0, const float* b0,
                           int act0, const float* Wg, const float* bg, const float* Wt, const float* bt, int act_m,
                           int act, float alpha, float* out, mpStream_t stream) {
  const char* what = "mp_relational_conv_f32";
  MP_REQUIRE(mode == MP_RELCONV_RGCN || mode == MP_RELCONV_FILM, "%s: unknown mode %d", what, mode);
  MP_REQUIRE(width_ok(K) && width_ok(U), "%s: K and U are each 32, 64 or 128, got K=%lld U=%lld", what, (long long)K,
             (long long)U);
  MP_REQUIRE(R >= 1 && R <= MP_RELCONV_MAX_RELATIONS, "%s: 1 <= R <= %d, got %lld", what, MP_RELCONV_MAX_RELATIONS,
             (long long)R);
  MP_REQUIRE(N >= 0 && E >= 0 && N < (int64_t{1} << 31) - TILE && E < (int64_t{1} << 31) - CHUNK,
             "%s: nodes and edges are indexed with 32 bits (N=%lld E=%lld)", what, (long long)N, (long long)E);
  MP_REQUIRE(act_ok(act) && act_ok(act0) && act_ok(act_m), "%s: unknown activation %d / %d / %d", what, act, act0, act_m);
  if (N == 0) return MP_OK;
  MP_REQUIRE(nodes && out && W, "%s: null pointer", what);
  MP_REQUIRE(E == 0 || (cols && ptr0 && rel), "%s: %lld edges without index columns, CSR or relations", what,
             (long long)E);
  if (mode == MP_RELCONV_RGCN) MP_REQUIRE(W0 != nullptr, "%s: the RGCN mode needs the self-loop kernel", what);
  else MP_REQUIRE(Wg && Wt, "%s: the FiLM mode needs both modulation kernels", what);
  RelConvArgs a;
  a.nodes = nodes; a.N = static_cast<int>(N);
  a.cols = cols; a.ptr0 = ptr0; a.perm0 = perm0; a.E = static_cast<int>(E);
  a.rel = rel; a.weights = weights; a.R = static_cast<int>(R);
  a.W = W; a.b = b;
  a.W0 = W0; a.b0 = b0; a.act0 = act0;
  a.Wg = Wg; a.bg = bg; a.Wt = Wt; a.bt = bt; a.act_m = act_m;
  a.act = act; a.alpha = alpha;
  a.out = out;
  const unsigned grid = static_cast<unsigned>(mp::ceil_div(N, TILE));
  hipStream_t s = mp::as_stream(stream);
  bool ok = false;
  switch (K) {
    case 32: ok = launch_u<32>(static_cast<int>(U), mode, grid, s, a); break;
    case 64: ok = launch_u<64>(static_cast<int>(U), mode, grid, s, a); break;
    case 128: ok = launch_u<128>(static_cast<int>(U), mode, grid, s, a); break;
    default: break;
  }
  MP_REQUIRE(ok, "%s: unserved sizes", what);
  return mp::check_launch(what);
}

}  // extern "C"
