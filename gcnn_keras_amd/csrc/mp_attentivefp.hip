// AttentiveFP (kgcnn/layers/conv/attentivefp_conv.py:75-107 AttentiveHeadFP.call, :196-220 PoolingNodesAttentive.call;
// kgcnn/literature/AttentiveFP.py:102-116): the edge-feature head of the first layer in two launches and the whole
// attentive readout in one.  FP32, no atomics, every sum in an order fixed by the list order and the lane layout: two runs
// give equal bits.
//
// Edge-feature head.  r = receiver (index column 0), s = sender, g_e the D edge features, n the node features (N, F),
// U the units.  The reference gathers n_r and n_s per edge, runs lay_fc1 on n_r, lay_fc2 on [n_s || g_e], the linear
// transform on the result, lay_alpha_activation on [fc1(n_r) || fc2(..)] and lay_alpha on that.  With W2 = lay_fc2.kernel
// (F + D, U), Wa = lay_alpha_activation.kernel (2U, U), a = lay_alpha.kernel (U):
//     hidden_e = act(X[s] + g_e W2[F:] + b2)          X  = n W2[:F]                    (N, U)
//     msg_e    = hidden_e Wl + bl
//     t_e      = act(P[r] + hidden_e Wa[U:] + ba)     P  = act(n W1 + b1) Wa[:U]       (N, U)
//     logit_e  = t_e . a
//     out[r]   = act_context(sum_e softmax_e(logit_e) msg_e)
// X and P are node-side Dense launches on row-block views of the layers' own kernels.
//
// afp_edge_kernel<U> walks tiles of mp_tile::TE = 32 receiver-sorted positions as gat_logits_v2_kernel does (4 waves;
// U = 64: wave w owns columns [16w, 16w + 16) of both 16-row blocks; U = 32: columns [16 (w & 1), +16) of row block
// w >> 1), and keeps its slabs of W2[F:] (D x 16), Wl and Wa[U:] (U x 16 each) in registers for the whole kernel:
//   phase 0  indices and the edge-feature tile (32 x D, zero-padded)                                         -> LDS
//   phase 1  G W2[F:] on v_mfma_f32_16x16x4_f32
//   phase 2  hidden = act(X[s] + product + b2)                                                               -> LDS
//   phase 3  two U x U products of the hidden tile on the matrix pipe: msg = hidden Wl + bl -> msg[position], and
//            t = act(P[r] + hidden Wa[U:] + ba)                                                              -> LDS
//   phase 4  thread e < 32 sums a[c] t[e][c] over c in column order on a float64 accumulator (one rounding: a logit of a
//            few hundred keeps the absolute accuracy its softmax weight needs, as in csrc/mp_gat.hip) -> logit[position]
// Both outputs are written in POSITION order (sorted by receiver): msg (E, U) is the one edge-sized feature tensor of
// the head, and the attend kernel reads a receiver's rows contiguously.  A position whose edge id, receiver or sender is
// out of range (mp_tile::load_pos) gets a zero row and a zero logit, and the attend kernel skips it.
//
// afp_attend_kernel<U>: one wave per receiver over [ptr0[r], ptr0[r + 1]): the three sweeps of mp_attend.h
// (gat_attend_kernel's, restated with the accessors as parameters) with the message row of position p read at msg[p],
// then the context activation.  Every row is written; a receiver without edges gets act_context(0).
//
// afp_readout_kernel: PoolingNodesAttentive.call after wn = n Wl + bl (one Dense launch), the loop over `depth` inside.
// Modelled on gru_ragged_last_kernel (csrc/mp_recurrent.hip): a workgroup of 8 waves owns 16 graphs = the rows of one A
// operand of v_mfma_f32_16x16x4_f32; the states h and the contexts live in LDS (row stride = 4 mod 64 floats).
//   prologue   h_g = sum or mean of the graph's node rows in list order (mp_pool_graph_f32's order);
//              term_i = n_i . w[U:] for every node of the tile's graphs (w = lay_alpha.kernel (2U)): loop-invariant, one
//              float64 per node in a node-sized workspace that only this workgroup writes and reads.
//   iteration  attention, a wave per graph (two graphs per wave): c_g = h_g . w[:U] + b (float64, lanes stride the
//              columns, xor butterfly); a_i = act(c_g + term_i) rounded once; maximum, sum of exponentials (lanes stride
//              the nodes, butterfly) and cont_g = act_context(sum_i softmax_i wn_i): chunks of 64 nodes, lane l holds
//              the weight of node l of the chunk, every lane adds its columns l, l + 64, ... in list order;
//              GRU cell: cont K and h R for the 16 graphs on the matrix pipe, wave w takes the 16-column blocks w and
//              w + 8 with its six accumulators per block, several k steps of loads in flight in front of their MFMAs;
//              the combine is mp_gru_combine_f32's, in its order, on mx = cont K + b_in and mh = h R + b_rec.
//   A graph without nodes has cont = act_context(0) in every iteration, as the layer sequence has.
#include "mp_attend.h"
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/attentivefp.h"

#include <type_traits>

namespace {

constexpr int TE = mp_tile::TE;
constexpr int MAXD = 64;      // widest edge feature
constexpr int KS = MAXD / 4;  // MFMA steps at the widest edge feature
constexpr int GS = MAXD + 1;  // row stride of the edge-feature tile

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct EdgeArgs {
  const float* X;        // (N, U) by the sender
  const float* P;        // (N, U) by the receiver
  const float* g;        // (E, D) edge features
  const float* W2e;      // (D, U)
  const float* b2;       // (U) nullable
  const float* Wl;       // (U, U)
  const float* bl;       // (U) nullable
  const float* Wae;      // (U, U)
  const float* ba;       // (U) nullable
  const float* a;        // (U)
  const int32_t* col0;   // (2, E) receivers | senders
  const int32_t* perm0;  // (E) sorted position -> edge, nullable
  float* logit;          // (E) in position order
  float* msg;            // (E, U) in position order
  int N, E, D;           // N, E below 2^31 (checked on the host)
  int act;
  float alpha;
};

template <int U>
__global__ __launch_bounds__(256) void afp_edge_kernel(EdgeArgs a) {
  constexpr int HS = U + 2;            // row stride of the hidden and t tiles: the 32 lanes of an A read hit 32 banks
  constexpr int RB = U == 64 ? 2 : 1;  // 16-row blocks per wave
  constexpr int KU = U / 4;            // MFMA steps of a U x U product
  __shared__ float gL[TE * GS];
  __shared__ float hL[TE * HS];
  __shared__ float tL[TE * HS];
  __shared__ int recvL[TE], sndL[TE], eidL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int D = a.D;
  const int col = (U == 64 ? 16 * wave : 16 * (wave & 1)) + (lane & 15), kq = lane >> 4;
  const int rb0 = U == 64 ? 0 : (wave >> 1);

  // B operands of step s: rows 4s + (lane >> 4), the wave's 16 columns; rows of W2e past D are zero
  float wc[KS], wl[KU], wa[KU];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + kq;
    wc[s] = k < D ? a.W2e[(size_t)k * U + col] : 0.0f;
  }
#pragma unroll
  for (int s = 0; s < KU; ++s) {
    const int k = 4 * s + kq;
    wl[s] = a.Wl[(size_t)k * U + col];
    wa[s] = a.Wae[(size_t)k * U + col];
  }
  const float b2 = a.b2 ? a.b2[col] : 0.0f, bl = a.bl ? a.bl[col] : 0.0f, ba = a.ba ? a.ba[col] : 0.0f;

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's phase 4 is done with the tiles in LDS
    // phase 0
    if (t < TE) {
      const mp_tile::Pos p = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p0, t, nv);
      recvL[t] = p.r; sndL[t] = p.s; eidL[t] = p.e;
    }
    __syncthreads();
    for (int i = t; i < TE * MAXD; i += 256) {
      const int e = i >> 6, k = i & (MAXD - 1);
      gL[e * GS + k] = (k < D && recvL[e] >= 0) ? a.g[(size_t)eidL[e] * D + k] : 0.0f;
    }
    __syncthreads();
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
        float hid = 0.0f;
        if (recvL[e] >= 0) hid = mp_apply_act(a.act, a.alpha, (a.X[(size_t)sndL[e] * U + col] + acc[rb][i]) + b2);
        hL[e * HS + col] = hid;
      }
    }
    __syncthreads();
    // phase 3
    f32x4 accm[RB], acct[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int i = 0; i < 4; ++i) { accm[rb][i] = 0.0f; acct[rb][i] = 0.0f; }
    {
      const float* ap = hL + (16 * rb0 + (lane & 15)) * HS + kq;
#pragma unroll
      for (int s = 0; s < KU; ++s) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const float av = ap[16 * rb * HS + 4 * s];
          accm[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wl[s], accm[rb], 0, 0, 0);
          acct[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wa[s], acct[rb], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = 16 * (rb0 + rb) + 4 * kq + i;
        const int r = recvL[e];
        float m = 0.0f, tv = 0.0f;
        if (r >= 0) {
          m = accm[rb][i] + bl;
          tv = mp_apply_act(a.act, a.alpha, (a.P[(size_t)r * U + col] + acct[rb][i]) + ba);
        }
        tL[e * HS + col] = tv;
        if (e < nv) a.msg[(size_t)(p0 + e) * U + col] = m;
      }
    }
    __syncthreads();
    // phase 4
    if (t < nv) {
      double sum = 0.0;
      for (int c = 0; c < U; ++c) sum += (double)tL[t * HS + c] * (double)a.a[c];
      a.logit[p0 + t] = recvL[t] >= 0 ? static_cast<float>(sum) : 0.0f;
    }
  }
}

struct AttendArgs {
  const float* msg;      // (E, U) by position
  const float* logit;    // (E) by position
  const int32_t* col0;   // (2, E)
  const int32_t* ptr0;   // (N + 1)
  const int32_t* perm0;  // nullable
  float* out;            // (N, U)
  int N, E;
  int act;
  float alpha;
};

template <int U>
__global__ __launch_bounds__(256) void afp_attend_kernel(AttendArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave0; r < a.N; r += nwaves) {
    int lo = a.ptr0[r], hi = a.ptr0[r + 1];
    lo = lo < 0 ? 0 : (lo > a.E ? a.E : lo);
    hi = hi < lo ? lo : (hi > a.E ? a.E : hi);
    const float acc = mp_attend::wave_rows<U>(
        lo, hi, lane,
        [&](int p, float* logit, int* key) {
          if (mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p, 0, 1).r < 0) return false;   // the edge kernel's skip rule
          *logit = a.logit[p];
          *key = p;
          return true;
        },
        [&](int p, int c) { return a.msg[(size_t)p * U + c]; });
    if (lane < U) a.out[(size_t)r * U + lane] = mp_apply_act(a.act, a.alpha, acc);
  }
}

// ---------------------------------------------------------------------------------------------------------- readout
constexpr int RO_ROWS = 16;
constexpr int RO_THREADS = 512;
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_MAX_UNITS = MP_AFP_READOUT_MAX_UNITS;
constexpr int RO_MAX_STRIDE = ((RO_MAX_UNITS + 63) / 64) * 64 + 4;
constexpr int RO_MAX_BLOCKS = (RO_MAX_UNITS / 16 + RO_WAVES - 1) / RO_WAVES;   // column blocks of one wave
constexpr int RO_CPL = RO_MAX_UNITS / 64;                                      // columns of one lane in the weighted sum
constexpr int RO_ITEMS = RO_ROWS * RO_MAX_UNITS / RO_THREADS;                  // (graph, column) sums of one thread
constexpr int RO_LOADS = 6;   // k steps x blocks whose six slab loads are in flight together (36 loads)
static_assert(RO_MAX_BLOCKS == 2, "the cell below is instantiated for one or two blocks per wave");

struct ReadoutArgs {
  const float* n;          // (n_nodes, U)
  const float* wn;         // (n_nodes, U) = n Wl + bl
  const int64_t* splits;   // (G + 1)
  const float* w;          // (2U) lay_alpha.kernel
  const float* b;          // (1) nullable
  const float* K;          // (U, 3U)
  const float* R;          // (U, 3U)
  const float* b_in;       // (3U) nullable
  const float* b_rec;      // (3U) nullable
  double* term;            // (n_nodes) workspace
  float* out;              // (G, U)
  int64_t n_nodes, G;
  int U, depth, pool_op, act, act_ctx, gru_act, rec_act;
  float alpha;
};

__global__ __launch_bounds__(RO_THREADS) void afp_readout_kernel(ReadoutArgs a) {
  __shared__ float hL[RO_ROWS * RO_MAX_STRIDE];
  __shared__ float cL[RO_ROWS * RO_MAX_STRIDE];
  __shared__ long long startL[RO_ROWS];
  __shared__ int lenL[RO_ROWS];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lc = lane & 15, kq = lane >> 4;
  const int U = a.U, U3 = 3 * U;
  const int S = ((U + 63) / 64) * 64 + 4;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * RO_ROWS;

  if (t < RO_ROWS) {
    const int64_t g = g0 + t;
    int64_t lo = 0, hi = 0;
    if (g < a.G) {
      lo = a.splits[g];
      hi = a.splits[g + 1];
      lo = lo < 0 ? 0 : (lo > a.n_nodes ? a.n_nodes : lo);
      hi = hi < lo ? lo : (hi > a.n_nodes ? a.n_nodes : hi);
    }
    startL[t] = lo;
    const int64_t len = hi - lo;
    lenL[t] = len > 0x7fffffff ? 0x7fffffff : static_cast<int>(len);
  }
  __syncthreads();

  // prologue: the pooled start states, every (graph, column) sum in list order.  A thread owns up to RO_ITEMS of them
  // and walks their node rows together, four rows per round: the loads of a round (up to 4 RO_ITEMS) are independent and
  // in flight at once - one sum at a time is one round trip per node row.
  {
    float acc[RO_ITEMS];
    const float* src[RO_ITEMS];
    int ln[RO_ITEMS];
    int longest = 0;
#pragma unroll
    for (int q = 0; q < RO_ITEMS; ++q) {
      const int i = t + q * RO_THREADS;
      const bool ok = i < RO_ROWS * U;
      const int row = ok ? i / U : 0, col = ok ? i - row * U : 0;
      ln[q] = ok ? lenL[row] : 0;
      src[q] = a.n + static_cast<size_t>(startL[row]) * U + col;
      acc[q] = 0.0f;
      longest = ln[q] > longest ? ln[q] : longest;
    }
    for (int k = 0; k < longest; k += 4) {
      float v[RO_ITEMS][4];
#pragma unroll
      for (int q = 0; q < RO_ITEMS; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[q][j] = k + j < ln[q] ? src[q][static_cast<size_t>(k + j) * U] : 0.0f;
#pragma unroll
      for (int q = 0; q < RO_ITEMS; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < ln[q]) acc[q] += v[q][j];
    }
#pragma unroll
    for (int q = 0; q < RO_ITEMS; ++q) {
      const int i = t + q * RO_THREADS;
      if (i < RO_ROWS * U) {
        const int row = i / U, col = i - row * U;
        if (a.pool_op == MP_MEAN && ln[q] > 0) acc[q] = acc[q] / static_cast<float>(ln[q]);
        hL[row * S + col] = acc[q];
      }
    }
  }
  // prologue: the loop-invariant node term of the logit over the tile's node rows (consecutive graphs: one range), four
  // lanes per node - lane s of a node adds its columns s, s + 4, ... in order, then two xor steps
  if (a.depth > 0) {
    long long lo = 0x7fffffffffffffffLL, hi = 0;
#pragma unroll
    for (int row = 0; row < RO_ROWS; ++row) {
      if (lenL[row] > 0) {
        lo = startL[row] < lo ? startL[row] : lo;
        hi = startL[row] + lenL[row] > hi ? startL[row] + lenL[row] : hi;
      }
    }
    const int sub = t & 3;
    if (hi <= lo) lo = hi = 0;   // no graph of the tile has nodes
    for (long long i = lo + (t >> 2); i < hi; i += RO_THREADS / 4) {   // the four lanes of a node run together
      const float* x = a.n + static_cast<size_t>(i) * U;
      double part = 0.0;
      for (int c = sub; c < U; c += 4) part += (double)x[c] * (double)a.w[U + c];
      part += __shfl_xor(part, 1, 64);
      part += __shfl_xor(part, 2, 64);
      if (sub == 0) a.term[i] = part;
    }
  }
  __syncthreads();

  const int blocks = (U + 15) / 16;
  const int my_blocks = wave < blocks ? (blocks - wave + RO_WAVES - 1) / RO_WAVES : 0;   // wave-uniform
  const int ksteps = U / 4;
  float hnew[RO_MAX_BLOCKS][4];

  // the GRU cell for a wave with NB column blocks: its blocks of `cont K` and `h R` and the combine, in registers (the
  // tiles in LDS are only read)
  auto cell = [&](auto nb_tag) {
    constexpr int NB = decltype(nb_tag)::value;
    constexpr int KG = RO_LOADS / NB;
    int colc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int col = 16 * (wave + j * RO_WAVES) + lc;
      colc[j] = col < U ? col : U - 1;   // the last block may be partial: work on a column inside, drop the result
    }
    f32x4 ax[NB][3], ay[NB][3];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) { ax[j][q][i] = 0.0f; ay[j][q][i] = 0.0f; }
    const float* apc = cL + lc * S + kq;
    const float* aph = hL + lc * S + kq;
    const float* bk = a.K + kq * U3;   // offsets into K and R stay below 3 u^2 < 2^18
    const float* br = a.R + kq * U3;
    int s = 0;
    for (; s + KG <= ksteps; s += KG) {
      float ac[KG], ah[KG], wk[NB][KG][3], wr[NB][KG][3];
#pragma unroll
      for (int q = 0; q < KG; ++q) {
        ac[q] = apc[4 * (s + q)];
        ah[q] = aph[4 * (s + q)];
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int gate = 0; gate < 3; ++gate) {
            wk[j][q][gate] = bk[4 * (s + q) * U3 + gate * U + colc[j]];
            wr[j][q][gate] = br[4 * (s + q) * U3 + gate * U + colc[j]];
          }
      }
#pragma unroll
      for (int q = 0; q < KG; ++q)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int gate = 0; gate < 3; ++gate) {
            ax[j][gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[q], wk[j][q][gate], ax[j][gate], 0, 0, 0);
            ay[j][gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[q], wr[j][q][gate], ay[j][gate], 0, 0, 0);
          }
    }
    for (; s < ksteps; ++s) {
      const float ac = apc[4 * s], ah = aph[4 * s];
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int gate = 0; gate < 3; ++gate) {
          ax[j][gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac, bk[4 * s * U3 + gate * U + colc[j]], ax[j][gate], 0, 0, 0);
          ay[j][gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah, br[4 * s * U3 + gate * U + colc[j]], ay[j][gate], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float bi[3], bh[3];
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) {
        bi[gate] = a.b_in ? a.b_in[gate * U + colc[j]] : 0.0f;
        bh[gate] = a.b_rec ? a.b_rec[gate * U + colc[j]] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hold = hL[(4 * kq + i) * S + colc[j]];
        const float zg = mp_apply_act(a.rec_act, 0.0f, (ax[j][0][i] + bi[0]) + (ay[j][0][i] + bh[0]));
        const float rg = mp_apply_act(a.rec_act, 0.0f, (ax[j][1][i] + bi[1]) + (ay[j][1][i] + bh[1]));
        const float hh = mp_apply_act(a.gru_act, 0.0f, (ax[j][2][i] + bi[2]) + rg * (ay[j][2][i] + bh[2]));
        hnew[j][i] = zg * hold + (1.0f - zg) * hh;
      }
    }
  };

  for (int it = 0; it < a.depth; ++it) {
    // attention: a wave per graph
    for (int row = wave; row < RO_ROWS; row += RO_WAVES) {
      const int len = lenL[row];
      const size_t start = static_cast<size_t>(startL[row]);
      double part = 0.0;
      for (int c = lane; c < U; c += 64) part += (double)hL[row * S + c] * (double)a.w[c];
      const double cg = mp_wave_sum(part) + (a.b ? (double)a.b[0] : 0.0);
      const double* term = a.term + start;
      const auto logit = [&](int k) { return mp_apply_act(a.act, a.alpha, static_cast<float>(cg + term[k])); };
      float mx = -INFINITY;
      for (int k = lane; k < len; k += 64) mx = fmaxf(mx, logit(k));
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      float ex = 0.0f;
      for (int k = lane; k < len; k += 64) ex += expf(logit(k) - mx);
      const float sum = mp_wave_sum(ex);
      float acc[RO_CPL];
#pragma unroll
      for (int q = 0; q < RO_CPL; ++q) acc[q] = 0.0f;
      for (int c0 = 0; c0 < len; c0 += 64) {   // wave-uniform bounds
        const float wv = c0 + lane < len ? expf(logit(c0 + lane) - mx) / sum : 0.0f;
        const int cnt = len - c0 < 64 ? len - c0 : 64;
        const float* base = a.wn + (start + c0) * U;
        for (int j0 = 0; j0 < cnt; j0 += 4) {   // four rows per round, their loads in flight together; j0 + 3 <= 63
          float wj[4], v[4][RO_CPL];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            wj[jj] = __shfl(wv, j0 + jj, 64);
#pragma unroll
            for (int q = 0; q < RO_CPL; ++q) {
              const int col = lane + 64 * q;
              v[jj][q] = (j0 + jj < cnt && col < U) ? base[static_cast<size_t>(j0 + jj) * U + col] : 0.0f;
            }
          }
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int q = 0; q < RO_CPL; ++q)
              if (j0 + jj < cnt && lane + 64 * q < U) acc[q] += wj[jj] * v[jj][q];
        }
      }
#pragma unroll
      for (int q = 0; q < RO_CPL; ++q) {
        const int col = lane + 64 * q;
        if (col < U) cL[row * S + col] = mp_apply_act(a.act_ctx, a.alpha, acc[q]);
      }
    }
    __syncthreads();
    if (my_blocks == 2) cell(std::integral_constant<int, 2>());
    else if (my_blocks == 1) cell(std::integral_constant<int, 1>());
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RO_MAX_BLOCKS; ++j) {
      const int col = 16 * (wave + j * RO_WAVES) + lc;
      if (j < my_blocks && col < U) {
#pragma unroll
        for (int i = 0; i < 4; ++i) hL[(4 * kq + i) * S + col] = hnew[j][i];
      }
    }
    __syncthreads();
  }
  for (int i = t; i < RO_ROWS * U; i += RO_THREADS) {
    const int row = i / U, col = i - row * U;
    if (g0 + row < a.G) a.out[static_cast<size_t>(g0 + row) * U + col] = hL[row * S + col];
  }
}

bool act_ok(int act) { return act >= MP_ACT_LINEAR && act <= MP_ACT_LAST; }

}  // namespace

extern "C" {

int mp_afp_edge_f32(int U, const float* X, const float* P, int64_t N, const float* edges, int D, const float* W2e,
                    const float* b2, const float* Wl, const float* bl, const float* Wae, const float* ba, const float* a,
                    const int32_t* cols, int64_t E, const int32_t* perm0, int act, float alpha, float* logit, float* msg,
                    mpStream_t stream) {
  const char* what = "mp_afp_edge_f32";
  MP_REQUIRE(U == 32 || U == 64, "%s: units must be 32 or 64, got %d", what, U);
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(D >= 1 && D <= MAXD, "%s: takes 1 to %d edge features, got %d", what, MAXD, D);
  MP_REQUIRE(act_ok(act), "%s: unknown activation code", what);
  if (E == 0) return MP_OK;
  MP_REQUIRE(X && P && edges && W2e && Wl && Wae && a && cols && logit && msg, "%s: null pointer", what);
  EdgeArgs k{X, P, edges, W2e, b2, Wl, bl, Wae, ba, a, cols, perm0, logit, msg, static_cast<int>(N), static_cast<int>(E), D,
             act, alpha};
  const int64_t tiles = mp_tile::tiles_of(E);
  const unsigned grid = static_cast<unsigned>(tiles < 1024 ? tiles : 1024);
  if (U == 64) afp_edge_kernel<64><<<grid, 256, 0, mp::as_stream(stream)>>>(k);
  else afp_edge_kernel<32><<<grid, 256, 0, mp::as_stream(stream)>>>(k);
  return mp::check_launch(what);
}

int mp_afp_attend_f32(int U, const float* msg, const float* logit, int64_t N, const int32_t* cols, int64_t E,
                      const int32_t* ptr0, const int32_t* perm0, int act_context, float alpha, float* out,
                      mpStream_t stream) {
  const char* what = "mp_afp_attend_f32";
  MP_REQUIRE(U == 32 || U == 64, "%s: units must be 32 or 64, got %d", what, U);
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(act_ok(act_context), "%s: unknown activation code", what);
  if (N == 0) return MP_OK;
  MP_REQUIRE(ptr0 && out, "%s: null pointer", what);
  MP_REQUIRE(E == 0 || (msg && logit && cols), "%s: null pointer", what);
  AttendArgs k{msg, logit, cols, ptr0, perm0, out, static_cast<int>(N), static_cast<int>(E), act_context, alpha};
  const unsigned grid = mp::grid_for(N * 64);
  if (U == 64) afp_attend_kernel<64><<<grid, 256, 0, mp::as_stream(stream)>>>(k);
  else afp_attend_kernel<32><<<grid, 256, 0, mp::as_stream(stream)>>>(k);
  return mp::check_launch(what);
}

int mp_afp_readout_f32(const float* n, const float* wn, int64_t n_nodes, const int64_t* row_splits, int64_t G, int U,
                       int depth, int pool_op, const float* w, const float* b, const float* K, const float* R,
                       const float* b_in, const float* b_rec, int act, float alpha, int act_context, int gru_act,
                       int rec_act, double* node_term, float* out, mpStream_t stream) {
  const char* what = "mp_afp_readout_f32";
  MP_REQUIRE(n_nodes >= 0 && G >= 0 && depth >= 0, "%s: bad sizes", what);
  MP_REQUIRE(U >= 4 && U % 4 == 0 && U <= RO_MAX_UNITS, "%s: units must be a multiple of 4, at most %d, got %d", what,
             RO_MAX_UNITS, U);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: the start state is pooled by sum or mean", what);
  MP_REQUIRE(act_ok(act) && act_ok(act_context) && act_ok(gru_act) && act_ok(rec_act), "%s: unknown activation", what);
  if (G == 0) return MP_OK;
  MP_REQUIRE(row_splits && out && (n_nodes == 0 || n), "%s: null pointer", what);
  MP_REQUIRE(depth == 0 || (w && K && R && (n_nodes == 0 || (wn && node_term))), "%s: null pointer", what);
  const int64_t grid = mp::ceil_div(G, RO_ROWS);
  MP_REQUIRE(grid < (int64_t{1} << 31), "%s: grid too large", what);
  ReadoutArgs k{n, wn, row_splits, w, b, K, R, b_in, b_rec, node_term, out, n_nodes, G, U, depth, pool_op, act,
                act_context, gru_act, rec_act, alpha};
  afp_readout_kernel<<<static_cast<unsigned>(grid), RO_THREADS, 0, mp::as_stream(stream)>>>(k);
  return mp::check_launch(what);
}

}  // extern "C"
