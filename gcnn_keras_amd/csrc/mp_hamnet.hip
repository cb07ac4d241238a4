// HamNet (kgcnn/layers/conv/hamnet_conv.py:508-528 HamNaiveDynMessage.call, :194-207 HamNetGlobalReadoutAttend.call,
// :358-368 HamNetFingerprintGenerator.call; kgcnn/literature/HamNet.py:134-156): the dynamic message step in two launches
// behind its node-side Dense launches, and the whole fingerprint generator in one.  FP32, no atomics, every sum in an order
// fixed by the list order and the lane layout: two runs give equal bits.  Vector code throughout: the per-edge products
// have K = 2C <= 16 rows, the step is bandwidth work.
//
// Message step.  u = receiver (index column 0, the column the attention pools on), v = sender, h (N, F) node rows,
// he (E, D) edge rows, p, q (N, C) momenta and coordinates, d_e = [p_v - p_u || q_v - q_u] (2C), formed per edge from the
// gathered rows (never as a difference of node-side dot products, which cancels away from the origin).  The reference
// gathers h_u, h_v, p and q per edge, concatenates [p_uv || q_uv || he] for dense_align and [h_u || p_uv || q_uv || h_v]
// for dense_e, runs dense_attend on the gathered h_v and pools by the segment softmax.  With w = dense_align.kernel
// (2C + D), W_e = dense_e.kernel (F + 2C + F, UE):
//     logit_e = w[:2C] . d_e + w[2C:] . he_e + b                       float64 accumulator, one rounding
//     mv[u]   = act_last(sum_e softmax_e(logit_e) T[v])                 T = act(h W_att + b_att)        (N, U)
//     me_e    = act(A[u] + d_e W_e[F:F+2C] + B[v] + b_e)                A = h W_e[:F], B = h W_e[F+2C:] (N, UE)
// T, A and B are node-side Dense launches (dense_attend acts on a gathered node row only, so it commutes with the gather)
// on row-block views of the layers' own kernels.
//
// hamnet_edge_kernel walks tiles of mp_tile::TE = 32 receiver-sorted positions (position p is edge perm0[p]), 256 threads:
//   phase 0  thread e < 32: receiver, sender, edge id (mp_tile::load_pos) and the difference row d_e            -> LDS
//   phase 1  eight lanes per position: lane s adds the float4 chunks s, s + 8, ... of he_e . w[2C:] in order on a float64
//            accumulator (products of two floats are exact there), three xor steps add the eight partials, lane 0 adds the
//            2C terms of d_e in column order and the bias, rounds once                                           -> logit[p]
//   phase 2  (me requested) a thread per (position, float4 of columns): A[u] and B[v] rows by 16-byte loads, d_e W_d from
//            the copy of W_d in LDS, 16-byte store                                                              -> me[e]
// logit (E) is written in POSITION order (the receiver pass reads a receiver's logits contiguously), me (E, UE) in EDGE
// order (it is the layer's output).  Sorted positions make consecutive rows of a tile read the same A[u] row.  A position
// whose edge id, receiver or sender is out of range gets a zero logit (and a zero me row where its edge id is valid), and
// the receiver pass skips it.  logit and me are the only edge-sized tensors written.
//
// hamnet_attend_kernel: one wave per receiver over [ptr0[r], ptr0[r + 1]): the three sweeps of mp_attend.h for a run-time
// width U <= 256 with the message row of position p gathered at T[v]: a row is Q = U / 4 float4 columns, LQ = the power of
// two above Q, the 64 lanes are 64 / LQ position groups x LQ float4 columns; group k adds positions k, k + 64 / LQ, ... of
// every chunk of 64 in list order, an xor butterfly adds the groups.  Every row is written; a receiver without edges gets
// act_last(0).
//
// hamnet_fingerprint_kernel: HamNetFingerprintGenerator.call behind M = act(h W_v2m + b) and T_i = act(h W_att,i + b_i)
// (1 + depth Dense launches), the loop over `depth` inside.  A workgroup of 8 waves owns 16 graphs, their states s (16, U)
// and messages m (16, UA) in LDS, as afp_readout_kernel does (csrc/mp_attentivefp.hip):
//   prologue   s_g = sum or mean of the graph's rows of M in list order.
//   iteration  term_n = h_n . w_i[U:] for the tile's nodes (w_i = dense_align.kernel of readout i, (U + F): the state
//              comes first in the reference's concatenation), four lanes per node on float64, into a node-sized workspace
//              that only this workgroup writes and reads;
//              attention, a wave per graph: c_g = s_g . w_i[:U] + b_i (float64), a_n = float(c_g + term_n); maximum, sum
//              of exponentials, m_g = elu(sum_n softmax_n(a_n) T_i[n]): chunks of 64 nodes, lane l holds the weight of
//              node l of the chunk, every lane adds its columns l, l + 64, ... in list order;
//              GRU cell i on vector code: a thread owns one column of the three gates for four graphs and adds m K_i and
//              s R_i over k in order; the combine is mp_gru_combine_f32's, in its order, then the layer's activation.
//   A graph without nodes starts from s = 0 and has m = act_attend(0) in every iteration, as the layer sequence has.
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/hamnet.h"

namespace {

constexpr int TE = mp_tile::TE;
constexpr int MAXC = MP_HAMNET_MAX_COORDS;   // widest coordinate row
constexpr int MAXW = MP_HAMNET_MAX_WIDTH;    // widest feature row (every width is a multiple of 4)
constexpr int DS = 2 * MAXC + 1; // row stride of the difference tile

bool act_ok(int act) { return act >= MP_ACT_LINEAR && act <= MP_ACT_LAST; }
bool width_ok(int64_t w) { return w >= 4 && w <= MAXW && w % 4 == 0; }

struct EdgeArgs {
  const float* A;        // (N, UE) by the receiver, null without me
  const float* B;        // (N, UE) by the sender, null without me
  const float* p;        // (N, C)
  const float* q;        // (N, C)
  const float* he;       // (E, D)
  const float* w;        // (2C + D) dense_align.kernel
  const float* b;        // (1) nullable
  const float* Wd;       // (2C, UE) rows F .. F + 2C of dense_e.kernel, null without me
  const float* be;       // (UE) nullable
  const int32_t* col0;   // (2, E) receivers | senders
  const int32_t* perm0;  // (E) sorted position -> edge, nullable
  float* logit;          // (E) in position order
  float* me;             // (E, UE) in edge order, nullable
  int N, E, C, D, UE;    // N, E below 2^31 (checked on the host)
  int act;
  float alpha;
};

__global__ __launch_bounds__(256) void hamnet_edge_kernel(EdgeArgs a) {
  __shared__ float dL[TE * DS];
  __shared__ float wdL[2 * MAXC * MAXW];
  __shared__ int recvL[TE], sndL[TE], eidL[TE];

  const int t = threadIdx.x;
  const int C = a.C, C2 = 2 * a.C, D = a.D, UE = a.UE;
  if (a.me) {
    for (int i = t; i < C2 * UE; i += 256) wdL[i] = a.Wd[i];
  }
  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's phase 2 is done with the tiles in LDS (and wdL is filled)
    // phase 0
    if (t < TE) {
      const mp_tile::Pos pos = mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p0, t, nv);
      recvL[t] = pos.r; sndL[t] = pos.s; eidL[t] = pos.e;
      if (pos.r >= 0) {
        const float* pu = a.p + (size_t)pos.r * C;
        const float* pv = a.p + (size_t)pos.s * C;
        const float* qu = a.q + (size_t)pos.r * C;
        const float* qv = a.q + (size_t)pos.s * C;
        for (int k = 0; k < C; ++k) {
          dL[t * DS + k] = pv[k] - pu[k];
          dL[t * DS + C + k] = qv[k] - qu[k];
        }
      } else {
        for (int k = 0; k < C2; ++k) dL[t * DS + k] = 0.0f;
      }
    }
    __syncthreads();
    // phase 1: position t >> 3, lane t & 7 of its eight (the eight lanes of a position sit in one wave)
    {
      const int e = t >> 3, sub = t & 7;
      const bool live = e < nv && recvL[e] >= 0;
      double part = 0.0;
      if (live) {
        const float4* row = reinterpret_cast<const float4*>(a.he + (size_t)eidL[e] * D);
        const float* ws = a.w + C2;   // 2C floats into the kernel: 16-byte aligned for even C only
        const float4* wr = reinterpret_cast<const float4*>(ws);
        const bool wvec = (reinterpret_cast<uintptr_t>(ws) & 15) == 0;
        for (int c4 = sub; c4 < D / 4; c4 += 8) {
          const float4 x = row[c4];
          float4 y;
          if (wvec) y = wr[c4];
          else y = make_float4(ws[4 * c4], ws[4 * c4 + 1], ws[4 * c4 + 2], ws[4 * c4 + 3]);
          part += (double)x.x * (double)y.x;
          part += (double)x.y * (double)y.y;
          part += (double)x.z * (double)y.z;
          part += (double)x.w * (double)y.w;
        }
      }
      part += __shfl_xor(part, 1, 64);
      part += __shfl_xor(part, 2, 64);
      part += __shfl_xor(part, 4, 64);
      if (sub == 0 && e < nv) {
        float out = 0.0f;
        if (live) {
          double sum = 0.0;
          for (int k = 0; k < C2; ++k) sum += (double)dL[e * DS + k] * (double)a.w[k];
          sum += part;
          if (a.b) sum += (double)a.b[0];
          out = static_cast<float>(sum);
        }
        a.logit[p0 + e] = out;
      }
    }
    // phase 2
    if (a.me) {
      const int q4 = UE / 4;
      for (int i = t; i < nv * q4; i += 256) {
        const int e = i / q4, c = 4 * (i - e * q4);
        const int r = recvL[e];
        if (r < 0) {
          // an edge id inside [0, E) whose receiver or sender is out of range: a zero row; an edge id outside has no row
          const int32_t raw = a.perm0 ? a.perm0[p0 + e] : p0 + e;
          if (raw >= 0 && raw < a.E) *reinterpret_cast<float4*>(a.me + (size_t)raw * UE + c) = make_float4(0.f, 0.f, 0.f, 0.f);
          continue;
        }
        const float4 av = *reinterpret_cast<const float4*>(a.A + (size_t)r * UE + c);
        const float4 bv = *reinterpret_cast<const float4*>(a.B + (size_t)sndL[e] * UE + c);
        float dw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < C2; ++k) {
          const float dk = dL[e * DS + k];
          const float4 wk = *reinterpret_cast<const float4*>(wdL + k * UE + c);
          dw[0] += dk * wk.x; dw[1] += dk * wk.y; dw[2] += dk * wk.z; dw[3] += dk * wk.w;
        }
        float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.be) bias = *reinterpret_cast<const float4*>(a.be + c);
        float4 o;
        o.x = mp_apply_act(a.act, a.alpha, ((av.x + dw[0]) + bv.x) + bias.x);
        o.y = mp_apply_act(a.act, a.alpha, ((av.y + dw[1]) + bv.y) + bias.y);
        o.z = mp_apply_act(a.act, a.alpha, ((av.z + dw[2]) + bv.z) + bias.z);
        o.w = mp_apply_act(a.act, a.alpha, ((av.w + dw[3]) + bv.w) + bias.w);
        *reinterpret_cast<float4*>(a.me + (size_t)eidL[e] * UE + c) = o;
      }
    }
  }
}

struct AttendArgs {
  const float* T;        // (N, U) by the sender
  const float* logit;    // (E) by position
  const int32_t* col0;   // (2, E)
  const int32_t* ptr0;   // (N + 1)
  const int32_t* perm0;  // nullable
  float* out;            // (N, U)
  int N, E, U;
  int act;
  float alpha;
};

__global__ __launch_bounds__(256) void hamnet_attend_kernel(AttendArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int U = a.U, Q = U / 4;
  int LQ = 1;
  while (LQ < Q) LQ <<= 1;       // 1 .. 64
  const int G = 64 / LQ;         // position groups of the wave in sweep 3
  const int c4 = lane & (LQ - 1), grp = lane / LQ;
  const bool owns = c4 < Q;
  for (int64_t r = wave0; r < a.N; r += nwaves) {
    int lo = a.ptr0[r], hi = a.ptr0[r + 1];
    lo = lo < 0 ? 0 : (lo > a.E ? a.E : lo);
    hi = hi < lo ? lo : (hi > a.E ? a.E : hi);
    // sender of position p, -1 for a position the edge kernel skipped
    const auto sender = [&](int p) { return mp_tile::load_pos(a.col0, a.perm0, a.N, a.E, p, 0, 1); };
    // sweep 1
    float mx = -INFINITY;
    for (int p = lo + lane; p < hi; p += 64)
      if (sender(p).r >= 0) mx = fmaxf(mx, a.logit[p]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    // sweep 2
    float part = 0.0f;
    for (int p = lo + lane; p < hi; p += 64)
      if (sender(p).r >= 0) part += expf(a.logit[p] - mx);
    const float sum = mp_wave_sum(part);
    // sweep 3
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c0 = lo; c0 < hi; c0 += 64) {   // wave-uniform bounds
      int key = 0;
      float w = 0.0f;
      if (c0 + lane < hi) {
        const mp_tile::Pos pos = sender(c0 + lane);
        if (pos.r >= 0) {
          w = expf(a.logit[c0 + lane] - mx) / sum;
          key = pos.s;
        }
      }
      const int n = hi - c0 < 64 ? hi - c0 : 64;
      for (int j = 0; j < n; j += G) {
        const int src = j + grp;             // at most 63; positions past n hold w = 0, key = 0
        const float wj = __shfl(w, src, 64);
        const int kj = __shfl(key, src, 64);
        if (wj != 0.0f && owns) {
          const float4 row = *reinterpret_cast<const float4*>(a.T + (size_t)kj * U + 4 * c4);
          acc.x += wj * row.x; acc.y += wj * row.y; acc.z += wj * row.z; acc.w += wj * row.w;
        }
      }
    }
    for (int off = 32; off >= LQ; off >>= 1) {   // the groups, in a fixed order
      acc.x += __shfl_xor(acc.x, off, 64);
      acc.y += __shfl_xor(acc.y, off, 64);
      acc.z += __shfl_xor(acc.z, off, 64);
      acc.w += __shfl_xor(acc.w, off, 64);
    }
    if (grp == 0 && owns) {
      float4 o;
      o.x = mp_apply_act(a.act, a.alpha, acc.x);
      o.y = mp_apply_act(a.act, a.alpha, acc.y);
      o.z = mp_apply_act(a.act, a.alpha, acc.z);
      o.w = mp_apply_act(a.act, a.alpha, acc.w);
      *reinterpret_cast<float4*>(a.out + (size_t)r * U + 4 * c4) = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ fingerprint
constexpr int FP_ROWS = 16;
constexpr int FP_THREADS = 512;
constexpr int FP_WAVES = FP_THREADS / 64;
constexpr int FP_STRIDE = MAXW + 4;
constexpr int FP_CPL = MAXW / 64;                          // columns of one lane in the weighted sum
constexpr int FP_GG = 4;                                   // graphs of one cell thread
constexpr int FP_ITEMS = MAXW * (FP_ROWS / FP_GG) / FP_THREADS;   // (column, graph group) items of one thread
static_assert(FP_ITEMS == 2, "the cell keeps two items per thread in registers");

struct FingerprintArgs {
  const float* h;          // (n_nodes, F)
  const float* M;          // (n_nodes, U) = act(h W_v2m + b)
  const int64_t* splits;   // (G + 1)
  const float* T[MP_HAMNET_MAX_DEPTH];      // (n_nodes, UA) = act(h W_att,i + b_i)
  const float* w[MP_HAMNET_MAX_DEPTH];      // (U + F)
  const float* b[MP_HAMNET_MAX_DEPTH];      // (1) nullable
  const float* K[MP_HAMNET_MAX_DEPTH];      // (UA, 3U)
  const float* R[MP_HAMNET_MAX_DEPTH];      // (U, 3U)
  const float* b_in[MP_HAMNET_MAX_DEPTH];   // (3U) nullable
  const float* b_rec[MP_HAMNET_MAX_DEPTH];  // (3U) nullable
  double* term;            // (n_nodes) workspace
  float* out;              // (G, U)
  int64_t n_nodes, G;
  int F, U, UA, depth, pool_op, act, act_attend, gru_act, rec_act;
  float alpha;
};

__global__ __launch_bounds__(FP_THREADS) void hamnet_fingerprint_kernel(FingerprintArgs a) {
  __shared__ float sL[FP_ROWS * FP_STRIDE];
  __shared__ float mL[FP_ROWS * FP_STRIDE];
  __shared__ long long startL[FP_ROWS];
  __shared__ int lenL[FP_ROWS];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int F = a.F, U = a.U, UA = a.UA, U3 = 3 * a.U;
  constexpr int S = FP_STRIDE;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * FP_ROWS;

  if (t < FP_ROWS) {
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

  // prologue: the pooled start states, every (graph, column) sum in list order (mp_pool_graph_f32's order)
  for (int i = t; i < FP_ROWS * U; i += FP_THREADS) {
    const int row = i / U, col = i - row * U;
    const int len = lenL[row];
    const float* src = a.M + static_cast<size_t>(startL[row]) * U + col;
    float acc = 0.0f;
#pragma unroll 4
    for (int k = 0; k < len; ++k) acc += src[static_cast<size_t>(k) * U];
    if (a.pool_op == MP_MEAN && len > 0) acc = acc / static_cast<float>(len);
    sL[row * S + col] = acc;
  }
  // the tile's node rows: consecutive graphs, one range
  long long nlo = 0x7fffffffffffffffLL, nhi = 0;
#pragma unroll
  for (int row = 0; row < FP_ROWS; ++row) {
    if (lenL[row] > 0) {
      nlo = startL[row] < nlo ? startL[row] : nlo;
      nhi = startL[row] + lenL[row] > nhi ? startL[row] + lenL[row] : nhi;
    }
  }
  if (nhi <= nlo) nlo = nhi = 0;   // no graph of the tile has nodes
  __syncthreads();

  for (int it = 0; it < a.depth; ++it) {
    const float* w = a.w[it];
    const float* T = a.T[it];
    // the node term of the logit, four lanes per node: lane s adds its columns s, s + 4, ... in order, two xor steps
    {
      const int sub = t & 3;
      for (long long i = nlo + (t >> 2); i < nhi; i += FP_THREADS / 4) {   // the four lanes of a node run together
        const float* x = a.h + static_cast<size_t>(i) * F;
        double part = 0.0;
        for (int c = sub; c < F; c += 4) part += (double)x[c] * (double)w[U + c];
        part += __shfl_xor(part, 1, 64);
        part += __shfl_xor(part, 2, 64);
        if (sub == 0) a.term[i] = part;
      }
    }
    __syncthreads();   // term is written and read by this workgroup only
    // attention: a wave per graph
    for (int row = wave; row < FP_ROWS; row += FP_WAVES) {
      const int len = lenL[row];
      const size_t start = static_cast<size_t>(startL[row]);
      double part = 0.0;
      for (int c = lane; c < U; c += 64) part += (double)sL[row * S + c] * (double)w[c];
      const double cg = mp_wave_sum(part) + (a.b[it] ? (double)a.b[it][0] : 0.0);
      const double* term = a.term + start;
      const auto logit = [&](int k) { return static_cast<float>(cg + term[k]); };
      float mx = -INFINITY;
      for (int k = lane; k < len; k += 64) mx = fmaxf(mx, logit(k));
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      float ex = 0.0f;
      for (int k = lane; k < len; k += 64) ex += expf(logit(k) - mx);
      const float sum = mp_wave_sum(ex);
      float acc[FP_CPL];
#pragma unroll
      for (int q = 0; q < FP_CPL; ++q) acc[q] = 0.0f;
      for (int c0 = 0; c0 < len; c0 += 64) {   // wave-uniform bounds
        const float wv = c0 + lane < len ? expf(logit(c0 + lane) - mx) / sum : 0.0f;
        const int cnt = len - c0 < 64 ? len - c0 : 64;
        const float* base = T + (start + c0) * UA;
        for (int j0 = 0; j0 < cnt; j0 += 4) {   // four rows per round, their loads in flight together; j0 + 3 <= 63
          float wj[4], v[4][FP_CPL];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            wj[jj] = __shfl(wv, j0 + jj, 64);
#pragma unroll
            for (int q = 0; q < FP_CPL; ++q) {
              const int col = lane + 64 * q;
              v[jj][q] = (j0 + jj < cnt && col < UA) ? base[static_cast<size_t>(j0 + jj) * UA + col] : 0.0f;
            }
          }
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int q = 0; q < FP_CPL; ++q)
              if (j0 + jj < cnt && lane + 64 * q < UA) acc[q] += wj[jj] * v[jj][q];
        }
      }
#pragma unroll
      for (int q = 0; q < FP_CPL; ++q) {
        const int col = lane + 64 * q;
        if (col < UA) mL[row * S + col] = mp_apply_act(a.act_attend, a.alpha, acc[q]);
      }
    }
    __syncthreads();
    // GRU cell `it`: item = (column, group of four graphs)
    float snew[FP_ITEMS][FP_GG];
    const float* K = a.K[it];
    const float* R = a.R[it];
#pragma unroll
    for (int q = 0; q < FP_ITEMS; ++q) {
      const int i = t + q * FP_THREADS;
      if (i < U * (FP_ROWS / FP_GG)) {   // offsets into K and R stay below 3 * 256^2 < 2^18
        const int gg = i / U, col = i - gg * U;
        float ax[3][FP_GG], ay[3][FP_GG];
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
#pragma unroll
          for (int j = 0; j < FP_GG; ++j) { ax[gate][j] = 0.0f; ay[gate][j] = 0.0f; }
        const float* mrow = mL + (FP_GG * gg) * S;
        const float* srow = sL + (FP_GG * gg) * S;
#pragma unroll 4
        for (int k = 0; k < UA; ++k) {
          const float k0 = K[k * U3 + col], k1 = K[k * U3 + U + col], k2 = K[k * U3 + 2 * U + col];
#pragma unroll
          for (int j = 0; j < FP_GG; ++j) {
            const float mv = mrow[j * S + k];
            ax[0][j] += mv * k0; ax[1][j] += mv * k1; ax[2][j] += mv * k2;
          }
        }
#pragma unroll 4
        for (int k = 0; k < U; ++k) {
          const float r0 = R[k * U3 + col], r1 = R[k * U3 + U + col], r2 = R[k * U3 + 2 * U + col];
#pragma unroll
          for (int j = 0; j < FP_GG; ++j) {
            const float sv = srow[j * S + k];
            ay[0][j] += sv * r0; ay[1][j] += sv * r1; ay[2][j] += sv * r2;
          }
        }
        float bi[3], bh[3];
#pragma unroll
        for (int gate = 0; gate < 3; ++gate) {
          bi[gate] = a.b_in[it] ? a.b_in[it][gate * U + col] : 0.0f;
          bh[gate] = a.b_rec[it] ? a.b_rec[it][gate * U + col] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < FP_GG; ++j) {
          const float hold = srow[j * S + col];
          const float zg = mp_apply_act(a.rec_act, 0.0f, (ax[0][j] + bi[0]) + (ay[0][j] + bh[0]));
          const float rg = mp_apply_act(a.rec_act, 0.0f, (ax[1][j] + bi[1]) + (ay[1][j] + bh[1]));
          const float hh = mp_apply_act(a.gru_act, 0.0f, (ax[2][j] + bi[2]) + rg * (ay[2][j] + bh[2]));
          snew[q][j] = mp_apply_act(a.act, a.alpha, zg * hold + (1.0f - zg) * hh);
        }
      }
    }
    __syncthreads();   // every thread is done reading the old states
#pragma unroll
    for (int q = 0; q < FP_ITEMS; ++q) {
      const int i = t + q * FP_THREADS;
      if (i < U * (FP_ROWS / FP_GG)) {
        const int gg = i / U, col = i - gg * U;
#pragma unroll
        for (int j = 0; j < FP_GG; ++j) sL[(FP_GG * gg + j) * S + col] = snew[q][j];
      }
    }
    __syncthreads();
  }
  for (int i = t; i < FP_ROWS * U; i += FP_THREADS) {
    const int row = i / U, col = i - row * U;
    if (g0 + row < a.G) a.out[static_cast<size_t>(g0 + row) * U + col] = sL[row * S + col];
  }
}

}  // namespace

extern "C" {

int mp_hamnet_edge_f32(const float* A, const float* B, int64_t N, int UE, const float* p, const float* q, int C,
                       const float* he, int D, const float* w_align, const float* b_align, const float* Wd,
                       const float* b_e, const int32_t* cols, int64_t E, const int32_t* perm0, int act, float alpha,
                       float* logit, float* me, mpStream_t stream) {
  const char* what = "mp_hamnet_edge_f32";
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(C >= 1 && C <= MAXC, "%s: takes 1 to %d coordinates, got %d", what, MAXC, C);
  MP_REQUIRE(width_ok(D), "%s: the edge width must be a multiple of 4 up to %d, got %d", what, MAXW, D);
  MP_REQUIRE(width_ok(UE), "%s: units_edge must be a multiple of 4 up to %d, got %d", what, MAXW, UE);
  MP_REQUIRE(act_ok(act), "%s: unknown activation code", what);
  if (E == 0) return MP_OK;
  MP_REQUIRE(p && q && he && w_align && cols && logit, "%s: null pointer", what);
  MP_REQUIRE(!me || (A && B && Wd), "%s: null pointer", what);
  MP_REQUIRE(mp::aligned16(he) && (!me || (mp::aligned16(A) && mp::aligned16(B) && mp::aligned16(Wd) &&
                                           mp::aligned16(me) && mp::aligned16(b_e))),
             "%s: feature rows must be 16-byte aligned", what);
  EdgeArgs k{A, B, p, q, he, w_align, b_align, Wd, b_e, cols, perm0, logit, me, static_cast<int>(N), static_cast<int>(E),
             C, D, UE, act, alpha};
  const int64_t tiles = mp_tile::tiles_of(E);
  const unsigned grid = static_cast<unsigned>(tiles < 2048 ? tiles : 2048);
  hamnet_edge_kernel<<<grid, 256, 0, mp::as_stream(stream)>>>(k);
  return mp::check_launch(what);
}

int mp_hamnet_attend_f32(int U, const float* T, const float* logit, int64_t N, const int32_t* cols, int64_t E,
                         const int32_t* ptr0, const int32_t* perm0, int act_last, float alpha, float* out,
                         mpStream_t stream) {
  const char* what = "mp_hamnet_attend_f32";
  MP_REQUIRE(width_ok(U), "%s: units must be a multiple of 4 up to %d, got %d", what, MAXW, U);
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(act_ok(act_last), "%s: unknown activation code", what);
  if (N == 0) return MP_OK;
  MP_REQUIRE(ptr0 && out, "%s: null pointer", what);
  MP_REQUIRE(E == 0 || (T && logit && cols), "%s: null pointer", what);
  MP_REQUIRE(mp::aligned16(T) && mp::aligned16(out), "%s: feature rows must be 16-byte aligned", what);
  AttendArgs k{T, logit, cols, ptr0, perm0, out, static_cast<int>(N), static_cast<int>(E), U, act_last, alpha};
  hamnet_attend_kernel<<<mp::grid_for(N * 64), 256, 0, mp::as_stream(stream)>>>(k);
  return mp::check_launch(what);
}

int mp_hamnet_fingerprint_f32(const float* h, const float* M, int64_t n_nodes, const int64_t* row_splits, int64_t G,
                              int F, int U, int UA, int depth, int pool_op, const float* const* T_host,
                              const float* const* w_host, const float* const* b_host, const float* const* K_host,
                              const float* const* R_host, const float* const* b_in_host,
                              const float* const* b_rec_host, int act, float alpha, int act_attend, int gru_act,
                              int rec_act, double* node_term, float* out, mpStream_t stream) {
  const char* what = "mp_hamnet_fingerprint_f32";
  MP_REQUIRE(n_nodes >= 0 && G >= 0, "%s: bad sizes", what);
  MP_REQUIRE(depth >= 0 && depth <= MP_HAMNET_MAX_DEPTH, "%s: depth must be 0 to %d, got %d", what, MP_HAMNET_MAX_DEPTH,
             depth);
  MP_REQUIRE(width_ok(F) && width_ok(U) && width_ok(UA),
             "%s: node width, units and units_attend must be multiples of 4 up to %d, got %d, %d, %d", what, MAXW, F, U,
             UA);
  MP_REQUIRE(pool_op == MP_SUM || pool_op == MP_MEAN, "%s: the start state is pooled by sum or mean", what);
  MP_REQUIRE(act_ok(act) && act_ok(act_attend) && act_ok(gru_act) && act_ok(rec_act), "%s: unknown activation", what);
  if (G == 0) return MP_OK;
  MP_REQUIRE(row_splits && out && (n_nodes == 0 || (h && M)), "%s: null pointer", what);
  MP_REQUIRE(depth == 0 || (T_host && w_host && K_host && R_host && (n_nodes == 0 || node_term)), "%s: null pointer",
             what);
  FingerprintArgs k{};
  k.h = h; k.M = M; k.splits = row_splits; k.term = node_term; k.out = out; k.n_nodes = n_nodes; k.G = G;
  k.F = F; k.U = U; k.UA = UA; k.depth = depth; k.pool_op = pool_op; k.act = act; k.act_attend = act_attend;
  k.gru_act = gru_act; k.rec_act = rec_act; k.alpha = alpha;
  for (int i = 0; i < depth; ++i) {
    MP_REQUIRE(w_host[i] && K_host[i] && R_host[i] && (n_nodes == 0 || T_host[i]), "%s: null pointer in iteration %d",
               what, i);
    k.T[i] = T_host[i]; k.w[i] = w_host[i]; k.K[i] = K_host[i]; k.R[i] = R_host[i];
    k.b[i] = b_host ? b_host[i] : nullptr;
    k.b_in[i] = b_in_host ? b_in_host[i] : nullptr;
    k.b_rec[i] = b_rec_host ? b_rec_host[i] : nullptr;
  }
  const int64_t grid = mp::ceil_div(G, FP_ROWS);
  MP_REQUIRE(grid < (int64_t{1} << 31), "%s: grid too large", what);
  hamnet_fingerprint_kernel<<<static_cast<unsigned>(grid), FP_THREADS, 0, mp::as_stream(stream)>>>(k);
  return mp::check_launch(what);
}

}  // extern "C"
