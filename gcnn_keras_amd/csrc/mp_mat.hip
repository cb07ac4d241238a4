// MAT (kgcnn/layers/conv/mat_conv.py:109-185, the Molecule Attention Transformer): all-pairs attention of a molecule on
// ragged rows, nothing of size n^2 in HBM.
//
// Rows are the atoms of the whole batch, C = H * U channels (head h owns columns [h U, (h+1) U)), s = sqrt(U), mol(i)
// the atoms of i's molecule from the node row splits:
//
//   att_c(i,j) = softmax over j in mol(i) of (q[i,c] s) k[j,c]                        per channel c
//   dist(i,j)  = exp(-d2) | softmax over j in mol(i) of d2 | d2,    d2 = (dx^2 + dy^2) + dz^2 of x_i - x_j
//   y[i,c] = la sum_j att_c(i,j) v[j,c] + ld sum_j dist(i,j) v[j,c]
//          + lg (sum over edges e with recv e = i of w[e] v[send e, c] + (add_identity ? v[i,c] : 0))
//
// The reference forms this on padded (batch, Nmax, Nmax, U) tensors per head, with a -1/epsilon mask in front of every
// softmax; on ragged rows the padded senders (weight exactly 0 after the mask) and padded receivers (multiplied by 0) do
// not exist.
//
// One 256-thread workgroup serves a (molecule, tile of R = MP_MAT_RECV_TILE receivers) pair; blockIdx.y strides over a
// molecule's receiver tiles.  A lane owns a channel of a 64-channel chunk, a wave 4 receivers of the tile: the senders
// stream through LDS in tiles of S = MP_MAT_SEND_TILE rows of k and v (one ds_read_b32 each per sender and lane, lanes on
// consecutive banks), and the four receivers' exponentials share them.  The distance weights of the (R x S) pairs are
// computed once per sender tile by all threads into LDS and read back as one broadcast 16-byte read per sender.
// The work is R x n x C exponentials per tile; every other cost is 1/4 (LDS reads) to 1/64 (distance weights) of it.
//
// The maximum under every exponential is exact and known before the pass: for the attention it is
// (q s) max_j k[j,c] where q s >= 0 and (q s) min_j k[j,c] otherwise - the product is monotonic in k in floating point
// too, so the largest score minus it is exactly 0 and no argument is positive; the per-channel extrema of k over the
// molecule come from a pre-pass of the workgroup.  For the softmax of d2 the row maximum comes from a pre-pass over the
// coordinates that forms d2 by the same expression.  q = 0 gives exp(0) everywhere: the uniform distribution.
// The attention scores are kept in units of log 2 (log2(e) folded into q s once per receiver and channel, the maximum
// formed from that same number), so every attention weight is one v_exp_f32.
//
// Edges are read through the receiver CSR (ptr0, perm0 nullable) in list order, senders clamped into [0, N) and flagged.
// No atomics on data, every sum in an order fixed by the inputs: equal bits on every call and stream.
// All loads are unconditional, from addresses clamped into the molecule; what lies outside is never accumulated (the
// sender loops run to the tile's count) or never written.
//
// Epilogue (template flag, the plain build carries none of it): the tile's y rows are kept in LDS and
// out[i] = h[i] + y[i] @ Wm with Wm (C, E) ("concat") or (U, E) applied to every head's columns ("sum": the sum over
// heads of y_h @ Wm is (sum_h y_h) @ Wm); y is never written.
#include "mp_common.h"
#include "../../include/mpengine/mat.h"

namespace {

constexpr int R = MP_MAT_RECV_TILE;   // receivers per workgroup: 4 per wave
constexpr int S = MP_MAT_SEND_TILE;   // senders per LDS tile
constexpr int CH = 64;                // channels per chunk = lanes of a wave
constexpr int RW = R / 4;             // receivers per wave
constexpr int EPI_C = MP_MAT_EPILOGUE_MAX_CHANNELS;
constexpr int EPI_E = MP_MAT_EPILOGUE_MAX_WIDTH;
constexpr float LOG2E = 1.4426950408889634f;
static_assert(R == 16 && RW == 4, "a wave reads its receivers' distance weights as one float4");
static_assert(S * CH == 16 * 256 && R * S == 4 * 256, "staging and pair loops are unrolled for 256 threads");

struct MatArgs {
  const float* q; const float* k; const float* v;   // (N, C) with leading dimensions
  int64_t ldq, ldk, ldv;
  const float* xyz;          // (N, 3)
  const int64_t* splits;     // (G + 1)
  const int32_t* ptr0;       // (N + 1) receiver CSR
  const int32_t* perm0;      // (M) nullable
  const int32_t* send;       // (M)
  const float* w;            // (M)
  const float* Wm;           // epilogue: (C, E) or (U, E)
  const float* h;            // epilogue: (N, E) nullable
  float* out;                // (N, C), with the epilogue (N, E)
  int32_t* flags;            // nullable
  int64_t N, M;
  int C, U, E, trafo, add_identity, merge_sum;
  float scale, la, ld, lg;
};

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

template <bool EPI>
__global__ __launch_bounds__(256) void mat_attention_kernel(MatArgs a) {
  __shared__ float ks[S * CH];
  __shared__ float vs[S * CH];
  __shared__ __align__(16) float gd[S * R];
  __shared__ float xs[S * 3];
  __shared__ float xr[R * 3];
  __shared__ float dmax[R];
  __shared__ float kext[2][4][CH];
  __shared__ float ys[EPI ? R * (EPI_C + 1) : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  int64_t n0 = a.splits[g], n1 = a.splits[g + 1];
  n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
  n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
  const int64_t n = n1 - n0;
  const int64_t tiles = (n + R - 1) / R;
  if (static_cast<int64_t>(blockIdx.y) >= tiles) return;   // workgroup-uniform, in front of every barrier
  const int64_t last = n1 - 1;
  const int C = a.C;
  const int ystride = C + 1;
  int local_flags = 0;

  for (int64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const int64_t r0 = n0 + tile * R;
    if (tid < R * 3) {
      const int64_t row = r0 + tid / 3 < n1 ? r0 + tid / 3 : last;
      xr[tid] = a.xyz[row * 3 + tid % 3];
    }
    if (a.trafo == MP_MAT_TRAFO_SOFTMAX) {
      // row maximum of d2: 16 threads per receiver stride over the molecule, then a butterfly inside the 16
      const int r = tid >> 4, sub = tid & 15;
      const int64_t ri = r0 + r < n1 ? r0 + r : last;
      const float ax = a.xyz[ri * 3], ay = a.xyz[ri * 3 + 1], az = a.xyz[ri * 3 + 2];
      float m = 0.0f;   // d2(i,i) = 0 is among the terms
      for (int64_t j = n0 + sub; j < n1; j += 16)
        m = fmaxf(m, dist2(ax, ay, az, a.xyz[j * 3], a.xyz[j * 3 + 1], a.xyz[j * 3 + 2]));
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
      if (sub == 0) dmax[r] = m;
    }
    for (int c0 = 0; c0 < C; c0 += CH) {
      const int c = c0 + lane < C ? c0 + lane : C - 1;
      // per-channel extrema of k over the molecule: wave w takes senders w, w + 4, ...
      {
        float lo = a.k[n0 * a.ldk + c], hi = lo;
        for (int64_t j = n0 + wave; j < n1; j += 4) {
          const float kv = a.k[j * a.ldk + c];
          lo = fminf(lo, kv);
          hi = fmaxf(hi, kv);
        }
        kext[0][wave][lane] = lo;
        kext[1][wave][lane] = hi;
      }
      __syncthreads();   // also orders xr and dmax in front of their readers
      const float kmin = fminf(fminf(kext[0][0][lane], kext[0][1][lane]), fminf(kext[0][2][lane], kext[0][3][lane]));
      const float kmax = fmaxf(fmaxf(kext[1][0][lane], kext[1][1][lane]), fmaxf(kext[1][2][lane], kext[1][3][lane]));
      float qs[RW], mx[RW], num[RW], den[RW], dsum[RW], dden[RW];
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const int64_t ri = r0 + wave * RW + i < n1 ? r0 + wave * RW + i : last;
        qs[i] = (a.q[ri * a.ldq + c] * a.scale) * LOG2E;   // scores in units of log 2: one v_exp_f32 per weight
        mx[i] = qs[i] * (qs[i] >= 0.0f ? kmax : kmin);
        num[i] = den[i] = dsum[i] = dden[i] = 0.0f;
      }
      for (int64_t j0 = n0; j0 < n1; j0 += S) {
        const int cnt = static_cast<int>(n1 - j0 < S ? n1 - j0 : S);
        // stage k and v: thread -> (row idx / 64, channel idx % 64), the rows past the molecule repeat its last row
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int idx = tid + i * 256;
          const int64_t row = j0 + (idx >> 6) < n1 ? j0 + (idx >> 6) : last;
          ks[idx] = a.k[row * a.ldk + c];
          vs[idx] = a.v[row * a.ldv + c];
        }
        if (tid < S * 3) {
          const int64_t row = j0 + tid / 3 < n1 ? j0 + tid / 3 : last;
          xs[tid] = a.xyz[row * 3 + tid % 3];
        }
        __syncthreads();
        // distance weights of the (S x R) pairs, gd[j][r]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = tid + i * 256;
          const int j = p >> 4, r = p & 15;
          const float d2 = dist2(xr[r * 3], xr[r * 3 + 1], xr[r * 3 + 2], xs[j * 3], xs[j * 3 + 1], xs[j * 3 + 2]);
          float wgt = d2;
          if (a.trafo == MP_MAT_TRAFO_EXP) wgt = expf(-d2);
          else if (a.trafo == MP_MAT_TRAFO_SOFTMAX) wgt = expf(d2 - dmax[r]);
          gd[p] = wgt;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
          const float kk = ks[j * CH + lane], vv = vs[j * CH + lane];
          const float4 g4 = *reinterpret_cast<const float4*>(gd + j * R + wave * RW);
          const float gg[RW] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
          for (int i = 0; i < RW; ++i) {
            const float e = __builtin_amdgcn_exp2f(qs[i] * kk - mx[i]);   // argument <= 0; below -126 the result is 0
            num[i] += e * vv;
            den[i] += e;
            dsum[i] += gg[i] * vv;
            dden[i] += gg[i];
          }
        }
        __syncthreads();
      }
      // adjacency: the receiver's edge list in list order, and the result
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const int rl = wave * RW + i;
        const bool live = r0 + rl < n1;   // wave-uniform
        const int64_t ri = live ? r0 + rl : last;
        int64_t ea = a.ptr0[ri], eb = a.ptr0[ri + 1];
        ea = ea < 0 ? 0 : (ea > a.M ? a.M : ea);
        eb = eb < ea ? ea : (eb > a.M ? a.M : eb);
        float adj = 0.0f;
        for (int64_t p = ea; p < eb; ++p) {
          int64_t e = a.perm0 != nullptr ? static_cast<int64_t>(a.perm0[p]) : p;
          e = e < 0 ? 0 : (e >= a.M ? a.M - 1 : e);
          int64_t sj = a.send[e];
          if (sj < 0 || sj >= a.N) { local_flags |= MP_FLAG_OOB; sj = sj < 0 ? 0 : a.N - 1; }
          adj += a.w[e] * a.v[sj * a.ldv + c];
        }
        if (a.add_identity) adj += a.v[ri * a.ldv + c];
        const float dterm = a.trafo == MP_MAT_TRAFO_SOFTMAX ? dsum[i] / dden[i] : dsum[i];
        const float y = (a.la * (num[i] / den[i]) + a.ld * dterm) + a.lg * adj;
        if (EPI) {
          if (c0 + lane < C) ys[rl * ystride + c0 + lane] = y;
        } else if (live && c0 + lane < C) {
          a.out[ri * C + c0 + lane] = y;
        }
      }
    }
    if (EPI) {
      __syncthreads();
      // out[r, e] = h[r, e] + sum_c y[r, c] Wm[row(c), e]: 16 threads per receiver, columns e = sub, sub + 16, ...
      const int r = tid >> 4, sub = tid & 15;
      const int64_t ri = r0 + r;
      if (ri < n1) {
        for (int e = sub; e < a.E; e += 16) {
          float acc = 0.0f;
          int wr = 0;   // row of Wm: c, or c mod U for the summed heads; U % 4 == 0, so a group of 4 never wraps inside
          for (int cc = 0; cc < C; cc += 4) {
            const float* wrow = a.Wm + static_cast<int64_t>(wr) * a.E + e;
            const float* yrow = ys + r * ystride + cc;
            acc += yrow[0] * wrow[0];
            acc += yrow[1] * wrow[a.E];
            acc += yrow[2] * wrow[2 * a.E];
            acc += yrow[3] * wrow[3 * a.E];
            wr += 4;
            if (a.merge_sum && wr == a.U) wr = 0;
          }
          a.out[ri * a.E + e] = a.h != nullptr ? a.h[ri * a.E + e] + acc : acc;
        }
      }
      __syncthreads();   // ys is rewritten by the next tile
    }
  }
  if (a.flags != nullptr) mp_publish_flags(a.flags, local_flags);
}

}  // namespace

extern "C" {

int mp_mat_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, int64_t N,
                         int H, int U, const float* xyz, const int64_t* node_splits, int64_t G, const int32_t* ptr0,
                         const int32_t* perm0, const int32_t* send, const float* w, int64_t M, int trafo,
                         float lambda_attention, float lambda_distance, float lambda_adjacency, int add_identity,
                         const float* Wm, int64_t E, int merge, const float* h, float* out, int32_t* flags,
                         mpStream_t stream) {
  const char* what = "mp_mat_attention_f32";
  MP_REQUIRE(H >= 1 && U >= 1 && static_cast<int64_t>(H) * U <= (1 << 20), "%s: bad sizes H=%d U=%d", what, H, U);
  const int64_t C = static_cast<int64_t>(H) * U;
  MP_REQUIRE(N >= 0 && G >= 0 && M >= 0 && N < (int64_t{1} << 31) - 1 && M < (int64_t{1} << 31) - 1 &&
                 G < (int64_t{1} << 31) - 1,
             "%s: bad sizes N=%lld G=%lld M=%lld", what, (long long)N, (long long)G, (long long)M);
  MP_REQUIRE(ldq >= C && ldk >= C && ldv >= C, "%s: leading dimensions below C=%lld", what, (long long)C);
  MP_REQUIRE(trafo == MP_MAT_TRAFO_NONE || trafo == MP_MAT_TRAFO_EXP || trafo == MP_MAT_TRAFO_SOFTMAX,
             "%s: unknown distance trafo %d", what, trafo);
  if (Wm != nullptr) {
    MP_REQUIRE(merge == MP_MAT_MERGE_CONCAT || merge == MP_MAT_MERGE_SUM, "%s: unknown merge %d", what, merge);
    MP_REQUIRE(U % 4 == 0 && C <= EPI_C && E >= 1 && E <= EPI_E,
               "%s: the merge epilogue serves U %% 4 == 0, C <= %d and 1 <= E <= %d, got U=%d C=%lld E=%lld", what, EPI_C,
               EPI_E, U, (long long)C, (long long)E);
  } else {
    MP_REQUIRE(h == nullptr, "%s: a residual needs the merge kernel", what);
  }
  if (N == 0 || G == 0) return MP_OK;
  MP_REQUIRE(q && k && v && xyz && node_splits && ptr0 && out, "%s: null pointer", what);
  MP_REQUIRE(M == 0 || (send && w), "%s: null pointer", what);
  MatArgs a{};
  a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.xyz = xyz; a.splits = node_splits;
  a.ptr0 = ptr0; a.perm0 = perm0; a.send = send; a.w = w; a.Wm = Wm; a.h = h; a.out = out; a.flags = flags;
  a.N = N; a.M = M; a.C = static_cast<int>(C); a.U = U; a.E = static_cast<int>(E); a.trafo = trafo;
  a.add_identity = add_identity ? 1 : 0; a.merge_sum = merge == MP_MAT_MERGE_SUM ? 1 : 0;
  a.scale = sqrtf(static_cast<float>(U));
  a.la = lambda_attention; a.ld = lambda_distance; a.lg = lambda_adjacency;
  // receiver-tile slots per molecule: twice the mean tile count, so that a molecule a few times the mean size is still
  // spread over workgroups; larger ones stride, smaller ones leave workgroups that return at once
  int64_t ty = mp::ceil_div(2 * N, G * R);
  ty = ty < 1 ? 1 : (ty > 1024 ? 1024 : ty);
  const dim3 grid(static_cast<unsigned>(G), static_cast<unsigned>(ty));
  if (Wm != nullptr) mat_attention_kernel<true><<<grid, 256, 0, mp::as_stream(stream)>>>(a);
  else mat_attention_kernel<false><<<grid, 256, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch(what);
}

}  // extern "C"
