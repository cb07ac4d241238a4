// CGCNN (kgcnn/literature/CGCNN.py:22-189, kgcnn/layers/conv/cgcnn_conv.py:9-128): inference batch normalisation and the
// fused gated edge step of one CGCNNLayer.
//
// Batch normalisation with the moving statistics (kgcnn/layers/norm.py:114-221 = Keras BatchNormalization, inference), in
// Keras' order of operations:  inv = (1 / sqrt(var + eps)) * gamma,  y = x * inv + (beta - mean * inv), no contraction.
// The four vectors are read where they are on every call.
//
// Fused gate step (cgcnn_conv.py:67-111), one launch plus a finishing pass:
//   z_s[e] = Pa_s[recv e] + Pb_s[send e] + g_e Wc_s + b_s          (likewise z_f)
//   m_e    = act_s(BN_s(z_s)) * sigmoid(BN_f(z_f))
//   u_i    = sum_{e: recv e = i} m_e                               in edge order
//   h'_i   = act_out(h_i + BN_out(u_i))
// Pa_* = h Wa_*, Pb_* = h Wb_* (N, 64) are made on the node side by four Dense launches on row blocks of the two kernels
// (read in place), so the per-edge Dense on [h_i, h_j, g] is two gathered rows plus the (D <= 64)-wide edge product.
// One workgroup (4 waves) walks tiles of 32 receiver-sorted edges:
//   phase 0  indices and the edge-feature tile G (32 x D, zero-padded to a multiple of 4 columns)             -> LDS
//   phase 1  G [Wc_s | Wc_f] on the matrix pipe: v_mfma_f32_16x16x4_f32, wave w owns output columns [16w, 16w+16) of
//            BOTH halves (four independent accumulators: two row blocks x {s, f}); its two D x 16 slabs live in 2 x 16
//            registers per lane for the whole kernel.  The s and the f value of one (edge, column) sit in the same lane
//            and register index, so the gate needs no exchange.
//   phase 2  per (edge, column): gathered rows + product + bias, BN affine, activations, product                -> LDS
//   phase 3  per-receiver sums in edge order by 64 threads (one per column): the walk of csrc/mp_edge_tile.h, which
//            states the rule for receivers cut by a tile boundary.  No atomics: two runs give equal bits.
// cgcnn_update_kernel then takes every node's u (direct, or the cut receiver's sum) and applies the node update in place;
// a node without edges has u = 0, and BN_out(0) = beta - mean * inv is NOT zero.
#include "mp_common.h"
#include "mp_edge_tile.h"
#include "../../include/mpengine/cgcnn.h"

namespace {

constexpr int F = 64;         // node width = units of the fused step
constexpr int TE = mp_tile::TE;   // edges per tile
constexpr int MAXD = 64;      // widest edge feature
constexpr int KS = MAXD / 4;  // MFMA steps at the widest edge feature
constexpr int GS = MAXD + 1;  // row stride of the edge-feature tile
constexpr int MS = F + 1;     // row stride of the message tile

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One batch normalisation's vectors (C each); gamma / beta nullable, on = 0: identity.
struct BnVec {
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  float eps;
  int on;
};

__device__ __forceinline__ void bn_affine(const BnVec& b, int c, float* inv_out, float* shift_out) {
  float inv = 1.0f, shift = 0.0f;
  if (b.on) {
    inv = 1.0f / sqrtf(b.var[c] + b.eps);
    if (b.gamma) inv *= b.gamma[c];
    shift = (b.beta ? b.beta[c] : 0.0f) - b.mean[c] * inv;
  }
  *inv_out = inv;
  *shift_out = shift;
}

__global__ void batchnorm_infer_kernel(const float* __restrict__ x, int64_t R, int C, BnVec b, int affine_only,
                                       float* __restrict__ out) {
  const int64_t total = R * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = static_cast<int>(i % C);
    float inv = 1.0f / sqrtf(b.var[c] + b.eps);
    if (b.gamma) inv *= b.gamma[c];
    if (affine_only) {   // the input reverse: g * inv
      out[i] = x[i] * inv;
    } else {
      const float shift = (b.beta ? b.beta[c] : 0.0f) - b.mean[c] * inv;
      out[i] = x[i] * inv + shift;
    }
  }
}

struct GateArgs {
  const float* Pa_s;     // (N, F) h Wa_s, gathered by the receiver
  const float* Pa_f;
  const float* Pb_s;     // (N, F) h Wb_s, gathered by the sender
  const float* Pb_f;
  const float* g;        // (E, D) edge features
  const int32_t* col0;   // (2, E) receivers | senders
  const int32_t* ptr0;   // (N+1) CSR of col0 over sorted positions
  const int32_t* perm0;  // (E) sorted position -> edge, nullable
  const float* Wc_s;     // (D, F)
  const float* Wc_f;
  const float* b_s;      // (F) nullable
  const float* b_f;
  BnVec bn_s, bn_f;
  float* out;            // (N, F): u of the receivers that lie inside one tile
  float* bnd;            // (tiles, 2, F)
  int N, E, D;           // N, E below 2^31 (checked on the host)
  int act_s;
  float alpha;
};

__global__ __launch_bounds__(256) void cgcnn_gate_kernel(GateArgs a) {
  __shared__ float gL[TE * GS];
  __shared__ float mL[TE * MS];
  __shared__ int recvL[TE], sndL[TE], eidL[TE];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int D = a.D;
  const int col = 16 * wave + (lane & 15), kq = lane >> 4;

  // B operand of step s: rows 4s + (lane >> 4), the wave's 16 columns; rows past D are zero
  float ws[KS], wf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + kq;
    ws[s] = k < D ? a.Wc_s[(size_t)k * F + col] : 0.0f;
    wf[s] = k < D ? a.Wc_f[(size_t)k * F + col] : 0.0f;
  }
  const float bs = a.b_s ? a.b_s[col] : 0.0f, bf = a.b_f ? a.b_f[col] : 0.0f;
  float inv_s, sh_s, inv_f, sh_f;
  bn_affine(a.bn_s, col, &inv_s, &sh_s);
  bn_affine(a.bn_f, col, &inv_f, &sh_f);

  const int tiles = (a.E + TE - 1) / TE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p0 = tile * TE;
    const int nv = a.E - p0 < TE ? a.E - p0 : TE;
    __syncthreads();   // the previous tile's walk is done with the tiles in LDS
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
    f32x4 acc_s[2], acc_f[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 4; ++i) { acc_s[rb][i] = 0.0f; acc_f[rb][i] = 0.0f; }
    {
      const float* ap = gL + (lane & 15) * GS + kq;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if (4 * s < D) {   // wave-uniform
          const float a0 = ap[4 * s], a1 = ap[16 * GS + 4 * s];
          acc_s[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, ws[s], acc_s[0], 0, 0, 0);
          acc_f[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wf[s], acc_f[0], 0, 0, 0);
          acc_s[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, ws[s], acc_s[1], 0, 0, 0);
          acc_f[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wf[s], acc_f[1], 0, 0, 0);
        }
      }
    }
    // phase 2: C layout of 16x16x4: col = lane & 15, row = 4 * (lane >> 4) + i
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = 16 * rb + 4 * kq + i;
        const int r = recvL[e];
        float m = 0.0f;
        if (r >= 0) {
          const size_t ro = (size_t)r * F + col, so = (size_t)sndL[e] * F + col;
          float zs = ((a.Pa_s[ro] + a.Pb_s[so]) + acc_s[rb][i]) + bs;
          float zf = ((a.Pa_f[ro] + a.Pb_f[so]) + acc_f[rb][i]) + bf;
          if (a.bn_s.on) zs = zs * inv_s + sh_s;
          if (a.bn_f.on) zf = zf * inv_f + sh_f;
          m = mp_apply_act(a.act_s, a.alpha, zs) * mp_apply_act(MP_ACT_SIGMOID, a.alpha, zf);
        }
        mL[e * MS + col] = m;
      }
    }
    __syncthreads();
    // phase 3
    if (t < F)
      mp_tile::walk<F>(recvL, nv, a.ptr0, a.out, a.bnd, tile, t, [=](int e) { return mL[e * MS + t]; });
  }
}

// u of every node (direct, a cut receiver's sum, or 0 without edges), then the node update in place.
__global__ void cgcnn_update_kernel(const int32_t* __restrict__ ptr0, int64_t N, const float* __restrict__ bnd,
                                    const float* __restrict__ h, BnVec bn, int act_out, float alpha,
                                    float* __restrict__ out) {
  const int64_t total = N * F;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / F;
    const int col = static_cast<int>(i - r * F);
    const int64_t s0 = ptr0[r], s1 = ptr0[r + 1];
    float u = 0.0f;
    if (s1 > s0 && !mp_tile::cut_sum<F>(bnd, s0, s1, col, &u)) u = out[i];
    if (bn.on) {
      float inv, shift;
      bn_affine(bn, col, &inv, &shift);
      u = u * inv + shift;
    }
    out[i] = mp_apply_act(act_out, alpha, h[i] + u);
  }
}

int make_bn(const char* what, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
            BnVec* b) {
  b->gamma = gamma; b->beta = beta; b->mean = mean; b->var = var; b->eps = eps;
  b->on = (mean || var) ? 1 : 0;
  MP_REQUIRE(!b->on || (mean && var), "%s: a batch normalisation needs both moving_mean and moving_variance", what);
  MP_REQUIRE(b->on || (!gamma && !beta), "%s: gamma / beta without moving statistics", what);
  MP_REQUIRE(!b->on || eps >= 0.0f, "%s: negative epsilon", what);
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_batchnorm_infer_f32(const float* x, int64_t R, int64_t C, const float* gamma, const float* beta,
                           const float* moving_mean, const float* moving_variance, float epsilon, float* out,
                           mpStream_t stream) {
  MP_REQUIRE(R >= 0 && C >= 1 && C < (int64_t(1) << 31), "mp_batchnorm_infer_f32: bad sizes");
  if (R == 0) return MP_OK;
  MP_REQUIRE(x && out && moving_variance, "mp_batchnorm_infer_f32: null pointer");
  MP_REQUIRE(moving_mean || !beta, "mp_batchnorm_infer_f32: beta without moving_mean (the reverse takes neither)");
  MP_REQUIRE(epsilon >= 0.0f, "mp_batchnorm_infer_f32: negative epsilon");
  BnVec b{gamma, beta, moving_mean, moving_variance, epsilon, 1};
  batchnorm_infer_kernel<<<mp::grid_for(R * C), 256, 0, mp::as_stream(stream)>>>(x, R, static_cast<int>(C), b,
                                                                                 moving_mean ? 0 : 1, out);
  return mp::check_launch("mp_batchnorm_infer_f32");
}

int mp_cgcnn_gate_ws_bytes(int64_t E, size_t* bytes_out_host) {
  MP_REQUIRE(E >= 0 && bytes_out_host, "mp_cgcnn_gate_ws_bytes: bad arguments");
  *bytes_out_host = mp_tile::ws_bytes(E, F);
  return MP_OK;
}

int mp_cgcnn_gate_f32(const float* h, const float* Pa_s, const float* Pa_f, const float* Pb_s, const float* Pb_f,
                      int64_t N, const float* edges, int D, const int32_t* cols, int64_t E, const int32_t* ptr0,
                      const int32_t* perm0, const float* Wc_s, const float* Wc_f, const float* b_s, const float* b_f,
                      const float* const* bn_host, const float* eps_host, int act_s, int act_out, float alpha, float* ws,
                      size_t ws_bytes, float* out, mpStream_t stream) {
  const char* what = "mp_cgcnn_gate_f32";
  MP_REQUIRE(mp_tile::sizes_ok(N, E), "%s: bad sizes", what);
  MP_REQUIRE(D >= 1 && D <= MAXD, "%s: the fused gate step takes 1 to %d edge features, got %d", what, MAXD, D);
  MP_REQUIRE(act_s >= 0 && act_out >= 0 && act_s <= MP_ACT_LAST && act_out <= MP_ACT_LAST, "%s: unknown activation code",
             what);
  MP_REQUIRE((bn_host == nullptr) == (eps_host == nullptr), "%s: bn and eps go together", what);
  BnVec bn[3];
  for (int i = 0; i < 3; ++i) {
    int rc = bn_host ? make_bn(what, bn_host[4 * i], bn_host[4 * i + 1], bn_host[4 * i + 2], bn_host[4 * i + 3],
                               eps_host[i], &bn[i])
                     : make_bn(what, nullptr, nullptr, nullptr, nullptr, 0.0f, &bn[i]);
    if (rc != MP_OK) return rc;
  }
  if (N == 0) return MP_OK;
  MP_REQUIRE(h && ptr0 && out, "%s: null pointer", what);
  const size_t need = mp_tile::ws_bytes(E, F);
  if (E > 0) {
    MP_REQUIRE(Pa_s && Pa_f && Pb_s && Pb_f && edges && cols && Wc_s && Wc_f && ws, "%s: null pointer", what);
    MP_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", what, ws_bytes, need);
    GateArgs a{};
    a.Pa_s = Pa_s; a.Pa_f = Pa_f; a.Pb_s = Pb_s; a.Pb_f = Pb_f; a.g = edges; a.col0 = cols; a.ptr0 = ptr0;
    a.perm0 = perm0; a.Wc_s = Wc_s; a.Wc_f = Wc_f; a.b_s = b_s; a.b_f = b_f; a.bn_s = bn[0]; a.bn_f = bn[1];
    a.out = out; a.bnd = ws; a.N = static_cast<int>(N); a.E = static_cast<int>(E); a.D = D; a.act_s = act_s;
    a.alpha = alpha;
    const int64_t tiles = mp_tile::tiles_of(E);
    cgcnn_gate_kernel<<<static_cast<unsigned>(tiles < 1024 ? tiles : 1024), 256, 0, mp::as_stream(stream)>>>(a);
    int rc = mp::check_launch(what);
    if (rc != MP_OK) return rc;
  }
  cgcnn_update_kernel<<<mp::grid_for(N * F), 256, 0, mp::as_stream(stream)>>>(ptr0, N, ws, h, bn[2], act_out, alpha, out);
  return mp::check_launch("mp_cgcnn_gate_f32 (update)");
}

}  // extern "C"
