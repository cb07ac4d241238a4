// DimeNet++ (kgcnn/literature/DimeNetPP.py:23-183): edge angles, the spherical basis and the fused triplet step of the
// interaction block, each with its reverse.
//
//   mp_vector_angle_f32 / _grad_f32    VectorAngle (kgcnn/layers/geom.py:382-446), row by row
//   mp_edge_angle_f32 / _grad_f32      EdgeAngle (geom.py:450-510): the gather of both edge vectors fused in
//   mp_spherical_basis_f32 / _grad_f32 SphericalBasisLayer (kgcnn/layers/conv/dimenet_conv.py:380-463)
//   mp_dimenet_triplet_f32 / _grad_f32 the triplet step of DimNetInteractionPPBlock (dimenet_conv.py:186-197)
//
// Angle pairs (n, m) index edges: n = A[t, 0] receives, m = A[t, 1] sends (GatherNodesOutgoing / PoolingLocalEdges).
// cols = the index plan's shifted int32 columns (2, T) of the angle list against the EDGE partition.  Every sum over
// triplets walks a CSR (ptr, stable-sort perm) in list order; reductions across a wave use a fixed butterfly: the same
// bits every run and on every stream, no float atomics.
#include <math.h>

#include "mp_common.h"
#include "../../include/mpengine/dimenet.h"

namespace {

constexpr int kWave = 64;
constexpr int kIntEmb = 64;     // int_emb_size of the fused triplet step
constexpr int kBasisEmb = 8;    // basis_emb_size of the fused triplet step
constexpr int kMaxSbf = 64;     // num_spherical * num_radial of the fused triplet step

// wave-wide sum as a wave-uniform (scalar-register) value
__device__ __forceinline__ float wave_sum(float v) { return mp_bcast(mp_wave_sum(v), 0); }

// ------------------------------------------------------------------------------------------------ angles
// VectorAngle: theta = atan2(|a x b|, a . b)
__device__ __forceinline__ float angle_of(const float a[3], const float b[3]) {
  const float c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
  const float x = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const float y = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
  return atan2f(y, x);
}

// d theta / da = a x (a x b) / (|a|^2 y) and d theta / db = (a x b) x b / (|b|^2 y), y = |a x b|: the cross-product
// form keeps its accuracy near collinear pairs, where (x a / |a|^2 - b) / y cancels.  At y = 0 (collinear vectors) both are
// zero: the sub-gradient the basis needs, since Y_l0 depends on theta through cos theta only and d cos theta vanishes
// there (the reference's tf.norm gradient is NaN).
__device__ __forceinline__ void angle_grad(const float a[3], const float b[3], float g, float ga[3], float gb[3]) {
  const float c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
  const float y = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
  const float aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  if (!(y > 0.0f) || !(aa > 0.0f) || !(bb > 0.0f)) {
    ga[0] = ga[1] = ga[2] = gb[0] = gb[1] = gb[2] = 0.0f;
    return;
  }
  const float sa = g / (y * aa), sb = g / (y * bb);
  ga[0] = sa * (a[1] * c2 - a[2] * c1);
  ga[1] = sa * (a[2] * c0 - a[0] * c2);
  ga[2] = sa * (a[0] * c1 - a[1] * c0);
  gb[0] = sb * (c1 * b[2] - c2 * b[1]);
  gb[1] = sb * (c2 * b[0] - c0 * b[2]);
  gb[2] = sb * (c0 * b[1] - c1 * b[0]);
}

__global__ void vector_angle_kernel(const float* __restrict__ v1, const float* __restrict__ v2, int64_t T,
                                    float* __restrict__ theta) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < T; t += stride) {
    const float a[3] = {v1[3 * t], v1[3 * t + 1], v1[3 * t + 2]};
    const float b[3] = {v2[3 * t], v2[3 * t + 1], v2[3 * t + 2]};
    theta[t] = angle_of(a, b);
  }
}

__global__ void vector_angle_grad_kernel(const float* __restrict__ v1, const float* __restrict__ v2, int64_t T,
                                         const float* __restrict__ g, float* __restrict__ g1, float* __restrict__ g2) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < T; t += stride) {
    const float a[3] = {v1[3 * t], v1[3 * t + 1], v1[3 * t + 2]};
    const float b[3] = {v2[3 * t], v2[3 * t + 1], v2[3 * t + 2]};
    float ga[3], gb[3];
    angle_grad(a, b, g[t], ga, gb);
    if (g1) { g1[3 * t] = ga[0]; g1[3 * t + 1] = ga[1]; g1[3 * t + 2] = ga[2]; }
    if (g2) { g2[3 * t] = gb[0]; g2[3 * t + 1] = gb[1]; g2[3 * t + 2] = gb[2]; }
  }
}

// the two scaled edge vectors of triplet t; false when an index is out of range
__device__ __forceinline__ bool edge_pair(const float* v, int64_t E, const int32_t* cols, int64_t T, const float* scale,
                                          int64_t t, float a[3], float b[3]) {
  const int32_t n = cols[t], m = cols[T + t];
  if (n < 0 || n >= E || m < 0 || m >= E) return false;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a[q] = v[3 * static_cast<int64_t>(n) + q];
    b[q] = v[3 * static_cast<int64_t>(m) + q];
    if (scale) { a[q] *= scale[q]; b[q] *= scale[3 + q]; }
  }
  return true;
}

__global__ void edge_angle_kernel(const float* __restrict__ v, int64_t E, const int32_t* __restrict__ cols, int64_t T,
                                  const float* __restrict__ scale, float* __restrict__ theta) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < T; t += stride) {
    float a[3], b[3];
    theta[t] = edge_pair(v, E, cols, T, scale, t, a, b) ? angle_of(a, b) : 0.0f;
  }
}

// per-triplet partials (2, T, 3) with respect to the UNSCALED edge vectors of n and m
__global__ void edge_angle_part_kernel(const float* __restrict__ v, int64_t E, const int32_t* __restrict__ cols,
                                       int64_t T, const float* __restrict__ scale, const float* __restrict__ g,
                                       float* __restrict__ part) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < T; t += stride) {
    float a[3], b[3], ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
    if (edge_pair(v, E, cols, T, scale, t, a, b)) angle_grad(a, b, g[t], ga, gb);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      part[3 * t + q] = scale ? ga[q] * scale[q] : ga[q];
      part[3 * (T + t) + q] = scale ? gb[q] * scale[3 + q] : gb[q];
    }
  }
}

// v_bar[e] = sum over both angle columns c, over the triplets with A[t, c] = e in list order, of part[c][t]: one wave
// per edge, lane-strided partial sums, fixed butterfly.
__global__ __launch_bounds__(64) void edge_angle_sum_kernel(const float* __restrict__ part, int64_t T,
                                                            const int32_t* __restrict__ ptr0,
                                                            const int32_t* __restrict__ perm0,
                                                            const int32_t* __restrict__ ptr1,
                                                            const int32_t* __restrict__ perm1,
                                                            float* __restrict__ v_bar) {
  const int lane = threadIdx.x;
  const int64_t e = blockIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int c = 0; c < 2; ++c) {
    const int32_t* ptr = c ? ptr1 : ptr0;
    const int32_t* perm = c ? perm1 : perm0;
    for (int32_t p = ptr[e] + lane; p < ptr[e + 1]; p += kWave) {
      const int64_t t = perm ? perm[p] : p;
      const float* src = part + 3 * (c * T + t);
      s0 += src[0]; s1 += src[1]; s2 += src[2];
    }
  }
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
  if (lane == 0) {
    v_bar[3 * e] = s0; v_bar[3 * e + 1] = s1; v_bar[3 * e + 2] = s2;
  }
}

// ------------------------------------------------------------------------------------------------ spherical basis
// Tables (host-built, float32, SphericalBasisLayer.__init__): zeros (L, R) | norm (L, R) | Legendre coefficients
// (L, KL) of x^(l - 2i), i = 0..l/2 | the Y_l0 prefactors sqrt((2l+1) / 4pi) (L); KL = L / 2 + 1.
struct SbfTables {
  const float* zeros;
  const float* norm;
  const float* leg;
  const float* ynorm;
  int L, R, KL;
};

__device__ __forceinline__ SbfTables sbf_tables(const float* tab, int L, int R) {
  SbfTables s;
  s.L = L; s.R = R; s.KL = L / 2 + 1;
  s.zeros = tab;
  s.norm = tab + L * R;
  s.leg = tab + 2 * L * R;
  s.ynorm = tab + 2 * L * R + L * s.KL;
  return s;
}

// j_l(x) by the reference's upward recursion (kgcnn/ops/polynom.py:50-86); jm1 = j_{l-1}(x) (j_1(x) for l = 0), which
// the derivative j_l' = j_{l-1} - (l+1)/x j_l needs (j_0' = -j_1).
__device__ __forceinline__ float bessel_j(float x, int l, float* jm1) {
  const float s = sinf(x), c = cosf(x);
  const float j0 = s / x;
  const float j1 = s / (x * x) - c / x;
  if (l == 0) { *jm1 = j1; return j0; }
  float jn = j0, jnn = j1;
  for (int i = 1; i < l; ++i) {
    const float tmp = jnn;
    jnn = static_cast<float>(2 * i + 1) / x * jnn - jn;
    jn = tmp;
  }
  *jm1 = jn;
  return jnn;
}

// SphericalBasisLayer.envelope (dimenet_conv.py:409-416) and its derivative; zero for u >= 1
__device__ __forceinline__ float envelope(float u, int p, float* denv) {
  const float a = -(p + 1) * (p + 2) / 2.0f, b = static_cast<float>(p * (p + 2)), c = -p * (p + 1) / 2.0f;
  if (!(u < 1.0f)) { *denv = 0.0f; return 0.0f; }
  float up2 = 1.0f;                         // u^(p-2)
  for (int i = 0; i < p - 2; ++i) up2 *= u;
  const float up1 = p >= 2 ? up2 * u : 1.0f;   // u^(p-1)
  *denv = -1.0f / (u * u) + a * (p - 1) * (p >= 2 ? up2 : 0.0f) + b * p * up1 + c * (p + 1) * (up1 * u);
  return 1.0f / u + a * up1 + b * (up1 * u) + c * (up1 * u * u);
}

// Y_l0(theta) = (sum_i leg[l, i] x^(l-2i)) * ynorm[l], x = cos theta, summed from the highest power down as the
// reference does (polynom.py:117-147); dY = d Y_l0 / d theta = -sin theta * ynorm[l] * P_l'(x)
__device__ __forceinline__ float y_l0(const SbfTables& tb, int l, float theta, float* dy) {
  const float x = cosf(theta);
  float sum = 0.0f, dsum = 0.0f;
  for (int i = 0; i <= l / 2; ++i) {
    const int pw = l - 2 * i;
    float xp = 1.0f, xd = 1.0f;               // x^pw, x^(pw-1)
    for (int q = 0; q < pw; ++q) xp *= x;
    for (int q = 0; q < pw - 1; ++q) xd *= x;
    const float cf = tb.leg[l * tb.KL + i];
    sum = sum + cf * xp;
    if (pw > 0) dsum = dsum + cf * static_cast<float>(pw) * xd;
  }
  if (dy) *dy = -sinf(theta) * (dsum * tb.ynorm[l]);
  return sum * tb.ynorm[l];
}

// rbf_env[e, l*R + k] = env(u) * (norm[l,k] * j_l(zeros[l,k] * u)), u = d_e / c (dimenet_conv.py:433-444)
__global__ void sbf_edge_kernel(const float* __restrict__ d, int64_t E, const float* __restrict__ tab, int L, int R,
                                float inv_cutoff, int p, float* __restrict__ rbf_env) {
  const SbfTables tb = sbf_tables(tab, L, R);
  const int LR = L * R;
  const int64_t total = E * LR;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int lk = static_cast<int>(i % LR);
    const int l = lk / R;
    const float u = d[i / LR] * inv_cutoff;
    float jm1, denv;
    const float j = bessel_j(u * tb.zeros[lk], l, &jm1);
    rbf_env[i] = envelope(u, p, &denv) * (tb.norm[lk] * j);
  }
}

// sbf[t, l*R + k] = rbf_env[A[t,1], l*R + k] * Y_l0(theta_t) (dimenet_conv.py:445-452)
__global__ void sbf_triplet_kernel(const float* __restrict__ rbf_env, int64_t E, const float* __restrict__ theta,
                                   const int32_t* __restrict__ cols, int64_t T, const float* __restrict__ tab, int L,
                                   int R, float* __restrict__ sbf) {
  const SbfTables tb = sbf_tables(tab, L, R);
  const int LR = L * R;
  const int64_t total = T * LR;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int lk = static_cast<int>(i % LR);
    const int64_t t = i / LR;
    const int32_t m = cols[T + t];
    float val = 0.0f;
    if (m >= 0 && m < E) val = rbf_env[static_cast<int64_t>(m) * LR + lk] * y_l0(tb, lk / R, theta[t], nullptr);
    sbf[i] = val;
  }
}

// theta_bar[t] = sum_l dY_l/dtheta * sum_k g[t, l*R+k] rbf_env[m, l*R+k]
__global__ void sbf_theta_grad_kernel(const float* __restrict__ rbf_env, int64_t E, const float* __restrict__ theta,
                                      const int32_t* __restrict__ cols, int64_t T, const float* __restrict__ tab, int L,
                                      int R, const float* __restrict__ g, float* __restrict__ theta_bar) {
  const SbfTables tb = sbf_tables(tab, L, R);
  const int LR = L * R;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < T; t += stride) {
    const int32_t m = cols[T + t];
    float acc = 0.0f;
    if (m >= 0 && m < E) {
      const float* gr = g + t * LR;
      const float* rr = rbf_env + static_cast<int64_t>(m) * LR;
      for (int l = 0; l < L; ++l) {
        float s = 0.0f;
        for (int k = 0; k < R; ++k) s += gr[l * R + k] * rr[l * R + k];
        float dy;
        y_l0(tb, l, theta[t], &dy);
        acc += s * dy;
      }
    }
    theta_bar[t] = acc;
  }
}

// d_bar[e] = sum_{l,k} d rbf_env[e, lk] / d d_e * sum_{t: A[t,1] = e} g[t, lk] Y_l(theta_t): one wave per edge, lane lk
// walks the edge's triplets in list order (CSR of column 1), then a fixed butterfly over lk.
__global__ __launch_bounds__(64) void sbf_dist_grad_kernel(const float* __restrict__ d, int64_t E,
                                                           const float* __restrict__ theta, int64_t T,
                                                           const int32_t* __restrict__ ptr1,
                                                           const int32_t* __restrict__ perm1,
                                                           const float* __restrict__ tab, int L, int R,
                                                           float inv_cutoff, int p, const float* __restrict__ g,
                                                           float* __restrict__ d_bar) {
  const SbfTables tb = sbf_tables(tab, L, R);
  const int LR = L * R;
  const int lane = threadIdx.x;
  const int64_t e = blockIdx.x;
  const int32_t beg = ptr1[e], end = ptr1[e + 1];
  const float u = d[e] * inv_cutoff;
  float denv;
  const float env = envelope(u, p, &denv);
  float acc = 0.0f;
  for (int lk = lane; lk < LR; lk += kWave) {
    const int l = lk / R;
    float w = 0.0f;
    for (int32_t q = beg; q < end; ++q) {
      const int64_t t = perm1 ? perm1[q] : q;
      w += g[t * LR + lk] * y_l0(tb, l, theta[t], nullptr);
    }
    if (beg == end) continue;
    const float z = tb.zeros[lk];
    float jm1;
    const float j = bessel_j(u * z, l, &jm1);
    const float jd = l == 0 ? -jm1 : jm1 - static_cast<float>(l + 1) / (u * z) * j;
    const float dr = (denv * (tb.norm[lk] * j) + env * (tb.norm[lk] * (z * jd))) * inv_cutoff;
    acc += w * dr;
  }
  acc = wave_sum(acc);
  if (lane == 0) d_bar[e] = acc;
}

// ------------------------------------------------------------------------------------------------ fused triplet step
// s_t = (sbf_t W1) W2 for 8 triplets at once: lane 8*s + k holds h[s][k] = sum_j sbf[t_s, j] W1[j, k].
__device__ __forceinline__ float triplet_h(const float* sbf, int nsbf, const float* s_w1, int64_t t, bool ok, int k) {
  float h = 0.0f;
  if (ok) {
    const float* row = sbf + t * nsbf;
    for (int j = 0; j < nsbf; ++j) h += row[j] * s_w1[j * kBasisEmb + k];
  }
  return h;
}

// out[n, c] = sum_{t: A[t,0] = n} xdown[A[t,1], c] * s_t[c]; one wave per receiver edge n, lane c owns channel c,
// triplets in list order over the CSR of column 0.  An edge without triplets gets a zero row.
__global__ __launch_bounds__(64) void triplet_fwd_kernel(const float* __restrict__ xdown, int64_t E,
                                                         const float* __restrict__ sbf, int nsbf,
                                                         const int32_t* __restrict__ cols, int64_t T,
                                                         const int32_t* __restrict__ ptr0,
                                                         const int32_t* __restrict__ perm0,
                                                         const float* __restrict__ W1, const float* __restrict__ W2,
                                                         float* __restrict__ out) {
  __shared__ float s_w1[kMaxSbf * kBasisEmb];
  const int lane = threadIdx.x;
  for (int i = lane; i < nsbf * kBasisEmb; i += kWave) s_w1[i] = W1[i];
  __syncthreads();
  float w2[kBasisEmb];
#pragma unroll
  for (int k = 0; k < kBasisEmb; ++k) w2[k] = W2[k * kIntEmb + lane];
  const int64_t n = mp_xcd_block(blockIdx.x, gridDim.x);
  const int32_t beg = ptr0[n], end = ptr0[n + 1];
  const int slot = lane >> 3, k = lane & 7;
  float acc = 0.0f;
  for (int32_t base = beg; base < end; base += 8) {
    const int32_t p = base + slot;
    const bool live = p < end;
    const int64_t t = live ? (perm0 ? perm0[p] : p) : 0;
    int m = live ? cols[T + t] : -1;
    const bool ok = live && m >= 0 && m < E;
    if (!ok) m = -1;
    const float h = triplet_h(sbf, nsbf, s_w1, t, ok, k);
    const int cnt = min(8, end - base);
    for (int s = 0; s < cnt; ++s) {
      const int ms = mp_bcast(m, 8 * s);
      if (ms < 0) continue;
      float v = 0.0f;
#pragma unroll
      for (int q = 0; q < kBasisEmb; ++q) v += mp_bcast(h, 8 * s + q) * w2[q];
      acc += xdown[static_cast<int64_t>(ms) * kIntEmb + lane] * v;
    }
  }
  out[n * kIntEmb + lane] = acc;
}

// Reverse, sender-ordered over the CSR of column 1: one wave per edge m.
//   xdown_bar[m, c] = sum_{t: A[t,1] = m} g[A[t,0], c] * s_t[c]                        (list order)
//   sbf_bar[t, j]   = sum_k W1[j, k] sum_c W2[k, c] g[A[t,0], c] xdown[m, c]            (each triplet once)
__global__ __launch_bounds__(64) void triplet_bwd_kernel(const float* __restrict__ xdown, int64_t E,
                                                         const float* __restrict__ sbf, int nsbf,
                                                         const int32_t* __restrict__ cols, int64_t T,
                                                         const int32_t* __restrict__ ptr1,
                                                         const int32_t* __restrict__ perm1,
                                                         const float* __restrict__ W1, const float* __restrict__ W2,
                                                         const float* __restrict__ g, float* __restrict__ xdown_bar,
                                                         float* __restrict__ sbf_bar) {
  __shared__ float s_w1[kMaxSbf * kBasisEmb];
  const int lane = threadIdx.x;
  for (int i = lane; i < nsbf * kBasisEmb; i += kWave) s_w1[i] = W1[i];
  __syncthreads();
  float w2[kBasisEmb];
#pragma unroll
  for (int k = 0; k < kBasisEmb; ++k) w2[k] = W2[k * kIntEmb + lane];
  const int64_t m = mp_xcd_block(blockIdx.x, gridDim.x);
  const float xd = xdown[m * kIntEmb + lane];
  const int32_t beg = ptr1[m], end = ptr1[m + 1];
  const int slot = lane >> 3, k = lane & 7;
  float acc = 0.0f;
  for (int32_t base = beg; base < end; base += 8) {
    const int32_t p = base + slot;
    const bool live = p < end;
    const int64_t t = live ? (perm1 ? perm1[p] : p) : 0;
    int n = live ? cols[t] : -1;
    if (n < 0 || n >= E) n = -1;
    const int ti = static_cast<int>(t);
    const float h = triplet_h(sbf, nsbf, s_w1, t, n >= 0, k);
    const int cnt = min(8, end - base);
    for (int s = 0; s < cnt; ++s) {
      const int ns = mp_bcast(n, 8 * s);
      const int64_t ts = static_cast<int64_t>(static_cast<uint32_t>(mp_bcast(ti, 8 * s)));
      const float gc = ns >= 0 ? g[static_cast<int64_t>(ns) * kIntEmb + lane] : 0.0f;
      float v = 0.0f;
#pragma unroll
      for (int q = 0; q < kBasisEmb; ++q) v += mp_bcast(h, 8 * s + q) * w2[q];
      acc += gc * v;
      if (sbf_bar) {
        const float uc = gc * xd;
        float gk[kBasisEmb];
#pragma unroll
        for (int q = 0; q < kBasisEmb; ++q) gk[q] = wave_sum(uc * w2[q]);
        if (lane < nsbf) {
          float sb = 0.0f;
#pragma unroll
          for (int q = 0; q < kBasisEmb; ++q) sb += s_w1[lane * kBasisEmb + q] * gk[q];
          sbf_bar[ts * nsbf + lane] = sb;
        }
      }
    }
  }
  if (xdown_bar) xdown_bar[m * kIntEmb + lane] = acc;
}

int check_sbf(const char* who, int64_t E, int64_t T, int L, int R, float cutoff, int exponent) {
  MP_REQUIRE(E >= 0 && T >= 0, "%s: bad sizes", who);
  MP_REQUIRE(L >= 1 && L <= MP_SBF_MAX_SPHERICAL && R >= 1 && R <= MP_SBF_MAX_RADIAL,
             "%s: num_spherical %d / num_radial %d outside [1, %d] / [1, %d]", who, L, R, MP_SBF_MAX_SPHERICAL,
             MP_SBF_MAX_RADIAL);
  MP_REQUIRE(cutoff > 0.0f && exponent >= 1 && exponent <= 32, "%s: bad cutoff / envelope exponent", who);
  return MP_OK;
}

int check_triplet(const char* who, int64_t E, int64_t T, int nsbf, int basis_emb, int int_emb) {
  MP_REQUIRE(E >= 0 && T >= 0 && E < (int64_t{1} << 31) && T < (int64_t{1} << 31), "%s: bad sizes", who);
  MP_REQUIRE(nsbf >= 1 && nsbf <= kMaxSbf && basis_emb == kBasisEmb && int_emb == kIntEmb,
             "%s: sizes (sbf %d, basis_emb %d, int_emb %d) outside the fused kernel's (<= %d, %d, %d)", who, nsbf,
             basis_emb, int_emb, kMaxSbf, kBasisEmb, kIntEmb);
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_vector_angle_f32(const float* v1, const float* v2, int64_t T, float* theta, mpStream_t stream) {
  MP_REQUIRE(T >= 0, "mp_vector_angle_f32: bad sizes");
  if (T == 0) return MP_OK;
  MP_REQUIRE(v1 && v2 && theta, "mp_vector_angle_f32: null pointer");
  vector_angle_kernel<<<mp::grid_for(T), 256, 0, mp::as_stream(stream)>>>(v1, v2, T, theta);
  return mp::check_launch("mp_vector_angle_f32");
}

int mp_vector_angle_grad_f32(const float* v1, const float* v2, int64_t T, const float* g, float* g1, float* g2,
                             mpStream_t stream) {
  MP_REQUIRE(T >= 0, "mp_vector_angle_grad_f32: bad sizes");
  if (T == 0) return MP_OK;
  MP_REQUIRE(v1 && v2 && g && (g1 || g2), "mp_vector_angle_grad_f32: null pointer");
  vector_angle_grad_kernel<<<mp::grid_for(T), 256, 0, mp::as_stream(stream)>>>(v1, v2, T, g, g1, g2);
  return mp::check_launch("mp_vector_angle_grad_f32");
}

int mp_edge_angle_f32(const float* v, int64_t E, const int32_t* cols, int64_t T, const float* scale, float* theta,
                      mpStream_t stream) {
  MP_REQUIRE(E >= 0 && T >= 0, "mp_edge_angle_f32: bad sizes");
  if (T == 0) return MP_OK;
  MP_REQUIRE(v && cols && theta, "mp_edge_angle_f32: null pointer");
  edge_angle_kernel<<<mp::grid_for(T), 256, 0, mp::as_stream(stream)>>>(v, E, cols, T, scale, theta);
  return mp::check_launch("mp_edge_angle_f32");
}

int mp_edge_angle_grad_ws_bytes(int64_t T, size_t* bytes_out_host) {
  MP_REQUIRE(T >= 0 && bytes_out_host, "mp_edge_angle_grad_ws_bytes: bad arguments");
  *bytes_out_host = sizeof(float) * 6 * static_cast<size_t>(T);
  return MP_OK;
}

int mp_edge_angle_grad_f32(const float* v, int64_t E, const int32_t* cols, int64_t T, const int32_t* ptr0,
                           const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1, const float* scale,
                           const float* g, float* ws, size_t ws_bytes, float* v_bar, mpStream_t stream) {
  MP_REQUIRE(E >= 0 && T >= 0, "mp_edge_angle_grad_f32: bad sizes");
  if (E == 0) return MP_OK;
  MP_REQUIRE(v && v_bar && ptr0 && ptr1, "mp_edge_angle_grad_f32: null pointer");
  hipStream_t s = mp::as_stream(stream);
  if (T == 0) {
    MP_HIP(hipMemsetAsync(v_bar, 0, sizeof(float) * 3 * static_cast<size_t>(E), s));
    return MP_OK;
  }
  MP_REQUIRE(cols && g, "mp_edge_angle_grad_f32: null pointer");
  const size_t need = sizeof(float) * 6 * static_cast<size_t>(T);
  MP_REQUIRE(ws && ws_bytes >= need, "mp_edge_angle_grad_f32: workspace %zu < %zu bytes", ws_bytes, need);
  edge_angle_part_kernel<<<mp::grid_for(T), 256, 0, s>>>(v, E, cols, T, scale, g, ws);
  int rc = mp::check_launch("mp_edge_angle_grad_f32");
  if (rc != MP_OK) return rc;
  edge_angle_sum_kernel<<<static_cast<unsigned>(E), 64, 0, s>>>(ws, T, ptr0, perm0, ptr1, perm1, v_bar);
  return mp::check_launch("mp_edge_angle_grad_f32");
}

int mp_spherical_basis_f32(const float* d, int64_t E, const float* theta, const int32_t* cols, int64_t T,
                           const float* tables, int num_spherical, int num_radial, float cutoff, int envelope_exponent,
                           float* rbf_env, float* sbf, mpStream_t stream) {
  int rc = check_sbf("mp_spherical_basis_f32", E, T, num_spherical, num_radial, cutoff, envelope_exponent);
  if (rc != MP_OK || E == 0) return rc;
  MP_REQUIRE(d && tables && rbf_env && (T == 0 || (theta && cols && sbf)), "mp_spherical_basis_f32: null pointer");
  hipStream_t s = mp::as_stream(stream);
  const int LR = num_spherical * num_radial;
  const int p = envelope_exponent + 1;
  sbf_edge_kernel<<<mp::grid_for(E * LR), 256, 0, s>>>(d, E, tables, num_spherical, num_radial, 1.0f / cutoff, p,
                                                         rbf_env);
  rc = mp::check_launch("mp_spherical_basis_f32");
  if (rc != MP_OK || T == 0) return rc;
  sbf_triplet_kernel<<<mp::grid_for(T * LR), 256, 0, s>>>(rbf_env, E, theta, cols, T, tables, num_spherical,
                                                            num_radial, sbf);
  return mp::check_launch("mp_spherical_basis_f32");
}

int mp_spherical_basis_grad_f32(const float* d, int64_t E, const float* theta, const int32_t* cols, int64_t T,
                                const int32_t* ptr1, const int32_t* perm1, const float* tables, int num_spherical,
                                int num_radial, float cutoff, int envelope_exponent, const float* rbf_env,
                                const float* g, float* d_bar, float* theta_bar, mpStream_t stream) {
  int rc = check_sbf("mp_spherical_basis_grad_f32", E, T, num_spherical, num_radial, cutoff, envelope_exponent);
  if (rc != MP_OK) return rc;
  hipStream_t s = mp::as_stream(stream);
  const int p = envelope_exponent + 1;
  if (d_bar && E > 0) {
    MP_REQUIRE(d && tables && ptr1 && (T == 0 || (theta && g)), "mp_spherical_basis_grad_f32: null pointer");
    sbf_dist_grad_kernel<<<static_cast<unsigned>(E), 64, 0, s>>>(d, E, theta, T, ptr1, perm1, tables, num_spherical,
                                                                 num_radial, 1.0f / cutoff, p, g, d_bar);
    rc = mp::check_launch("mp_spherical_basis_grad_f32");
    if (rc != MP_OK) return rc;
  }
  if (theta_bar && T > 0) {
    MP_REQUIRE(rbf_env && theta && cols && tables && g, "mp_spherical_basis_grad_f32: null pointer");
    sbf_theta_grad_kernel<<<mp::grid_for(T), 256, 0, s>>>(rbf_env, E, theta, cols, T, tables, num_spherical,
                                                            num_radial, g, theta_bar);
    rc = mp::check_launch("mp_spherical_basis_grad_f32");
  }
  return rc;
}

int mp_dimenet_triplet_f32(const float* xdown, int64_t E, const float* sbf, int nsbf, const int32_t* cols, int64_t T,
                           const int32_t* ptr0, const int32_t* perm0, const float* W1, int basis_emb, const float* W2,
                           int int_emb, float* out, mpStream_t stream) {
  int rc = check_triplet("mp_dimenet_triplet_f32", E, T, nsbf, basis_emb, int_emb);
  if (rc != MP_OK || E == 0) return rc;
  MP_REQUIRE(xdown && ptr0 && W1 && W2 && out && (T == 0 || (sbf && cols)), "mp_dimenet_triplet_f32: null pointer");
  triplet_fwd_kernel<<<static_cast<unsigned>(E), 64, 0, mp::as_stream(stream)>>>(xdown, E, sbf, nsbf, cols, T, ptr0,
                                                                                  perm0, W1, W2, out);
  return mp::check_launch("mp_dimenet_triplet_f32");
}

int mp_dimenet_triplet_grad_f32(const float* xdown, int64_t E, const float* sbf, int nsbf, const int32_t* cols,
                                int64_t T, const int32_t* ptr1, const int32_t* perm1, const float* W1, int basis_emb,
                                const float* W2, int int_emb, const float* g, float* xdown_bar, float* sbf_bar,
                                mpStream_t stream) {
  int rc = check_triplet("mp_dimenet_triplet_grad_f32", E, T, nsbf, basis_emb, int_emb);
  if (rc != MP_OK || E == 0) return rc;
  MP_REQUIRE(xdown && ptr1 && W1 && W2 && g && (xdown_bar || sbf_bar) && (T == 0 || (sbf && cols)),
             "mp_dimenet_triplet_grad_f32: null pointer");
  triplet_bwd_kernel<<<static_cast<unsigned>(E), 64, 0, mp::as_stream(stream)>>>(xdown, E, sbf, nsbf, cols, T, ptr1,
                                                                                  perm1, W1, W2, g, xdown_bar,
                                                                                  sbf_bar);
  return mp::check_launch("mp_dimenet_triplet_grad_f32");
}

}  // extern "C"
