// Second derivatives for training on forces (kgcnn/model/force.py:159-186 under the fork's force_schnet.py:163-205,
// where the loss holds F = -dE/dx): the loss gradient has to flow through the reverse pass itself.  Every first-order
// rule of gcnn_keras_amd/autograd.py on the SchNet force path is either linear in its upstream gradient (gather,
// segment sum, pooling, add / sub / mul, the Dense GEMMs: their reverse is another forward kernel) or an elementwise
// derivative of mp_backward.hip.  This file holds the reverse of the latter: for y = g * f'(x) and an upstream h on y,
// g_bar = h * f'(x) and x_bar = h * g * f''(x), both from one pass over the saved inputs.  Either output may be NULL.
#include "mp_common.h"
#include "../../include/mpengine/backward.h"

namespace {

// y = gy * act'(pre) (mp_activation_grad_f32, modules.py:15-90 / activ.py:15) -> pre_bar = h gy act''(pre),
// gy_bar = h act'(pre)
__global__ void activation_grad2_kernel(int act, float alpha, const float* __restrict__ pre,
                                        const float* __restrict__ gy, const float* __restrict__ h, int64_t n,
                                        float* __restrict__ pre_bar, float* __restrict__ gy_bar) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = pre[i], hv = h[i];
    if (pre_bar) pre_bar[i] = hv * gy[i] * mp_act_grad2(act, alpha, x);
    if (gy_bar) gy_bar[i] = hv * mp_act_grad(act, alpha, x);
  }
}

// gd = sum_k gy_k phi_k'(d) (mp_gauss_basis_grad_f32, geom.py:567-571), phi_k = exp(-gamma u_k^2),
// u_k = (d - offset) - mu_k:  d_bar = h sum_k gy_k phi_k''(d), phi'' = (4 gamma^2 u^2 - 2 gamma) phi;
// gy_bar_k = h phi_k'(d) = h (-2 gamma u_k) phi_k.  mu_k, gamma and the float order are those of the first-order kernel.
__global__ void gauss_grad2_kernel(const float* __restrict__ d, int64_t M, int bins, float distance, float gamma,
                                   float offset, const float* __restrict__ gy, const float* __restrict__ h,
                                   float* __restrict__ d_bar, float* __restrict__ gy_bar) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const float fbins = static_cast<float>(bins);
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < M; e += stride) {
    const float hv = h[e];
    float acc = 0.0f;
    for (int k = 0; k < bins; ++k) {
      const float mu = static_cast<float>(k) / fbins * distance;
      const float v = (d[e] - offset) - mu;
      const float phi = expf(-gamma * v * v);
      if (d_bar) acc += gy[e * bins + k] * ((4.0f * gamma * gamma * v * v - 2.0f * gamma) * phi);
      if (gy_bar) gy_bar[e * bins + k] = hv * (phi * (-2.0f * gamma * v));
    }
    if (d_bar) d_bar[e] = hv * acc;
  }
}

// gx = gy x / f on the (R, D, C) view of mp_euclidean_norm_grad_f32 (geom.py:181-193), f = sqrt(s), s = sum_d x_d^2
// (+ 1e-7 with add_eps).  For an upstream h (R, D, C) on gx:  gy_bar = (h . x) / f,
// x_bar = gy (h / f - (h . x) x / f^3).  s <= 0: zero, as the first-order kernel's sub-gradient at the cusp.
__global__ void euclidean_norm_grad2_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                            const float* __restrict__ h, int64_t R, int64_t D, int64_t C, int flags,
                                            float* __restrict__ x_bar, float* __restrict__ gy_bar) {
  const int64_t total = R * C;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const bool add_eps = flags & 2;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t c = t % C, r = t / C;
    float s = 0.0f, hx = 0.0f;
    for (int64_t d = 0; d < D; ++d) {
      const float v = x[(r * D + d) * C + c];
      s += v * v;
      hx += h[(r * D + d) * C + c] * v;
    }
    if (add_eps) s += 1e-7f;
    if (s <= 0.0f) {
      if (gy_bar) gy_bar[t] = 0.0f;
      if (x_bar)
        for (int64_t d = 0; d < D; ++d) x_bar[(r * D + d) * C + c] = 0.0f;
      continue;
    }
    const float f = sqrtf(s);
    const float inv_f = 1.0f / f;
    if (gy_bar) gy_bar[t] = hx * inv_f;
    if (x_bar) {
      const float g = gy[t];
      const float hx_f3 = hx * inv_f * inv_f * inv_f;
      for (int64_t d = 0; d < D; ++d) {
        const int64_t i = (r * D + d) * C + c;
        x_bar[i] = g * (h[i] * inv_f - hx_f3 * x[i]);
      }
    }
  }
}

}  // namespace

extern "C" {

int mp_activation_grad2_f32(int act, float act_alpha, const float* pre, const float* gy, const float* h,
                            float* pre_bar, float* gy_bar, int64_t n, mpStream_t stream) {
  MP_REQUIRE(n >= 0 && act >= MP_ACT_LINEAR && act <= MP_ACT_LAST, "mp_activation_grad2_f32: bad arguments");
  if (n == 0 || (!pre_bar && !gy_bar)) return MP_OK;
  MP_REQUIRE(pre && h && (gy || !pre_bar), "mp_activation_grad2_f32: null pointer");
  activation_grad2_kernel<<<mp::grid_for(n), 256, 0, mp::as_stream(stream)>>>(act, act_alpha, pre, gy, h, n, pre_bar,
                                                                               gy_bar);
  return mp::check_launch("mp_activation_grad2_f32");
}

int mp_gauss_basis_grad2_f32(const float* d, int64_t M, int bins, float distance, float sigma, float offset,
                             const float* gy, const float* h, float* d_bar, float* gy_bar, mpStream_t stream) {
  MP_REQUIRE(M >= 0 && bins >= 1 && sigma != 0.0f, "mp_gauss_basis_grad2_f32: bad arguments");
  if (M == 0 || (!d_bar && !gy_bar)) return MP_OK;
  MP_REQUIRE(d && h && (gy || !d_bar), "mp_gauss_basis_grad2_f32: null pointer");
  const float gamma = static_cast<float>(1.0 / static_cast<double>(sigma) / static_cast<double>(sigma) / 2.0);
  gauss_grad2_kernel<<<mp::grid_for(M), 256, 0, mp::as_stream(stream)>>>(d, M, bins, distance, gamma, offset, gy, h,
                                                                          d_bar, gy_bar);
  return mp::check_launch("mp_gauss_basis_grad2_f32");
}

int mp_euclidean_norm_grad2_f32(const float* x, const float* gy, const float* h, int64_t R, int64_t D, int64_t C,
                                int flags, float* x_bar, float* gy_bar, mpStream_t stream) {
  MP_REQUIRE(R >= 0 && D >= 1 && C >= 1, "mp_euclidean_norm_grad2_f32: bad sizes");
  MP_REQUIRE((flags & ~(2 | 4)) == 0, "mp_euclidean_norm_grad2_f32: only the plain norm (add_eps, no_nan) has a "
             "second derivative here, flags %d", flags);
  if (R == 0 || (!x_bar && !gy_bar)) return MP_OK;
  MP_REQUIRE(x && h && (gy || !x_bar), "mp_euclidean_norm_grad2_f32: null pointer");
  euclidean_norm_grad2_kernel<<<mp::grid_for(R * C), 256, 0, mp::as_stream(stream)>>>(x, gy, h, R, D, C, flags, x_bar,
                                                                                       gy_bar);
  return mp::check_launch("mp_euclidean_norm_grad2_f32");
}

}  // extern "C"
