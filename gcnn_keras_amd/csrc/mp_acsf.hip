// Atom-centred symmetry functions of HDNNP2nd (kgcnn/layers/conv/acsf_conv.py, Behler 2011):
//
//   mp_acsf_g2_f32 / _g4_f32            forward, out (N, R*m)            acsf_conv.py:158-210 / :419-494
//   mp_acsf_g2_jvp_f32 / _g4_jvp_f32    g_bar[i, rel, m] = sum dG_m/dx . (h_i, h_j[, h_k])   (forward mode)
//   mp_acsf_g2_grad_f32 / _g4_grad_f32  dx (N,3) = sum_m g[i, rel, m] dG_m/dx                 (reverse mode)
//
// Forward and JVP are receiver-parallel: one wave per receiver i walks its pairs / triplets (CSR of index column 0) in
// list order, 64 at a time.  Lane t computes the per-pair / per-triplet terms of entry t once - distances, cos theta,
// the cutoff values at the relation's first cutoff - and the wave then steps through the 64 entries; the entry's values
// are broadcast by v_readlane and lane m evaluates function m of the entry's relation.  Every output slot rel*m + mm is
// accumulated in LDS by the one lane that owns mm (mm = lane mod 64): in entry order, no atomics, same bits every run.
//
// The reverse: the receiver's row of g is staged in LDS, lane t takes entry t and sums over the functions; the
// per-endpoint coordinate partials of every entry are written to a workspace (K, M, 3), and a second kernel adds them
// per node over the CSR of each index column in list order (a fixed wave reduction per node): deterministic.
//
// Tables: params (R, m, P) or the target-set form (E, R, m, P), P = 3 (eta, rs, rc) for G2 and 4 (eta, zeta, lambda, rc)
// for G4, indexed by (zi slot, relation).  rmap (31) maps an atomic number to its element slot, pmap (31*31) a pair of
// atomic numbers to its G4 relation; -1 = no entry.  Unmapped elements contribute nothing: the reference's out-of-range
// gather of the parameters gives zeros on a GPU and its out-of-range relational scatter is dropped.
#include <math.h>

#include "mp_common.h"
#include "../../include/mpengine/hdnnp.h"

namespace {

constexpr int kMaxZ = 31;          // ACSFG2._max_atomic_number
constexpr int kAccMax = 2048;      // R*m floats of one receiver row held in LDS
constexpr int kParMax = 2048;      // parameter table floats staged in LDS (else read through L1)
constexpr float kPi = 3.14159265358979323846f;

struct AcsfArgs {
  const float* xyz;
  const int64_t* z;
  int64_t N;
  const int32_t* cols;   // (K, M) shifted index columns
  int64_t M;
  const int32_t* ptr[3];
  const int32_t* perm[3];
  const int32_t* rmap;
  const int32_t* pmap;
  const float* params;
  int nrel, nfun, ncenter;   // ncenter 0: rank-3 table
  float mult;                // 0: no multiplicity
  const float* h;            // JVP upstream (N,3)
  const float* g;            // reverse upstream (N, R*m)
  float* out;                // forward / JVP output (N, R*m)
  float* part;               // reverse partials (K, M, 3)
};

__device__ __forceinline__ int elem_slot(const int32_t* rmap, int64_t z) {
  return (z >= 0 && z < kMaxZ) ? rmap[z] : -1;
}

// kgcnn's fc with the clip (no where): 0.5 (cos(pi clip(r, -rc, rc) / rc) + 1), and its derivative (zero outside the clip)
__device__ __forceinline__ float fc_of(float r, float rc) {
  const float c = fminf(fmaxf(r, -rc), rc);
  return (cosf(c * kPi / rc) + 1.0f) * 0.5f;
}
__device__ __forceinline__ float dfc_of(float r, float rc) {
  if (!(r >= -rc && r <= rc)) return 0.0f;
  return -0.5f * sinf(r * kPi / rc) * (kPi / rc);
}

// relation of entry e and its neighbour indices; -1 when an endpoint is out of range or unmapped
template <bool G4>
__device__ __forceinline__ int entry_rel(const AcsfArgs& a, int64_t e, int& j, int& k) {
  j = a.cols[a.M + e];
  k = G4 ? a.cols[2 * a.M + e] : 0;
  if (j < 0 || j >= a.N || k < 0 || k >= a.N) return -1;
  int rel;
  if (G4) {
    const int64_t zj = a.z[j], zk = a.z[k];
    rel = (zj >= 0 && zj < kMaxZ && zk >= 0 && zk < kMaxZ) ? a.pmap[zj * kMaxZ + zk] : -1;
  } else {
    rel = elem_slot(a.rmap, a.z[j]);
  }
  return (rel >= 0 && rel < a.nrel) ? rel : -1;
}

__device__ __forceinline__ float dist3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// Stage the parameter table in LDS when it fits; returns the pointer the kernel reads it through.
template <int P>
__device__ const float* stage_params(const AcsfArgs& a, float* s_par) {
  const int64_t table = static_cast<int64_t>(a.ncenter ? a.ncenter : 1) * a.nrel * a.nfun * P;
  if (table > kParMax) return a.params;
  for (int64_t t = threadIdx.x; t < table; t += blockDim.x) s_par[t] = a.params[t];
  __syncthreads();
  return s_par;
}

// ------------------------------------------------------------------ forward / JVP: one wave (block) per receiver
template <bool G4, bool JVP>
__global__ __launch_bounds__(64) void acsf_rows_kernel(AcsfArgs a) {
  constexpr int P = G4 ? 4 : 3;
  __shared__ float s_acc[kAccMax];
  __shared__ float s_par[kParMax];
  const float* par = stage_params<P>(a, s_par);
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int nfun = a.nfun, width = a.nrel * nfun;
  for (int rel = 0; rel < a.nrel; ++rel)
    for (int mm = lane; mm < nfun; mm += 64) s_acc[rel * nfun + mm] = 0.0f;
  int crow = 0;
  bool ok = true;
  if (a.ncenter) {
    const int c = elem_slot(a.rmap, a.z[i]);
    ok = c >= 0 && c < a.ncenter;
    crow = ok ? c * a.nrel : 0;
  }
  const float xi0 = a.xyz[3 * i], xi1 = a.xyz[3 * i + 1], xi2 = a.xyz[3 * i + 2];
  float hi0 = 0.f, hi1 = 0.f, hi2 = 0.f;
  if (JVP) { hi0 = a.h[3 * i]; hi1 = a.h[3 * i + 1]; hi2 = a.h[3 * i + 2]; }
  const int32_t beg = a.ptr[0][i], end = ok ? a.ptr[0][i + 1] : beg;
  for (int32_t base = beg; base < end; base += 64) {
    const int32_t p = base + lane;
    int rel = -1;
    float rij = 1.f, rik = 1.f, rjk = 1.f, cs = 0.f, rc0 = 0.f, fij = 0.f, fik = 0.f, fjk = 0.f;
    float drij = 0.f, drik = 0.f, drjk = 0.f, dcs = 0.f;
    if (p < end) {
      const int64_t e = a.perm[0] ? a.perm[0][p] : p;
      int j, k;
      rel = entry_rel<G4>(a, e, j, k);
      if (rel >= 0) {
        const float vij0 = xi0 - a.xyz[3 * j], vij1 = xi1 - a.xyz[3 * j + 1], vij2 = xi2 - a.xyz[3 * j + 2];
        rij = dist3(vij0, vij1, vij2);
        rc0 = par[((crow + rel) * nfun) * P + (P - 1)];
        fij = fc_of(rij, rc0);
        float hij0 = 0.f, hij1 = 0.f, hij2 = 0.f;
        if (JVP) {
          hij0 = hi0 - a.h[3 * j]; hij1 = hi1 - a.h[3 * j + 1]; hij2 = hi2 - a.h[3 * j + 2];
          drij = (vij0 * hij0 + vij1 * hij1 + vij2 * hij2) / rij;
        }
        if (G4) {
          const float vik0 = xi0 - a.xyz[3 * k], vik1 = xi1 - a.xyz[3 * k + 1], vik2 = xi2 - a.xyz[3 * k + 2];
          const float vjk0 = vik0 - vij0, vjk1 = vik1 - vij1, vjk2 = vik2 - vij2;   // x_j - x_k
          rik = dist3(vik0, vik1, vik2);
          rjk = dist3(vjk0, vjk1, vjk2);
          cs = (vij0 * vik0 + vij1 * vik1 + vij2 * vik2) / rij / rik;
          fik = fc_of(rik, rc0);
          fjk = fc_of(rjk, rc0);
          if (JVP) {
            const float hik0 = hi0 - a.h[3 * k], hik1 = hi1 - a.h[3 * k + 1], hik2 = hi2 - a.h[3 * k + 2];
            const float hjk0 = hik0 - hij0, hjk1 = hik1 - hij1, hjk2 = hik2 - hij2;
            drik = (vik0 * hik0 + vik1 * hik1 + vik2 * hik2) / rik;
            drjk = (vjk0 * hjk0 + vjk1 * hjk1 + vjk2 * hjk2) / rjk;
            // d cos = (dcos/dv_ij) . h_ij + (dcos/dv_ik) . h_ik
            const float inv = 1.0f / (rij * rik);
            dcs = (vik0 * hij0 + vik1 * hij1 + vik2 * hij2 + vij0 * hik0 + vij1 * hik1 + vij2 * hik2) * inv -
                  cs * ((vij0 * hij0 + vij1 * hij1 + vij2 * hij2) / (rij * rij) +
                        (vik0 * hik0 + vik1 * hik1 + vik2 * hik2) / (rik * rik));
          }
        }
      }
    }
    const int cnt = min(64, end - base);
    for (int s = 0; s < cnt; ++s) {
      const int r = mp_bcast(rel, s);
      if (r < 0) continue;
      const float Rij = mp_bcast(rij, s), Rc0 = mp_bcast(rc0, s), Fij0 = mp_bcast(fij, s);
      const float Rik = G4 ? mp_bcast(rik, s) : 0.f, Rjk = G4 ? mp_bcast(rjk, s) : 0.f, Cs = G4 ? mp_bcast(cs, s) : 0.f;
      const float Fik0 = G4 ? mp_bcast(fik, s) : 0.f, Fjk0 = G4 ? mp_bcast(fjk, s) : 0.f;
      const float dRij = JVP ? mp_bcast(drij, s) : 0.f;
      const float dRik = (JVP && G4) ? mp_bcast(drik, s) : 0.f, dRjk = (JVP && G4) ? mp_bcast(drjk, s) : 0.f;
      const float dCs = (JVP && G4) ? mp_bcast(dcs, s) : 0.f;
      const float* prow = par + static_cast<int64_t>(crow + r) * nfun * P;
      for (int mm = lane; mm < nfun; mm += 64) {
        const float eta = prow[mm * P], rc = prow[mm * P + P - 1];
        const bool same = rc == Rc0;
        const float Fij = same ? Fij0 : fc_of(Rij, rc);
        float val;
        if constexpr (!G4) {
          const float rs = prow[mm * P + 1];
          const float u = Rij - rs;
          const float gs = expf(-(u * u * eta));
          if (JVP) {
            val = (gs * (-2.0f * eta * u) * Fij + gs * dfc_of(Rij, rc)) * dRij;
          } else {
            val = gs * Fij;
          }
        } else {
          const float zeta = prow[mm * P + 1], lam = prow[mm * P + 2];
          const float Fik = same ? Fik0 : fc_of(Rik, rc), Fjk = same ? Fjk0 : fc_of(Rjk, rc);
          const float b = Cs * lam + 1.0f;
          float A = exp2f(1.0f - zeta) * powf(b, zeta);
          if (a.mult != 0.0f) A = A / a.mult;
          const float E = expf(-(Rij * Rij * eta)) * expf(-(Rik * Rik * eta)) * expf(-(Rjk * Rjk * eta));
          const float F = Fij * Fik * Fjk;
          if (JVP) {
            float dA = exp2f(1.0f - zeta) * zeta * powf(b, zeta - 1.0f) * lam;
            if (a.mult != 0.0f) dA = dA / a.mult;
            const float dF = dfc_of(Rij, rc) * Fik * Fjk * dRij + Fij * dfc_of(Rik, rc) * Fjk * dRik +
                             Fij * Fik * dfc_of(Rjk, rc) * dRjk;
            const float dE = -2.0f * eta * (Rij * dRij + Rik * dRik + Rjk * dRjk) * E;
            val = dA * dCs * E * F + A * (dE * F + E * dF);
          } else {
            val = A * E * F;
          }
        }
        s_acc[r * nfun + mm] += val;
      }
    }
  }
  float* orow = a.out + i * width;
  for (int rel = 0; rel < a.nrel; ++rel)
    for (int mm = lane; mm < nfun; mm += 64) orow[rel * nfun + mm] = s_acc[rel * nfun + mm];
}

// ------------------------------------------------------------------ reverse: per-entry endpoint partials
template <bool G4>
__global__ __launch_bounds__(64) void acsf_grad_entries_kernel(AcsfArgs a) {
  constexpr int P = G4 ? 4 : 3;
  constexpr int K = G4 ? 3 : 2;
  __shared__ float s_g[kAccMax];
  __shared__ float s_par[kParMax];
  const float* par = stage_params<P>(a, s_par);
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int nfun = a.nfun, width = a.nrel * nfun;
  for (int t = lane; t < width; t += 64) s_g[t] = a.g[i * width + t];
  __syncthreads();
  int crow = 0;
  bool ok = true;
  if (a.ncenter) {
    const int c = elem_slot(a.rmap, a.z[i]);
    ok = c >= 0 && c < a.ncenter;
    crow = ok ? c * a.nrel : 0;
  }
  const float xi0 = a.xyz[3 * i], xi1 = a.xyz[3 * i + 1], xi2 = a.xyz[3 * i + 2];
  const int32_t beg = a.ptr[0][i], end = a.ptr[0][i + 1];
  for (int32_t p = beg + lane; p < end; p += 64) {
    const int64_t e = a.perm[0] ? a.perm[0][p] : p;
    float d[K][3];
#pragma unroll
    for (int c = 0; c < K; ++c) d[c][0] = d[c][1] = d[c][2] = 0.0f;
    int j, k;
    const int rel = ok ? entry_rel<G4>(a, e, j, k) : -1;
    if (rel >= 0) {
      const float* prow = par + static_cast<int64_t>(crow + rel) * nfun * P;
      const float* grow = s_g + rel * nfun;
      const float vij0 = xi0 - a.xyz[3 * j], vij1 = xi1 - a.xyz[3 * j + 1], vij2 = xi2 - a.xyz[3 * j + 2];
      const float rij = dist3(vij0, vij1, vij2);
      if constexpr (!G4) {
        float c_ij = 0.0f;
        for (int mm = 0; mm < nfun; ++mm) {
          const float eta = prow[mm * P], rs = prow[mm * P + 1], rc = prow[mm * P + 2];
          const float u = rij - rs;
          const float gs = expf(-(u * u * eta));
          c_ij += grow[mm] * (gs * (-2.0f * eta * u) * fc_of(rij, rc) + gs * dfc_of(rij, rc));
        }
        const float s = c_ij / rij;
        d[0][0] = s * vij0; d[0][1] = s * vij1; d[0][2] = s * vij2;
        d[1][0] = -d[0][0]; d[1][1] = -d[0][1]; d[1][2] = -d[0][2];
      } else {
        const float vik0 = xi0 - a.xyz[3 * k], vik1 = xi1 - a.xyz[3 * k + 1], vik2 = xi2 - a.xyz[3 * k + 2];
        const float vjk0 = vik0 - vij0, vjk1 = vik1 - vij1, vjk2 = vik2 - vij2;
        const float rik = dist3(vik0, vik1, vik2), rjk = dist3(vjk0, vjk1, vjk2);
        const float cs = (vij0 * vik0 + vij1 * vik1 + vij2 * vik2) / rij / rik;
        const float rc0 = prow[P - 1];
        const float fij0 = fc_of(rij, rc0), fik0 = fc_of(rik, rc0), fjk0 = fc_of(rjk, rc0);
        const float dij0 = dfc_of(rij, rc0), dik0 = dfc_of(rik, rc0), djk0 = dfc_of(rjk, rc0);
        float c_cos = 0.f, c_ij = 0.f, c_ik = 0.f, c_jk = 0.f;
        for (int mm = 0; mm < nfun; ++mm) {
          const float eta = prow[mm * P], zeta = prow[mm * P + 1], lam = prow[mm * P + 2], rc = prow[mm * P + 3];
          const bool same = rc == rc0;
          const float fij = same ? fij0 : fc_of(rij, rc), fik = same ? fik0 : fc_of(rik, rc);
          const float fjk = same ? fjk0 : fc_of(rjk, rc);
          const float dij = same ? dij0 : dfc_of(rij, rc), dik = same ? dik0 : dfc_of(rik, rc);
          const float djk = same ? djk0 : dfc_of(rjk, rc);
          const float b = cs * lam + 1.0f;
          const float sc = exp2f(1.0f - zeta);
          float A = sc * powf(b, zeta), dA = sc * zeta * powf(b, zeta - 1.0f) * lam;
          if (a.mult != 0.0f) { A = A / a.mult; dA = dA / a.mult; }
          const float E = expf(-(rij * rij * eta)) * expf(-(rik * rik * eta)) * expf(-(rjk * rjk * eta));
          const float F = fij * fik * fjk;
          const float gm = grow[mm];
          c_cos += gm * dA * E * F;
          const float ge = gm * A * E;
          c_ij += ge * (-2.0f * eta * rij * F + dij * fik * fjk);
          c_ik += ge * (-2.0f * eta * rik * F + fij * dik * fjk);
          c_jk += ge * (-2.0f * eta * rjk * F + fij * fik * djk);
        }
        const float inv = 1.0f / (rij * rik), cij2 = cs / (rij * rij), cik2 = cs / (rik * rik);
        const float sij = c_ij / rij, sik = c_ik / rik, sjk = c_jk / rjk;
        const float vij[3] = {vij0, vij1, vij2}, vik[3] = {vik0, vik1, vik2}, vjk[3] = {vjk0, vjk1, vjk2};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float gij = c_cos * (vik[q] * inv - cij2 * vij[q]) + sij * vij[q];
          const float gik = c_cos * (vij[q] * inv - cik2 * vik[q]) + sik * vik[q];
          const float gjk = sjk * vjk[q];
          d[0][q] = gij + gik;
          d[1][q] = gjk - gij;
          d[2][q] = -gik - gjk;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
      float* dst = a.part + (c * a.M + e) * 3;
      dst[0] = d[c][0]; dst[1] = d[c][1]; dst[2] = d[c][2];
    }
  }
}

// dx[n] = sum over index columns c, over entries e with cols[c][e] = n (CSR order) of part[c][e]; one wave per node,
// lane-strided partial sums and a fixed butterfly: the same bits every run.
__global__ __launch_bounds__(64) void acsf_endpoint_sum_kernel(AcsfArgs a, int K, float* dx) {
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int c = 0; c < K; ++c) {
    const int32_t beg = a.ptr[c][n], end = a.ptr[c][n + 1];
    const int32_t* perm = a.perm[c];
    for (int32_t t = beg + lane; t < end; t += 64) {
      const int64_t e = perm ? perm[t] : t;
      const float* src = a.part + (c * a.M + e) * 3;
      s0 += src[0]; s1 += src[1]; s2 += src[2];
    }
  }
  s0 = mp_wave_sum(s0); s1 = mp_wave_sum(s1); s2 = mp_wave_sum(s2);
  if (lane == 0) {
    dx[3 * n] = s0; dx[3 * n + 1] = s1; dx[3 * n + 2] = s2;
  }
}

int check_common(const char* who, const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                 const int32_t* ptr0, const int32_t* rmap, const float* params, int nrel, int nfun, int ncenter) {
  MP_REQUIRE(N >= 0 && M >= 0 && nrel >= 1 && nfun >= 1 && ncenter >= 0, "%s: bad sizes", who);
  MP_REQUIRE(static_cast<int64_t>(nrel) * nfun <= kAccMax, "%s: R*m = %d exceeds %d", who, nrel * nfun, kAccMax);
  if (N == 0) return MP_OK;
  MP_REQUIRE(xyz && z && ptr0 && rmap && params && (cols || M == 0), "%s: null pointer", who);
  return MP_OK;
}

AcsfArgs make_args(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M, const int32_t* rmap,
                   const int32_t* pmap, const float* params, int nrel, int nfun, int ncenter, float mult) {
  AcsfArgs a{};
  a.xyz = xyz; a.z = z; a.N = N; a.cols = cols; a.M = M; a.rmap = rmap; a.pmap = pmap; a.params = params;
  a.nrel = nrel; a.nfun = nfun; a.ncenter = ncenter; a.mult = mult;
  return a;
}

template <bool G4, bool JVP>
int launch_rows(const char* who, AcsfArgs a, mpStream_t stream) {
  acsf_rows_kernel<G4, JVP><<<static_cast<unsigned>(a.N), 64, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch(who);
}

template <bool G4>
int launch_grad(const char* who, AcsfArgs a, float* ws, size_t ws_bytes, float* dx, mpStream_t stream) {
  constexpr int K = G4 ? 3 : 2;
  hipStream_t s = mp::as_stream(stream);
  if (a.M == 0) {
    MP_HIP(hipMemsetAsync(dx, 0, sizeof(float) * 3 * static_cast<size_t>(a.N), s));
    return MP_OK;
  }
  const size_t need = sizeof(float) * 3 * K * static_cast<size_t>(a.M);
  MP_REQUIRE(ws && ws_bytes >= need, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
  a.part = ws;
  acsf_grad_entries_kernel<G4><<<static_cast<unsigned>(a.N), 64, 0, s>>>(a);
  int rc = mp::check_launch(who);
  if (rc != MP_OK) return rc;
  acsf_endpoint_sum_kernel<<<static_cast<unsigned>(a.N), 64, 0, s>>>(a, K, dx);
  return mp::check_launch(who);
}

}  // namespace

extern "C" {

int mp_acsf_grad_ws_bytes(int64_t M, int K, size_t* bytes_out_host) {
  MP_REQUIRE(M >= 0 && (K == 2 || K == 3) && bytes_out_host, "mp_acsf_grad_ws_bytes: bad arguments");
  *bytes_out_host = sizeof(float) * 3 * static_cast<size_t>(K) * static_cast<size_t>(M);
  return MP_OK;
}

int mp_acsf_g2_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0,
                   const int32_t* perm0, const int32_t* rmap, const float* params, int nrel, int nfun, int ncenter,
                   float* out, mpStream_t stream) {
  int rc = check_common("mp_acsf_g2_f32", xyz, z, N, cols, M, ptr0, rmap, params, nrel, nfun, ncenter);
  if (rc != MP_OK || N == 0) return rc;
  MP_REQUIRE(out, "mp_acsf_g2_f32: null output");
  AcsfArgs a = make_args(xyz, z, N, cols, M, rmap, nullptr, params, nrel, nfun, ncenter, 0.0f);
  a.ptr[0] = ptr0; a.perm[0] = perm0; a.out = out;
  return launch_rows<false, false>("mp_acsf_g2_f32", a, stream);
}

int mp_acsf_g4_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0,
                   const int32_t* perm0, const int32_t* rmap, const int32_t* pmap, const float* params, int nrel,
                   int nfun, int ncenter, float multiplicity, float* out, mpStream_t stream) {
  int rc = check_common("mp_acsf_g4_f32", xyz, z, N, cols, M, ptr0, rmap, params, nrel, nfun, ncenter);
  if (rc != MP_OK || N == 0) return rc;
  MP_REQUIRE(out && pmap, "mp_acsf_g4_f32: null pointer");
  AcsfArgs a = make_args(xyz, z, N, cols, M, rmap, pmap, params, nrel, nfun, ncenter, multiplicity);
  a.ptr[0] = ptr0; a.perm[0] = perm0; a.out = out;
  return launch_rows<true, false>("mp_acsf_g4_f32", a, stream);
}

int mp_acsf_g2_jvp_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                       const int32_t* ptr0, const int32_t* perm0, const int32_t* rmap, const float* params, int nrel,
                       int nfun, int ncenter, const float* h, float* g_bar, mpStream_t stream) {
  int rc = check_common("mp_acsf_g2_jvp_f32", xyz, z, N, cols, M, ptr0, rmap, params, nrel, nfun, ncenter);
  if (rc != MP_OK || N == 0) return rc;
  MP_REQUIRE(h && g_bar, "mp_acsf_g2_jvp_f32: null pointer");
  AcsfArgs a = make_args(xyz, z, N, cols, M, rmap, nullptr, params, nrel, nfun, ncenter, 0.0f);
  a.ptr[0] = ptr0; a.perm[0] = perm0; a.h = h; a.out = g_bar;
  return launch_rows<false, true>("mp_acsf_g2_jvp_f32", a, stream);
}

int mp_acsf_g4_jvp_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                       const int32_t* ptr0, const int32_t* perm0, const int32_t* rmap, const int32_t* pmap,
                       const float* params, int nrel, int nfun, int ncenter, float multiplicity, const float* h,
                       float* g_bar, mpStream_t stream) {
  int rc = check_common("mp_acsf_g4_jvp_f32", xyz, z, N, cols, M, ptr0, rmap, params, nrel, nfun, ncenter);
  if (rc != MP_OK || N == 0) return rc;
  MP_REQUIRE(pmap && h && g_bar, "mp_acsf_g4_jvp_f32: null pointer");
  AcsfArgs a = make_args(xyz, z, N, cols, M, rmap, pmap, params, nrel, nfun, ncenter, multiplicity);
  a.ptr[0] = ptr0; a.perm[0] = perm0; a.h = h; a.out = g_bar;
  return launch_rows<true, true>("mp_acsf_g4_jvp_f32", a, stream);
}

int mp_acsf_g2_grad_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                        const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                        const int32_t* rmap, const float* params, int nrel, int nfun, int ncenter, const float* g,
                        float* ws, size_t ws_bytes, float* dx, mpStream_t stream) {
  int rc = check_common("mp_acsf_g2_grad_f32", xyz, z, N, cols, M, ptr0, rmap, params, nrel, nfun, ncenter);
  if (rc != MP_OK || N == 0) return rc;
  MP_REQUIRE(g && dx && ptr1, "mp_acsf_g2_grad_f32: null pointer");
  AcsfArgs a = make_args(xyz, z, N, cols, M, rmap, nullptr, params, nrel, nfun, ncenter, 0.0f);
  a.ptr[0] = ptr0; a.perm[0] = perm0; a.ptr[1] = ptr1; a.perm[1] = perm1; a.g = g;
  return launch_grad<false>("mp_acsf_g2_grad_f32", a, ws, ws_bytes, dx, stream);
}

int mp_acsf_g4_grad_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                        const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                        const int32_t* ptr2, const int32_t* perm2, const int32_t* rmap, const int32_t* pmap,
                        const float* params, int nrel, int nfun, int ncenter, float multiplicity, const float* g,
                        float* ws, size_t ws_bytes, float* dx, mpStream_t stream) {
  int rc = check_common("mp_acsf_g4_grad_f32", xyz, z, N, cols, M, ptr0, rmap, params, nrel, nfun, ncenter);
  if (rc != MP_OK || N == 0) return rc;
  MP_REQUIRE(pmap && g && dx && ptr1 && ptr2, "mp_acsf_g4_grad_f32: null pointer");
  AcsfArgs a = make_args(xyz, z, N, cols, M, rmap, pmap, params, nrel, nfun, ncenter, multiplicity);
  a.ptr[0] = ptr0; a.perm[0] = perm0; a.ptr[1] = ptr1; a.perm[1] = perm1; a.ptr[2] = ptr2; a.perm[2] = perm2;
  a.g = g;
  return launch_grad<true>("mp_acsf_g4_grad_f32", a, ws, ws_bytes, dx, stream);
}

}  // extern "C"
