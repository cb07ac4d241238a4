// Charge equilibration and Gaussian-charge electrostatics of HDNNP4th (kgcnn/layers/conv/hdnnp_conv.py, Ko et al. 2021):
//
//   mp_cent_charge_f32        q (N): Q of [[A, 1], [1^T, 0]] [Q; lambda] = [chi; Qtot], one system per molecule  :148-258
//   mp_cent_charge_grad_f32   chi_bar (N), x_bar (N,3) of an upstream gQ (N)
//   mp_gauss_energy_f32       E (G) = sum over range_indices of q_i q_j f_ij / mult + sum_i q_i^2 / (2 sqrt(pi) sigma_i)  :391-428
//   mp_gauss_energy_grad_f32  q_bar (N), x_bar (N,3) of an upstream gE (G)
//
// A_ii = J[z_i] + 1 / (sigma[z_i] sqrt(pi)); A_ij = f(r_ij) = erf(r_ij / (sqrt(2) gamma_ij)) / r_ij over ALL atom pairs of
// the molecule, gamma_ij = sqrt(sigma_i^2 + sigma_j^2), and f = 0 where the reference's divide_no_nan gives 0 (r = 0 or
// gamma = 0).  A is the Coulomb Gram matrix of the Gaussian charge densities plus a positive hardness diagonal, so it is
// symmetric positive definite for distinct atom positions: the solve is a Cholesky factorisation plus the Schur complement
// of the border, u = A^-1 1, v = A^-1 chi, lambda = (1^T v - Qtot) / (1^T u), Q = v - lambda u.
//
// Solve: one wave per molecule.  The lower triangle of A (n <= MP_CENT_MAX_ATOMS = 128 atoms: 8256 doubles, 66 KB) is built
// from the coordinates and the tables in LDS and factored in place in FP64, right-looking: column k is divided by its pivot
// and the trailing triangle is updated one column per lane.  Both right-hand sides share the forward and back substitution.
// Every LDS word is written by one lane in a fixed order and every sum is a lane-strided partial followed by a fixed
// butterfly: the same bits every run, no atomics.  A non-positive (or NaN) pivot ends the factorisation: that molecule's
// outputs are NaN.  The reverse refactors A (no workspace), solves A [u, y] = [1, gQ], mu = 1^T y / 1^T u, w = y - mu u
// (the adjoint of the bordered system), chi_bar = w and x_bar_i = -sum_{j != i} (w_i Q_j + w_j Q_i) f'(r_ij) (x_i - x_j) /
// r_ij, one lane per atom walking j in order.
//
// Electrostatic energy: one wave per molecule over its range_indices (edge row splits) and its atoms, accumulated in FP64 and
// reduced by a fixed butterfly.  Its reverse is one wave per molecule, one lane per atom walking the CSR of index column 0
// and then of column 1 in list order (each pair term is evaluated once per endpoint): deterministic without a workspace.
// Atomic numbers outside [0, ntab) read sigma = J = 0, as the reference's out-of-range gather does on a GPU.
#include <math.h>

#include "mp_common.h"
#include "../../include/mpengine/hdnnp.h"

namespace {

constexpr int kMaxAtoms = MP_CENT_MAX_ATOMS;
constexpr int kTri = kMaxAtoms * (kMaxAtoms + 1) / 2;
constexpr double kSqrtPi = 1.7724538509055160273;
constexpr double kTwoOverSqrtPi = 1.1283791670955125739;
constexpr double kSqrt2 = 1.4142135623730950488;

struct CentArgs {
  const float* xyz;
  const int64_t* z;
  const int64_t* node_splits;
  const float* rhs;        // forward: chi; reverse: gQ
  const float* qtot;       // forward only
  const float* q;          // reverse only: the forward's charges
  const float* sigma;
  const float* hardness;
  int ntab;
  float* q_out;
  float* chi_bar;
  float* x_bar;
};

struct GaussArgs {
  const float* xyz;
  const int64_t* z;
  const float* q;
  const int64_t* node_splits;
  int64_t N;
  const int32_t* cols;     // (2, M) shifted index columns
  int64_t M;
  const int64_t* edge_splits;
  const int32_t* ptr0;
  const int32_t* perm0;
  const int32_t* ptr1;
  const int32_t* perm1;
  const float* sigma;
  int ntab;
  float mult;              // 0: no division
  const float* g_energy;
  float* energy;
  float* q_bar;
  float* x_bar;
};

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // j <= i

__device__ __forceinline__ float table_at(const float* t, int ntab, int64_t z) {
  return (z >= 0 && z < ntab) ? t[z] : 0.0f;
}

// f(r) = erf(r / (sqrt(2) gamma)) / r and df/dr; both 0 where divide_no_nan gives 0
__device__ __forceinline__ double pair_f(double r, double gamma) {
  if (r == 0.0 || gamma == 0.0) return 0.0;
  return erf(r / (kSqrt2 * gamma)) / r;
}
__device__ __forceinline__ double pair_df(double r, double gamma) {
  if (r == 0.0 || gamma == 0.0) return 0.0;
  const double a = 1.0 / (kSqrt2 * gamma);
  return (kTwoOverSqrtPi * a * exp(-(a * r) * (a * r)) * r - erf(a * r)) / (r * r);
}

template <bool REVERSE>
__device__ void cent_write_nan(const CentArgs& a, int64_t base, int n) {
  const float qnan = __int_as_float(0x7fc00000);
  for (int i = threadIdx.x; i < n; i += 64) {
    if (!REVERSE) a.q_out[base + i] = qnan;
    if (REVERSE && a.chi_bar) a.chi_bar[base + i] = qnan;
    if (REVERSE && a.x_bar) {
      a.x_bar[3 * (base + i)] = qnan;
      a.x_bar[3 * (base + i) + 1] = qnan;
      a.x_bar[3 * (base + i) + 2] = qnan;
    }
  }
}

// ------------------------------------------------------------------ charge solve: one wave per molecule
template <bool REVERSE>
__global__ __launch_bounds__(64) void cent_solve_kernel(CentArgs a) {
  __shared__ double s_a[kTri];             // lower triangle of A, factored in place into L (pivots in s_ld)
  __shared__ double s_ld[kMaxAtoms];
  __shared__ double s_x[kMaxAtoms * 3];
  __shared__ double s_sig[kMaxAtoms];
  __shared__ double s_u[kMaxAtoms];        // rhs 1   -> u = A^-1 1
  __shared__ double s_v[kMaxAtoms];        // rhs chi -> v = A^-1 chi   (reverse: gQ -> A^-1 gQ -> w)
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int64_t base = a.node_splits[g];
  const int64_t n64 = a.node_splits[g + 1] - base;
  if (n64 <= 0) return;
  if (n64 > kMaxAtoms) {   // rejected by the caller before any launch; never index past the LDS arrays
    cent_write_nan<REVERSE>(a, base, static_cast<int>(n64));
    return;
  }
  const int n = static_cast<int>(n64);
  for (int i = lane; i < n; i += 64) {
    const int64_t zi = a.z[base + i];
    const double sg = table_at(a.sigma, a.ntab, zi);
    s_sig[i] = sg;
    s_x[3 * i] = a.xyz[3 * (base + i)];
    s_x[3 * i + 1] = a.xyz[3 * (base + i) + 1];
    s_x[3 * i + 2] = a.xyz[3 * (base + i) + 2];
    s_a[tri(i, i)] = static_cast<double>(table_at(a.hardness, a.ntab, zi)) + 1.0 / sg / kSqrtPi;
    s_u[i] = 1.0;
    s_v[i] = a.rhs[base + i];
  }
  __syncthreads();
  for (int i = 1; i < n; ++i) {
    for (int j = lane; j < i; j += 64) {
      const double d0 = s_x[3 * i] - s_x[3 * j], d1 = s_x[3 * i + 1] - s_x[3 * j + 1];
      const double d2 = s_x[3 * i + 2] - s_x[3 * j + 2];
      const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      s_a[tri(i, j)] = pair_f(r, sqrt(s_sig[i] * s_sig[i] + s_sig[j] * s_sig[j]));
    }
  }
  __syncthreads();

  // Cholesky A = L L^T, right-looking; the break is uniform (every lane reads the same pivot after a barrier)
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    const double d = s_a[tri(k, k)];
    if (!(d > 0.0)) { ok = false; break; }
    const double lkk = sqrt(d);
    if (lane == 0) s_ld[k] = lkk;
    for (int i = k + 1 + lane; i < n; i += 64) s_a[tri(i, k)] /= lkk;
    __syncthreads();
    for (int j = k + 1 + lane; j < n; j += 64) {
      const double ljk = s_a[tri(j, k)];
      for (int i = j; i < n; ++i) s_a[tri(i, j)] -= s_a[tri(i, k)] * ljk;
    }
    __syncthreads();
  }
  if (!ok) {
    cent_write_nan<REVERSE>(a, base, n);
    return;
  }

  // L y = b, then L^T x = y, for both right-hand sides
  for (int k = 0; k < n; ++k) {
    const double lkk = s_ld[k];
    const double y0 = s_u[k] / lkk, y1 = s_v[k] / lkk;
    __syncthreads();
    if (lane == 0) { s_u[k] = y0; s_v[k] = y1; }
    for (int i = k + 1 + lane; i < n; i += 64) {
      const double l = s_a[tri(i, k)];
      s_u[i] -= l * y0;
      s_v[i] -= l * y1;
    }
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {
    const double lkk = s_ld[k];
    const double x0 = s_u[k] / lkk, x1 = s_v[k] / lkk;
    __syncthreads();
    if (lane == 0) { s_u[k] = x0; s_v[k] = x1; }
    for (int i = lane; i < k; i += 64) {
      const double l = s_a[tri(k, i)];
      s_u[i] -= l * x0;
      s_v[i] -= l * x1;
    }
    __syncthreads();
  }

  double su = 0.0, sv = 0.0;
  for (int i = lane; i < n; i += 64) { su += s_u[i]; sv += s_v[i]; }
  su = mp_wave_sum(su);
  sv = mp_wave_sum(sv);
  if (!REVERSE) {
    const double lam = (sv - static_cast<double>(a.qtot[g])) / su;
    for (int i = lane; i < n; i += 64) a.q_out[base + i] = static_cast<float>(s_v[i] - lam * s_u[i]);
    return;
  }
  const double mu = sv / su;
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const double w = s_v[i] - mu * s_u[i];
    s_v[i] = w;
    s_u[i] = a.q[base + i];        // u is spent: the forward's charges take its place
    if (a.chi_bar) a.chi_bar[base + i] = static_cast<float>(w);
  }
  if (!a.x_bar) return;
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const double wi = s_v[i], qi = s_u[i], si = s_sig[i];
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double d0 = s_x[3 * i] - s_x[3 * j], d1 = s_x[3 * i + 1] - s_x[3 * j + 1];
      const double d2 = s_x[3 * i + 2] - s_x[3 * j + 2];
      const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      const double df = pair_df(r, sqrt(si * si + s_sig[j] * s_sig[j]));
      if (df == 0.0) continue;
      const double c = -(wi * s_u[j] + s_v[j] * qi) * df / r;
      b0 += c * d0;
      b1 += c * d1;
      b2 += c * d2;
    }
    a.x_bar[3 * (base + i)] = static_cast<float>(b0);
    a.x_bar[3 * (base + i) + 1] = static_cast<float>(b1);
    a.x_bar[3 * (base + i) + 2] = static_cast<float>(b2);
  }
}

// ------------------------------------------------------------------ electrostatic energy: one wave per molecule
__device__ __forceinline__ bool in_range(int32_t v, int64_t N) { return v >= 0 && v < N; }

__device__ __forceinline__ double atom_sigma(const GaussArgs& a, int64_t i) {
  return table_at(a.sigma, a.ntab, a.z[i]);
}

__global__ __launch_bounds__(64) void gauss_energy_kernel(GaussArgs a) {
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  double pair = 0.0, self = 0.0;
  for (int64_t e = a.edge_splits[g] + lane; e < a.edge_splits[g + 1]; e += 64) {
    const int32_t i = a.cols[e], j = a.cols[a.M + e];
    if (!in_range(i, a.N) || !in_range(j, a.N)) continue;
    const double d0 = static_cast<double>(a.xyz[3 * i]) - a.xyz[3 * j];
    const double d1 = static_cast<double>(a.xyz[3 * i + 1]) - a.xyz[3 * j + 1];
    const double d2 = static_cast<double>(a.xyz[3 * i + 2]) - a.xyz[3 * j + 2];
    const double si = atom_sigma(a, i), sj = atom_sigma(a, j);
    pair += static_cast<double>(a.q[i]) * a.q[j] * pair_f(sqrt(d0 * d0 + d1 * d1 + d2 * d2), sqrt(si * si + sj * sj));
  }
  for (int64_t i = a.node_splits[g] + lane; i < a.node_splits[g + 1]; i += 64) {
    const double si = atom_sigma(a, i), qi = a.q[i];
    if (si != 0.0) self += qi * qi / si;
  }
  pair = mp_wave_sum(pair);
  self = mp_wave_sum(self);
  if (lane == 0) {
    if (a.mult != 0.0f) pair /= static_cast<double>(a.mult);
    a.energy[g] = static_cast<float>(pair + self / (2.0 * kSqrtPi));
  }
}

__global__ __launch_bounds__(64) void gauss_energy_grad_kernel(GaussArgs a) {
  const int64_t g = blockIdx.x;
  const double ge = a.g_energy[g];
  const double gp = a.mult != 0.0f ? ge / static_cast<double>(a.mult) : ge;
  for (int64_t i = a.node_splits[g] + threadIdx.x; i < a.node_splits[g + 1]; i += 64) {
    const double xi0 = a.xyz[3 * i], xi1 = a.xyz[3 * i + 1], xi2 = a.xyz[3 * i + 2];
    const double si = atom_sigma(a, i), qi = a.q[i];
    double qb = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int c = 0; c < 2; ++c) {
      const int32_t* ptr = c == 0 ? a.ptr0 : a.ptr1;
      const int32_t* perm = c == 0 ? a.perm0 : a.perm1;
      const int32_t* other = a.cols + (c == 0 ? a.M : 0);
      for (int32_t t = ptr[i]; t < ptr[i + 1]; ++t) {
        const int64_t e = perm ? perm[t] : t;
        const int32_t j = other[e];
        if (!in_range(j, a.N)) continue;
        const double d0 = xi0 - a.xyz[3 * j], d1 = xi1 - a.xyz[3 * j + 1], d2 = xi2 - a.xyz[3 * j + 2];
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double sj = atom_sigma(a, j), gam = sqrt(si * si + sj * sj);
        const double qj = a.q[j];
        qb += qj * pair_f(r, gam);
        const double df = pair_df(r, gam);
        if (df != 0.0) {
          const double s = qi * qj * df / r;
          b0 += s * d0;
          b1 += s * d1;
          b2 += s * d2;
        }
      }
    }
    qb *= gp;
    if (si != 0.0) qb += ge * qi / (si * kSqrtPi);
    if (a.q_bar) a.q_bar[i] = static_cast<float>(qb);
    if (a.x_bar) {
      a.x_bar[3 * i] = static_cast<float>(gp * b0);
      a.x_bar[3 * i + 1] = static_cast<float>(gp * b1);
      a.x_bar[3 * i + 2] = static_cast<float>(gp * b2);
    }
  }
}

}  // namespace

extern "C" {

int mp_cent_charge_f32(const float* xyz, const int64_t* z, const int64_t* node_splits, int64_t G, int64_t N,
                       const float* chi, const float* qtot, const float* sigma, const float* hardness, int ntab,
                       float* q, mpStream_t stream) {
  MP_REQUIRE(G >= 0 && N >= 0 && ntab >= 1, "mp_cent_charge_f32: bad sizes");
  if (G == 0 || N == 0) return MP_OK;
  MP_REQUIRE(xyz && z && node_splits && chi && qtot && sigma && hardness && q, "mp_cent_charge_f32: null pointer");
  CentArgs a{};
  a.xyz = xyz; a.z = z; a.node_splits = node_splits; a.rhs = chi; a.qtot = qtot; a.sigma = sigma;
  a.hardness = hardness; a.ntab = ntab; a.q_out = q;
  cent_solve_kernel<false><<<static_cast<unsigned>(G), 64, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_cent_charge_f32");
}

int mp_cent_charge_grad_f32(const float* xyz, const int64_t* z, const int64_t* node_splits, int64_t G, int64_t N,
                            const float* q, const float* gq, const float* sigma, const float* hardness, int ntab,
                            float* chi_bar, float* x_bar, mpStream_t stream) {
  MP_REQUIRE(G >= 0 && N >= 0 && ntab >= 1, "mp_cent_charge_grad_f32: bad sizes");
  if (G == 0 || N == 0 || (!chi_bar && !x_bar)) return MP_OK;
  MP_REQUIRE(xyz && z && node_splits && q && gq && sigma && hardness, "mp_cent_charge_grad_f32: null pointer");
  CentArgs a{};
  a.xyz = xyz; a.z = z; a.node_splits = node_splits; a.rhs = gq; a.q = q; a.sigma = sigma; a.hardness = hardness;
  a.ntab = ntab; a.chi_bar = chi_bar; a.x_bar = x_bar;
  cent_solve_kernel<true><<<static_cast<unsigned>(G), 64, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_cent_charge_grad_f32");
}

int mp_gauss_energy_f32(const float* xyz, const int64_t* z, const float* q, const int64_t* node_splits, int64_t G,
                        int64_t N, const int32_t* cols, int64_t M, const int64_t* edge_splits, const float* sigma,
                        int ntab, float multiplicity, float* energy, mpStream_t stream) {
  MP_REQUIRE(G >= 0 && N >= 0 && M >= 0 && ntab >= 1, "mp_gauss_energy_f32: bad sizes");
  if (G == 0) return MP_OK;
  MP_REQUIRE(node_splits && edge_splits && sigma && energy && (N == 0 || (xyz && z && q)) && (M == 0 || cols),
             "mp_gauss_energy_f32: null pointer");
  GaussArgs a{};
  a.xyz = xyz; a.z = z; a.q = q; a.node_splits = node_splits; a.N = N; a.cols = cols; a.M = M;
  a.edge_splits = edge_splits; a.sigma = sigma; a.ntab = ntab; a.mult = multiplicity; a.energy = energy;
  gauss_energy_kernel<<<static_cast<unsigned>(G), 64, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_gauss_energy_f32");
}

int mp_gauss_energy_grad_f32(const float* xyz, const int64_t* z, const float* q, const int64_t* node_splits, int64_t G,
                             int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0, const int32_t* perm0,
                             const int32_t* ptr1, const int32_t* perm1, const float* sigma, int ntab,
                             float multiplicity, const float* g_energy, float* q_bar, float* x_bar,
                             mpStream_t stream) {
  MP_REQUIRE(G >= 0 && N >= 0 && M >= 0 && ntab >= 1, "mp_gauss_energy_grad_f32: bad sizes");
  if (G == 0 || N == 0 || (!q_bar && !x_bar)) return MP_OK;
  MP_REQUIRE(xyz && z && q && node_splits && g_energy && sigma && ptr0 && ptr1 && (M == 0 || cols),
             "mp_gauss_energy_grad_f32: null pointer");
  GaussArgs a{};
  a.xyz = xyz; a.z = z; a.q = q; a.node_splits = node_splits; a.N = N; a.cols = cols; a.M = M;
  a.ptr0 = ptr0; a.perm0 = perm0; a.ptr1 = ptr1; a.perm1 = perm1; a.sigma = sigma; a.ntab = ntab;
  a.mult = multiplicity; a.g_energy = g_energy; a.q_bar = q_bar; a.x_bar = x_bar;
  gauss_energy_grad_kernel<<<static_cast<unsigned>(G), 64, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_gauss_energy_grad_f32");
}

}  // extern "C"
