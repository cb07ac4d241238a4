// Extensive energy / force label scaler (kgcnn/data/transform/scaler/mol.py:38-98, force.py:164-222): a ridge regression
// of the total energy on the per-molecule element counts removes the atomic offsets, the residual's standard deviation
// rescales energies and forces.  Labels enter as float64 (or float32) on the device, every sum below is FP64.
//
//   mp_scaler_species_count     counts (G, 95) int32, presence mask (95), selection list (96)            mol.py:55-67
//   mp_scaler_fit_ws_bytes      workspace of the two chunked passes below
//   mp_scaler_normal_f64        A = X^T W X + alpha I (K, K), b = X^T W y (K, S), weighted means         Ridge.fit
//   mp_scaler_solve_f64         Cholesky of A, coef (K, S), intercept (S), the 95 x S offset table       Ridge.fit
//   mp_scaler_residual_std_f64  scale (S) = std(y - X coef - intercept, axis 0)                          mol.py:69-73
//   mp_scaler_apply             (E - offset) / scale, F / scale and the inverse, one launch              force.py:164-222
//
// K, the number of species present, is known on the device only (selection[95]); the host never reads it between the
// launches, so a whole fit is one stream of launches behind which the caller reads the weights back once.  Buffers are
// sized for K = 95 by the caller; the kernels address them with the K they read.
//
// Order of every floating-point sum (the same bits on every run and stream, no float atomics):
//  - rows go in chunks of MP_SCALER_CHUNK_ROWS graphs, one slab of partial sums per chunk; a second launch adds the slabs
//    in chunk order (the scheme of mp_dense_wgrad_f32);
//  - inside a chunk the normal-equation kernel walks the rows in order, one thread per matrix element; the column sums
//    and the residual sums are one row per thread followed by a halving tree in LDS;
//  - a graph's offset is a lane-strided partial over its atoms followed by the fixed butterfly of mp_wave_sum.
// The histogram uses integer LDS atomics (order-free).  Numbers outside [0, 95) are never counted and never indexed.
#include <math.h>

#include "mp_common.h"
#include "../../include/mpengine/scaler.h"

namespace {

constexpr int kZ = MP_SCALER_MAX_NUMBER;
constexpr int kChunk = MP_SCALER_CHUNK_ROWS;
constexpr int kMaxS = MP_SCALER_MAX_STATES;
constexpr int kTile = 32;                       // rows of a chunk staged in LDS at a time
constexpr int kTri = kZ * (kZ + 1) / 2;

static_assert(kChunk == 256 && kChunk % kTile == 0, "one thread per chunk row in the tree-reduced kernels");

// atomic number of atom i as Keras casts it (float -> int truncates), -1 outside [0, 95) (NaN included)
__device__ __forceinline__ int number_at(const void* z, int kind, int64_t i) {
  if (kind == MP_DT_F32) {
    const float v = static_cast<const float*>(z)[i];
    return (v > -1.0f && v < static_cast<float>(kZ)) ? static_cast<int>(v) : -1;
  }
  const int64_t v = kind == MP_DT_I32 ? static_cast<int64_t>(static_cast<const int32_t*>(z)[i])
                                      : static_cast<const int64_t*>(z)[i];
  return (v >= 0 && v < kZ) ? static_cast<int>(v) : -1;
}

__device__ __forceinline__ double real_at(const void* p, int kind, int64_t i) {
  return kind == MP_DT_F64 ? static_cast<const double*>(p)[i] : static_cast<double>(static_cast<const float*>(p)[i]);
}

__device__ __forceinline__ void raise_flag(int32_t* flags, bool mine, int bit) {
  if (__ballot(mine) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flags, bit);
}

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // j <= i

// ------------------------------------------------------------------ species counts: one wave per graph
__global__ __launch_bounds__(64) void species_count_kernel(const void* z, int kind, const int64_t* splits, int64_t N,
                                                           int32_t* counts, int32_t* mask, int32_t* flags) {
  __shared__ int s_hist[kZ];
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  for (int k = lane; k < kZ; k += 64) s_hist[k] = 0;
  __syncthreads();
  int64_t lo = splits[g], hi = splits[g + 1];
  if (lo < 0) lo = 0;
  if (hi > N) hi = N;
  bool oob = false;
  for (int64_t i = lo + lane; i < hi; i += 64) {
    const int k = number_at(z, kind, i);
    if (k < 0) oob = true; else atomicAdd(&s_hist[k], 1);
  }
  __syncthreads();
  for (int k = lane; k < kZ; k += 64) {
    const int c = s_hist[k];
    counts[g * kZ + k] = c;
    if (c > 0) mask[k] = 1;            // every writer stores the same word
  }
  raise_flag(flags, oob, MP_FLAG_OOB);
}

// selection[0..K) = the numbers present in ascending order (np.unique), -1 behind them, selection[95] = K
__global__ void species_select_kernel(const int32_t* mask, int32_t* sel) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int K = 0;
  for (int k = 0; k < kZ; ++k)
    if (mask[k] != 0) sel[K++] = k;
  for (int j = K; j < kZ; ++j) sel[j] = -1;
  sel[kZ] = K;
}

// ------------------------------------------------------------------ ridge normal equations
struct FitArgs {
  const int32_t* counts;   // (G, 95)
  const int32_t* sel;      // (96)
  int64_t G;
  const void* y;           // (G, S)
  int y_kind;
  int S;
  const double* w;         // (G) or null
  const double* mean;      // (K + S) weighted column means (zeros without an intercept)
  const double* coef;      // (K, S)
  const double* intercept; // (S)
  double* slab;            // per-chunk partial sums
};

// column c of row r of [X | y]: X = the count columns of the species present
__device__ __forceinline__ double design_at(const FitArgs& a, int K, int64_t r, int c) {
  return c < K ? static_cast<double>(a.counts[r * kZ + a.sel[c]]) : real_at(a.y, a.y_kind, r * a.S + (c - K));
}

// sum over the 256 threads of the block, valid in thread 0: halving tree, the same order every run
__device__ __forceinline__ double block_tree_sum(double v, double* s_red) {
  const int tid = threadIdx.x;
  s_red[tid] = v;
  __syncthreads();
  for (int off = kChunk / 2; off > 0; off >>= 1) {
    if (tid < off) s_red[tid] += s_red[tid + off];
    __syncthreads();
  }
  const double out = s_red[0];
  __syncthreads();
  return out;
}

// slab[chunk][c] = sum_r w_r [X | y | 1][r][c] over the rows of the chunk, c < K + S + 1
__global__ __launch_bounds__(kChunk) void colsum_chunk_kernel(FitArgs a) {
  __shared__ double s_red[kChunk];
  const int K = a.sel[kZ], W = K + a.S + 1;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kChunk + threadIdx.x;
  const bool live = r < a.G;
  const double w = live ? (a.w ? a.w[r] : 1.0) : 0.0;
  for (int c = 0; c < W; ++c) {
    const double v = live ? (c + 1 < W ? w * design_at(a, K, r, c) : w) : 0.0;
    const double sum = block_tree_sum(v, s_red);
    if (threadIdx.x == 0) a.slab[static_cast<int64_t>(blockIdx.x) * W + c] = sum;
  }
}

// slab[chunk][j][c] = sum_r w_r z[r][j] z[r][c], z = [X | y] - mean, j < K, c < K + S: rows in order, one thread per (j, c)
__global__ __launch_bounds__(256) void normal_chunk_kernel(FitArgs a) {
  __shared__ double s_z[kTile * (kZ + kMaxS)];
  __shared__ double s_w[kTile];
  const int tid = threadIdx.x;
  const int K = a.sel[kZ], C = K + a.S, E = K * C;
  double* slab = a.slab + static_cast<int64_t>(blockIdx.x) * E;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kChunk;
  for (int t = 0; t < kChunk / kTile; ++t) {
    const int64_t base = row0 + static_cast<int64_t>(t) * kTile;
    if (base >= a.G) break;                                   // uniform
    const int rows = a.G - base < kTile ? static_cast<int>(a.G - base) : kTile;
    for (int q = tid; q < rows * C; q += 256) {
      const int r = q / C, c = q - r * C;
      s_z[r * C + c] = design_at(a, K, base + r, c) - a.mean[c];
    }
    if (tid < rows) s_w[tid] = a.w ? a.w[base + tid] : 1.0;
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
      const int j = e / C, c = e - j * C;
      double acc = t == 0 ? 0.0 : slab[e];
      for (int r = 0; r < rows; ++r) acc += s_w[r] * s_z[r * C + j] * s_z[r * C + c];
      slab[e] = acc;
    }
    __syncthreads();
  }
}

enum { FINISH_MEAN = 0, FINISH_NORMAL = 1, FINISH_RESID_MEAN = 2, FINISH_RESID_STD = 3 };

struct FinishArgs {
  const double* slab;
  const int32_t* sel;
  int64_t chunks;
  int64_t G;
  int S;
  int mode;
  double alpha;
  double* out0;   // MEAN: mean (K + S); NORMAL: A (K, K); RESID_*: (S)
  double* out1;   // NORMAL: b (K, S)
};

// adds the slabs in chunk order, one thread per element
__global__ __launch_bounds__(256) void finish_kernel(FinishArgs a) {
  const int K = a.sel[kZ], C = K + a.S;
  const int width = a.mode == FINISH_MEAN ? C + 1 : (a.mode == FINISH_NORMAL ? K * C : a.S);
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= width) return;
  double acc = 0.0;
  for (int64_t ch = 0; ch < a.chunks; ++ch) acc += a.slab[ch * width + e];
  if (a.mode == FINISH_MEAN) {
    if (e == C) return;
    double wsum = 0.0;
    for (int64_t ch = 0; ch < a.chunks; ++ch) wsum += a.slab[ch * width + C];
    a.out0[e] = acc / wsum;
  } else if (a.mode == FINISH_NORMAL) {
    const int j = e / C, c = e - j * C;
    if (c < K) a.out0[j * K + c] = j == c ? acc + a.alpha : acc;
    else a.out1[j * a.S + (c - K)] = acc;
  } else if (a.mode == FINISH_RESID_MEAN) {
    a.out0[e] = acc / static_cast<double>(a.G);
  } else {
    a.out0[e] = sqrt(acc / static_cast<double>(a.G));
  }
}

// ------------------------------------------------------------------ solve: one wave, Cholesky in FP64 LDS (mp_cent.hip)
struct SolveArgs {
  const double* A;      // (K, K)
  const double* b;      // (K, S)
  const double* mean;   // (K + S)
  const int32_t* sel;
  int S;
  int fit_intercept;
  double* coef;         // (95, S): rows [0, K) = coefficients in selection order, zeros behind
  double* intercept;    // (S)
  double* table;        // (95, S): coef scattered by atomic number, zeros elsewhere
  int32_t* status;      // 0, or 1 + the column of the non-positive pivot
};

__global__ __launch_bounds__(64) void solve_kernel(SolveArgs a) {
  __shared__ double s_a[kTri];
  __shared__ double s_ld[kZ];
  __shared__ double s_x[kZ * kMaxS];
  const int lane = threadIdx.x;
  __shared__ int s_row[kZ];                  // row of a number in the selection, -1 for a number absent from the fit
  const int K = a.sel[kZ], S = a.S;
  for (int z = lane; z < kZ; z += 64) s_row[z] = -1;
  __syncthreads();
  for (int k = lane; k < K; k += 64) s_row[a.sel[k]] = k;
  for (int i = 0; i < K; ++i)
    for (int j = lane; j <= i; j += 64) s_a[tri(i, j)] = a.A[i * K + j];
  for (int q = lane; q < K * S; q += 64) s_x[q] = a.b[q];
  __syncthreads();

  // A = L L^T, right-looking; the break is uniform (every lane reads the same pivot after a barrier)
  int bad = 0;
  for (int k = 0; k < K; ++k) {
    const double d = s_a[tri(k, k)];
    if (!(d > 0.0)) { bad = k + 1; break; }
    const double lkk = sqrt(d);
    if (lane == 0) s_ld[k] = lkk;
    for (int i = k + 1 + lane; i < K; i += 64) s_a[tri(i, k)] /= lkk;
    __syncthreads();
    for (int j = k + 1 + lane; j < K; j += 64) {
      const double ljk = s_a[tri(j, k)];
      for (int i = j; i < K; ++i) s_a[tri(i, j)] -= s_a[tri(i, k)] * ljk;
    }
    __syncthreads();
  }
  if (lane == 0) a.status[0] = bad;
  if (bad) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int q = lane; q < kZ * S; q += 64) {
      a.coef[q] = q < K * S ? qnan : 0.0;
      a.table[q] = s_row[q / S] >= 0 ? qnan : 0.0;
    }
    for (int s = lane; s < S; s += 64) a.intercept[s] = qnan;
    return;
  }

  // L y = b, then L^T x = y, for the S right-hand sides
  for (int k = 0; k < K; ++k) {
    const double lkk = s_ld[k];
    for (int s = lane; s < S; s += 64) s_x[k * S + s] /= lkk;
    __syncthreads();
    for (int q = lane; q < (K - k - 1) * S; q += 64) {
      const int i = k + 1 + q / S, s = q % S;
      s_x[i * S + s] -= s_a[tri(i, k)] * s_x[k * S + s];
    }
    __syncthreads();
  }
  for (int k = K - 1; k >= 0; --k) {
    const double lkk = s_ld[k];
    for (int s = lane; s < S; s += 64) s_x[k * S + s] /= lkk;
    __syncthreads();
    for (int q = lane; q < k * S; q += 64) {
      const int i = q / S, s = q % S;
      s_x[i * S + s] -= s_a[tri(k, i)] * s_x[k * S + s];
    }
    __syncthreads();
  }
  for (int q = lane; q < kZ * S; q += 64) {
    const int row = s_row[q / S];
    a.coef[q] = q < K * S ? s_x[q] : 0.0;
    a.table[q] = row >= 0 ? s_x[row * S + q % S] : 0.0;
  }
  // intercept_ = y_mean - x_mean . coef (sklearn's _set_intercept), the species in order
  for (int s = lane; s < S; s += 64) {
    double v = 0.0;
    if (a.fit_intercept) {
      double dot = 0.0;
      for (int k = 0; k < K; ++k) dot += a.mean[k] * s_x[k * S + s];
      v = a.mean[K + s] - dot;
    }
    a.intercept[s] = v;
  }
}

// ------------------------------------------------------------------ residual scale
// PASS 0: slab[chunk][s] = sum_r d[r][s]; PASS 1: sum_r (d[r][s] - mean[s])^2; d = y - (X coef + intercept)
template <int PASS>
__global__ __launch_bounds__(kChunk) void resid_chunk_kernel(FitArgs a) {
  __shared__ double s_red[kChunk];
  const int K = a.sel[kZ], S = a.S;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kChunk + threadIdx.x;
  const bool live = r < a.G;
  for (int s = 0; s < S; ++s) {
    double v = 0.0;
    if (live) {
      double pred = 0.0;
      for (int k = 0; k < K; ++k) pred += static_cast<double>(a.counts[r * kZ + a.sel[k]]) * a.coef[k * S + s];
      v = real_at(a.y, a.y_kind, r * S + s) - (pred + a.intercept[s]);
      if (PASS == 1) { v -= a.mean[s]; v = v * v; }
    }
    const double sum = block_tree_sum(v, s_red);
    if (threadIdx.x == 0) a.slab[static_cast<int64_t>(blockIdx.x) * S + s] = sum;
  }
}

__global__ void fill_ones_kernel(double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = 1.0;
}

// ------------------------------------------------------------------ apply: one wave per graph, energies and forces
struct ApplyArgs {
  const void* z;
  int z_kind;
  const int64_t* splits;
  int64_t N;
  int S;
  int inverse;
  const double* table;      // (95, S)
  const int32_t* present;   // (95)
  const double* intercept;  // (S)
  const double* scale;      // (S)
  const void* e_in;         // (G, S) or null
  int e_in_kind;
  void* e_out;
  int e_out_kind;
  const float* f_in;        // (N, 3 S) or null
  float* f_out;
  double* offset_out;       // (G, S) or null
  int32_t* flags;
};

__global__ __launch_bounds__(64) void apply_kernel(ApplyArgs a) {
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int S = a.S;
  int64_t lo = a.splits[g], hi = a.splits[g + 1];
  if (lo < 0) lo = 0;
  if (hi > a.N) hi = a.N;
  if (a.e_in || a.offset_out) {
    bool oob = false, unknown = false;
    for (int s = 0; s < S; ++s) {
      double part = 0.0;
      for (int64_t i = lo + lane; i < hi; i += 64) {
        const int k = number_at(a.z, a.z_kind, i);
        if (k < 0) oob = true;
        else if (a.present[k] == 0) unknown = true;
        else part += a.table[k * S + s];
      }
      const double offset = a.intercept[s] + mp_wave_sum(part);
      if (lane == 0) {
        if (a.offset_out) a.offset_out[g * S + s] = offset;
        if (a.e_in) {
          const double e = real_at(a.e_in, a.e_in_kind, g * S + s);
          const double v = a.inverse ? e * a.scale[s] + offset : (e - offset) / a.scale[s];
          if (a.e_out_kind == MP_DT_F64) static_cast<double*>(a.e_out)[g * S + s] = v;
          else static_cast<float*>(a.e_out)[g * S + s] = static_cast<float>(v);
        }
      }
    }
    raise_flag(a.flags, oob, MP_FLAG_OOB);
    raise_flag(a.flags, unknown, MP_FLAG_UNKNOWN_SPECIES);
  }
  if (a.f_in) {
    const int64_t first = lo * 3 * S, count = (hi - lo) * 3 * S;
    for (int64_t q = lane; q < count; q += 64) {
      const double sc = a.scale[S == 1 ? 0 : static_cast<int>(q % S)];
      const double f = a.f_in[first + q];
      a.f_out[first + q] = static_cast<float>(a.inverse ? f * sc : f / sc);
    }
  }
}

inline bool number_kind_ok(int kind) { return kind == MP_DT_F32 || kind == MP_DT_I32 || kind == MP_DT_I64; }
inline bool real_kind_ok(int kind) { return kind == MP_DT_F32 || kind == MP_DT_F64; }
inline int64_t chunks_of(int64_t G) { return mp::ceil_div(G, kChunk); }
inline size_t slab_bytes(int64_t G, int S) {
  return static_cast<size_t>(chunks_of(G)) * kZ * (kZ + S) * sizeof(double);     // >= chunks * (K + S + 1) too
}

}  // namespace

extern "C" {

int mp_scaler_species_count(const void* numbers, int number_kind, const int64_t* node_splits, int64_t G, int64_t N,
                            int32_t* counts, int32_t* mask, int32_t* selection, int32_t* flags, mpStream_t stream) {
  MP_REQUIRE(G >= 0 && G <= 0x7fffffff && N >= 0, "mp_scaler_species_count: bad sizes");
  MP_REQUIRE(number_kind_ok(number_kind), "mp_scaler_species_count: numbers must be float32, int32 or int64");
  MP_REQUIRE(mask && selection && flags, "mp_scaler_species_count: null pointer");
  MP_REQUIRE(G == 0 || (node_splits && counts && (N == 0 || numbers)), "mp_scaler_species_count: null pointer");
  hipStream_t st = mp::as_stream(stream);
  MP_HIP(hipMemsetAsync(mask, 0, kZ * sizeof(int32_t), st));
  if (G > 0)
    species_count_kernel<<<static_cast<unsigned>(G), 64, 0, st>>>(numbers, number_kind, node_splits, N, counts, mask,
                                                                  flags);
  species_select_kernel<<<1, 64, 0, st>>>(mask, selection);
  return mp::check_launch("mp_scaler_species_count");
}

int mp_scaler_fit_ws_bytes(int64_t G, int S, size_t* bytes_out_host) {
  MP_REQUIRE(G >= 0 && S >= 1 && S <= kMaxS && bytes_out_host, "mp_scaler_fit_ws_bytes: bad arguments");
  *bytes_out_host = slab_bytes(G, S);
  return MP_OK;
}

int mp_scaler_normal_f64(const int32_t* counts, const int32_t* selection, int64_t G, const void* y, int y_kind, int S,
                         const double* sample_weight, double alpha, int fit_intercept, double* A, double* b,
                         double* mean, void* ws, size_t ws_bytes, mpStream_t stream) {
  MP_REQUIRE(G >= 1 && G <= 0x7fffffff && S >= 1 && S <= kMaxS, "mp_scaler_normal_f64: bad sizes (1 <= S <= %d)", kMaxS);
  MP_REQUIRE(real_kind_ok(y_kind), "mp_scaler_normal_f64: y must be float32 or float64");
  MP_REQUIRE(counts && selection && y && A && b && mean && ws, "mp_scaler_normal_f64: null pointer");
  MP_REQUIRE(ws_bytes >= slab_bytes(G, S), "mp_scaler_normal_f64: workspace too small");
  hipStream_t st = mp::as_stream(stream);
  const int64_t chunks = chunks_of(G);
  FitArgs f{};
  f.counts = counts; f.sel = selection; f.G = G; f.y = y; f.y_kind = y_kind; f.S = S; f.w = sample_weight;
  f.mean = mean; f.slab = static_cast<double*>(ws);
  FinishArgs fin{};
  fin.slab = f.slab; fin.sel = selection; fin.chunks = chunks; fin.G = G; fin.S = S; fin.alpha = alpha;
  if (fit_intercept) {
    colsum_chunk_kernel<<<static_cast<unsigned>(chunks), kChunk, 0, st>>>(f);
    fin.mode = FINISH_MEAN; fin.out0 = mean;
    finish_kernel<<<1, 256, 0, st>>>(fin);                    // K + S + 1 <= 128 elements
  } else {
    MP_HIP(hipMemsetAsync(mean, 0, (kZ + S) * sizeof(double), st));
  }
  normal_chunk_kernel<<<static_cast<unsigned>(chunks), 256, 0, st>>>(f);
  fin.mode = FINISH_NORMAL; fin.out0 = A; fin.out1 = b;
  finish_kernel<<<static_cast<unsigned>(mp::ceil_div(kZ * (kZ + S), 256)), 256, 0, st>>>(fin);
  return mp::check_launch("mp_scaler_normal_f64");
}

int mp_scaler_solve_f64(const double* A, const double* b, const double* mean, const int32_t* selection, int S,
                        int fit_intercept, double* coef, double* intercept, double* table, int32_t* status,
                        mpStream_t stream) {
  MP_REQUIRE(S >= 1 && S <= kMaxS, "mp_scaler_solve_f64: bad sizes (1 <= S <= %d)", kMaxS);
  MP_REQUIRE(A && b && mean && selection && coef && intercept && table && status, "mp_scaler_solve_f64: null pointer");
  SolveArgs a{};
  a.A = A; a.b = b; a.mean = mean; a.sel = selection; a.S = S; a.fit_intercept = fit_intercept; a.coef = coef;
  a.intercept = intercept; a.table = table; a.status = status;
  solve_kernel<<<1, 64, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_scaler_solve_f64");
}

int mp_scaler_residual_std_f64(const int32_t* counts, const int32_t* selection, int64_t G, const void* y, int y_kind,
                               int S, const double* coef, const double* intercept, int standardize, double* scale,
                               void* ws, size_t ws_bytes, mpStream_t stream) {
  MP_REQUIRE(G >= 1 && G <= 0x7fffffff && S >= 1 && S <= kMaxS, "mp_scaler_residual_std_f64: bad sizes");
  MP_REQUIRE(scale, "mp_scaler_residual_std_f64: null pointer");
  hipStream_t st = mp::as_stream(stream);
  if (!standardize) {
    fill_ones_kernel<<<1, 64, 0, st>>>(scale, S);
    return mp::check_launch("mp_scaler_residual_std_f64");
  }
  MP_REQUIRE(real_kind_ok(y_kind), "mp_scaler_residual_std_f64: y must be float32 or float64");
  MP_REQUIRE(counts && selection && y && coef && intercept && ws, "mp_scaler_residual_std_f64: null pointer");
  MP_REQUIRE(ws_bytes >= slab_bytes(G, S), "mp_scaler_residual_std_f64: workspace too small");
  const int64_t chunks = chunks_of(G);
  double* slab = static_cast<double*>(ws);
  double* resid_mean = slab + chunks * S;                    // behind the S-wide slabs, inside slab_bytes
  FitArgs f{};
  f.counts = counts; f.sel = selection; f.G = G; f.y = y; f.y_kind = y_kind; f.S = S; f.coef = coef;
  f.intercept = intercept; f.mean = resid_mean; f.slab = slab;
  FinishArgs fin{};
  fin.slab = slab; fin.sel = selection; fin.chunks = chunks; fin.G = G; fin.S = S;
  resid_chunk_kernel<0><<<static_cast<unsigned>(chunks), kChunk, 0, st>>>(f);
  fin.mode = FINISH_RESID_MEAN; fin.out0 = resid_mean;
  finish_kernel<<<1, 256, 0, st>>>(fin);
  resid_chunk_kernel<1><<<static_cast<unsigned>(chunks), kChunk, 0, st>>>(f);
  fin.mode = FINISH_RESID_STD; fin.out0 = scale;
  finish_kernel<<<1, 256, 0, st>>>(fin);
  return mp::check_launch("mp_scaler_residual_std_f64");
}

int mp_scaler_apply(const void* numbers, int number_kind, const int64_t* node_splits, int64_t G, int64_t N, int S,
                    int inverse, const double* table, const int32_t* present, const double* intercept,
                    const double* scale, const void* energy_in, int energy_in_kind, void* energy_out,
                    int energy_out_kind, const float* force_in, float* force_out, double* offset_out, int32_t* flags,
                    mpStream_t stream) {
  MP_REQUIRE(G >= 0 && G <= 0x7fffffff && N >= 0 && S >= 1 && S <= kMaxS, "mp_scaler_apply: bad sizes");
  if (G == 0) return MP_OK;
  MP_REQUIRE(number_kind_ok(number_kind), "mp_scaler_apply: numbers must be float32, int32 or int64");
  MP_REQUIRE(node_splits && table && present && intercept && scale && flags && (N == 0 || numbers),
             "mp_scaler_apply: null pointer");
  MP_REQUIRE(!energy_in || (energy_out && real_kind_ok(energy_in_kind) && real_kind_ok(energy_out_kind)),
             "mp_scaler_apply: energies are float32 or float64 and need an output");
  MP_REQUIRE(!force_in || force_out, "mp_scaler_apply: forces need an output");
  if (!energy_in && !force_in && !offset_out) return MP_OK;
  ApplyArgs a{};
  a.z = numbers; a.z_kind = number_kind; a.splits = node_splits; a.N = N; a.S = S; a.inverse = inverse; a.table = table;
  a.present = present; a.intercept = intercept; a.scale = scale; a.e_in = energy_in; a.e_in_kind = energy_in_kind;
  a.e_out = energy_out; a.e_out_kind = energy_out_kind; a.f_in = force_in; a.f_out = force_out;
  a.offset_out = offset_out; a.flags = flags;
  apply_kernel<<<static_cast<unsigned>(G), 64, 0, mp::as_stream(stream)>>>(a);
  return mp::check_launch("mp_scaler_apply");
}

}  // extern "C"
