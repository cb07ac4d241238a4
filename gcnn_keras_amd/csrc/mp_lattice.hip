// Periodic cells: on-GPU SetRangePeriodic (kgcnn/graph/preprocessor.py:371-441 -> range_neighbour_lattice,
// kgcnn/graph/geom.py:172-368, exclusive mode, no self loops) and ShiftPeriodicLattice (kgcnn/layers/geom.py:76-123).
//
// Rule: receiver i is connected to every (sender j, image n) with |x_j + n L - x_i| <= max_distance, except
// (j = i, n = 0); an atom's own images are neighbours.  Per receiver the neighbours come in ascending distance and are
// cut after the first max_neighbours; receivers come in node order.  The reference builds a super-cell and argsorts an
// N x (N C) distance matrix per structure in NumPy; the super-cell is only a superset, the distance test decides.  Here
// the candidates of a pair (i, j) are the integers of the exact image box given by the cell's perpendicular heights
//   h_k = V / |a_{k+1} x a_{k+2}|,  f = (x_j - x_i) L^-1,  n_k in [ceil(-r_c/h_k - f_k - eps), floor(r_c/h_k - f_k + eps)]
// (inverse and f in FP64; eps widens the box, which is harmless), so atoms outside the cell need no wrapping.
//
// Distance: s = (n0 a0 + n1 a1) + n2 a2, d = |(x_j + s) - x_i| in float32 - the arithmetic of ShiftPeriodicLattice
// followed by NodeDistanceEuclidean, so range_attributes are the distances the crystal models compute.  The test is
// d <= max_distance in float32 (the reference's +1e-8 is below float32 resolution at these magnitudes).
// Order inside a receiver: (float32 distance, sender id, image lexicographic) - a total order, so exact ties (images n
// and -n of an atom's own copies) come out the same on every run.
//
// One wave per receiver.  Lanes stride over the (sender, image) candidates; hits are compacted into LDS by ballot and
// prefix popcount; the fill pass sorts them there with a bitonic network.  The count pass needs no sort: the number of
// kept neighbours is min(hits, max_neighbours).  Limits (each sets a flag bit, nothing is cut silently):
// MP_PERIODIC_MAX_HITS neighbours inside the cutoff per receiver before the max_neighbours cut,
// MP_PERIODIC_MAX_CANDIDATES box candidates per receiver, |n_k| <= MP_PERIODIC_MAX_IMAGE, |V| > 0.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "mp_common.h"
#include "../../include/mpengine/cgcnn.h"
#include "../../include/mpengine/geometry.h"

namespace {

constexpr int kCap = MP_PERIODIC_MAX_HITS;
constexpr int kImg = MP_PERIODIC_MAX_IMAGE;
constexpr double kBoxEps = 1e-3;  // in units of the lattice vectors

struct Cell {
  double inv[3][3];  // inv[c][k]: f_k = sum_c dx_c inv[c][k]
  double reach[3];   // r_c / h_k
  int w[3];          // integers a box can hold along k
  int per_sender;
  bool ok;
};

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// Every lane computes the same nine numbers of its graph's cell.  Returns MP_PERIODIC_FLAG_* bits (0: usable).
__device__ __forceinline__ int load_cell(const float* __restrict__ lat, float rc, int64_t n, Cell* c) {
  double a[3][3];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) a[r][k] = static_cast<double>(lat[r * 3 + k]);
  double x[3][3];
  cross3(a[1], a[2], x[0]);
  cross3(a[2], a[0], x[1]);
  cross3(a[0], a[1], x[2]);
  const double vol = a[0][0] * x[0][0] + a[0][1] * x[0][1] + a[0][2] * x[0][2];
  double scale = 1.0;
  for (int r = 0; r < 3; ++r) scale *= sqrt(a[r][0] * a[r][0] + a[r][1] * a[r][1] + a[r][2] * a[r][2]);
  c->ok = false;
  if (!(fabs(vol) > 1e-9 * scale) || !(fabs(vol) < 1e300)) return MP_PERIODIC_FLAG_SINGULAR;
  double total = static_cast<double>(n);
  for (int k = 0; k < 3; ++k) {
    const double xn = sqrt(x[k][0] * x[k][0] + x[k][1] * x[k][1] + x[k][2] * x[k][2]);
    c->reach[k] = static_cast<double>(rc) * xn / fabs(vol);
    for (int r = 0; r < 3; ++r) c->inv[r][k] = x[k][r] / vol;
    const double w = floor(2.0 * c->reach[k] + 2.0 * kBoxEps) + 1.0;
    if (!(w <= 2.0 * kImg + 1.0)) return MP_PERIODIC_FLAG_IMAGE_RANGE;
    c->w[k] = static_cast<int>(w);
    total *= w;
  }
  if (!(total <= static_cast<double>(MP_PERIODIC_MAX_CANDIDATES))) return MP_PERIODIC_FLAG_CAPACITY;
  c->per_sender = c->w[0] * c->w[1] * c->w[2];
  c->ok = true;
  return 0;
}

__device__ __forceinline__ int pack_image(int n0, int n1, int n2) {
  return ((n0 + kImg + 1) << 20) | ((n1 + kImg + 1) << 10) | (n2 + kImg + 1);  // order = lexicographic (n0, n1, n2)
}

// Hits of receiver `a` (global node id) compacted into LDS in candidate order; returns their number (may exceed kCap,
// entries past kCap are not stored) and ORs limit bits into *flag_bits.  STORE=false only counts.
template <bool STORE>
__device__ __forceinline__ int collect_hits(const float* __restrict__ xyz, const float* __restrict__ lat, int64_t base,
                                            int64_t n, int64_t i, float rc, const Cell& cell, unsigned* s_d, int* s_j,
                                            int* s_img, int* flag_bits) {
  const int lane = threadIdx.x & 63;
  const float xi0 = xyz[(base + i) * 3 + 0], xi1 = xyz[(base + i) * 3 + 1], xi2 = xyz[(base + i) * 3 + 2];
  const int total = static_cast<int>(n) * cell.per_sender;  // <= MP_PERIODIC_MAX_CANDIDATES (load_cell)
  int hits = 0;
  for (int c0 = 0; c0 < total; c0 += 64) {
    const int c = c0 + lane;
    bool hit = false;
    float d = 0.0f;
    int j = 0, img = 0;
    if (c < total) {
      j = c / cell.per_sender;
      int o = c - j * cell.per_sender;
      const int o2 = o % cell.w[2];
      o /= cell.w[2];
      const int o1 = o % cell.w[1], o0 = o / cell.w[1];
      const float xj0 = xyz[(base + j) * 3 + 0], xj1 = xyz[(base + j) * 3 + 1], xj2 = xyz[(base + j) * 3 + 2];
      const double dx[3] = {static_cast<double>(xj0) - xi0, static_cast<double>(xj1) - xi1,
                            static_cast<double>(xj2) - xi2};
      const int off[3] = {o0, o1, o2};
      int nk[3];
      bool inside = true, in_range = true;
      for (int k = 0; k < 3; ++k) {
        const double f = dx[0] * cell.inv[0][k] + dx[1] * cell.inv[1][k] + dx[2] * cell.inv[2][k];
        const double lo = ceil(-cell.reach[k] - f - kBoxEps), hi = floor(cell.reach[k] - f + kBoxEps);
        const double v = lo + off[k];
        inside = inside && v <= hi;
        in_range = in_range && v >= -static_cast<double>(kImg) && v <= static_cast<double>(kImg);
        nk[k] = in_range ? static_cast<int>(v) : 0;
      }
      if (inside && !in_range) *flag_bits |= MP_PERIODIC_FLAG_IMAGE_RANGE;
      if (inside && in_range && !(j == i && nk[0] == 0 && nk[1] == 0 && nk[2] == 0)) {
        const float t0 = static_cast<float>(nk[0]), t1 = static_cast<float>(nk[1]), t2 = static_cast<float>(nk[2]);
        const float s0 = (t0 * lat[0] + t1 * lat[3]) + t2 * lat[6];
        const float s1 = (t0 * lat[1] + t1 * lat[4]) + t2 * lat[7];
        const float s2 = (t0 * lat[2] + t1 * lat[5]) + t2 * lat[8];
        const float e0 = (xj0 + s0) - xi0, e1 = (xj1 + s1) - xi1, e2 = (xj2 + s2) - xi2;
        d = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
        hit = d <= rc;
        img = pack_image(nk[0], nk[1], nk[2]);
      }
    }
    const unsigned long long mask = __ballot(hit);
    if constexpr (STORE) {
      const int slot = hits + __popcll(mask & ((1ull << lane) - 1ull));
      if (hit && slot < kCap) {
        s_d[slot] = __float_as_uint(d);  // d >= 0: the bit pattern orders like the value
        s_j[slot] = j;
        s_img[slot] = img;
      }
    }
    hits += __popcll(mask);
  }
  return hits;
}

__device__ __forceinline__ bool key_less(unsigned da, int ja, int ia, unsigned db, int jb, int ib) {
  if (da != db) return da < db;
  if (ja != jb) return ja < jb;
  return ia < ib;
}

template <bool FILL>
__global__ __launch_bounds__(64) void periodic_graph_kernel(
    const float* __restrict__ xyz, const int64_t* __restrict__ node_splits, const float* __restrict__ lattice, int64_t G,
    int64_t N, float rc, int max_neighbours, int32_t* __restrict__ counts, int32_t* __restrict__ flags,
    const int32_t* __restrict__ node_ptr, int64_t M, int64_t* __restrict__ idx_out, int64_t* __restrict__ image_out,
    int32_t* __restrict__ recv, int32_t* __restrict__ send, float* __restrict__ dist) {
  __shared__ unsigned s_d[FILL ? kCap : 1];
  __shared__ int s_j[FILL ? kCap : 1];
  __shared__ int s_img[FILL ? kCap : 1];
  const int lane = threadIdx.x;
  for (int64_t a = blockIdx.x; a < N; a += gridDim.x) {
    const int64_t g = mp_owner_of(node_splits, G, a);
    const int64_t base = node_splits[g];
    const int64_t n = node_splits[g + 1] - base;
    const float* lat = lattice + g * 9;
    Cell cell;
    int bits = load_cell(lat, rc, n, &cell);
    int hits = 0;
    if (cell.ok) hits = collect_hits<FILL>(xyz, lat, base, n, a - base, rc, cell, s_d, s_j, s_img, &bits);
    if (hits > kCap) {
      bits |= MP_PERIODIC_FLAG_CAPACITY;
      hits = 0;
    }
    int keep = (max_neighbours >= 0 && hits > max_neighbours) ? max_neighbours : hits;
    if constexpr (!FILL) {
      int any = bits;
      for (int off = 32; off > 0; off >>= 1) any |= __shfl_xor(any, off, 64);
      if (lane == 0) {
        if (any != 0) atomicOr(flags, any);
        counts[a] = any != 0 ? 0 : keep;  // the host raises on the flag; no edge of a refused receiver is counted
      }
    } else {
      const int64_t start = node_ptr[a];
      const int64_t room = static_cast<int64_t>(node_ptr[a + 1]) - start;
      if (keep > room) keep = static_cast<int>(room < 0 ? 0 : room);
      int p = 1;
      while (p < hits) p <<= 1;
      for (int t = hits + lane; t < p; t += 64) {  // pad to a power of two with keys that sort last
        s_d[t] = 0xFFFFFFFFu;
        s_j[t] = 0x7FFFFFFF;
        s_img[t] = 0x7FFFFFFF;
      }
      __syncthreads();
      for (int k = 2; k <= p; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
          for (int t = lane; t < (p >> 1); t += 64) {
            const int lo = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));
            const int hi = lo | jj;
            const unsigned dl = s_d[lo], dh = s_d[hi];
            const int jl = s_j[lo], jh = s_j[hi], il = s_img[lo], ih = s_img[hi];
            const bool up = (lo & k) == 0;
            if (key_less(dh, jh, ih, dl, jl, il) == up) {
              s_d[lo] = dh; s_d[hi] = dl;
              s_j[lo] = jh; s_j[hi] = jl;
              s_img[lo] = ih; s_img[hi] = il;
            }
          }
          __syncthreads();
        }
      }
      for (int r = lane; r < keep; r += 64) {
        const int64_t pos = start + r;
        if (pos < 0 || pos >= M) continue;
        const int j = s_j[r], img = s_img[r];
        idx_out[pos * 2] = a - base;
        idx_out[pos * 2 + 1] = j;
        if (image_out) {
          image_out[pos * 3 + 0] = static_cast<int64_t>((img >> 20) & 0x3FF) - (kImg + 1);
          image_out[pos * 3 + 1] = static_cast<int64_t>((img >> 10) & 0x3FF) - (kImg + 1);
          image_out[pos * 3 + 2] = static_cast<int64_t>(img & 0x3FF) - (kImg + 1);
        }
        if (recv) recv[pos] = static_cast<int32_t>(a);
        if (send) send[pos] = static_cast<int32_t>(base + j);
        if (dist) dist[pos] = __uint_as_float(s_d[r]);
      }
      __syncthreads();  // the next receiver of this block overwrites the LDS lists
    }
  }
}

__global__ void periodic_edge_splits_kernel(const int32_t* __restrict__ node_ptr, const int64_t* __restrict__ node_splits,
                                            int64_t G, int64_t* __restrict__ edge_splits) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g <= G; g += stride)
    edge_splits[g] = node_ptr[node_splits[g]];
}

__global__ void lattice_shift_kernel(const float* __restrict__ pos, const int64_t* __restrict__ image,
                                     const float* __restrict__ lattice, const int64_t* __restrict__ edge_splits,
                                     int64_t G, int64_t M, float* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < M; e += stride) {
    const float* lat = lattice + mp_owner_of(edge_splits, G, e) * 9;
    const float n0 = static_cast<float>(image[e * 3 + 0]), n1 = static_cast<float>(image[e * 3 + 1]),
                n2 = static_cast<float>(image[e * 3 + 2]);
    for (int c = 0; c < 3; ++c) out[e * 3 + c] = pos[e * 3 + c] + ((n0 * lat[c] + n1 * lat[3 + c]) + n2 * lat[6 + c]);
  }
}

// FracToRealCoordinates (kgcnn/layers/geom.py:1012-1052): the einsum 'ij,ikj->ik', r_k = (f_0 A[k][0] + f_1 A[k][1]) +
// f_2 A[k][2] - the lattice matrix times the row, whatever the reference's docstring says.  transposed: the reverse,
// g_j = (r_0 A[0][j] + r_1 A[1][j]) + r_2 A[2][j].
__global__ void frac_to_real_kernel(const float* __restrict__ frac, const float* __restrict__ lattice,
                                    const int64_t* __restrict__ row_splits, int64_t G, int64_t M, int transposed,
                                    float* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < M; e += stride) {
    const float* lat = lattice + mp_owner_of(row_splits, G, e) * 9;
    const float f0 = frac[e * 3 + 0], f1 = frac[e * 3 + 1], f2 = frac[e * 3 + 2];
    for (int k = 0; k < 3; ++k) {
      const int i0 = transposed ? k : 3 * k, step = transposed ? 3 : 1;
      out[e * 3 + k] = (f0 * lat[i0] + f1 * lat[i0 + step]) + f2 * lat[i0 + 2 * step];
    }
  }
}

unsigned receiver_grid(int64_t N) { return static_cast<unsigned>(N < 256 * 64 ? (N < 1 ? 1 : N) : 256 * 64); }

}  // namespace

extern "C" {

int mp_lattice_shift_f32(const float* pos, const int64_t* image, const float* lattice, const int64_t* edge_splits,
                         int64_t G, int64_t M, float* out, mpStream_t stream) {
  MP_REQUIRE(G >= 0 && M >= 0, "mp_lattice_shift_f32: bad sizes");
  if (M == 0) return MP_OK;
  MP_REQUIRE(pos && image && lattice && edge_splits && out && G > 0, "mp_lattice_shift_f32: null pointer / no graphs");
  lattice_shift_kernel<<<mp::grid_for(M), 256, 0, mp::as_stream(stream)>>>(pos, image, lattice, edge_splits, G, M, out);
  return mp::check_launch("mp_lattice_shift_f32");
}

int mp_frac_to_real_f32(const float* frac, const float* lattice, const int64_t* row_splits, int64_t G, int64_t M,
                        int transposed, float* out, mpStream_t stream) {
  MP_REQUIRE(G >= 0 && M >= 0, "mp_frac_to_real_f32: bad sizes");
  if (M == 0) return MP_OK;
  MP_REQUIRE(frac && lattice && row_splits && out && G > 0, "mp_frac_to_real_f32: null pointer / no graphs");
  frac_to_real_kernel<<<mp::grid_for(M), 256, 0, mp::as_stream(stream)>>>(frac, lattice, row_splits, G, M,
                                                                          transposed ? 1 : 0, out);
  return mp::check_launch("mp_frac_to_real_f32");
}

int mp_radius_graph_periodic_workspace_bytes(int64_t N, size_t* bytes_out_host) {
  return mp_radius_graph_workspace_bytes(N, bytes_out_host);
}

int mp_radius_graph_periodic_count_f32(const float* xyz, const int64_t* node_splits, const float* lattice, int64_t G,
                                       int64_t N, float max_distance, int max_neighbours, int32_t* node_ptr,
                                       int64_t* edge_splits, int32_t* flags, void* ws, size_t ws_bytes,
                                       mpStream_t stream) {
  MP_REQUIRE(G >= 0 && N >= 0 && node_ptr && edge_splits && flags && ws,
             "mp_radius_graph_periodic_count_f32: bad arguments");
  MP_REQUIRE(N < (int64_t{1} << 31), "mp_radius_graph_periodic_count_f32: N must fit int32");
  MP_REQUIRE(max_distance >= 0.0f && max_distance < 1e30f,
             "mp_radius_graph_periodic_count_f32: a periodic cell needs a finite max_distance >= 0");
  size_t need = 0;
  int rc = mp_radius_graph_periodic_workspace_bytes(N, &need);
  if (rc != MP_OK) return rc;
  MP_REQUIRE(ws_bytes >= need, "mp_radius_graph_periodic_count_f32: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = mp::as_stream(stream);
  const size_t head = mp::align256(sizeof(int32_t) * static_cast<size_t>(N + 1));
  int32_t* counts = static_cast<int32_t*>(ws);
  void* temp = static_cast<char*>(ws) + head;
  size_t temp_bytes = ws_bytes - head;
  MP_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * static_cast<size_t>(N + 1), s));
  MP_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), s));
  if (N > 0) {
    MP_REQUIRE(xyz && node_splits && lattice && G > 0, "mp_radius_graph_periodic_count_f32: null pointer / no graphs");
    periodic_graph_kernel<false><<<receiver_grid(N), 64, 0, s>>>(xyz, node_splits, lattice, G, N, max_distance,
                                                                 max_neighbours, counts, flags, nullptr, 0, nullptr,
                                                                 nullptr, nullptr, nullptr, nullptr);
  }
  MP_HIP(rocprim::exclusive_scan(temp, temp_bytes, counts, node_ptr, int32_t{0}, static_cast<size_t>(N + 1),
                                 rocprim::plus<int32_t>(), s, false));
  if (G > 0) periodic_edge_splits_kernel<<<mp::grid_for(G + 1), 256, 0, s>>>(node_ptr, node_splits, G, edge_splits);
  else MP_HIP(hipMemsetAsync(edge_splits, 0, sizeof(int64_t), s));
  return mp::check_launch("mp_radius_graph_periodic_count_f32");
}

int mp_radius_graph_periodic_fill_f32(const float* xyz, const int64_t* node_splits, const float* lattice, int64_t G,
                                      int64_t N, float max_distance, int max_neighbours, const int32_t* node_ptr,
                                      int64_t M, int64_t* idx_out, int64_t* image_out, int32_t* recv, int32_t* send,
                                      float* dist, mpStream_t stream) {
  MP_REQUIRE(G >= 0 && N >= 0 && M >= 0, "mp_radius_graph_periodic_fill_f32: bad sizes");
  if (N == 0 || M == 0) return MP_OK;
  MP_REQUIRE(xyz && node_splits && lattice && node_ptr && idx_out && G > 0,
             "mp_radius_graph_periodic_fill_f32: null pointer");
  MP_REQUIRE(max_distance >= 0.0f && max_distance < 1e30f,
             "mp_radius_graph_periodic_fill_f32: a periodic cell needs a finite max_distance >= 0");
  periodic_graph_kernel<true><<<receiver_grid(N), 64, 0, mp::as_stream(stream)>>>(
      xyz, node_splits, lattice, G, N, max_distance, max_neighbours, nullptr, nullptr, node_ptr, M, idx_out, image_out,
      recv, send, dist);
  return mp::check_launch("mp_radius_graph_periodic_fill_f32");
}

}  // extern "C"
