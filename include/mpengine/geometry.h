/*
 * mpengine/geometry.h - norms, radial bases, edge geometry, SetRange, SetAngle, periodic cells.
 * Defined in csrc/: mp_elementwise.hip, mp_radius.hip, mp_angle.hip, mp_lattice.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_GEOMETRY_H
#define MPENGINE_GEOMETRY_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- geometry ------------------------------- */
/* EuclideanNorm._compute_euclidean_norm, kgcnn/layers/geom.py:181-193 on an (R, D, C) view reducing D:
 * out (R,C) = [1/]sqrt(relu(sum_d x^2) [+eps]). flags: bit0 invert, bit1 add_eps, bit2 no_nan, bit3 square_norm. */
int mp_euclidean_norm_f32(const float* x, int64_t R, int64_t D, int64_t C, int flags, float* out, mpStream_t stream);
/* ScalarProduct, geom.py:261: out (R,C) = sum_d a*b. */
int mp_scalar_product_f32(const float* a, const float* b, int64_t R, int64_t D, int64_t C, float* out,
                          mpStream_t stream);
/* GaussBasisLayer, geom.py:567-571. */
int mp_gauss_basis_f32(const float* d, int64_t M, int bins, float distance, float sigma, float offset, float* out,
                       mpStream_t stream);
/* BesselBasisLayer, geom.py:772-785 (poly envelope, frequencies (num_radial) trainable weight). */
int mp_bessel_basis_f32(const float* d, int64_t M, const float* frequencies, int num_radial, float cutoff,
                        int envelope_exponent, float* out, mpStream_t stream);
/* CosCutOffEnvelope, geom.py:831-837. */
int mp_cos_cutoff_f32(const float* d, int64_t n, float cutoff, float* out, mpStream_t stream);

/* Fused NodePosition -> LazySubtract -> EuclideanNorm (Schnet.py:116-117, PAiNN.py:116-118) on prepared columns:
 * dist (M) = ||x_i - x_j||, dir (M,3) nullable = (x_i-x_j)*divide_no_nan(1, dist). */
int mp_edge_geometry_f32(const float* xyz, int64_t N, const int32_t* recv, const int32_t* send, int64_t M,
                         float* dist, float* dir, mpStream_t stream);

/* ChangeTensorType ragged -> (padded, mask), kgcnn/layers/casting.py:79-84. */
int mp_ragged_to_padded_f32(const float* values, const int64_t* row_splits, int64_t G, int64_t Nmax, int64_t row_elems,
                            float* padded, float* mask, mpStream_t stream);

/* ---------------------------------------------------------------- on-GPU SetRange (next: SURVEY 8f.2) ---- */
/* SetRange.call, kgcnn/graph/preprocessor.py:288-314 via define_adjacency_from_distance (kgcnn/graph/adj.py:537-593),
 * exclusive mode, no self loops, for a whole ragged batch of coordinates xyz (N,3): pass 1 counts the edges of every
 * receiving atom and scans them (node_ptr (N+1) int32 = receiver CSR, edge_splits (G+1) int64); the caller reads
 * M = node_ptr[N] to size the outputs; pass 2 writes the (M,2) int64 sample indices in row-major (i,j) order and,
 * optionally, int32 receiver / sender ids and the edge distances (range_attributes).  max_distance < 0 or
 * max_neighbours < 0 disables that criterion. */
int mp_radius_graph_workspace_bytes(int64_t N, size_t* bytes_out_host);
int mp_radius_graph_count_f32(const float* xyz, const int64_t* node_splits, int64_t G, int64_t N, float max_distance,
                              int max_neighbours, int32_t* node_ptr, int64_t* edge_splits, void* ws, size_t ws_bytes,
                              mpStream_t stream);
int mp_radius_graph_fill_f32(const float* xyz, const int64_t* node_splits, int64_t G, int64_t N, float max_distance,
                             int max_neighbours, const int32_t* node_ptr, int64_t M, int64_t* idx_out, int32_t* recv,
                             int32_t* send, float* dist, mpStream_t stream);

/* ---------------------------------------------------------------- on-GPU SetAngle ------------------------ */
/* SetAngle.call, kgcnn/graph/preprocessor.py:354-368 via get_angle_indices / get_angle (kgcnn/graph/adj.py:300-415),
 * allow_self_edges=False, for a whole ragged batch of edge lists.  edge_cols (2,M): the shifted, clamped int32 columns
 * of the edge list's index plan; ptr (N+1) / perm (M, or NULL when the column is sorted): the plan's CSR over column
 * pos_fix.  pos_k is the position of k in edge_pairing, pos_fix the other one, pos_ij = 0 if the pairing names i,
 * else 1.  Partners of edge n = (i, j): the edges m != n with idx[m, pos_fix] == idx[n, pos_ij], without those equal to
 * (i, j) / (j, i) unless allow_multi_edges / allow_reverse_edges.  Order: by n, then m ascending.
 * Pass 1 counts the partners of every edge and scans them in int64: off (M+1) = first output row of every edge,
 * angle_splits (G+1) int64; the caller reads A = off[M] to size the outputs.  Pass 2 writes, each pointer nullable:
 * triples (A,3) int64 node ids (i, j, k) local to the graph, pairs (A,2) int64 edge ids (n, m) local to the graph's
 * edge list, triple_cols (3,A) / pair_cols (2,A) int32 shifted ids (the index-plan columns of the triples against the
 * node partition and of the pairs against the edge partition), theta (A) = atan2(|v1 x v2|, v1 . v2) with
 * v1 = x_i - x_j, v2 = x_j - x_k, and the column-0 CSRs triple_ptr (N+1; needs edge_ptr0, the edge list's column-0
 * CSR, and is meaningful when that column is sorted) and pair_ptr (M+1).  A >= 2^31 is MP_EINVAL.  M == 0 or G == 0
 * returns MP_OK without touching the device. */
int mp_angle_list_workspace_bytes(int64_t M, size_t* bytes_out_host);
int mp_angle_list_count_i32(const int32_t* edge_cols, int64_t M, int64_t N, const int32_t* ptr, const int32_t* perm,
                            const int64_t* edge_splits, int64_t G, int pos_fix, int pos_ij, int allow_multi_edges,
                            int allow_reverse_edges, int64_t* off, int64_t* angle_splits, void* ws, size_t ws_bytes,
                            mpStream_t stream);
int mp_angle_list_fill_f32(const int32_t* edge_cols, int64_t M, int64_t N, const int32_t* ptr, const int32_t* perm,
                           const int64_t* node_splits, const int64_t* edge_splits, int64_t G, int pos_fix, int pos_ij,
                           int pos_k, int allow_multi_edges, int allow_reverse_edges, const int64_t* off, int64_t A,
                           const float* xyz, int64_t* triples, int64_t* pairs, int32_t* triple_cols,
                           int32_t* pair_cols, float* theta, const int32_t* edge_ptr0, int32_t* triple_ptr,
                           int32_t* pair_ptr, mpStream_t stream);

/* ---------------------------------------------------------------- periodic cells ------------------------- */
/* ShiftPeriodicLattice.call, kgcnn/layers/geom.py:100-123: out[e] = pos[e] + ((n0 a0 + n1 a1) + n2 a2) with
 * n = image[e] (M,3) int64 and a_k the rows of lattice[g(e)] (G,3,3), g(e) from the edge row_splits (G+1); the
 * reference's reduce_sum order, no contraction.  M == 0 returns MP_OK without touching the device.
 *
 * SetRangePeriodic.call, kgcnn/graph/preprocessor.py:413-441 via range_neighbour_lattice (kgcnn/graph/geom.py:172-368),
 * exclusive mode, no self loops, for a ragged batch of coordinates xyz (N,3) with one cell lattice (G,3,3) per graph
 * (lattice vectors in rows).  Receiver i is connected to every (sender j, image n) with |(x_j + n L) - x_i| <=
 * max_distance in float32 (the shift as above), except (j = i, n = 0); per receiver in the order (distance, sender,
 * image lexicographic), cut after max_neighbours (< 0: no cut); receivers in node order.  Pass 1 writes node_ptr (N+1)
 * int32 = receiver CSR, edge_splits (G+1) int64 and the flag word (zeroed first, then mp_periodic_flag bits; a receiver
 * that raised one counts no edge); the caller reads M = node_ptr[N] and the flag word to size the outputs.  Pass 2
 * writes the (M,2) int64 sample indices (i, j), the (M,3) int64 images and, each nullable, the int32 receiver / sender
 * ids and the distances (range_attributes).  max_distance must be finite and >= 0.  As in mp_radius_graph_*, node_ptr is
 * int32: the caller keeps N x degree below 2^31 (2^31 edges are 50 GB of outputs). */
#define MP_PERIODIC_MAX_HITS 1024           /* neighbours inside the cutoff per receiver, before the max_neighbours cut */
#define MP_PERIODIC_MAX_IMAGE 511           /* |n_k| of an image index */
#define MP_PERIODIC_MAX_CANDIDATES 1048576  /* (sender, image) candidates of the image boxes per receiver */
enum mp_periodic_flag { MP_PERIODIC_FLAG_CAPACITY = 1, MP_PERIODIC_FLAG_IMAGE_RANGE = 2, MP_PERIODIC_FLAG_SINGULAR = 4 };
int mp_lattice_shift_f32(const float* pos, const int64_t* image, const float* lattice, const int64_t* edge_splits,
                         int64_t G, int64_t M, float* out, mpStream_t stream);
int mp_radius_graph_periodic_workspace_bytes(int64_t N, size_t* bytes_out_host);
int mp_radius_graph_periodic_count_f32(const float* xyz, const int64_t* node_splits, const float* lattice, int64_t G,
                                       int64_t N, float max_distance, int max_neighbours, int32_t* node_ptr,
                                       int64_t* edge_splits, int32_t* flags, void* ws, size_t ws_bytes,
                                       mpStream_t stream);
int mp_radius_graph_periodic_fill_f32(const float* xyz, const int64_t* node_splits, const float* lattice, int64_t G,
                                      int64_t N, float max_distance, int max_neighbours, const int32_t* node_ptr,
                                      int64_t M, int64_t* idx_out, int64_t* image_out, int32_t* recv, int32_t* send,
                                      float* dist, mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_GEOMETRY_H */
