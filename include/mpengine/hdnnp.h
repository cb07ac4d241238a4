/*
 * mpengine/hdnnp.h - HDNNP2nd symmetry functions and relational MLP, HDNNP4th charge equilibration.
 * Defined in csrc/: mp_acsf.hip, mp_relational.hip, mp_cent.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_HDNNP_H
#define MPENGINE_HDNNP_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- HDNNP2nd: symmetry functions ------------ */
/* Atom-centred symmetry functions (csrc/mp_acsf.hip), Behler's HDNNP2nd (kgcnn/literature/HDNNP2nd.py:154-242).
 * xyz (N,3); z (N) int64 atomic numbers; cols = the index plan's shifted int32 columns (K, M) of the pair list (K = 2,
 * (i, j)) or the triplet list (K = 3, (i, j, k)); ptrc / permc = CSR offsets (N+1) and stable-sort permutation
 * (nullable when column c is sorted) of index column c.  out / g / g_bar are (N, nrel*nfun): out[i, rel*nfun + m].
 * params: (nrel, nfun, P) or, with ncenter > 0, the target-set form (ncenter, nrel, nfun, P) indexed by the receiver's
 * element slot; P = 3 (eta, rs, rc) for G2, 4 (eta, zeta, lambda, rc) for G4.  rmap (31): atomic number -> element
 * slot; pmap (31*31): (z_j, z_k) -> G4 relation; -1 = no entry.  An element without an entry contributes nothing as a
 * neighbour (G2) or as a pair (G4), and a receiver without one gets a zero row from a target-set table: the
 * reference's out-of-range gather of the parameters gives zeros on a GPU and its out-of-range scatter is dropped.
 * Atomic numbers outside [0, 31) count as unmapped.  nrel*nfun <= 2048.
 *
 * mp_acsf_g2_f32: acsf_conv.py:158-210, exp(-eta (r_ij - rs)^2) fc(r_ij), fc = 0.5 (cos(pi clip(r, -rc, rc) / rc) + 1),
 *   summed into the relation of z_j.
 * mp_acsf_g4_f32: acsf_conv.py:419-494, 2^(1-zeta) (1 + lambda cos_ijk)^zeta exp(-eta (r_ij^2 + r_ik^2 + r_jk^2))
 *   fc_ij fc_ik fc_jk (/ multiplicity when it is not 0), summed into the relation of (z_j, z_k); powf semantics.
 * mp_acsf_g*_jvp_f32: forward mode, g_bar[i, rel, m] = sum over i's pairs / triplets of dG_m/dx . (h_i, h_j[, h_k]),
 *   h (N,3): the second-order piece that training through forces needs (d/dbase of base^zeta = zeta base^(zeta-1)).
 * mp_acsf_g*_grad_f32: reverse mode, dx (N,3) = d(sum g . G)/dx; per-entry endpoint partials in ws
 *   (mp_acsf_grad_ws_bytes), added per node over the CSR of every index column: deterministic, no float atomics.
 * All are receiver-parallel over the CSR of column 0; N = 0 needs no device. */
int mp_acsf_grad_ws_bytes(int64_t M, int K, size_t* bytes_out_host);
int mp_acsf_g2_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0,
                   const int32_t* perm0, const int32_t* rmap, const float* params, int nrel, int nfun, int ncenter,
                   float* out, mpStream_t stream);
int mp_acsf_g4_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0,
                   const int32_t* perm0, const int32_t* rmap, const int32_t* pmap, const float* params, int nrel,
                   int nfun, int ncenter, float multiplicity, float* out, mpStream_t stream);
int mp_acsf_g2_jvp_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                       const int32_t* ptr0, const int32_t* perm0, const int32_t* rmap, const float* params, int nrel,
                       int nfun, int ncenter, const float* h, float* g_bar, mpStream_t stream);
int mp_acsf_g4_jvp_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                       const int32_t* ptr0, const int32_t* perm0, const int32_t* rmap, const int32_t* pmap,
                       const float* params, int nrel, int nfun, int ncenter, float multiplicity, const float* h,
                       float* g_bar, mpStream_t stream);
int mp_acsf_g2_grad_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                        const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                        const int32_t* rmap, const float* params, int nrel, int nfun, int ncenter, const float* g,
                        float* ws, size_t ws_bytes, float* dx, mpStream_t stream);
int mp_acsf_g4_grad_f32(const float* xyz, const int64_t* z, int64_t N, const int32_t* cols, int64_t M,
                        const int32_t* ptr0, const int32_t* perm0, const int32_t* ptr1, const int32_t* perm1,
                        const int32_t* ptr2, const int32_t* perm2, const int32_t* rmap, const int32_t* pmap,
                        const float* params, int nrel, int nfun, int ncenter, float multiplicity, const float* g,
                        float* ws, size_t ws_bytes, float* dx, mpStream_t stream);

/* RelationalDense (csrc/mp_relational.hip, kgcnn/layers/relational.py:219-238 without num_bases / num_blocks).
 * W (nrel, K, U): one kernel per relation; b (U) shared; rel (R) int64; a relation outside [0, nrel) uses a zero
 * kernel (TF-GPU gather), i.e. its row is act(b).  mode 0: y (R,U) = act(x (R,K) W[rel] + b), pre_out (R,U) nullable
 * keeps the pre-activation.  mode 1 (transposed, the reverse pass): y (R,K) = (x (R,U) * act'(pre)) W[rel]^T, pre
 * nullable (no factor), no bias.  FP32, one launch for every relation, no host read-back (graph-capturable).
 * mp_relational_dense_wgrad_f32: dW[q] (K,U) = sum over the rows of relation q of x^T g, rows grouped by a stable sort
 * on the device and added in row order; db (U) = sum_r g[r]; either output nullable; deterministic. */
int mp_relational_dense_f32(const float* x, int64_t R, int64_t K, const int64_t* rel, int64_t nrel, const float* W,
                            const float* b, int64_t U, int act, float act_alpha, int mode, const float* pre,
                            float* pre_out, float* y, mpStream_t stream);
int mp_relational_dense_wgrad_ws_bytes(int64_t R, int64_t nrel, size_t* bytes_out_host);
int mp_relational_dense_wgrad_f32(const float* x, int64_t R, int64_t K, const int64_t* rel, int64_t nrel,
                                  const float* g, int64_t U, float* dW, float* db, void* ws, size_t ws_bytes,
                                  mpStream_t stream);

/* ---------------------------------------------------------------- HDNNP4th: charge equilibration ---------- */
/* CENT charges and Gaussian-charge electrostatics (csrc/mp_cent.hip), Ko et al.'s fourth-generation HDNNP
 * (kgcnn/literature/HDNNP4th.py:25-189).  xyz (N,3); z (N) int64 atomic numbers; node_splits (G+1) int64 row splits of
 * the molecules; sigma / hardness: per-atomic-number tables of ntab entries (the reference's 97, Z = 0..96); an atomic
 * number outside [0, ntab) reads 0 (the reference's out-of-range gather on a GPU).
 *
 * mp_cent_charge_f32: hdnnp_conv.py:148-258, per molecule the bordered system [[A, 1], [1^T, 0]] [Q; lambda] =
 *   [chi; Qtot] over ALL atom pairs of the molecule: A_ii = J[z_i] + 1 / (sigma_i sqrt(pi)), A_ij = erf(r_ij / (sqrt(2)
 *   gamma_ij)) / r_ij with gamma_ij = sqrt(sigma_i^2 + sigma_j^2) (0 where divide_no_nan gives 0); right-hand side +chi
 *   as the reference.  qtot (G).  One wave per molecule, the matrix in LDS, Cholesky + Schur complement in FP64.  At most
 *   MP_CENT_MAX_ATOMS atoms per molecule (the caller rejects larger ones; the kernel writes NaN for them), a molecule
 *   whose factorisation meets a non-positive pivot gets NaN charges, a 0-atom molecule produces nothing.
 * mp_cent_charge_grad_f32: its reverse for an upstream gQ (N), given the forward's charges q: w = A^-1 gQ - mu A^-1 1,
 *   mu = 1^T A^-1 gQ / 1^T A^-1 1; chi_bar = w, x_bar_i = -sum_{j != i} (w_i Q_j + w_j Q_i) f'(r_ij) (x_i - x_j) / r_ij.
 *   Refactors A (no workspace); either output nullable.
 * mp_gauss_energy_f32: hdnnp_conv.py:391-428, energy (G) = sum over the molecule's range_indices (cols = the index plan's
 *   shifted int32 columns (2, M), edge_splits (G+1)) of q_i q_j f(r_ij) / multiplicity (no division when it is 0) + sum
 *   over its atoms of divide_no_nan(q_i^2, sigma_i) / (2 sqrt(pi)).
 * mp_gauss_energy_grad_f32: its reverse for an upstream g_energy (G): q_bar (N), x_bar (N,3), per atom over the CSR
 *   (ptrc / permc, permc nullable when column c is sorted) of both index columns in list order; either output nullable.
 * Deterministic (fixed per-molecule reduction order, no float atomics); N = 0 or G = 0 needs no device. */
#define MP_CENT_MAX_ATOMS 128
int mp_cent_charge_f32(const float* xyz, const int64_t* z, const int64_t* node_splits, int64_t G, int64_t N,
                       const float* chi, const float* qtot, const float* sigma, const float* hardness, int ntab,
                       float* q, mpStream_t stream);
int mp_cent_charge_grad_f32(const float* xyz, const int64_t* z, const int64_t* node_splits, int64_t G, int64_t N,
                            const float* q, const float* gq, const float* sigma, const float* hardness, int ntab,
                            float* chi_bar, float* x_bar, mpStream_t stream);
int mp_gauss_energy_f32(const float* xyz, const int64_t* z, const float* q, const int64_t* node_splits, int64_t G,
                        int64_t N, const int32_t* cols, int64_t M, const int64_t* edge_splits, const float* sigma,
                        int ntab, float multiplicity, float* energy, mpStream_t stream);
int mp_gauss_energy_grad_f32(const float* xyz, const int64_t* z, const float* q, const int64_t* node_splits, int64_t G,
                             int64_t N, const int32_t* cols, int64_t M, const int32_t* ptr0, const int32_t* perm0,
                             const int32_t* ptr1, const int32_t* perm1, const float* sigma, int ntab,
                             float multiplicity, const float* g_energy, float* q_bar, float* x_bar,
                             mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_HDNNP_H */
