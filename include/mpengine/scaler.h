/*
 * mpengine/scaler.h - the extensive energy / force label scaler.
 * Defined in csrc/: mp_scaler.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_SCALER_H
#define MPENGINE_SCALER_H

#include "core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- extensive energy / force label scaler ------------
 * kgcnn/data/transform/scaler/mol.py:38-98 (_ExtensiveMolecularScalerBase._fit / _predict) and
 * kgcnn/data/transform/scaler/force.py:164-222 (EnergyForceExtensiveLabelScaler.transform / inverse_transform): a ridge
 * regression of the molecular energies (G, S) on the per-molecule element counts, the population standard deviation of
 * the residual, and the transform itself.  Everything floating-point is FP64 with a fixed summation order (rows in chunks
 * of MP_SCALER_CHUNK_ROWS, slabs added in chunk order): the same bits on every run and stream, no float atomics.
 * K, the number of species present, stays on the device (selection[95]); buffers are sized for K = 95.  number_kind:
 * MP_DT_F32 (cast as Keras casts: truncation), MP_DT_I32 or MP_DT_I64.  y / energy kinds: MP_DT_F32 or MP_DT_F64.
 *
 * mp_scaler_species_count: mol.py:55-67.  counts (G, 95) int32 = per-graph histogram of the atomic numbers (one wave per
 *   graph, integer LDS atomics), mask (95) int32 = 1 where any graph holds the number, selection (96) int32 = the numbers
 *   present in ascending order, -1 behind them, selection[95] = K.  A number outside [0, 95) is not counted and ORs
 *   MP_FLAG_OOB into *flags (the caller zeroes the word).  N = node_splits[G]; splits are clamped to [0, N].
 * mp_scaler_fit_ws_bytes: workspace of the two calls below for G graphs and S states.
 * mp_scaler_normal_f64: Ridge.fit's normal equations.  A (K, K) = X^T W X + alpha I and b (K, S) = X^T W y with X the
 *   count columns selection[0..K), W = diag(sample_weight (G) or 1); fit_intercept centres X and y by their weighted
 *   means first (sklearn's _preprocess_data), which land in mean (K + S) (zeros otherwise).  Buffers: A 95*95, b 95*S,
 *   mean 95+S doubles.
 * mp_scaler_solve_f64: one workgroup, Cholesky of A in FP64 LDS, forward and back substitution for the S right-hand
 *   sides.  coef (95, S): rows [0, K) in selection order, zeros behind; intercept (S) = y_mean - x_mean . coef or 0;
 *   table (95, S) = coef scattered by atomic number, 0 for absent numbers.  *status = 0, or 1 + the column of a
 *   non-positive pivot (then coef, table and intercept are NaN); the host raises ValueError.
 * mp_scaler_residual_std_f64: mol.py:69-73.  scale (S) = sqrt(mean((d - mean(d))^2)) of d = y - (X coef + intercept),
 *   two passes; ones when standardize = 0.
 * mp_scaler_apply: force.py:164-178 (inverse = 0) and :207-222 (inverse = 1) in one launch, one wave per graph.  The
 *   graph's offset (S) = intercept + sum over its atoms of table[Z], straight from the ragged numbers.  Forward:
 *   energy_out = (energy_in - offset) / scale, force_out = force_in / scale; inverse: energy_in * scale + offset,
 *   force_in * scale.  Energies (G, S), forces (N, 3 * S) float32 (that is (N, 3) for S = 1 and (N, 3, S) otherwise),
 *   offset_out (G, S) FP64; energy_in, force_in and offset_out are each nullable.  An atomic number with present[Z] = 0
 *   contributes 0 (the reference's behaviour, which prints a warning) and ORs MP_FLAG_UNKNOWN_SPECIES into *flags, one
 *   outside [0, 95) contributes 0 and ORs MP_FLAG_OOB.  Outputs may alias their inputs. */
#define MP_SCALER_MAX_NUMBER 95
#define MP_SCALER_CHUNK_ROWS 256
#define MP_SCALER_MAX_STATES 32
int mp_scaler_species_count(const void* numbers, int number_kind, const int64_t* node_splits, int64_t G, int64_t N,
                            int32_t* counts, int32_t* mask, int32_t* selection, int32_t* flags, mpStream_t stream);
int mp_scaler_fit_ws_bytes(int64_t G, int S, size_t* bytes_out_host);
int mp_scaler_normal_f64(const int32_t* counts, const int32_t* selection, int64_t G, const void* y, int y_kind, int S,
                         const double* sample_weight, double alpha, int fit_intercept, double* A, double* b,
                         double* mean, void* ws, size_t ws_bytes, mpStream_t stream);
int mp_scaler_solve_f64(const double* A, const double* b, const double* mean, const int32_t* selection, int S,
                        int fit_intercept, double* coef, double* intercept, double* table, int32_t* status,
                        mpStream_t stream);
int mp_scaler_residual_std_f64(const int32_t* counts, const int32_t* selection, int64_t G, const void* y, int y_kind,
                               int S, const double* coef, const double* intercept, int standardize, double* scale,
                               void* ws, size_t ws_bytes, mpStream_t stream);
int mp_scaler_apply(const void* numbers, int number_kind, const int64_t* node_splits, int64_t G, int64_t N, int S,
                    int inverse, const double* table, const int32_t* present, const double* intercept,
                    const double* scale, const void* energy_in, int energy_in_kind, void* energy_out,
                    int energy_out_kind, const float* force_in, float* force_out, double* offset_out, int32_t* flags,
                    mpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_SCALER_H */
