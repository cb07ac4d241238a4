// The segment-softmax attention of one wave over one receiver's range of sorted positions, for afp_attend_kernel
// (csrc/mp_attentivefp.hip: message rows stored by position).  The sweeps are gat_attend_kernel's (csrc/mp_gat.hip:
// message rows gathered by the sender), with the position and row accessors as parameters.  gat_attend_kernel keeps its
// own text: built on this header its instruction stream came out 5 % longer and the default GAT / GATv2 models replayed
// 1.5 % / 3.3 % slower in two runs each.  Header-only: no kernels, no entry points.
//
//   sweep 1  the maximum: lane l takes positions l, l + 64, ...; butterfly maximum (exact in any order).
//   sweep 2  the sum of exp(logit - max): every lane adds its own positions in list order, then the xor butterfly of
//            mp_wave_sum adds the 64 partials in a fixed order.
//   sweep 3  the weighted rows: the segment in chunks of 64 positions; lane l holds (row key, weight) of position l of the
//            chunk, weight = exp(logit - max) / sum; the 64 lanes are 64 / U position groups x U columns; group k adds
//            positions k, k + 64 / U, ... of every chunk in list order, the groups are added in group order.
// The order of every sum is fixed by the list order and the lane layout alone: no atomics, two runs give equal bits.
#pragma once
#include "mp_common.h"

namespace mp_attend {

// pos(p, &logit, &key): false for a position the logit kernels skip, else its logit and the key of its message row;
// row(key, col): column `col` of that message row.  Returns, in the lanes of group 0 (lane < U), column lane of
// sum_p softmax_p(logit_p) row_p over [lo, hi); 0 for an empty range.  lo, hi wave-uniform; U 32 or 64.
template <int U, class PosFn, class RowFn>
__device__ __forceinline__ float wave_rows(int lo, int hi, int lane, const PosFn& pos, const RowFn& row) {
  constexpr int G = 64 / U;   // position groups of the wave in sweep 3
  const int col = lane % U, grp = lane / U;
  // sweep 1
  float mx = -INFINITY;
  for (int p = lo + lane; p < hi; p += 64) {
    float l;
    int k;
    if (pos(p, &l, &k)) mx = fmaxf(mx, l);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  // sweep 2
  float part = 0.0f;
  for (int p = lo + lane; p < hi; p += 64) {
    float l;
    int k;
    if (pos(p, &l, &k)) part += expf(l - mx);
  }
  const float sum = mp_wave_sum(part);
  // sweep 3
  float acc = 0.0f;
  for (int c0 = lo; c0 < hi; c0 += 64) {   // wave-uniform bounds
    int key = 0;
    float w = 0.0f;
    if (c0 + lane < hi) {
      float l;
      int k;
      if (pos(c0 + lane, &l, &k)) {
        w = expf(l - mx) / sum;
        key = k;
      }
    }
    const int n = hi - c0 < 64 ? hi - c0 : 64;
    for (int j = 0; j < n; j += G) {
      const int src = j + grp;             // positions past n hold w = 0, key = 0
      const float wj = __shfl(w, src, 64);
      const int kj = __shfl(key, src, 64);
      if (wj != 0.0f) acc += wj * row(kj, col);
    }
  }
  if (G == 2) {
    const float other = __shfl(acc, lane + 32, 64);   // group 0 + group 1
    acc += other;
  }
  return acc;
}

}  // namespace mp_attend
