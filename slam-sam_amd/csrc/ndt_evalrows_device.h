// ndt_evalrows_device.h -- the block row of a lane-per-item evaluator (internal; HIP).  k_d2d_eval (ndt_d2d.hip) and
// k_ct_eval (ndt_ct.hip) give every lane one item and its EV_WORDS sums; the sums go lane -> wave (xor butterfly) ->
// block (LDS, wave order) -> one row per block, and k_eval_rows_sum (ndt_eval_rows.hip) adds a pose's rows in a fixed
// order.  No float atomics: a pose's launch and its rows do not depend on the other poses of a call, so it gives the
// bits it gives alone.
#pragma once

#include "ndt_device.h"

namespace ndt {

__device__ __forceinline__ double eval_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  return v;   // (a + b and b + a are the same bits: every lane holds the same sum)
}

// rows[blockIdx.x] = the block's sums of `words`, every thread of the block calling (WAVES x 64 threads, s_part:
// WAVES x EV_WORDS doubles of LDS).  EV_FAIL and, without HESSIAN, the 21 Hessian words are not summed: they are 0.
template <int WAVES, bool HESSIAN>
__device__ __forceinline__ void eval_block_row(const double (&words)[EV_WORDS], double (*s_part)[EV_WORDS], double* __restrict__ rows) {
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < EV_WORDS; ++k) {
    const bool skip = k == EV_FAIL || (!HESSIAN && k >= EV_H && k < EV_H + 21);
    const double s = skip ? 0.0 : eval_wave_sum(words[k]);
    if (lane == 0) s_part[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < EV_WORDS) {
    double s = s_part[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) s += s_part[wv][threadIdx.x];
    rows[(size_t)blockIdx.x * EV_WORDS + threadIdx.x] = s;
  }
}

}  // namespace ndt
