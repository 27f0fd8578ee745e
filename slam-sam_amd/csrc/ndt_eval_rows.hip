// ndt_eval_rows.hip -- what the lane-per-item evaluations share behind their kernels (see ndt_engine.h): D2D
// (ndt_d2d.hip), continuous time (ndt_ct.hip) and GICP (ndt_gicp.hip) each give a lane one item and write one row of EV_WORDS sums per block
// (eval_block_row, ndt_evalrows_device.h).  Here:
//   k_eval_rows_sum        a pose's rows added in a fixed order, one block per pose
//   lane_eval_rows         the host driver: buffers, one launch per pose through the caller's callback, the sum, the copy
//   lane_eval_supported    what such an evaluation can work with
//   finish_words           raw sums -> finished words, for these two and for ndt_eval_derivatives
//   lane_align             newton_align over such an evaluation
#include "ndt_engine.h"

namespace ndt {

namespace {

constexpr int SUM_THREADS = 256, SUM_SEGS = SUM_THREADS / EV_WORDS;   // threads per word

// out[k] = the nb rows of pose k added in a fixed order: SUM_SEGS strided partial sums per word, then those in order
__global__ void __launch_bounds__(SUM_THREADS) k_eval_rows_sum(const double* __restrict__ rows, int nb, double* __restrict__ out) {
  __shared__ double s_seg[SUM_SEGS][EV_WORDS];
  const int word = (int)(threadIdx.x % EV_WORDS), seg = (int)(threadIdx.x / EV_WORDS);
  const double* r = rows + (size_t)blockIdx.x * (size_t)nb * EV_WORDS;
  double s = 0.0;
  for (int b = seg; b < nb; b += SUM_SEGS) s += r[(size_t)b * EV_WORDS + word];
  s_seg[seg][word] = s;
  __syncthreads();
  if (threadIdx.x < EV_WORDS) {
    double t = s_seg[0][word];
#pragma unroll
    for (int k = 1; k < SUM_SEGS; ++k) t += s_seg[k][word];
    out[(size_t)blockIdx.x * EV_WORDS + word] = t;
  }
}

}  // namespace

namespace engine {

void launch_eval_rows_sum(const double* rows, int nb, int K, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_rows_sum, dim3((unsigned)K), dim3(SUM_THREADS), 0, s, rows, nb, out);
}

int lane_eval_supported(ndt_handle* h, const char* what) {
  const std::string w(what);
  if (h->red.mode() != NDT_REDUCE_NONE) return fail(h, NDT_ERR_UNSUPPORTED, w + ": multi-rank evaluation is not supported");
  if (h->prm.search_method != NDT_DIRECT1 && h->prm.search_method != NDT_DIRECT7)
    return fail(h, NDT_ERR_UNSUPPORTED, w + ": the search method must be DIRECT1 or DIRECT7");
  if (h->tgt.is_union()) return fail(h, NDT_ERR_UNSUPPORTED, w + ": a multi-grid union target is not supported");
  if (!h->tgt.have_grid() || h->tgt.n_valid() <= 0) return fail(h, NDT_ERR_NO_TARGET, "no target voxel grid (setInputTarget first)");
  return NDT_OK;
}

int lane_eval_rows(ndt_handle* h, const char* what, int nb, int K, const std::function<void(int, double*)>& launch, double* out) {
  EvalRowBufs& b = h->evrows;
  HIP_TRY(h, b.rows.ensure((size_t)K * (size_t)nb * EV_WORDS));
  HIP_TRY(h, b.out.ensure((size_t)K * EV_WORDS));
  HIP_TRY(h, b.out_h.ensure((size_t)K * EV_WORDS));
  hipStream_t s = h->stream;
  for (int k = 0; k < K; ++k) launch(k, b.rows.p + (size_t)k * (size_t)nb * EV_WORDS);   // one launch per pose: a pose's rows are what they are alone
  launch_eval_rows_sum(b.rows.p, nb, K, b.out.p, s);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(b.out_h.h, b.out.p, (size_t)K * EV_WORDS * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  std::memcpy(out, b.out_h.h, (size_t)K * EV_WORDS * sizeof(double));
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(out[(size_t)k * EV_WORDS + EV_SCORE]))
      return fail(h, NDT_ERR_HIP, std::string(what) + " evaluation returned a non-finite score");
  return NDT_OK;
}

void finish_words(ndt_handle* h, const double pose6[6], bool need_h, double* w) {
  Eval e;
  unpack_eval(w, &e);
  finish_eval(h->prm, h->have_reg ? h->reg_pose : nullptr, pose6, need_h, &e);
  w[EV_SCORE] = e.score;
  for (int i = 0; i < 6; ++i) w[EV_G + i] = e.g[i];
  if (need_h) {   // (without it finish_eval leaves the Hessian words as they came)
    int idx = EV_H;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) w[idx++] = e.H[6 * i + j];
  }
}

int lane_align(ndt_handle* h, int64_t n_items, const float guess[16], const LaneEvalFn& raw, ndt_result* out,
               const ndt_params* prm) {
  const ndt_params& pr = prm ? *prm : h->prm;
  EvalFn fn = [h, &raw, &pr](const double* p, const float*, bool need_h, Eval* e) {
    double words[EV_WORDS];
    if (int r = raw(p, need_h, words)) return r;
    unpack_eval(words, e);
    finish_eval(pr, h->have_reg ? h->reg_pose : nullptr, p, need_h, e);
    return 0;
  };
  // the product path of ndt_align (the Hessian in every trial, the memo on); no iteration history
  const int rc = newton_align(pr, n_items, guess, fn, out, /*hessian_in_trials=*/true);
  h->keepwarm.touch();
  return rc;
}

}  // namespace engine
}  // namespace ndt
