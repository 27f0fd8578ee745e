// ndt_newton.h -- host side of align(): Newton iterations with a More-Thuente
// line search on the 6-vector pose, driving an abstract derivative evaluator
// (the HIP kernels in production).  Internal header.
#pragma once

#include <cmath>
#include <functional>
#include <vector>

#include "../../include/ndt_hip.h"

namespace ndt {

// One global evaluation (already summed over shards / GPUs).
struct Eval {
  double score = 0;
  double g[6] = {0, 0, 0, 0, 0, 0};
  double H[36];  // row-major, symmetric
  double nvtl_sum = 0;
  double n_with = 0;
  double n_pairs = 0;
};

// pose6 -> f32 4x4 (column-major), R = Rx*Ry*Rz built in f32
void pose_to_matrix(const double p[6], float T[16]);
// inverse, angles as Eigen's eulerAngles(0,1,2) returns them
void matrix_to_pose(const float T[16], double p[6]);
// Gauss constants d1, d2 (ref: extern/svn_ndt/include/svn_ndt_impl.hpp:80-131)
void gauss_constants(double resolution, double outlier_ratio, double* d1, double* d2);
// angle tables (ref: svn_ndt_impl.hpp:255-334)
void angle_tables(const double p[6], float jang[24], float hang[45]);
// expands NDT_EVAL_WORDS packed words into an Eval
void unpack_eval(const double* w, Eval* e);
// Word 31 of the packed words (EV_FAIL, ndt_device.h): with several summing blocks only one of them owns it, the others say
// "gave up" by publishing their words as NaN -- read as a lost row, code 1 (a word 31 that is raised already stays as it is).
inline void mark_lost_rows(double* w) {
  if (w[NDT_EVAL_WORDS - 1] != 0.0) return;   // (a NaN there compares unequal too)
  for (int v = 0; v < NDT_EVAL_WORDS; ++v)
    if (std::isnan(w[v])) { w[NDT_EVAL_WORDS - 1] = 1.0; return; }
}
// What evaluate() does about a raised word 31 before a host-side cross-rank sum (the reasons stand there); whatever it
// does not repeat -- 3 has been finished by the host before this is asked -- is left to the final failure check.
enum class Recovery { None, RelaunchPoseTimeout, RelaunchMissingRows, TicketedRetry };
inline Recovery recovery_for(double fail_word, bool via_mailbox, bool safe_retry, bool dev_out) {
  if (fail_word == 2.0 && via_mailbox) return Recovery::RelaunchPoseTimeout;
  if (fail_word == 1.0 && via_mailbox) return Recovery::RelaunchMissingRows;
  if (fail_word == 1.0 && !via_mailbox && !safe_retry && !dev_out) return Recovery::TicketedRetry;
  return Recovery::None;
}
// adds the ridge / regularisation terms and applies the non-finite guards
void finish_eval(const ndt_params& prm, const float* reg_pose, const double p[6], bool need_h, Eval* e);

// fn(pose6, T, need_hessian, out) -> 0 on success
using EvalFn = std::function<int(const double*, const float*, bool, Eval*)>;

// pclomp::NdtResult's per-iteration arrays [RECALLED: tier4 ndt_omp, absent submodule]: entry 0 is the initial guess
// (transform only: its score arrays hold the first evaluation), one entry per Newton iteration after it
struct IterHistory {
  std::vector<float> transforms;            // 16 floats per entry, column-major
  std::vector<double> transform_probability, nvtl;
  void clear() { transforms.clear(); transform_probability.clear(); nvtl.clear(); }
  void push(const float T[16], double tp, double nv) {
    transforms.insert(transforms.end(), T, T + 16);
    transform_probability.push_back(tp);
    nvtl.push_back(nv);
  }
  size_t size() const { return transform_probability.size(); }
};

// state of one bracket end of the More-Thuente search
struct SearchEnd {
  double a, f, g;
};

// One evaluation a NewtonMachine asks for.
struct EvalRequest {
  double p[6];
  float T[16];
  bool need_h;
};

// The Newton / More-Thuente loop of one align as a resumable state machine: next() runs the host arithmetic up to the
// next evaluation that has to be launched (or to the end of the loop), the caller evaluates the request into slot()
// and calls deliver().  Requests the memo can answer (hessian_in_trials: the product path) never leave the machine.
// Driven alone it is newton_align; newton_align_batch drives K of them in lockstep.
//
// hessian_in_trials: ask for the Hessian in every line-search trial instead of one extra
// evaluation at the accepted step (same numbers -- the extra evaluation is at the pose of
// the last trial -- one launch fewer per Newton iteration that needed trials).
class NewtonMachine {
 public:
  NewtonMachine(const ndt_params& prm, int64_t n_source_total, const float guess[16], bool hessian_in_trials,
                IterHistory* history = nullptr);
  // true: *req (valid until deliver) must be evaluated into slot(); false: the loop has stopped (status())
  bool next(const EvalRequest** req);
  Eval* slot() { return &cur_; }
  // the evaluator's return code for the request of the last next(); rc != 0 ends the loop with that code
  void deliver(int rc);
  bool done() const { return st_ == St::Done; }
  int status() const { return rc_; }
  // the result of a stopped loop (ms_total / ms_device are the caller's); after a failed evaluation: zeros and the
  // transform reached so far
  void result(ndt_result* out) const;

 private:
  enum class St { Start, First, Newton, LsFirst, LsLoop, LsTrial, LsEnd, LsReeval, AfterLs, Wait, Done };
  bool ask(const double p[6], const float* T, bool need_h, St then);
  void record(const float* T, const Eval& e);
  void stop(int rc, bool converged);

  ndt_params prm_;
  int64_t n_total_;
  bool h_in_trials_, memo_;
  IterHistory* history_;
  St st_ = St::Start, then_ = St::Start;
  EvalRequest req_;
  int rc_ = 0;
  // Newton state
  double p_[6], score_ = 0, g_[6], H_[36], dp_[6];
  float guess_[16], T_[16], final_T_[16];
  int iters_ = 0;
  bool converged_ = false;
  // line-search state (More-Thuente on phi(a) = -score(p + a dp); see NewtonMachine::next)
  SearchEnd lo_{}, up_{};
  double phi0_ = 0, dphi0_ = 0, a_ = 0, a_max_ = 0, a_min_ = 0, phi_ = 0, dphi_ = 0, psi_ = 0, dpsi_ = 0, xt_[6];
  bool collapsed_ = false, open_ = true;
  int trials_ = 0;
  double s_keep_ = 0, g_keep_[6];
  // the current evaluation and the memo of the last launched one
  Eval cur_;
  int n_evals_ = 0, n_reused_ = 0;
  bool have_last_ = false, last_h_ = false;
  double last_p_[6];
  float last_T_[16];
  Eval last_;
};

int newton_align(const ndt_params& prm, int64_t n_source_total, const float guess[16],
                 const EvalFn& fn, ndt_result* out, bool hessian_in_trials = false, IterHistory* history = nullptr);

// K aligns in lockstep, one batched evaluation per round.  fn(n, reqs, outs) evaluates the n requests of the hypotheses
// still live in this round (in hypothesis order) into outs[0..n).  In every round each live machine runs on the host
// (memo hits included) until it asks for a launched evaluation or stops, so it takes exactly one slot; the call returns
// when the last one has stopped (or with the first failing evaluation's code).  out[k] as newton_align's for guess k,
// ms_total the wall time of the whole call.  rounds_out (nullable): the number of batched evaluations.
using BatchEvalFn = std::function<int(int n, const EvalRequest* const* reqs, Eval* const* outs)>;
int newton_align_batch(const ndt_params& prm, int64_t n_source_total, const float* guesses16, int K,
                       const BatchEvalFn& fn, ndt_result* out, bool hessian_in_trials = false, int* rounds_out = nullptr);

// cov = -(H + eps I)^-1, optionally with the [rotation, translation] block order of a GTSAM
// Pose3 noise model (ref: run/pipeline.cpp:594-596, src/registercallback.cpp:170-186).
// Returns false when H + eps I is singular or not finite.
bool result_covariance(const double H[36], double eps, bool gtsam_order, double cov[36]);

}  // namespace ndt
