// ndt_ct.hip -- continuous-time NDT: a scan captured in motion registered with one pose PER POINT, blended between the
// known begin pose and the unknown end pose by the point's time factor (see ndt_engine.h; the rule is stated in
// include/ndt_hip.h).
//   ndt_set_source_times*           one float per point of the current point source, kept on the device
//   ndt_eval_derivatives_ct         per pose one launch of k_ct_eval<HESSIAN, D7> -- one point per lane: its own pose, three
//                                   sincos in f64, the moved point, its neighbours by ndt_neighbors_device.h as every
//                                   evaluator's -- and one launch of the fixed-order sum over all poses (lane_eval_rows)
//   ndt_align_ct                    newton_align over that evaluation
//   ndt_transform_source_ct*        k_ct_apply: the deskewed scan under a result
// What a pair adds to gradient and Hessian is linear in f v and f (B - d2 v v^T) (v = B mu, f = d1 d2 e) once the point's
// j_c and h_cd are fixed, so a lane sums those nine numbers over its <= 7 pairs and meets j and h once, behind the pairs.
// Sums: lane -> wave -> block -> one row per block (eval_block_row, ndt_evalrows_device.h) -> k_eval_rows_sum in fixed
// order; the host side around the launches (lane_eval_rows, finish_words, lane_align) is ndt_eval_rows.hip's, shared with
// D2D.  The source is read as handed over (vx / vy / vz); the block-ordered copy, the align state and the iteration
// history of the handle are not touched.
#include "ndt_engine.h"
#include "ndt_evalrows_device.h"
#include "ndt_neighbors_device.h"

namespace ndt {

namespace {

constexpr int CT_THREADS = 256, CT_WAVES = CT_THREADS / 64;

struct CtPoses {
  double b[6], p[6];   // begin and end pose [x, y, z, roll, pitch, yaw]
};

// x moved by the pose q, one rotation after the other, every operation one f64 rounding:
//   u = Rz(yaw) x,  v = Ry(pitch) u,  w = Rx(roll) v,  x' = w + t
struct CtMoved {
  double sr, cr, sp, cp, sy, cy;
  double u[3], v[3], w[3], m[3];
};

// a_i and the point's pose; false: the time is not finite
__device__ __forceinline__ bool ct_pose(const CtPoses& P, float alpha, double* a_out, double q[6]) {
  if (!isfinite(alpha)) return false;
  const double a = alpha < 0.0f ? 0.0 : alpha > 1.0f ? 1.0 : (double)alpha;
#pragma unroll
  for (int c = 0; c < 6; ++c) q[c] = a == 1.0 ? P.p[c] : a == 0.0 ? P.b[c] : P.b[c] + a * (P.p[c] - P.b[c]);
  *a_out = a;
  return true;
}

__device__ __forceinline__ void ct_move(const double q[6], const double x[3], CtMoved& M) {
  sincos(q[3], &M.sr, &M.cr);
  sincos(q[4], &M.sp, &M.cp);
  sincos(q[5], &M.sy, &M.cy);
  M.u[0] = M.cy * x[0] - M.sy * x[1];
  M.u[1] = M.sy * x[0] + M.cy * x[1];
  M.u[2] = x[2];
  M.v[0] = M.cp * M.u[0] + M.sp * M.u[2];
  M.v[1] = M.u[1];
  M.v[2] = M.cp * M.u[2] - M.sp * M.u[0];
  M.w[0] = M.v[0];
  M.w[1] = M.cr * M.v[1] - M.sr * M.v[2];
  M.w[2] = M.sr * M.v[1] + M.cr * M.v[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) M.m[a] = M.w[a] + q[a];
}

// o = Rx(roll) Ry(pitch) c and o = Rx(roll) c
__device__ __forceinline__ void ct_rx(const CtMoved& M, const double c[3], double o[3]) {
  o[0] = c[0];
  o[1] = M.cr * c[1] - M.sr * c[2];
  o[2] = M.sr * c[1] + M.cr * c[2];
}
__device__ __forceinline__ void ct_rxry(const CtMoved& M, const double c[3], double o[3]) {
  const double d[3] = {M.cp * c[0] + M.sp * c[2], c[1], M.cp * c[2] - M.sp * c[0]};
  ct_rx(M, d, o);
}

__device__ __forceinline__ double ct_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// One point per lane: its pose, the moved point, the neighbours of the f32-rounded moved point (neighbor_cells7: DIRECT1 /
// DIRECT7, the pair order of every evaluator), the pairs, and the block's row of EV_WORDS sums (word 31 = 0).
template <bool HESSIAN, bool D7>
__global__ void __launch_bounds__(CT_THREADS)
k_ct_eval(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const float* __restrict__ alpha,
          int n, GridGeom g, const int* __restrict__ cell2leaf, const LeafStats* __restrict__ stats, CtPoses P, double d1, double d2,
          double* __restrict__ rows) {
  __shared__ double s_part[CT_WAVES][EV_WORDS];
  const int i = (int)(blockIdx.x * CT_THREADS + threadIdx.x);
  double words[EV_WORDS];
#pragma unroll
  for (int k = 0; k < EV_WORDS; ++k) words[k] = 0.0;
  double a = 0.0, q[6];
  float xf = 0.0f, yf = 0.0f, zf = 0.0f;
  bool live = false;
  if (i < n) {
    xf = sx[i]; yf = sy[i]; zf = sz[i];
    live = ct_pose(P, alpha[i], &a, q) && isfinite(xf) && isfinite(yf) && isfinite(zf);
  }
  if (live) {
    const double x[3] = {(double)xf, (double)yf, (double)zf};
    CtMoved M;
    ct_move(q, x, M);
    float xt = (float)M.m[0], yt = (float)M.m[1], zt = (float)M.m[2];
    const bool finite = isfinite(xt) && isfinite(yt) && isfinite(zt);
    if (!finite) { xt = 0.0f; yt = 0.0f; zt = 0.0f; }   // as k_point_scores: no NaN / Inf reaches the index casts
    int cell[7], slots[7];
    neighbor_cells7<D7>(xt, yt, zt, g, cell);
    neighbor_slots7<D7>(cell, finite, cell2leaf, slots);
    double score = 0.0, best = 0.0, fw[3] = {0.0, 0.0, 0.0};
    double Mxx = 0.0, Mxy = 0.0, Mxz = 0.0, Myy = 0.0, Myz = 0.0, Mzz = 0.0;   // sum of f (B - d2 v v^T)
    int npairs = 0;
#pragma unroll
    for (int k = 0; k < (D7 ? 7 : 1); ++k) {
      const int slot = slots[k];
      if (slot < 0) continue;
      const LeafStats& L = stats[slot];
      const double mu[3] = {M.m[0] - L.mean[0], M.m[1] - L.mean[1], M.m[2] - L.mean[2]};
      const double Bxx = L.icov[0], Bxy = L.icov[1], Bxz = L.icov[2], Byy = L.icov[4], Byz = L.icov[5], Bzz = L.icov[8];
      const double v[3] = {(Bxx * mu[0] + Bxy * mu[1]) + Bxz * mu[2], (Bxy * mu[0] + Byy * mu[1]) + Byz * mu[2],
                           (Bxz * mu[0] + Byz * mu[1]) + Bzz * mu[2]};
      const double e = exp(-d2 * ct_dot(mu, v) * 0.5);
      if (!(e >= 0.0 && e <= 1.0)) continue;   // the evaluation's guard (a NaN fails both compares)
      const double sc = -d1 * e;
      score += sc;
      best = fmax(best, sc);
      npairs += 1;
      const double f = (d1 * d2) * e;
      fw[0] += f * v[0]; fw[1] += f * v[1]; fw[2] += f * v[2];
      if (HESSIAN) {
        Mxx += f * (Bxx - d2 * (v[0] * v[0])); Mxy += f * (Bxy - d2 * (v[0] * v[1])); Mxz += f * (Bxz - d2 * (v[0] * v[2]));
        Myy += f * (Byy - d2 * (v[1] * v[1])); Myz += f * (Byz - d2 * (v[1] * v[2])); Mzz += f * (Bzz - d2 * (v[2] * v[2]));
      }
    }
    if (npairs > 0) {
      // j_c = d x' / d (p_i)_c for roll, pitch, yaw, straight from the chain u -> v -> w
      double j[3][3];
      j[0][0] = 0.0; j[0][1] = -M.w[2]; j[0][2] = M.w[1];
      const double dv[3] = {M.v[2], 0.0, -M.v[0]};          // (dRy / dpitch) u
      ct_rx(M, dv, j[1]);
      const double du[3] = {-M.u[1], M.u[0], 0.0};          // (dRz / dyaw) x
      ct_rxry(M, du, j[2]);
      words[EV_SCORE] = score;
      words[EV_NVTL] = best;
      words[EV_NWITH] = 1.0;
      words[EV_NPAIRS] = (double)npairs;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        words[EV_G + c] = a * fw[c];
        words[EV_G + 3 + c] = a * ct_dot(fw, j[c]);
      }
      if (HESSIAN) {
        const double a2 = a * a;
        // translation block: M itself; translation x rotation: M j_d; rotation block: j_c^T M j_d + (f v)^T h_cd
        double Mj[3][3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          Mj[d][0] = (Mxx * j[d][0] + Mxy * j[d][1]) + Mxz * j[d][2];
          Mj[d][1] = (Mxy * j[d][0] + Myy * j[d][1]) + Myz * j[d][2];
          Mj[d][2] = (Mxz * j[d][0] + Myz * j[d][1]) + Mzz * j[d][2];
        }
        // h_cd = d2 x' / d (p_i)_c d (p_i)_d: rr, rp, ry, pp, py, yy
        double h[6][3];
        h[0][0] = 0.0; h[0][1] = -M.w[1]; h[0][2] = -M.w[2];
        h[1][0] = 0.0; h[1][1] = -j[1][2]; h[1][2] = j[1][1];
        h[2][0] = 0.0; h[2][1] = -j[2][2]; h[2][2] = j[2][1];
        const double d2v[3] = {-M.v[0], 0.0, -M.v[2]};      // (d2Ry / dpitch2) u
        ct_rx(M, d2v, h[3]);
        const double dvu[3] = {M.sp * M.u[1], 0.0, M.cp * M.u[1]};   // (dRy / dpitch) (dRz / dyaw) x
        ct_rx(M, dvu, h[4]);
        const double d2u[3] = {-M.u[0], -M.u[1], 0.0};      // (d2Rz / dyaw2) x
        ct_rxry(M, d2u, h[5]);
        // upper triangle row by row: rows 0 .. 2 hold 6 + 5 + 4 words, then the rotation block
        words[EV_H + 0] = a2 * Mxx; words[EV_H + 1] = a2 * Mxy; words[EV_H + 2] = a2 * Mxz;
        words[EV_H + 6] = a2 * Myy; words[EV_H + 7] = a2 * Myz;
        words[EV_H + 11] = a2 * Mzz;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          words[EV_H + 3 + d] = a2 * Mj[d][0];
          words[EV_H + 8 + d] = a2 * Mj[d][1];
          words[EV_H + 12 + d] = a2 * Mj[d][2];
        }
        int q2 = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int d = c; d < 3; ++d) {
            words[EV_H + 15 + q2] = a2 * (ct_dot(j[c], Mj[d]) + ct_dot(fw, h[q2]));
            ++q2;
          }
      }
    }
  }
  // lane -> wave -> block
  eval_block_row<CT_WAVES, HESSIAN>(words, s_part, rows);
}

// The deskewed scan: point i moved by its own pose, in the target's frame (frame 1) or brought back into the END pose's
// frame (frame 0: R(e)^T (x' - t(e)), the rotations undone one after the other); f64, rounded to f32 once.  A point whose
// pose IS the end pose, number for number, comes back as it is in frame 0.
__global__ void __launch_bounds__(CT_THREADS)
k_ct_apply(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const float* __restrict__ alpha,
           int n, CtPoses P, int frame, float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz) {
  const int i = (int)(blockIdx.x * CT_THREADS + threadIdx.x);
  if (i >= n) return;
  const float xf = sx[i], yf = sy[i], zf = sz[i];
  double a, q[6];
  float rx = nanf(""), ry = nanf(""), rz = nanf("");
  if (ct_pose(P, alpha[i], &a, q) && isfinite(xf) && isfinite(yf) && isfinite(zf)) {
    bool same = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) same = same && q[c] == P.p[c];
    if (frame == 0 && same) {
      rx = xf; ry = yf; rz = zf;
    } else {
      const double x[3] = {(double)xf, (double)yf, (double)zf};
      CtMoved M;
      ct_move(q, x, M);
      double y[3] = {M.m[0], M.m[1], M.m[2]};
      if (frame == 0) {
        double sr, cr, sp, cp, sy_, cy_;
        sincos(P.p[3], &sr, &cr);
        sincos(P.p[4], &sp, &cp);
        sincos(P.p[5], &sy_, &cy_);
        const double w[3] = {M.m[0] - P.p[0], M.m[1] - P.p[1], M.m[2] - P.p[2]};
        const double v[3] = {w[0], cr * w[1] + sr * w[2], cr * w[2] - sr * w[1]};      // Rx^T
        const double u[3] = {cp * v[0] - sp * v[2], v[1], sp * v[0] + cp * v[2]};      // Ry^T
        y[0] = cy_ * u[0] + sy_ * u[1];                                                 // Rz^T
        y[1] = cy_ * u[1] - sy_ * u[0];
        y[2] = u[2];
      }
      rx = (float)y[0]; ry = (float)y[1]; rz = (float)y[2];
    }
  }
  ox[i] = rx; oy[i] = ry; oz[i] = rz;
}

int ct_blocks(size_t n) { return (int)((n + CT_THREADS - 1) / CT_THREADS); }

}  // namespace

namespace engine {
namespace {

// the point source and its times, for every _ct call
int ct_source_ready(ndt_handle* h) {
  if (int rc = settle_source(h)) return rc;
  if (h->n_src == 0 || !h->vx) return fail(h, NDT_ERR_NO_SOURCE, "no source cloud (setInputSource first)");
  if (h->ct.n != h->n_src) return fail(h, NDT_ERR_NO_SOURCE, "no source times (ndt_set_source_times after the source)");
  return NDT_OK;
}

// what a CT evaluation can work with: DIRECT1 / DIRECT7 on a single grid, one rank; then target, source and times
int ct_ready(ndt_handle* h) {
  if (int rc = settle(h)) return rc;
  if (int rc = lane_eval_supported(h, "CT")) return rc;
  return ct_source_ready(h);
}

// The blend is linear in the angles as given, so the begin pose's are brought onto the branch of the angles `ref3` (the
// end pose's, or the guess's): of the two Euler triples of its rotation -- (r, p, y) and (r + pi, pi - p, y + pi) -- each
// angle shifted by a multiple of 2 pi to within pi of its counterpart, the triple that then lies nearer (sum of the
// three absolute differences; a tie keeps the first).  A begin pose on the branch already comes back bit for bit.
void ct_fit_begin(const double begin6[6], const double ref3[3], double out6[6]) {
  const double pi = 3.14159265358979323846, two_pi = 2.0 * pi;
  double cand[2][3] = {{begin6[3], begin6[4], begin6[5]}, {begin6[3] + pi, pi - begin6[4], begin6[5] + pi}}, dist[2] = {0.0, 0.0};
  for (int t = 0; t < 2; ++t)
    for (int c = 0; c < 3; ++c) {
      const double turns = std::round((cand[t][c] - ref3[c]) / two_pi);
      if (turns != 0.0) cand[t][c] -= two_pi * turns;
      dist[t] += std::fabs(cand[t][c] - ref3[c]);
    }
  std::memcpy(out6, begin6, 3 * sizeof(double));
  std::memcpy(out6 + 3, cand[dist[1] < dist[0] ? 1 : 0], 3 * sizeof(double));
}

// K end poses -> K x EV_WORDS raw sums in `out`; ct_ready has passed.  fit: the begin pose is fitted to each end pose
// (the public evaluation); the align hands over the one it fitted to its guess
int ct_eval_raw(ndt_handle* h, const double begin6[6], const double* poses6, int K, bool need_h, double* out, bool fit) {
  const int n = (int)h->n_src, nb = ct_blocks(h->n_src);
  double d1, d2;
  gauss_constants((double)h->prm.resolution, h->prm.outlier_ratio, &d1, &d2);
  const bool d7 = h->prm.search_method == NDT_DIRECT7;
  const dim3 grid((unsigned)nb), block(CT_THREADS);
  return lane_eval_rows(h, "CT", nb, K, [&](int k, double* rows) {
    CtPoses P;
    std::memcpy(P.p, poses6 + 6 * (size_t)k, sizeof(P.p));
    if (fit) ct_fit_begin(begin6, P.p + 3, P.b);
    else std::memcpy(P.b, begin6, sizeof(P.b));
#define NDT_CT_LAUNCH(H, D7) \
  hipLaunchKernelGGL((k_ct_eval<H, D7>), grid, block, 0, h->stream, h->vx, h->vy, h->vz, h->ct.alpha.p, n, h->geom, h->cell2leaf.p, \
                     h->stats.p, P, d1, d2, rows)
    if (need_h) { if (d7) NDT_CT_LAUNCH(true, true); else NDT_CT_LAUNCH(true, false); }
    else { if (d7) NDT_CT_LAUNCH(false, true); else NDT_CT_LAUNCH(false, false); }
#undef NDT_CT_LAUNCH
  }, out);
}

int ct_apply(ndt_handle* h, const double begin6[6], const double end6[6], int frame, float* ox, float* oy, float* oz) {
  CtPoses P;
  std::memcpy(P.p, end6, sizeof(P.p));
  ct_fit_begin(begin6, P.p + 3, P.b);
  hipLaunchKernelGGL(k_ct_apply, dim3((unsigned)ct_blocks(h->n_src)), dim3(CT_THREADS), 0, h->stream, h->vx, h->vy, h->vz,
                     h->ct.alpha.p, (int)h->n_src, P, frame, ox, oy, oz);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

bool ct_too_many(size_t n) { return n > (size_t)std::numeric_limits<int>::max() / 2; }

int ct_times_size(ndt_handle* h, size_t n) {
  if (n != h->n_src)
    return fail(h, NDT_ERR_INVALID_ARG, "source times: " + std::to_string(n) + " times for a source of " + std::to_string(h->n_src) + " points");
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_set_source_times(ndt_handle* h, const float* alpha, size_t n) {
  if (!h || (n && !alpha) || ct_too_many(n)) return NDT_ERR_INVALID_ARG;
  if (n == 0) { h->ct.n = 0; return NDT_OK; }
  if (int rc = ct_times_size(h, n)) return rc;
  if (int rc = bind_device(h)) return rc;
  HIP_TRY(h, h->ct.alpha.ensure(n));
  h->ct.n = 0;   // (from here on the previous times are gone)
  HIP_TRY(h, hipMemcpyAsync(h->ct.alpha.p, alpha, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->ct.n = n;
  return NDT_OK;
}

int ndt_set_source_times_device(ndt_handle* h, const float* d_alpha, size_t n) {
  if (!h || (n && !d_alpha) || ct_too_many(n)) return NDT_ERR_INVALID_ARG;
  if (n == 0) { h->ct.n = 0; return NDT_OK; }
  if (int rc = ct_times_size(h, n)) return rc;
  if (int rc = bind_device(h)) return rc;
  HIP_TRY(h, h->ct.alpha.ensure(n));
  h->ct.n = 0;
  HIP_TRY(h, hipMemcpyAsync(h->ct.alpha.p, d_alpha, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // the caller's array is consumed during the call
  h->ct.n = n;
  return NDT_OK;
}

int64_t ndt_source_times_info(const ndt_handle* h) { return h ? (int64_t)h->ct.n : NDT_ERR_INVALID_ARG; }

int ndt_eval_derivatives_ct(ndt_handle* h, const double begin_pose6[6], const double* poses6, int K, int compute_hessian,
                            double* out) {
  if (!h || !begin_pose6 || !poses6 || !out || K <= 0 || !all_finite(begin_pose6, 6)) return NDT_ERR_INVALID_ARG;
  for (int k = 0; k < K; ++k)
    if (!all_finite(poses6 + 6 * (size_t)k, 6)) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = ct_ready(h)) return rc;
  if (int rc = ct_eval_raw(h, begin_pose6, poses6, K, compute_hessian != 0, out, /*fit=*/true)) return rc;
  for (int k = 0; k < K; ++k) finish_words(h, poses6 + 6 * (size_t)k, compute_hessian != 0, out + (size_t)k * EV_WORDS);
  return NDT_OK;
}

int ndt_align_ct(ndt_handle* h, const double begin_pose6[6], const float guess[16], ndt_result* out) {
  if (!h || !begin_pose6 || !guess || !out || !all_finite(begin_pose6, 6)) return NDT_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));   // what every failure before the loop leaves: the guess, not converged
  std::memcpy(out->final_transformation, guess, sizeof(float) * 16);
  if (int rc = bind_device(h)) return rc;
  h->keepwarm.touch();
  if (int rc = ct_ready(h)) return rc;
  // the begin pose fitted ONCE, to the pose the loop starts from (matrix_to_pose folds the roll into [0, pi], so a guess
  // with a slightly negative roll starts on the other triple): the objective does not change under the loop
  double b[6], g6[6];
  matrix_to_pose(guess, g6);
  if (all_finite(g6, 6)) ct_fit_begin(begin_pose6, g6 + 3, b);
  else std::memcpy(b, begin_pose6, sizeof(b));
  return lane_align(h, (int64_t)h->n_src, guess, [h, &b](const double* p, bool need_h, double* words) {
    return ct_eval_raw(h, b, p, 1, need_h, words, /*fit=*/false);
  }, out);
}

int ndt_transform_source_ct_device(ndt_handle* h, const double begin_pose6[6], const double end_pose6[6], int frame, float* ox,
                                   float* oy, float* oz, size_t cap) {
  if (!h || !begin_pose6 || !end_pose6 || !ox || !oy || !oz || (frame != 0 && frame != 1) || !all_finite(begin_pose6, 6) ||
      !all_finite(end_pose6, 6))
    return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = ct_source_ready(h)) return rc;
  if (cap < h->n_src) return over_capacity(h, h->n_src);
  return ct_apply(h, begin_pose6, end_pose6, frame, ox, oy, oz);
}

int ndt_transform_source_ct(ndt_handle* h, const double begin_pose6[6], const double end_pose6[6], int frame, float* out_xyz,
                            size_t cap_points) {
  if (!h || !begin_pose6 || !end_pose6 || !out_xyz || (frame != 0 && frame != 1) || !all_finite(begin_pose6, 6) ||
      !all_finite(end_pose6, 6))
    return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = ct_source_ready(h)) return rc;
  const size_t n = h->n_src;
  if (cap_points < n) return over_capacity(h, n);
  HIP_TRY(h, h->ct.xyz.ensure(3 * n));
  float* d = h->ct.xyz.p;
  if (int rc = ct_apply(h, begin_pose6, end_pose6, frame, d, d + n, d + 2 * n)) return rc;
  return download_strided(h, d, n, n, cap_points, out_xyz, 3 * sizeof(float), -1);
}

}  // extern "C"
