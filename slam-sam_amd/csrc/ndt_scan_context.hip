// ndt_scan_context.hip -- Scan Context place recognition over the device keyframe archive (see ndt_engine.h; the rule is
// written out in include/ndt_hip.h).  A scan becomes a rings x sectors matrix of maximum heights (k_sc_bins: block-private
// LDS bins, integer atomics only, merged once per block; k_sc_finish: the minimum-count rule), the descriptors of the
// archived scans sit in a bank beside the archive, and k_sc_match compares one query with every entry of the bank at every
// cyclic column shift: one workgroup per entry, one lane per shift, fixed order, f64.
#include "ndt_engine.h"

namespace ndt {
namespace engine {
namespace {

constexpr int SC_THREADS = 256;           // k_sc_bins / k_sc_finish
constexpr int SC_POINTS_PER_BLOCK = 512;  // two points per thread and one merge of the touched bins per block
constexpr int SC_MAX_BLOCKS = 2048;
constexpr int SC_MAX_RINGS = 32, SC_MAX_SECTORS = 128;
constexpr int SC_COLS = 4;                // k_sc_match: query columns whose dot products run side by side

struct ScBinArgs {
  int R, S;
  float max_radius, z_sign, lift;
};

__device__ __forceinline__ bool sc_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// c_k of the header: the products are exact in f64, so the sign of the difference is
__device__ __forceinline__ double sc_cross(const float* dir, int k, float x, float y) {
  return (double)dir[2 * k] * (double)y - (double)dir[2 * k + 1] * (double)x;
}

// LDS: [height bits (R x S) | counts (R x S) | the sector table (2 S floats)].  acc: the same two arrays in HBM, zero
// before the launch.  Heights are >= +0, so their bit patterns order as unsigned integers.
__global__ void __launch_bounds__(SC_THREADS) k_sc_bins(const float* __restrict__ px, const float* __restrict__ py,
                                                        const float* __restrict__ pz, int n, ScBinArgs a,
                                                        const float* __restrict__ dir_g, uint32_t* __restrict__ acc) {
  extern __shared__ uint32_t sc_lds[];
  const int bins = a.R * a.S;
  uint32_t* lh = sc_lds;
  uint32_t* lc = sc_lds + bins;
  float* dir = reinterpret_cast<float*>(sc_lds + 2 * bins);
  for (int i = (int)threadIdx.x; i < 2 * bins; i += SC_THREADS) sc_lds[i] = 0u;
  for (int i = (int)threadIdx.x; i < 2 * a.S; i += SC_THREADS) dir[i] = dir_g[i];
  __syncthreads();
  const double max_r = (double)a.max_radius;
  const float sectors_per_rad = (float)a.S * 0.15915494f;
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < (long long)n; i += (long long)gridDim.x * SC_THREADS) {
    const float x = px[i], y = py[i], z = pz[i];
    if (!sc_finite(x) || !sc_finite(y) || !sc_finite(z) || (x == 0.0f && y == 0.0f)) continue;
    const double r2 = (double)x * (double)x + (double)y * (double)y;
    const double rho = sqrt(r2);
    if (!(rho < max_r)) continue;
    const int ring = min((int)(rho * (double)a.R / max_r), a.R - 1);
    // the sector: a guess from atan2f, settled by the exact tests (backwards while c_s < 0, forwards while c_{s+1} >= 0;
    // either walk is monotone, and a guess is off by one at most unless atan2f is far off)
    float ang = atan2f(y, x);
    if (ang < 0.0f) ang += 6.2831855f;
    int s = min(max((int)(ang * sectors_per_rad), 0), a.S - 1);
    for (int step = 0; step < a.S; ++step) {
      if (sc_cross(dir, s, x, y) < 0.0) { s = s == 0 ? a.S - 1 : s - 1; continue; }
      const int s1 = s + 1 == a.S ? 0 : s + 1;
      if (sc_cross(dir, s1, x, y) < 0.0) break;
      s = s1;
    }
    const float hgt = a.z_sign * z + a.lift;
    const int b = ring * a.S + s;
    atomicAdd(&lc[b], 1u);
    if (hgt > 0.0f) atomicMax(&lh[b], __float_as_uint(hgt));
  }
  __syncthreads();
  for (int b = (int)threadIdx.x; b < bins; b += SC_THREADS) {
    const uint32_t c = lc[b];
    if (c == 0u) continue;
    atomicAdd(&acc[bins + b], c);
    if (lh[b]) atomicMax(&acc[b], lh[b]);
  }
}

__global__ void __launch_bounds__(SC_THREADS) k_sc_finish(const uint32_t* __restrict__ acc, int bins, int min_points,
                                                          float* __restrict__ desc, int32_t* __restrict__ count) {
  const int b = (int)(blockIdx.x * SC_THREADS + threadIdx.x);
  if (b >= bins) return;
  const int32_t c = (int32_t)acc[bins + b];
  desc[b] = c < min_points ? 0.0f : __uint_as_float(acc[b]);
  if (count) count[b] = c;
}

// One workgroup per bank entry (order[blockIdx.x]: its slot), one lane per shift (S > 64: two waves).
// LDS: [nQ (S) | nC (S) | d (S) | Q (R x S) doubles | m (S) ints | C (R x S) floats].  Q is held in f64: its element is the
// same for every lane (a broadcast read) and needs no conversion in the inner loop; C's read is consecutive across lanes.
// The product of two f32 values is exact in f64, so fma(q, c, dot) IS dot + q * c of the rule, in one instruction.
__global__ void __launch_bounds__(128) k_sc_match(const float* __restrict__ query, const float* __restrict__ bank,
                                                  const int* __restrict__ order, int R, int S, double* __restrict__ dist,
                                                  int32_t* __restrict__ shift, int32_t* __restrict__ cols) {
  extern __shared__ double sc_match_lds[];
  const int bins = R * S, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  double* nQ = sc_match_lds;
  double* nC = nQ + S;
  double* dn = nC + S;
  double* Q = dn + S;
  int* mn = reinterpret_cast<int*>(Q + bins);
  float* Cm = reinterpret_cast<float*>(mn + S);
  const float* Cg = bank + (size_t)order[blockIdx.x] * (size_t)bins;
  if ((bins & 3) == 0) {   // (then every slot of the bank starts on 16 bytes) four 16-byte loads in flight per lane and matrix
    const float4* q4 = reinterpret_cast<const float4*>(query);
    const float4* c4 = reinterpret_cast<const float4*>(Cg);
    const int n4 = bins >> 2;
    for (int i0 = tid; i0 < n4; i0 += 4 * nt) {
      float4 q[4], c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = min(i0 + u * nt, n4 - 1);
        q[u] = q4[i];
        c[u] = c4[i];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * nt;
        if (i >= n4) break;
        Q[4 * i] = (double)q[u].x; Q[4 * i + 1] = (double)q[u].y; Q[4 * i + 2] = (double)q[u].z; Q[4 * i + 3] = (double)q[u].w;
        Cm[4 * i] = c[u].x; Cm[4 * i + 1] = c[u].y; Cm[4 * i + 2] = c[u].z; Cm[4 * i + 3] = c[u].w;
      }
    }
  } else {
    for (int i = tid; i < bins; i += nt) { Q[i] = (double)query[i]; Cm[i] = Cg[i]; }
  }
  __syncthreads();
  for (int j = tid; j < S; j += nt) {
    double q = 0.0, c = 0.0;
    for (int r = 0; r < R; ++r) {
      const double qv = Q[r * S + j], cv = (double)Cm[r * S + j];
      q += qv * qv;
      c += cv * cv;
    }
    nQ[j] = sqrt(q);
    nC[j] = sqrt(c);
  }
  __syncthreads();
  for (int n = tid; n < S; n += nt) {
    // Four columns at a time: their dot products are four independent chains over r (each in the rule's order), which
    // hides the latency of the LDS reads and of the f64 adds; a column the rule skips is computed and dropped, and the
    // sum takes the columns in ascending j.
    double sum = 0.0;
    int m = 0;
    for (int j0 = 0; j0 < S; j0 += SC_COLS) {
      double dot[SC_COLS];
      int jq[SC_COLS], jc[SC_COLS];
#pragma unroll
      for (int u = 0; u < SC_COLS; ++u) {
        jq[u] = min(j0 + u, S - 1);          // (past the last column: read column S - 1 again, use nothing)
        jc[u] = jq[u] + n >= S ? jq[u] + n - S : jq[u] + n;
        dot[u] = 0.0;
      }
#pragma unroll 4
      for (int r = 0; r < R; ++r) {   // (unrolled: the LDS reads of four rings are in flight before the first fma waits)
#pragma unroll
        for (int u = 0; u < SC_COLS; ++u) dot[u] = fma(Q[r * S + jq[u]], (double)Cm[r * S + jc[u]], dot[u]);
      }
#pragma unroll
      for (int u = 0; u < SC_COLS; ++u) {
        const double a = nQ[jq[u]], b = nC[jc[u]];
        if (j0 + u < S && a != 0.0 && b != 0.0) {
          sum += 1.0 - dot[u] / (a * b);
          ++m;
        }
      }
    }
    dn[n] = m > 0 ? sum / (double)m : 1.0;
    mn[n] = m;
  }
  __syncthreads();
  if (tid == 0) {
    double best = dn[0];
    int at = 0;
    for (int n = 1; n < S; ++n)
      if (dn[n] < best) { best = dn[n]; at = n; }
    dist[blockIdx.x] = best;
    shift[blockIdx.x] = at;
    cols[blockIdx.x] = mn[at];
  }
}

bool sc_params_ok(const ndt_scan_context_params* p) {
  return p->n_rings >= 1 && p->n_rings <= SC_MAX_RINGS && p->n_sectors >= 3 && p->n_sectors <= SC_MAX_SECTORS &&
         std::isfinite(p->max_radius) && p->max_radius > 0.0f && (p->z_sign == 1.0f || p->z_sign == -1.0f) &&
         std::isfinite(p->lift) && p->min_points_per_bin >= 1;
}

void sc_sector_table(int S, float* dir) {
  for (int k = 0; k < S; ++k) {
    const double a = 2.0 * M_PI * (double)k / (double)S;
    dir[2 * k] = (float)std::cos(a);
    dir[2 * k + 1] = (float)std::sin(a);
  }
}

int sc_table(ndt_handle* h) {
  ScanContextBufs& sc = h->sc;
  if (sc.table_valid) return NDT_OK;
  float dir[2 * SC_MAX_SECTORS];
  sc_sector_table(sc.prm.n_sectors, dir);
  HIP_TRY(h, sc.dir.ensure(2 * SC_MAX_SECTORS));
  HIP_TRY(h, hipMemcpyAsync(sc.dir.p, dir, 2 * (size_t)sc.prm.n_sectors * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // (`dir` is this frame's)
  sc.table_valid = true;
  return NDT_OK;
}

// the descriptor of n points in device memory into d_desc / d_count (device memory, d_count may be null): enqueued
int sc_descriptor(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n, float* d_desc, int32_t* d_count) {
  ScanContextBufs& sc = h->sc;
  if (n > (size_t)std::numeric_limits<int>::max() / 2) return fail(h, NDT_ERR_INVALID_ARG, "cloud too large");
  int rc = sc_table(h);
  if (rc) return rc;
  const int bins = (int)sc.bins();
  hipStream_t s = h->stream;
  HIP_TRY(h, sc.acc.ensure(2 * (size_t)SC_MAX_RINGS * SC_MAX_SECTORS));
  HIP_TRY(h, hipMemsetAsync(sc.acc.p, 0, 2 * (size_t)bins * sizeof(uint32_t), s));
  if (n) {
    const ScBinArgs a{sc.prm.n_rings, sc.prm.n_sectors, sc.prm.max_radius, sc.prm.z_sign, sc.prm.lift};
    const unsigned blocks = (unsigned)std::min<size_t>((n + SC_POINTS_PER_BLOCK - 1) / SC_POINTS_PER_BLOCK, SC_MAX_BLOCKS);
    const size_t lds = (2 * (size_t)bins + 2 * (size_t)a.S) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_sc_bins, dim3(blocks), dim3(SC_THREADS), lds, s, dx, dy, dz, (int)n, a, sc.dir.p, sc.acc.p);
    HIP_TRY(h, hipGetLastError());
  }
  hipLaunchKernelGGL(k_sc_finish, dim3((unsigned)((bins + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s, sc.acc.p, bins,
                     sc.prm.min_points_per_bin, d_desc, d_count);
  HIP_TRY(h, hipGetLastError());
  return NDT_OK;
}

// ... into the call's scratch (sc.desc, sc.count), for the forms that answer to the host
int sc_descriptor_scratch(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n) {
  HIP_TRY(h, h->sc.desc.ensure((size_t)SC_MAX_RINGS * SC_MAX_SECTORS));
  HIP_TRY(h, h->sc.count.ensure((size_t)SC_MAX_RINGS * SC_MAX_SECTORS));
  return sc_descriptor(h, dx, dy, dz, n, h->sc.desc.p, h->sc.count.p);
}

int sc_download(ndt_handle* h, float* desc, int32_t* count) {
  const size_t bins = h->sc.bins();
  if (desc) HIP_TRY(h, hipMemcpyAsync(desc, h->sc.desc.p, bins * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (count) HIP_TRY(h, hipMemcpyAsync(count, h->sc.count.p, bins * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

// The slot of entry `id`: its own, a freed one, or the next; the bank grows by doubling (the entries move on the stream).
// A fresh slot is not yet an entry: the caller adds it to `ids` once the slot is written (bank_commit).
int sc_bank_slot(ndt_handle* h, int64_t id, int* slot, bool* fresh) {
  ScanContextBufs& sc = h->sc;
  auto it = sc.ids.find(id);
  *fresh = it == sc.ids.end();
  if (!*fresh) { *slot = it->second; return NDT_OK; }
  if (!sc.free_slots.empty()) { *slot = sc.free_slots.back(); return NDT_OK; }
  const size_t used = sc.ids.size(), bins = sc.bins();
  if (used >= sc.bank_slots()) {
    const size_t want = std::max<size_t>(64, 2 * sc.bank_slots());
    DevBuf<float> grown;
    HIP_TRY(h, grown.ensure(want * bins));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(grown.p, sc.bank.p, used * bins * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { grown.release(); HIP_TRY(h, e); }
    sc.bank.release();
    sc.bank = grown;
  }
  *slot = (int)used;
  return NDT_OK;
}

void sc_bank_commit(ndt_handle* h, int64_t id, int slot, bool fresh) {
  ScanContextBufs& sc = h->sc;
  if (!fresh) return;
  if (!sc.free_slots.empty() && sc.free_slots.back() == slot) sc.free_slots.pop_back();
  sc.ids[id] = slot;
  sc.order_valid = false;
}

// the query (device memory) against every entry; awaited
int64_t sc_match(ndt_handle* h, const float* d_query, int64_t* ids, double* distance, int32_t* shift, int32_t* columns, size_t cap) {
  ScanContextBufs& sc = h->sc;
  const size_t m = sc.ids.size();
  if (m == 0) return 0;
  if (cap < m) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(m) + " bank entries");
  hipStream_t s = h->stream;
  const int R = sc.prm.n_rings, S = sc.prm.n_sectors;
  if (!sc.order_valid) {
    std::vector<int> slots;
    slots.reserve(m);
    for (const auto& kv : sc.ids) slots.push_back(kv.second);
    HIP_TRY(h, sc.order.ensure(m));
    HIP_TRY(h, hipMemcpyAsync(sc.order.p, slots.data(), m * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));   // (`slots` is this frame's)
    sc.order_valid = true;
  }
  HIP_TRY(h, sc.mdist.ensure(m));
  HIP_TRY(h, sc.mshift.ensure(m));
  HIP_TRY(h, sc.mcols.ensure(m));
  const size_t lds = (3 * (size_t)S + sc.bins()) * sizeof(double) + (size_t)S * sizeof(int) + sc.bins() * sizeof(float);
  hipLaunchKernelGGL(k_sc_match, dim3((unsigned)m), dim3(S <= 64 ? 64 : 128), lds, s, d_query, sc.bank.p, sc.order.p, R, S,
                     sc.mdist.p, sc.mshift.p, sc.mcols.p);
  HIP_TRY(h, hipGetLastError());
  if (distance) HIP_TRY(h, hipMemcpyAsync(distance, sc.mdist.p, m * sizeof(double), hipMemcpyDeviceToHost, s));
  if (shift) HIP_TRY(h, hipMemcpyAsync(shift, sc.mshift.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (columns) HIP_TRY(h, hipMemcpyAsync(columns, sc.mcols.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (ids) {
    size_t k = 0;
    for (const auto& kv : sc.ids) ids[k++] = kv.first;
  }
  return (int64_t)m;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

void ndt_scan_context_default_params(ndt_scan_context_params* p) {
  if (!p) return;
  *p = ndt_scan_context_params{20, 60, 80.0f, 1.0f, 2.0f, 1};
}

int ndt_scan_context_set_params(ndt_handle* h, const ndt_scan_context_params* p) {
  if (!h || !p || !sc_params_ok(p)) return NDT_ERR_INVALID_ARG;
  ScanContextBufs& sc = h->sc;
  if (std::memcmp(&sc.prm, p, sizeof(*p)) == 0) return NDT_OK;
  if (sc.prm.n_sectors != p->n_sectors) sc.table_valid = false;
  sc.prm = *p;
  sc.clear_bank();   // its descriptors were made under other parameters
  return NDT_OK;
}

int ndt_scan_context_get_params(const ndt_handle* h, ndt_scan_context_params* p) {
  if (!h || !p) return NDT_ERR_INVALID_ARG;
  *p = h->sc.prm;
  return NDT_OK;
}

int ndt_scan_context_sector_table(int n_sectors, float* dir_xy) {
  if (!dir_xy || n_sectors < 3 || n_sectors > SC_MAX_SECTORS) return NDT_ERR_INVALID_ARG;
  sc_sector_table(n_sectors, dir_xy);
  return NDT_OK;
}

int ndt_scan_context_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n, float* d_desc,
                            int32_t* d_count_or_null) {
  if (!h || !d_desc || ((!dx || !dy || !dz) && n)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  rc = sc_descriptor(h, dx, dy, dz, n, d_desc, d_count_or_null);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

int ndt_scan_context(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, float* desc, int32_t* count_or_null) {
  if (!h || !desc || (!xyz && n) || !layout_valid(stride_bytes, -1)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  ScanContextBufs& sc = h->sc;
  if (n) {
    settle_discard_keep_grid(h);   // (the upload goes through the target lane's staging)
    rc = upload_soa(h, h->lane_t, h->stream, xyz, nullptr, nullptr, nullptr, n, stride_bytes, sc.ux, sc.uy, sc.uz, true);
    if (rc) return rc;
  }
  rc = sc_descriptor_scratch(h, sc.ux.p, sc.uy.p, sc.uz.p, n);
  if (rc) return rc;
  return sc_download(h, desc, count_or_null);
}

int ndt_scan_context_keyframe(ndt_handle* h, int64_t id, float* desc_or_null, int32_t* count_or_null) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  auto it = h->keyframes.find(id);
  if (it == h->keyframes.end()) return fail(h, NDT_ERR_INVALID_ARG, "unknown keyframe id");
  const ndt_handle::Keyframe& kf = it->second;
  int slot = 0;
  bool fresh = false;
  rc = sc_bank_slot(h, id, &slot, &fresh);
  if (rc) return rc;
  // (the archive is written on the engine's stream: the descriptor is enqueued behind the keyframe's transfer)
  rc = sc_descriptor_scratch(h, kf.x.p, kf.y.p, kf.z.p, kf.n);
  if (rc) return rc;
  const size_t bins = h->sc.bins();
  HIP_TRY(h, hipMemcpyAsync(h->sc.bank.p + (size_t)slot * bins, h->sc.desc.p, bins * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  rc = sc_download(h, desc_or_null, count_or_null);
  if (rc) return rc;
  sc_bank_commit(h, id, slot, fresh);
  return NDT_OK;
}

int ndt_scan_context_bank_put(ndt_handle* h, int64_t id, const float* desc) {
  if (!h || !desc) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  int slot = 0;
  bool fresh = false;
  rc = sc_bank_slot(h, id, &slot, &fresh);
  if (rc) return rc;
  const size_t bins = h->sc.bins();
  HIP_TRY(h, hipMemcpyAsync(h->sc.bank.p + (size_t)slot * bins, desc, bins * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  sc_bank_commit(h, id, slot, fresh);
  return NDT_OK;
}

int ndt_scan_context_bank_get(ndt_handle* h, int64_t id, float* desc) {
  if (!h || !desc) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  auto it = h->sc.ids.find(id);
  if (it == h->sc.ids.end()) return fail(h, NDT_ERR_INVALID_ARG, "unknown descriptor bank id");
  const size_t bins = h->sc.bins();
  HIP_TRY(h, hipMemcpyAsync(desc, h->sc.bank.p + (size_t)it->second * bins, bins * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

int ndt_scan_context_bank_erase(ndt_handle* h, int64_t id) {
  if (!h) return NDT_ERR_INVALID_ARG;
  auto it = h->sc.ids.find(id);
  if (it == h->sc.ids.end()) return fail(h, NDT_ERR_INVALID_ARG, "unknown descriptor bank id");
  h->sc.free_slots.push_back(it->second);
  h->sc.ids.erase(it);
  h->sc.order_valid = false;
  return NDT_OK;
}

int ndt_scan_context_bank_clear(ndt_handle* h) {
  if (!h) return NDT_ERR_INVALID_ARG;
  h->sc.clear_bank();
  return NDT_OK;
}

int64_t ndt_scan_context_bank_count(const ndt_handle* h) { return h ? (int64_t)h->sc.ids.size() : NDT_ERR_INVALID_ARG; }

int64_t ndt_scan_context_match(ndt_handle* h, const float* desc, int64_t* ids, double* distance, int32_t* shift, int32_t* columns,
                               size_t cap) {
  if (!h || !desc) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (h->sc.ids.empty()) return 0;
  const size_t bins = h->sc.bins();
  HIP_TRY(h, h->sc.desc.ensure((size_t)SC_MAX_RINGS * SC_MAX_SECTORS));
  HIP_TRY(h, hipMemcpyAsync(h->sc.desc.p, desc, bins * sizeof(float), hipMemcpyHostToDevice, h->stream));
  return sc_match(h, h->sc.desc.p, ids, distance, shift, columns, cap);
}

int64_t ndt_scan_context_match_keyframe(ndt_handle* h, int64_t id, int64_t* ids, double* distance, int32_t* shift, int32_t* columns,
                                        size_t cap) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  auto it = h->sc.ids.find(id);
  if (it == h->sc.ids.end()) return fail(h, NDT_ERR_INVALID_ARG, "unknown descriptor bank id");
  return sc_match(h, h->sc.bank.p + (size_t)it->second * h->sc.bins(), ids, distance, shift, columns, cap);
}

}  // extern "C"
