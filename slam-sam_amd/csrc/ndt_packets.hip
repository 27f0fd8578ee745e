// ndt_packets.hip -- a lidar frame's UDP payloads to the range image on the device, and on through the unprojection
// (include/ndt_hip.h has the contract and the format table, DESIGN 7j the rules; ndt_packets.cpp is the host pre-pass that
// reads the headers).  The accepted packets lie in the packed packet buffer, one slot each; the pre-pass gives, per image
// column, the dword offset of its first pixel in that buffer (col_src, -1: no column), and
//   k_decode_packets   one thread per pixel i = col * n_rows + row gathers the pixel's three dwords at col_src + 3 * row
//                      and writes range (u32), reflectivity (u8), signal and nir (u16); a wave's lanes that share a column
//                      read one contiguous run of 768 bytes.  The block reads col_src of ITS columns once into LDS, as
//                      unp_load_cols does.  Integer work only, no atomics, no LDS beyond that table.
//   k_gather_u16       signal and nir of the points an unprojection selected, through its pixel index
// The image then goes through unproject_device (ndt_unproject.hip) unchanged.  Everything on the engine's stream.
#include "ndt_engine.h"
#include "ndt_deskew_device.h"
#include "ndt_trajectory.h"

namespace ndt {

namespace {

// Every col_src >= 0 the host pass produces satisfies col_src + 3 * n_rows <= dwords of the packet buffer: the column's
// pixels end inside its packet, the packet inside its slot, the slot below the buffer's capacity (pkt::Pass::take), and
// decode_frame checks exactly that bound on the host in front of the launch.  The kernel does not test it again.
__global__ void __launch_bounds__(DSK_THREADS) k_decode_packets(const uint32_t* __restrict__ packets, const int32_t* __restrict__ col_src,
                                                               unsigned int n_rows, unsigned int n, uint32_t range_mask,
                                                               uint32_t* __restrict__ o_range, uint8_t* __restrict__ o_refl,
                                                               uint16_t* __restrict__ o_signal, uint16_t* __restrict__ o_nir) {
  __shared__ int32_t s_src[DSK_THREADS];
  const unsigned int first = blockIdx.x * DSK_THREADS, last = min(first + DSK_THREADS - 1u, n - 1u);
  const unsigned int c0 = first / n_rows, c1 = last / n_rows;   // (first < n: the grid has ceil(n / 256) blocks)
  if (c0 + threadIdx.x <= c1) s_src[threadIdx.x] = col_src[c0 + threadIdx.x];
  __syncthreads();
  const unsigned int i = first + threadIdx.x;
  if (i >= n) return;
  const unsigned int col = i / n_rows, row = i - col * n_rows;
  const int32_t src = s_src[col - c0];
  uint32_t d0 = 0u, d1 = 0u, d2 = 0u;
  if (src >= 0) {
    const uint32_t* p = packets + (size_t)src + 3u * row;
    d0 = p[0];
    d1 = p[1];
    d2 = p[2];
  }
  o_range[i] = d0 & range_mask;
  if (o_refl) o_refl[i] = (uint8_t)(d1 & 0xFFu);
  if (o_signal) o_signal[i] = (uint16_t)(d1 >> 16);
  if (o_nir) o_nir[i] = (uint16_t)(d2 & 0xFFFFu);
}

// out[j] = in[index[j]] for the m points written (index null: the organised form, j itself)
__global__ void __launch_bounds__(DSK_THREADS) k_gather_u16(const int32_t* __restrict__ index, unsigned int m,
                                                           const uint16_t* __restrict__ signal, const uint16_t* __restrict__ nir,
                                                           uint16_t* __restrict__ o_signal, uint16_t* __restrict__ o_nir) {
  const unsigned int j = blockIdx.x * DSK_THREADS + threadIdx.x;
  if (j >= m) return;
  const unsigned int i = index ? (unsigned int)index[j] : j;
  if (o_signal) o_signal[j] = signal[i];
  if (o_nir) o_nir[j] = nir[i];
}

}  // namespace

namespace engine {
namespace {

size_t pkt_pixels(const ndt_handle* h) { return (size_t)h->scan.n_cols * (size_t)h->scan.n_rows; }

// what every call on the frame in progress needs
int frame_check(ndt_handle* h, const char* who) {
  if (h->scan.n_cols == 0) return fail(h, NDT_ERR_INVALID_ARG, std::string(who) + ": no scan model set (ndt_scan_model_set)");
  if (h->pkt.pass.f.profile < 0) return fail(h, NDT_ERR_INVALID_ARG, std::string(who) + ": no packet format set (ndt_packet_format_set)");
  return NDT_OK;
}
int frame_ready(ndt_handle* h, const char* who) {
  const int rc = frame_check(h, who);
  if (rc) return rc;
  if (h->pkt.pass.info.n_columns == 0) return fail(h, NDT_ERR_INVALID_ARG, std::string(who) + ": no accepted column in the frame in progress");
  return NDT_OK;
}

// The frame in progress -> the range image in device memory: the column table goes up through its pinned staging (the
// times straight to d_col_t), then ONE launch of k_decode_packets.  Enqueued, not awaited.
int decode_frame(ndt_handle* h, uint32_t* d_range, uint8_t* d_refl, uint16_t* d_signal, uint16_t* d_nir, float* d_col_t) {
  PacketBufs& b = h->pkt;
  const pkt::Format& f = b.pass.f;
  const size_t nc = (size_t)f.n_cols, n = pkt_pixels(h);
  // (the staging may still feed the previous decode's copies: wait for the stream before it is rewritten)
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, b.cols_h.ensure(2 * nc));
  HIP_TRY(h, b.col_src.ensure(nc));
  int32_t* src = reinterpret_cast<int32_t*>(b.cols_h.h);
  float* col_t = reinterpret_cast<float*>(b.cols_h.h + nc);
  b.pass.finish(std::numeric_limits<double>::quiet_NaN(), src, col_t, nullptr);
  // the bound the kernel relies on: a column's 3 * n_rows dwords lie inside the slots that have been copied up
  const size_t words = b.pass.slots * (f.slot / 4);
  for (size_t m = 0; m < nc; ++m)
    if (src[m] >= 0 && (size_t)src[m] + 3 * (size_t)f.n_rows > words) return fail(h, NDT_ERR_HIP, "packets: a column offset outside the packet buffer");
  HIP_TRY(h, hipMemcpyAsync(b.col_src.p, src, nc * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(d_col_t, col_t, nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const uint32_t mask = f.profile == NDT_LIDAR_PROFILE_LEGACY ? 0x000FFFFFu : 0x0007FFFFu;
  const unsigned nb = (unsigned)((n + DSK_THREADS - 1) / DSK_THREADS);
  hipLaunchKernelGGL(k_decode_packets, dim3(nb), dim3(DSK_THREADS), 0, h->stream, b.dev.p, b.col_src.p, (unsigned int)f.n_rows,
                     (unsigned int)n, mask, d_range, d_refl, d_signal, d_nir);
  HIP_TRY(h, hipGetLastError());
  return NDT_OK;
}

// ... into the handle's scratch: ScanModelBufs::in in its [range | col_t | reflectivity] layout, signal and nir (when
// wanted) beside it
struct ScratchImage {
  const uint32_t* range;
  const float* col_t;
  const uint8_t* refl;
};
int decode_to_scratch(ndt_handle* h, bool with_extras, ScratchImage* img) {
  ScanModelBufs& s = h->scan;
  const size_t n = pkt_pixels(h), nc = (size_t)s.n_cols;
  HIP_TRY(h, s.in.ensure(n + nc + (n + 3) / 4));
  if (with_extras) {
    HIP_TRY(h, h->pkt.sig.ensure(n));
    HIP_TRY(h, h->pkt.nir.ensure(n));
  }
  img->range = s.in.p;
  img->col_t = reinterpret_cast<const float*>(s.in.p + n);
  img->refl = reinterpret_cast<const uint8_t*>(s.in.p + n + nc);
  return decode_frame(h, s.in.p, reinterpret_cast<uint8_t*>(s.in.p + n + nc), with_extras ? h->pkt.sig.p : nullptr,
                      with_extras ? h->pkt.nir.p : nullptr, reinterpret_cast<float*>(s.in.p + n));
}

// signal and nir of the m points written (index null: pixel j itself) into device arrays; enqueued
int gather_extras(ndt_handle* h, const int32_t* d_index, size_t m, uint16_t* o_signal, uint16_t* o_nir) {
  if (m == 0 || (!o_signal && !o_nir)) return NDT_OK;
  const unsigned nb = (unsigned)((m + DSK_THREADS - 1) / DSK_THREADS);
  hipLaunchKernelGGL(k_gather_u16, dim3(nb), dim3(DSK_THREADS), 0, h->stream, d_index, (unsigned int)m, h->pkt.sig.p, h->pkt.nir.p,
                     o_signal, o_nir);
  HIP_TRY(h, hipGetLastError());
  return NDT_OK;
}

// ... and down into host arrays; awaited
int download_extras(ndt_handle* h, const int32_t* d_index, size_t m, uint16_t* signal_out, uint16_t* nir_out) {
  if (m == 0 || (!signal_out && !nir_out)) return NDT_OK;
  PacketBufs& b = h->pkt;
  HIP_TRY(h, b.sig_out.ensure(m));
  HIP_TRY(h, b.nir_out.ensure(m));
  HIP_TRY(h, b.back.ensure(2 * pkt_pixels(h)));
  const int rc = gather_extras(h, d_index, m, signal_out ? b.sig_out.p : nullptr, nir_out ? b.nir_out.p : nullptr);
  if (rc) return rc;
  if (signal_out) HIP_TRY(h, hipMemcpyAsync(b.back.h, b.sig_out.p, m * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
  if (nir_out) HIP_TRY(h, hipMemcpyAsync(b.back.h + m, b.nir_out.p, m * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (signal_out) std::memcpy(signal_out, b.back.h, m * sizeof(uint16_t));
  if (nir_out) std::memcpy(nir_out, b.back.h + m, m * sizeof(uint16_t));
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_packet_format_set(ndt_handle* h, int profile, int columns_per_packet) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (h->scan.n_cols == 0) return fail(h, NDT_ERR_INVALID_ARG, "packet format: no scan model set (ndt_scan_model_set)");
  pkt::Format f;
  if (!pkt::format_make(profile, columns_per_packet, h->scan.n_cols, h->scan.n_rows, &f))
    return fail(h, NDT_ERR_INVALID_ARG, "packet format: unknown profile, columns_per_packet below 1 or a frame of more than 2^31 dwords");
  int rc = bind_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // (a frame in progress may still be on its way up)
  PacketBufs& b = h->pkt;
  b.drop();
  const size_t words = f.capacity * (f.slot / 4);
  HIP_TRY(h, b.stage.ensure(words));
  HIP_TRY(h, b.dev.ensure(words));
  b.pass.begin(f);
  return NDT_OK;
}

int ndt_packet_format_get(const ndt_handle* h, int* profile, int* columns_per_packet) {
  if (!h || !profile || !columns_per_packet) return NDT_ERR_INVALID_ARG;
  const pkt::Format& f = h->pkt.pass.f;
  *profile = f.profile < 0 ? -1 : f.profile;
  *columns_per_packet = f.profile < 0 ? 0 : f.cpp;
  return NDT_OK;
}

size_t ndt_packet_size(const ndt_handle* h) { return (h && h->pkt.pass.f.profile >= 0) ? h->pkt.pass.f.packet : 0; }

int ndt_packet_frame_begin(ndt_handle* h) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = frame_check(h, "packet frame");
  if (rc) return rc;
  rc = bind_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // no slot of the staging is rewritten while a copy out of it is in flight
  const pkt::Format f = h->pkt.pass.f;
  h->pkt.pass.begin(f);
  return NDT_OK;
}

int ndt_packet_frame_push(ndt_handle* h, const uint8_t* packets, const size_t* bytes_each, size_t n_packets, size_t stride_bytes,
                          size_t* n_taken) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!n_taken) return fail(h, NDT_ERR_INVALID_ARG, "packet frame: n_taken is NULL");
  *n_taken = 0;
  int rc = frame_check(h, "packet frame");
  if (rc) return rc;
  if (n_packets && (!packets || !bytes_each)) return fail(h, NDT_ERR_INVALID_ARG, "packet frame: the packets or their sizes are NULL");
  for (size_t k = 0; k < n_packets; ++k)
    if (bytes_each[k] > stride_bytes) return fail(h, NDT_ERR_INVALID_ARG, "packet frame: a packet is longer than stride_bytes");
  rc = bind_device(h);
  if (rc) return rc;
  PacketBufs& b = h->pkt;
  pkt::Pass& pass = b.pass;
  const pkt::Format& f = pass.f;
  // an overfull call takes nothing: keep what it could change (only when it can reach the capacity at all)
  pkt::Pass saved;
  const bool may_overflow = pass.slots + n_packets > f.capacity;
  if (may_overflow) saved = pass;
  const size_t slot0 = pass.slots;
  pass.info.next_frame_pending = 0;
  size_t taken = 0;
  for (; taken < n_packets; ++taken) {
    const uint8_t* p = packets + taken * stride_bytes;
    if (pass.slots == f.capacity) {
      // would this packet need a slot?  (a copy of the pass answers without changing the frame)
      pkt::Pass probe = pass;
      if (probe.take(p, bytes_each[taken]) == pkt::ACCEPTED) {
        pass = saved;
        return fail(h, NDT_ERR_INVALID_ARG, "packet frame: frame overfull (" + std::to_string(f.capacity) + " packets hold)");
      }
    }
    const pkt::Taken t = pass.take(p, bytes_each[taken]);
    if (t == pkt::NEXT_FRAME) break;
    if (t == pkt::ACCEPTED) std::memcpy(reinterpret_cast<uint8_t*>(b.stage.h) + (pass.slots - 1) * f.slot, p, f.packet);
  }
  if (pass.slots > slot0)
    HIP_TRY(h, hipMemcpyAsync(b.dev.p + slot0 * (f.slot / 4), b.stage.h + slot0 * (f.slot / 4), (pass.slots - slot0) * f.slot,
                              hipMemcpyHostToDevice, h->stream));
  *n_taken = taken;
  return NDT_OK;
}

int ndt_packet_frame_get_info(const ndt_handle* h, ndt_packet_frame_info* info) {
  if (!h || !info) return NDT_ERR_INVALID_ARG;
  h->pkt.pass.finish(std::numeric_limits<double>::quiet_NaN(), nullptr, nullptr, info);
  return NDT_OK;
}

int ndt_decode_packet_frame_device(ndt_handle* h, uint32_t* d_range_mm, uint8_t* d_reflectivity, uint16_t* d_signal, uint16_t* d_nir,
                                   float* d_col_t) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = frame_ready(h, "decode packets");
  if (rc) return rc;
  if (!d_range_mm || !d_col_t) return fail(h, NDT_ERR_INVALID_ARG, "decode packets: the range image or the column times are NULL");
  {
    const size_t n = pkt_pixels(h);
    const void* outs[5] = {d_range_mm, d_reflectivity, d_signal, d_nir, d_col_t};
    const size_t bytes[5] = {n * 4, n, n * 2, n * 2, (size_t)h->scan.n_cols * 4};
    for (int a = 0; a < 5; ++a)
      for (int c = a + 1; c < 5; ++c)
        if (ranges_overlap(outs[a], bytes[a], outs[c], bytes[c])) return fail(h, NDT_ERR_INVALID_ARG, "decode packets: two outputs overlap");
  }
  rc = bind_device(h);
  if (rc) return rc;
  rc = decode_frame(h, d_range_mm, d_reflectivity, d_signal, d_nir, d_col_t);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

int ndt_unproject_packet_frame_device(ndt_handle* h, const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16,
                                      int n_knots, const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* ox,
                                      float* oy, float* oz, float* o_intensity, float* o_t, int32_t* d_index_out, uint16_t* d_signal_out,
                                      uint16_t* d_nir_out, size_t cap, size_t* n_out) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!n_out) return fail(h, NDT_ERR_INVALID_ARG, "unproject: n_out is NULL");
  *n_out = 0;
  int rc = frame_ready(h, "unproject packets");
  if (rc) return rc;
  const size_t n = pkt_pixels(h);
  const bool extras = d_signal_out || d_nir_out;
  {
    const size_t m = std::min(cap, n);
    const void* outs[6] = {ox, oy, oz, o_intensity, o_t, d_index_out};
    const void* ex[2] = {d_signal_out, d_nir_out};
    for (const void* e : ex)
      for (const void* o : outs)
        if (ranges_overlap(e, m * sizeof(uint16_t), o, m * sizeof(float))) return fail(h, NDT_ERR_INVALID_ARG, "unproject packets: signal_out or nir_out overlaps another output");
    if (ranges_overlap(ex[0], m * sizeof(uint16_t), ex[1], m * sizeof(uint16_t)))
      return fail(h, NDT_ERR_INVALID_ARG, "unproject packets: signal_out and nir_out overlap");
  }
  rc = bind_device(h);
  if (rc) return rc;
  ScratchImage img;
  rc = decode_to_scratch(h, extras, &img);   // (into the handle's own scratch: a refusal below has written nothing of the caller's)
  if (rc) return rc;
  // the compacting form gathers through the pixel index: the handle's own when the caller wants none
  int32_t* index = d_index_out;
  if (extras && filter_or_null && !index) {
    HIP_TRY(h, h->scan.index.ensure(n));
    index = h->scan.index.p;
  }
  rc = ndt_unproject_device(h, img.range, img.refl, img.col_t, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null,
                            filter_or_null, ox, oy, oz, o_intensity, o_t, index, cap, n_out);
  if (rc) return rc;
  rc = gather_extras(h, filter_or_null ? index : nullptr, *n_out, d_signal_out, d_nir_out);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

int ndt_unproject_packet_frame(ndt_handle* h, const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16,
                               int n_knots, const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* out,
                               size_t stride_bytes, long intensity_offset_bytes, float* t_out, int32_t* index_out, uint16_t* signal_out,
                               uint16_t* nir_out, size_t cap, size_t* n_out) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!n_out) return fail(h, NDT_ERR_INVALID_ARG, "unproject: n_out is NULL");
  *n_out = 0;
  int rc = frame_ready(h, "unproject packets");
  if (rc) return rc;
  // the checks of ndt_unproject, in its order
  traj::KnotRow rows[traj::MAX_KNOTS];
  rc = unproject_check(h, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  if (!out && cap) return fail(h, NDT_ERR_INVALID_ARG, "unproject: the output cloud is NULL");
  if (!layout_valid(stride_bytes, intensity_offset_bytes)) return fail(h, NDT_ERR_INVALID_ARG, "unproject: invalid output layout");
  const bool has_i = intensity_offset_bytes >= 0, extras = signal_out || nir_out;
  const size_t n = pkt_pixels(h);
  if (!filter_or_null && cap < n) {
    *n_out = n;
    return over_capacity(h, n);
  }
  rc = bind_device(h);
  if (rc) return rc;
  ScratchImage img;
  rc = decode_to_scratch(h, extras, &img);
  if (rc) return rc;
  ScanModelBufs& b = h->scan;
  HIP_TRY(h, b.stage.ensure(5 * n + 64));   // (carries the result down: 5 floats per point)
  HIP_TRY(h, b.out.ensure(5 * n));
  HIP_TRY(h, b.index.ensure(n));
  float* o = b.out.p;
  const bool want_index = index_out || (extras && filter_or_null);
  rc = unproject_device(h, img.range, img.refl, img.col_t, gate_or_null, rows, n_knots, filter_or_null, o, o + n, o + 2 * n,
                        has_i ? o + 3 * n : nullptr, t_out ? o + 4 * n : nullptr, want_index ? b.index.p : nullptr, n, n_out);
  if (rc) return rc;
  if (*n_out > cap) return over_capacity(h, *n_out);
  rc = download_extras(h, filter_or_null ? b.index.p : nullptr, *n_out, signal_out, nir_out);
  if (rc) return rc;
  SideColumns side;
  side.d_f32 = o + 4 * n;
  side.f32_out = t_out;
  side.d_i32 = b.index.p;
  side.i32_out = index_out;
  return download_strided(h, o, n, *n_out, cap, out, stride_bytes, intensity_offset_bytes, reinterpret_cast<float*>(b.stage.h), side);
}

int ndt_keyframe_put_from_packets(ndt_handle* h, int64_t id, const ndt_range_gate* gate_or_null, const double* knot_t,
                                  const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                                  const ndt_scan_filter* filter_or_null, uint16_t* signal_out, uint16_t* nir_out, size_t* n_kept) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = frame_ready(h, "unproject packets");
  if (rc) return rc;
  traj::KnotRow rows[traj::MAX_KNOTS];
  rc = unproject_check(h, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  rc = bind_device(h);
  if (rc) return rc;
  const bool extras = signal_out || nir_out;
  ScratchImage img;
  rc = decode_to_scratch(h, extras, &img);
  if (rc) return rc;
  const ndt_scan_filter keep_valid{};   // an archive holds no NaN points: no filter = the zeroed one
  const size_t n = pkt_pixels(h);
  if (extras) HIP_TRY(h, h->scan.index.ensure(n));
  // every argument error has been reported by now; a HIP error from here on leaves keyframe `id` with no point, as
  // ndt_keyframe_put_from_ranges does
  ndt_handle::Keyframe& kf = keyframe_claim(h, id, n);
  kf.n = 0;
  HIP_TRY(h, kf.x.ensure(n));
  HIP_TRY(h, kf.y.ensure(n));
  HIP_TRY(h, kf.z.ensure(n));
  size_t m = 0;
  rc = unproject_device(h, img.range, img.refl, img.col_t, gate_or_null, rows, n_knots, filter_or_null ? filter_or_null : &keep_valid,
                        kf.x.p, kf.y.p, kf.z.p, nullptr, nullptr, extras ? h->scan.index.p : nullptr, n, &m);
  if (rc) return rc;
  kf.n = m;
  if (n_kept) *n_kept = m;
  return download_extras(h, h->scan.index.p, m, signal_out, nir_out);
}

}  // extern "C"
