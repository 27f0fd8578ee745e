// ndt_sort_plan.h -- the plan rule of the radix sort (ndt_sort.hip): how many bits a key range needs and how those bits
// are split into digits.  Host and device; no HIP header, so that tests/cpp/sanitize_host.cpp checks it under a plain
// host compiler.  The host's plan writer (sort_put_plan), the build's device-side geometry (derive_geometry) and the
// source ordering (k_source_keys) all state the rule through these two functions.
#pragma once

#if defined(__HIPCC__)
#define NDT_SORT_HD __host__ __device__
#else
#define NDT_SORT_HD
#endif

namespace ndt {

constexpr int SORT_MAX_PASSES = 4;   // digits of at most 8 bits over 32-bit keys (BuildGeom::width / shift)

// Bits that hold the keys 0 .. v: floor(log2 v) + 1, and 0 for v <= 0.  The limits stay with the caller: a sort key has
// at least 1 bit and at most 32 (31 for the source's block keys), the voxel map's axis extents may have 0.
NDT_SORT_HD inline int sort_key_bits(long long v) {
  int b = 0;
  while (b < 62 && (1ll << b) <= v) ++b;
  return b;
}

// digit passes that `bits` key bits need when nothing was planned
NDT_SORT_HD inline int sort_passes_for_bits(int bits) { return (bits + 7) / 8; }

// `bits` key bits over `passes` digits (1 .. SORT_MAX_PASSES), the wider digits first: width[i] = bits / passes +
// (i < bits % passes), shift[i] = the widths before it; both zero from `passes` on.
NDT_SORT_HD inline void sort_split_bits(int bits, int passes, int width[SORT_MAX_PASSES], int shift[SORT_MAX_PASSES]) {
  const int base = bits / passes, rem = bits % passes;
  int sh = 0;
  for (int i = 0; i < SORT_MAX_PASSES; ++i) {
    const bool used = i < passes;
    width[i] = used ? base + (i < rem ? 1 : 0) : 0;
    shift[i] = used ? sh : 0;
    sh += width[i];
  }
}

}  // namespace ndt
