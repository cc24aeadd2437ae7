// Content-defined chunking (CDC), defined once for host and device: the gear
// table, the rolling hash, the candidate test, and (host only) the sequential
// boundary selection. The candidate kernel (core/hip/cdc.hip), the engine's
// overflow path and the host model exposed through _core all run this file.
//
// Rolling hash. h(i) = sum_{k=0..31} G[b[i-k]] << k  (mod 2^32); bytes before
// offset 0 contribute nothing. Equivalently h = (h << 1) + G[b], started at 0:
// a term older than 32 steps has been shifted out, so the value at i is exact
// from ANY start at or before i - 31. That is what lets every lane of the
// kernel roll its own run after a 32-byte warm-up. The hash is 32 bits wide on
// purpose: the VALU is, and `(h << 1) + g` is one v_lshl_add_u32.
//
// Candidate. Position i is a candidate at `bits` when the top `bits` bits of
// h(i) are zero, i.e. h(i) < 2^(32 - bits).
//
// Gear table. G[v] = mix(kSeed + v * phi) >> 1, never zero. The values are 31
// bits wide by construction: a window of 32 equal bytes v hashes to
// G[v] * (2^32 - 1) = -G[v] (mod 2^32), and with 0 < G[v] < 2^31 its top bit
// is set, so a constant run is no candidate at any `bits` >= 1. Zero padding
// and zero-initialised rows are therefore cut by `max` alone and can never
// make hits dense. No seed could give that to a full 32-bit table (each value
// would need its top bit clear by chance); the seed only has to keep every
// value non-zero, which the static_assert below checks.
//
// Selection (host, sequential). With (min, bits, max) and chunk start s the
// chunk ends at e = i + 1 for the first candidate i with min <= i + 1 - s <=
// max; without one at s + max, or at the end of the blob if that comes first.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#ifndef MX_HD
#define MX_HD __host__ __device__
#endif
#else
#ifndef MX_HD
#define MX_HD
#endif
#endif

namespace modelx {
namespace cdc {

constexpr uint32_t kWindow = 32;
constexpr uint32_t kSeed = 0x4d58c0deu;

constexpr uint32_t kDefaultMin = 32u << 10;
constexpr uint32_t kDefaultBits = 16;
constexpr uint32_t kDefaultMax = 256u << 10;
constexpr uint32_t kMinFloor = 64;
constexpr uint32_t kMaxCeil = 16u << 20;
constexpr uint32_t kBitsCeil = 24;

// murmur3's 32-bit finaliser over a Weyl sequence, top bit dropped
MX_HD constexpr uint32_t gear(uint32_t v) {
  uint32_t x = kSeed + v * 0x9e3779b9u;
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x >> 1;
}

struct GearTable {
  uint32_t g[256];
};

constexpr GearTable make_gear_table() {
  GearTable t{};
  for (uint32_t v = 0; v < 256; v++) t.g[v] = gear(v);
  return t;
}

constexpr bool gear_table_nonzero() {
  for (uint32_t v = 0; v < 256; v++)
    if (gear(v) == 0) return false;
  return true;
}
static_assert(gear_table_nonzero(), "kSeed gives a zero gear value: pick another");

MX_HD constexpr uint32_t roll(uint32_t h, uint32_t g) { return (h << 1) + g; }

// h < threshold(bits)  <=>  the top `bits` bits of h are zero (1 <= bits <= 31)
MX_HD constexpr uint32_t threshold(uint32_t bits) { return 1u << (32 - bits); }

constexpr bool valid_bits(uint64_t bits) { return bits >= 1 && bits <= kBitsCeil; }

constexpr bool valid_params(uint64_t min, uint64_t bits, uint64_t max) {
  return kMinFloor <= min && min <= max && max <= kMaxCeil && valid_bits(bits);
}

// Every candidate position of data[0, n), ascending, appended to *out as
// base + i. `skip` leading positions are rolled but not reported (the warm-up
// of a range that starts inside a blob).
inline void candidates(const uint8_t* data, size_t n, uint32_t bits, uint64_t base, size_t skip,
                       std::vector<uint64_t>* out) {
  static constexpr GearTable kGear = make_gear_table();
  const uint32_t thr = threshold(bits);
  uint32_t h = 0;
  for (size_t i = 0; i < n; i++) {
    h = roll(h, kGear.g[data[i]]);
    if (h < thr && i >= skip) out->push_back(base + i);
  }
}

// Chunks (offset, length) of a `size`-byte blob from its ascending candidate
// positions. An empty blob has no chunks.
inline std::vector<std::pair<uint64_t, uint64_t>> select(const std::vector<uint64_t>& cand,
                                                         uint64_t size, uint64_t min,
                                                         uint64_t max) {
  std::vector<std::pair<uint64_t, uint64_t>> out;
  size_t c = 0;
  for (uint64_t s = 0; s < size;) {
    while (c < cand.size() && cand[c] + 1 < s + min) c++;  // s only grows: c never backs up
    uint64_t e = s + max < size ? s + max : size;
    if (c < cand.size() && cand[c] + 1 <= e) e = cand[c] + 1;
    out.emplace_back(s, e - s);
    s = e;
  }
  return out;
}

inline std::vector<std::pair<uint64_t, uint64_t>> chunks(const uint8_t* data, size_t n,
                                                         uint64_t min, uint32_t bits,
                                                         uint64_t max) {
  std::vector<uint64_t> cand;
  candidates(data, n, bits, 0, 0, &cand);
  return select(cand, n, min, max);
}

}  // namespace cdc
}  // namespace modelx
