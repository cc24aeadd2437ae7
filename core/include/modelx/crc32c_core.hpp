// CRC-32C (Castagnoli) arithmetic, compiled for host and device alike: the
// byte table, the bytewise update that is the host model, multiplication in
// GF(2)[x]/P, "advance a register through n zero bytes" (mul_xn), combine,
// and the generators of the stride tables the kernel (core/hip/crc32c.hip)
// copies into LDS. The kernel, the engine's host path and modelx-s3d's upload
// check all run this one definition.
//
// Conventions. The polynomial is reflected (0x82F63B78): bit 31 of a register
// is the coefficient of x^0, bit 0 that of x^31. A *raw* register starts at 0
// and has no final xor; it is linear over GF(2) in the message, and feeding a
// zero byte multiplies it by x^8. The CRC proper of a message M of n bytes is
//   crc(M) = raw(M) ^ mul_xn(0xFFFFFFFF, n) ^ 0xFFFFFFFF,
// equivalently a register started at 0xFFFFFFFF and inverted at the end.
// crc(b"123456789") == 0xE3069283.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__x86_64__)
#include <nmmintrin.h>
#define MODELX_CRC32C_SSE42 1
#endif

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
namespace crc32c {

constexpr uint32_t kPoly = 0x82F63B78u;
constexpr uint32_t kInit = 0xFFFFFFFFu;  // initial value and final xor
constexpr uint32_t kOne = 0x80000000u;   // the polynomial 1

// Entry b of the byte table: b * x^32 mod P, i.e. a register holding b
// advanced through one zero byte. Computed, not looked up, so device code can
// build its LDS copy and the finishing step can do without one.
MX_HD constexpr uint32_t table_entry(uint32_t b) {
  for (int i = 0; i < 8; i++) b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
  return b;
}

struct ByteTable {
  uint32_t t[256];
};

constexpr ByteTable make_byte_table() {
  ByteTable bt{};
  for (uint32_t b = 0; b < 256; b++) bt.t[b] = table_entry(b);
  return bt;
}

// a * b mod P. 32 shift-and-add steps; off every hot path.
MX_HD constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - (a >> 31));               // coefficient of x^i in a
    a <<= 1;
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));  // b *= x
  }
  return p;
}

// v[k] = x^(8 * 2^k) mod P: the factors of square-and-multiply over a
// byte count, squared once at compile time instead of on every call.
struct PowTable {
  uint32_t v[64];
};

constexpr PowTable make_pow_table() {
  PowTable pt{};
  uint32_t p = 0x00800000u;  // x^8
  for (int k = 0; k < 64; k++) {
    pt.v[k] = p;
    p = gf_mul(p, p);
  }
  return pt;
}

// The register `crc` advanced through `nbytes` zero bytes: crc * x^(8*nbytes)
// mod P, one multiplication per set bit of nbytes. `pow2` is make_pow_table()'s
// array (the device passes its own copy of it).
MX_HD constexpr uint32_t mul_xn(uint32_t crc, uint64_t nbytes, const uint32_t* pow2) {
  for (int k = 0; nbytes; k++, nbytes >>= 1)
    if (nbytes & 1u) crc = gf_mul(crc, pow2[k]);
  return crc;
}

// x^(8*nbytes) mod P at compile time (kernel constants).
constexpr uint32_t xpow8n(uint64_t nbytes) {
  PowTable pt = make_pow_table();
  return mul_xn(kOne, nbytes, pt.v);
}

// One byte into a register (raw or conventional alike), table computed.
MX_HD constexpr uint32_t update_byte(uint32_t s, uint8_t byte) {
  return table_entry((s ^ byte) & 0xFFu) ^ (s >> 8);
}

// The stride tables of the kernel: adv.t[k][b] = (b << 8k) * x^(8*stride), so
// that "advance s through `stride` zero bytes" is the xor of four lookups,
// one per byte of s. The top byte holds the lowest powers; each lower byte is
// the one above it times x^8, i.e. one more zero-byte step.
struct StrideTables {
  uint32_t t[4][256];
};

constexpr StrideTables make_stride_tables(uint64_t stride) {
  StrideTables st{};
  uint32_t k = xpow8n(stride);
  for (uint32_t b = 0; b < 256; b++) {
    uint32_t v = gf_mul(b << 24, k);
    for (int j = 3; j >= 0; j--) {
      st.t[j][b] = v;
      v = update_byte(v, 0);
    }
  }
  return st;
}

// ---- the kernel's split of a range, shared with the engine's sizing --------

constexpr uint64_t kSegmentBytes = 128u << 10;  // bytes one wave folds before it reduces
constexpr uint64_t kRowBytes = 1024;            // 64 lanes x one 16 B load

// Bytes of a range before its first 16 B aligned address (all of a range
// that ends sooner): they go bytewise.
MX_HD constexpr uint64_t head_bytes(uint64_t addr, uint64_t len) {
  uint64_t h = (0u - addr) & 15u;
  return h < len ? h : len;
}

// Segments of a range: its aligned body in pieces of kSegmentBytes, the last
// one shorter. A range that is all head has none.
MX_HD constexpr uint64_t segment_count(uint64_t addr, uint64_t len) {
  uint64_t body = len - head_bytes(addr, len);
  return (body + kSegmentBytes - 1) / kSegmentBytes;
}

// ---- host ------------------------------------------------------------------

inline const uint32_t* pow_table() {
  static constexpr PowTable kPow = make_pow_table();
  return kPow.v;
}

inline uint32_t mul_xn(uint32_t crc, uint64_t nbytes) { return mul_xn(crc, nbytes, pow_table()); }

// crc(A || B) from crc(A), crc(B) and len(B). The initial values and final
// xors cancel: crc(A||B) = crc(A) * x^(8 lenB) ^ crc(B) over conventional
// values, because B's own initial-value term is exactly what A's final xor
// turns into once advanced.
inline uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return mul_xn(crc_a, len_b) ^ crc_b;
}

// The host model: a conventional register (start at kInit, invert at the
// end) through n bytes, one table lookup per byte.
inline uint32_t update_bytewise(uint32_t s, const void* data, size_t n) {
  static constexpr ByteTable kTable = make_byte_table();
  const uint8_t* p = static_cast<const uint8_t*>(data);
  for (size_t i = 0; i < n; i++) s = kTable.t[(s ^ p[i]) & 0xFFu] ^ (s >> 8);
  return s;
}

#ifdef MODELX_CRC32C_SSE42
__attribute__((target("sse4.2"))) inline uint32_t update_sse42(uint32_t s, const void* data,
                                                               size_t n) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint64_t s64 = s;
  for (; n >= 8; n -= 8, p += 8) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    s64 = _mm_crc32_u64(s64, w);
  }
  s = static_cast<uint32_t>(s64);
  for (; n; n--, p++) s = _mm_crc32_u8(s, *p);
  return s;
}
#endif

// Same register, with the SSE4.2 crc32 instruction where the CPU has it.
inline uint32_t update(uint32_t s, const void* data, size_t n) {
#ifdef MODELX_CRC32C_SSE42
  static const bool has_sse42 = __builtin_cpu_supports("sse4.2");
  if (has_sse42) return update_sse42(s, data, n);
#endif
  return update_bytewise(s, data, n);
}

inline uint32_t crc(const void* data, size_t n, bool model = false) {
  return (model ? update_bytewise(kInit, data, n) : update(kInit, data, n)) ^ kInit;
}

}  // namespace crc32c
}  // namespace modelx
