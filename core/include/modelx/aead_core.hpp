// ChaCha20-Poly1305 (RFC 8439) arithmetic, compiled for host and device alike:
// the ChaCha20 quarter round and block, Poly1305 in five 26-bit limbs with
// 64-bit accumulators, and the sealed-blob layout of the client-side
// encryption. The kernel (core/hip/aead.hip), the engine's host functions and
// the CPU client all run this one definition; the sequential seal/open below
// is the host model the kernel is tested against.
//
// Sealed blob. The n >= 1 stored bytes P are cut into segments of `seg` bytes
// (a multiple of kRowBytes, kMinSegmentBytes..kMaxSegmentBytes), the last one
// shorter. Segment i is sealed with the RFC 8439 section 2.8 AEAD under the
// blob key: nonce LE32(1 if i is the last segment else 0) + LE64(i), empty
// AAD, the Poly1305 key from block counter 0, data from counter 1. The sealed
// blob is the ciphertext at P's offsets followed by one 16-byte tag per
// segment, in order: n + 16 * nseg bytes.
//
// Poly1305 conventions. A field element is five limbs, value
// sum(v[i] << 26i) mod 2^130 - 5. A limb is "loose": mulmod and carry return
// limbs below 2^26 + 2^11, and mulmod takes limbs up to 2^28 in its first
// factor and below 2^27 in its second, so a sum of two loose elements can be
// multiplied without a carry in between. With empty AAD the MAC input is the
// ciphertext zero-padded to 16 bytes and then LE64(0) + LE64(len): every
// block is a full 16 bytes and carries the 2^128 bit.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

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
namespace aead {

constexpr uint64_t kRowBytes = 1024;  // 64 lanes x one 16 B word: the kernel's trip
constexpr uint64_t kMinSegmentBytes = 1024;
constexpr uint64_t kMaxSegmentBytes = 16ull << 20;
constexpr uint64_t kDefaultSegmentBytes = 128u << 10;
constexpr uint64_t kTagBytes = 16;
constexpr uint64_t kKeyBytes = 32;

MX_HD constexpr bool valid_segment(uint64_t seg) {
  return seg >= kMinSegmentBytes && seg <= kMaxSegmentBytes && seg % kRowBytes == 0;
}

MX_HD constexpr uint64_t segment_count(uint64_t n, uint64_t seg) { return (n + seg - 1) / seg; }

MX_HD constexpr uint64_t sealed_size(uint64_t n, uint64_t seg) {
  return n + kTagBytes * segment_count(n, seg);
}

// The key as the eight little-endian words of the ChaCha state; passed to the
// kernel by value.
struct Key {
  uint32_t w[8];
};

// ---- ChaCha20 ---------------------------------------------------------------

constexpr uint32_t kSigma0 = 0x61707865u, kSigma1 = 0x3320646eu, kSigma2 = 0x79622d32u,
                   kSigma3 = 0x6b206574u;  // "expand 32-byte k"

MX_HD inline uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

MX_HD inline void quarter_round(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b; d ^= a; d = rotl(d, 16);
  c += d; b ^= c; b = rotl(b, 12);
  a += b; d ^= a; d = rotl(d, 8);
  c += d; b ^= c; b = rotl(b, 7);
}

// Nonce words of segment `index`: state words 13, 14 and 15.
MX_HD inline void segment_nonce(uint64_t index, bool last, uint32_t nonce[3]) {
  nonce[0] = last ? 1u : 0u;
  nonce[1] = static_cast<uint32_t>(index);
  nonce[2] = static_cast<uint32_t>(index >> 32);
}

// One 64-byte block as sixteen little-endian words.
MX_HD inline void chacha_block(const Key& key, uint32_t counter, const uint32_t nonce[3],
                               uint32_t out[16]) {
  uint32_t in[16] = {kSigma0,   kSigma1,   kSigma2,   kSigma3,
                     key.w[0],  key.w[1],  key.w[2],  key.w[3],
                     key.w[4],  key.w[5],  key.w[6],  key.w[7],
                     counter,   nonce[0],  nonce[1],  nonce[2]};
  uint32_t x[16];
  for (int i = 0; i < 16; i++) x[i] = in[i];
  for (int i = 0; i < 10; i++) {
    quarter_round(x[0], x[4], x[8], x[12]);
    quarter_round(x[1], x[5], x[9], x[13]);
    quarter_round(x[2], x[6], x[10], x[14]);
    quarter_round(x[3], x[7], x[11], x[15]);
    quarter_round(x[0], x[5], x[10], x[15]);
    quarter_round(x[1], x[6], x[11], x[12]);
    quarter_round(x[2], x[7], x[8], x[13]);
    quarter_round(x[3], x[4], x[9], x[14]);
  }
  for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}

// ---- Poly1305 ---------------------------------------------------------------

constexpr uint32_t kLimbMask = 0x3ffffffu;

struct Fe {
  uint32_t v[5];
};

// The 16-byte block whose little-endian words are w, plus hibit * 2^128.
MX_HD inline Fe fe_from_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3,
                              uint32_t hibit) {
  Fe f;
  f.v[0] = w0 & kLimbMask;
  f.v[1] = ((w0 >> 26) | (w1 << 6)) & kLimbMask;
  f.v[2] = ((w1 >> 20) | (w2 << 12)) & kLimbMask;
  f.v[3] = ((w2 >> 14) | (w3 << 18)) & kLimbMask;
  f.v[4] = (w3 >> 8) | (hibit << 24);
  return f;
}

// r of a Poly1305 key: its first four words, clamped.
MX_HD inline Fe fe_clamped_r(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  return fe_from_words(w0 & 0x0fffffffu, w1 & 0x0ffffffcu, w2 & 0x0ffffffcu, w3 & 0x0ffffffcu,
                       0);
}

// The block that closes the MAC of `len` ciphertext bytes with empty AAD.
MX_HD inline Fe fe_length_block(uint64_t len) {
  return fe_from_words(0, 0, static_cast<uint32_t>(len), static_cast<uint32_t>(len >> 32), 1);
}

MX_HD inline Fe fe_one() { return Fe{{1, 0, 0, 0, 0}}; }

MX_HD inline Fe fe_add(const Fe& a, const Fe& b) {
  Fe f;
  for (int i = 0; i < 5; i++) f.v[i] = a.v[i] + b.v[i];
  return f;
}

// Wide limbs (each below 2^59) to loose limbs; 2^130 = 5 wraps the top carry.
MX_HD inline Fe fe_carry(uint64_t d0, uint64_t d1, uint64_t d2, uint64_t d3, uint64_t d4) {
  Fe f;
  d1 += d0 >> 26;
  d2 += d1 >> 26;
  d3 += d2 >> 26;
  d4 += d3 >> 26;
  uint64_t h0 = (d0 & kLimbMask) + (d4 >> 26) * 5u;
  f.v[0] = static_cast<uint32_t>(h0) & kLimbMask;
  f.v[1] = (static_cast<uint32_t>(d1) & kLimbMask) + static_cast<uint32_t>(h0 >> 26);
  f.v[2] = static_cast<uint32_t>(d2) & kLimbMask;
  f.v[3] = static_cast<uint32_t>(d3) & kLimbMask;
  f.v[4] = static_cast<uint32_t>(d4) & kLimbMask;
  return f;
}

// The multiples 5*b[1..4] that a multiplication by b folds the high partial
// products with; kept next to b where b is used more than once.
struct Fe5 {
  uint32_t v[4];
};

MX_HD inline Fe5 fe_times5(const Fe& b) {
  return Fe5{{b.v[1] * 5u, b.v[2] * 5u, b.v[3] * 5u, b.v[4] * 5u}};
}

// a * b mod 2^130 - 5; s must be fe_times5(b). Limbs of a up to 2^28, of b
// below 2^27: every accumulator stays below 5 * 2^28 * 5 * 2^27 < 2^60.
MX_HD inline Fe fe_mulmod(const Fe& a, const Fe& b, const Fe5& s) {
  const uint64_t a0 = a.v[0], a1 = a.v[1], a2 = a.v[2], a3 = a.v[3], a4 = a.v[4];
  uint64_t d0 = a0 * b.v[0] + a1 * s.v[3] + a2 * s.v[2] + a3 * s.v[1] + a4 * s.v[0];
  uint64_t d1 = a0 * b.v[1] + a1 * b.v[0] + a2 * s.v[3] + a3 * s.v[2] + a4 * s.v[1];
  uint64_t d2 = a0 * b.v[2] + a1 * b.v[1] + a2 * b.v[0] + a3 * s.v[3] + a4 * s.v[2];
  uint64_t d3 = a0 * b.v[3] + a1 * b.v[2] + a2 * b.v[1] + a3 * b.v[0] + a4 * s.v[3];
  uint64_t d4 = a0 * b.v[4] + a1 * b.v[3] + a2 * b.v[2] + a3 * b.v[1] + a4 * b.v[0];
  return fe_carry(d0, d1, d2, d3, d4);
}

MX_HD inline Fe fe_mulmod(const Fe& a, const Fe& b) { return fe_mulmod(a, b, fe_times5(b)); }

// (h mod 2^130 - 5) + s mod 2^128, as the tag's four little-endian words.
// h loose; s is the second half of the Poly1305 key.
MX_HD inline void fe_tag(const Fe& h, const uint32_t s[4], uint32_t tag[4]) {
  // all limbs strictly below 2^26, the value below 2^130
  uint32_t h0 = h.v[0], h1 = h.v[1], h2 = h.v[2], h3 = h.v[3], h4 = h.v[4];
  uint32_t c;
  c = h1 >> 26; h1 &= kLimbMask; h2 += c;
  c = h2 >> 26; h2 &= kLimbMask; h3 += c;
  c = h3 >> 26; h3 &= kLimbMask; h4 += c;
  c = h4 >> 26; h4 &= kLimbMask; h0 += c * 5u;
  c = h0 >> 26; h0 &= kLimbMask; h1 += c;
  c = h1 >> 26; h1 &= kLimbMask; h2 += c;
  c = h2 >> 26; h2 &= kLimbMask; h3 += c;
  c = h3 >> 26; h3 &= kLimbMask; h4 += c;
  // g = h + 5 - 2^130; take it when it is not negative, i.e. h >= p
  uint32_t g0 = h0 + 5u;
  c = g0 >> 26; g0 &= kLimbMask;
  uint32_t g1 = h1 + c;
  c = g1 >> 26; g1 &= kLimbMask;
  uint32_t g2 = h2 + c;
  c = g2 >> 26; g2 &= kLimbMask;
  uint32_t g3 = h3 + c;
  c = g3 >> 26; g3 &= kLimbMask;
  uint32_t g4 = h4 + c - (1u << 26);
  uint32_t take_g = (g4 >> 31) - 1u;  // all ones when g4 did not wrap
  h0 = (h0 & ~take_g) | (g0 & take_g);
  h1 = (h1 & ~take_g) | (g1 & take_g);
  h2 = (h2 & ~take_g) | (g2 & take_g);
  h3 = (h3 & ~take_g) | (g3 & take_g);
  h4 = (h4 & ~take_g) | (g4 & take_g & kLimbMask);
  uint64_t f;
  f = static_cast<uint64_t>(h0 | (h1 << 26)) + s[0];
  tag[0] = static_cast<uint32_t>(f);
  f = static_cast<uint64_t>((h1 >> 6) | (h2 << 20)) + s[1] + (f >> 32);
  tag[1] = static_cast<uint32_t>(f);
  f = static_cast<uint64_t>((h2 >> 12) | (h3 << 14)) + s[2] + (f >> 32);
  tag[2] = static_cast<uint32_t>(f);
  f = static_cast<uint64_t>((h3 >> 18) | (h4 << 8)) + s[3] + (f >> 32);
  tag[3] = static_cast<uint32_t>(f);
}

// ---- host model ---------------------------------------------------------------

inline Key key_from_bytes(const uint8_t key32[32]) {
  Key k;
  std::memcpy(k.w, key32, 32);  // little-endian hosts only, as the rest of the core
  return k;
}

// Seal (open == false) or open one segment, sequentially: src -> dst (which
// may be the same), the tag of the ciphertext into tag[16]. Opening writes
// the plaintext whatever the tag; the caller compares.
inline void crypt_segment(const Key& key, uint64_t index, bool last, bool open,
                          const uint8_t* src, uint64_t len, uint8_t* dst, uint8_t tag[16]) {
  uint32_t nonce[3], ks[16];
  segment_nonce(index, last, nonce);
  chacha_block(key, 0, nonce, ks);
  const Fe r = fe_clamped_r(ks[0], ks[1], ks[2], ks[3]);
  const Fe5 r5 = fe_times5(r);
  const uint32_t s[4] = {ks[4], ks[5], ks[6], ks[7]};
  Fe h{{0, 0, 0, 0, 0}};
  for (uint64_t off = 0; off < len; off += 64) {
    chacha_block(key, static_cast<uint32_t>(1 + off / 64), nonce, ks);
    const uint64_t take = len - off < 64 ? len - off : 64;
    uint8_t in[64] = {0}, out[64] = {0};
    std::memcpy(in, src + off, take);
    for (uint64_t i = 0; i < take; i++)
      out[i] = in[i] ^ static_cast<uint8_t>(ks[i / 4] >> (8 * (i % 4)));
    std::memcpy(dst + off, out, take);
    const uint8_t* mac = open ? in : out;  // zero-padded ciphertext
    for (uint64_t b = 0; b < take; b += 16) {
      uint32_t w[4];
      std::memcpy(w, mac + b, 16);
      h = fe_mulmod(fe_add(h, fe_from_words(w[0], w[1], w[2], w[3], 1)), r, r5);
    }
  }
  h = fe_mulmod(fe_add(h, fe_length_block(len)), r, r5);
  uint32_t t[4];
  fe_tag(h, s, t);
  std::memcpy(tag, t, 16);
}

// src[0, n) -> dst[0, sealed_size(n, seg)). n >= 1, seg valid.
inline void seal_blob(const Key& key, const uint8_t* src, uint64_t n, uint64_t seg,
                      uint8_t* dst) {
  const uint64_t nseg = segment_count(n, seg);
  for (uint64_t i = 0; i < nseg; i++) {
    const uint64_t off = i * seg, len = n - off < seg ? n - off : seg;
    crypt_segment(key, i, i == nseg - 1, false, src + off, len, dst + off,
                  dst + n + kTagBytes * i);
  }
}

// stored[0, sealed_size(n, seg)) -> dst[0, n) (which may be `stored`). Returns
// the first segment whose tag does not match, or -1; all segments are
// written either way, and the tags compared without an early exit.
inline int64_t open_blob(const Key& key, const uint8_t* stored, uint64_t n, uint64_t seg,
                         uint8_t* dst) {
  const uint64_t nseg = segment_count(n, seg);
  int64_t bad = -1;
  for (uint64_t i = 0; i < nseg; i++) {
    const uint64_t off = i * seg, len = n - off < seg ? n - off : seg;
    uint8_t tag[16], want[16];
    std::memcpy(want, stored + n + kTagBytes * i, 16);  // before dst may cover it
    crypt_segment(key, i, i == nseg - 1, true, stored + off, len, dst + off, tag);
    uint8_t diff = 0;
    for (int b = 0; b < 16; b++) diff |= tag[b] ^ want[b];
    if (diff && bad < 0) bad = static_cast<int64_t>(i);
  }
  return bad;
}

}  // namespace aead
}  // namespace modelx
