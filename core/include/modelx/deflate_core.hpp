// DEFLATE (RFC 1951) in a gzip member (RFC 1952), defined once for host and
// device: the round-based parse rules, the length and distance codes, the
// length-limited Huffman builder, the block header writer, the LSB-first bit
// writer, the stored fallback, the per-chunk bound and the CRC-32. The chunk
// kernel (core/hip/deflate.hip) and the host model below run this file, and
// the kernel's output equals the host model's byte for byte.
//
// Stream. The input is cut into chunks of kChunkBytes (32 KiB: the chunk and
// its output image share one LDS region in the kernel, see deflate.hip). Each
// chunk is compressed on its own, so no distance exceeds 32767. A chunk
// becomes one dynamic-Huffman block followed by an empty stored block, which
// ends it on a byte boundary (as Z_SYNC_FLUSH does), or, when that is not
// smaller, one stored block of n + 5 bytes. The last chunk's final block
// (the empty stored one, or the stored one) carries BFINAL. Chunks
// concatenate by byte copy.
//
// Parse. Greedy, minimum match 4, maximum 258 (a longer repeat continues as
// the next match), in rounds of kRound positions. A position p at or past
// `next` (the first position the earlier rounds left uncovered) with four
// bytes ahead of it looks up two candidates: the hash table's entry as the
// EARLIER rounds left it, and p - 1 (a run). The longer match wins; on equal
// length the run. Only after every position of the round has looked up does
// the round insert all its positions, table[h] = max(table[h], p + 1): the
// highest position wins whatever order the insertions come in, so the table
// after a round is a function of the bytes alone. Then the round is walked
// from max(next, base): a position with a match emits it and skips its
// length, any other emits a literal.
//
// Huffman builder (the approach of zstd_enc.hpp's huf_build_enc, to a limit
// of 15 bits, 7 for the code-length code): Shannon lengths ceil(log2(total /
// count)), clipped to the limit, then the Kraft sum is brought to exactly one:
// while it is too large the rarest symbol that can grow grows (ties: highest
// symbol), while it is too small the most frequent symbol whose share fits
// the gap shrinks (ties: highest symbol). Each step is an arg-max over the
// alphabet, which the kernel takes across the workgroup. An alphabet with no
// used symbol gets one 1-bit code on symbol 0 (a block without a match still
// declares one distance code); one used symbol gets one bit, and where the
// format demands a complete code (lit/len, code lengths) a second unused
// symbol gets the other 1-bit code.
//
// Header. HLIT/HDIST are trimmed to the last used symbol; the code lengths are
// sent one by one (no symbols 16-18); HCLEN is trimmed in the RFC's order.
//
// CRC-32 (IEEE, reflected 0xEDB88320), same conventions as crc32c_core.hpp:
// bit 31 of a register is x^0; a raw register starts at 0 and is linear in the
// message. The kernel leaves one raw value per chunk; the host joins them by
// reg = reg * x^(8 n) ^ raw from reg = 0xFFFFFFFF.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
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
namespace deflate {

constexpr uint32_t kChunkBytes = 32u << 10;
constexpr uint32_t kRound = 64;
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kMaxMatch = 258;
constexpr uint32_t kHashBits = 12;
constexpr uint32_t kNumLL = 286, kNumD = 30, kNumCL = 19;
constexpr uint32_t kLLBits = 15, kCLBits = 7;
constexpr uint32_t kStoredOverhead = 5;  // BFINAL/BTYPE byte, LEN, NLEN
constexpr uint32_t kGzipHeaderBytes = 10, kGzipTrailerBytes = 8;
// CM=8, FLG=0, MTIME=0, XFL=0, OS=255 (unknown)
constexpr uint8_t kGzipHeader[kGzipHeaderBytes] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
constexpr uint32_t kStoredFlag = 0x80000000u;  // in a chunk's reported size

MX_HD constexpr uint64_t chunk_count(uint64_t size) {
  return (size + kChunkBytes - 1) / kChunkBytes;
}
// Most bytes a chunk of n bytes becomes: the stored form, which is chosen
// whenever the Huffman form is not strictly smaller.
MX_HD constexpr uint32_t chunk_bound(uint32_t n) { return n + kStoredOverhead; }
MX_HD constexpr uint64_t gzip_bound(uint64_t size) {
  uint64_t chunks = chunk_count(size);
  return kGzipHeaderBytes + size + kStoredOverhead * (chunks ? chunks : 1) + kGzipTrailerBytes;
}

// ---- CRC-32 -----------------------------------------------------------------

namespace crc32 {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kInit = 0xFFFFFFFFu;

MX_HD constexpr uint32_t table_entry(uint32_t b) {
  for (int i = 0; i < 8; i++) b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
  return b;
}

MX_HD constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}

// v[k] = x^(8 * 2^k) mod P
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

// `reg` advanced through nbytes zero bytes.
MX_HD constexpr uint32_t mul_xn(uint32_t reg, uint64_t nbytes, const uint32_t* pow2) {
  for (int k = 0; nbytes; k++, nbytes >>= 1)
    if (nbytes & 1u) reg = gf_mul(reg, pow2[k]);
  return reg;
}

inline const uint32_t* pow_table() {
  static constexpr PowTable kPow = make_pow_table();
  return kPow.v;
}

// A register (raw or conventional) through n bytes, the host model.
inline uint32_t update(uint32_t s, const void* data, size_t n) {
  struct Table {
    uint32_t t[256];
  };
  static const Table kTable = [] {
    Table t{};
    for (uint32_t b = 0; b < 256; b++) t.t[b] = table_entry(b);
    return t;
  }();
  const uint8_t* p = static_cast<const uint8_t*>(data);
  for (size_t i = 0; i < n; i++) s = kTable.t[(s ^ p[i]) & 0xFFu] ^ (s >> 8);
  return s;
}

}  // namespace crc32

// ---- symbols ----------------------------------------------------------------

MX_HD inline uint32_t highbit(uint32_t v) { return 31u - static_cast<uint32_t>(__builtin_clz(v)); }

// Length code (symbol 257 + code) of a match of len3 + 3 bytes, its extra
// bit count and extra value.
MX_HD inline uint32_t len_code(uint32_t len3) {
  if (len3 < 8) return len3;
  if (len3 == 255) return 28;
  uint32_t e = highbit(len3) - 2;
  return 4 * e + 4 + ((len3 >> e) & 3u);
}
MX_HD inline uint32_t len_extra_bits(uint32_t code) {
  return (code < 8 || code == 28) ? 0 : (code >> 2) - 1;
}
// Distance code of dist1 + 1, its extra bit count; the extra value is the low
// bits of dist1.
MX_HD inline uint32_t dist_code(uint32_t dist1) {
  if (dist1 < 4) return dist1;
  uint32_t e = highbit(dist1) - 1;
  return 2 * e + 2 + ((dist1 >> e) & 1u);
}
MX_HD inline uint32_t dist_extra_bits(uint32_t code) { return code < 4 ? 0 : (code >> 1) - 1; }

// A token: a literal byte, or kTokMatch | (len - 3) << 16 | (dist - 1).
constexpr uint32_t kTokMatch = 0x80000000u;
MX_HD inline uint32_t make_match(uint32_t len, uint32_t dist) {
  return kTokMatch | ((len - 3) << 16) | (dist - 1);
}

// ---- parse ------------------------------------------------------------------

MX_HD inline uint32_t load32(const uint8_t* b, uint32_t p) {
  return b[p] | (uint32_t)b[p + 1] << 8 | (uint32_t)b[p + 2] << 16 | (uint32_t)b[p + 3] << 24;
}
MX_HD inline uint32_t hash32(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

// Common prefix of the bytes at a < p, at most maxl (p + maxl <= n).
MX_HD inline uint32_t match_len(const uint8_t* b, uint32_t a, uint32_t p, uint32_t maxl) {
  uint32_t l = 0;
  while (l + 4 <= maxl && load32(b, a + l) == load32(b, p + l)) l += 4;
  while (l < maxl && b[a + l] == b[p + l]) l++;
  return l;
}

// The match of position p (p + 4 <= n) given its table entry (position + 1,
// or 0): length << 16 | distance, or 0 without a match of kMinMatch.
MX_HD inline uint32_t find_match(const uint8_t* b, uint32_t n, uint32_t p, uint32_t entry) {
  uint32_t maxl = n - p < kMaxMatch ? n - p : kMaxMatch;
  uint32_t len = 0, dist = 0;
  if (entry) {
    uint32_t l = match_len(b, entry - 1, p, maxl);
    if (l >= kMinMatch) len = l, dist = p - (entry - 1);
  }
  if (p && dist != 1) {
    uint32_t l = match_len(b, p - 1, p, maxl);
    if (l >= kMinMatch && l >= len) len = l, dist = 1;
  }
  return len << 16 | dist;
}

// ---- trees ------------------------------------------------------------------

struct Trees {
  uint32_t hist_ll[288], hist_d[32], hist_cl[20];
  uint16_t code_ll[288], code_d[32], code_cl[20];
  uint8_t len_ll[288], len_d[32], len_cl[20];
  uint32_t cells[3];  // arg-max exchange of the builder
};

// How a group of threads runs the builder: the host is a group of one.
struct HostCtx {
  static constexpr uint32_t tid = 0, width = 1;
  void sync() const {}
  // max of v over the group; `cells` are three words at zero, `iter` counts
  // the calls
  uint32_t group_max(uint32_t v, uint32_t*, uint32_t) const { return v; }
};

// What one build_lengths call did, for the host's chunk_stats: the Kraft
// steps it took and how many of them made a code longer.
struct BuildSteps {
  uint32_t steps, shrink;
};

// Code lengths of `nsym` symbols from their counts, at most `maxbits` long.
// Every thread of the group calls it with the same arguments and gets the
// same answer; false if the lengths could not be made exact (the caller then
// stores the chunk). Counts are below 2^16. `steps`, if given, is filled on
// the host; device code ignores it.
template <class Ctx>
MX_HD inline bool build_lengths(const Ctx& cx, const uint32_t* hist, uint32_t nsym,
                                uint32_t maxbits, bool complete, uint8_t* len, uint32_t* cells,
                                BuildSteps* steps = nullptr) {
#if !defined(__HIP_DEVICE_COMPILE__)
  if (steps) steps->steps = steps->shrink = 0;
#else
  (void)steps;
#endif
  uint32_t total = 0, used = 0, one = 0;
  for (uint32_t s = 0; s < nsym; s++)
    if (hist[s]) total += hist[s], used++, one = s;
  for (uint32_t s = cx.tid; s < nsym; s += cx.width) {
    uint32_t l = 0;
    if (hist[s] && used >= 2) {
      while (((uint64_t)hist[s] << l) < total) l++;
      if (l > maxbits) l = maxbits;
    }
    len[s] = static_cast<uint8_t>(l);
  }
  if (cx.tid == 0) cells[0] = cells[1] = cells[2] = 0;
  cx.sync();
  if (used < 2) {
    if (cx.tid == 0) {
      len[used ? one : 0] = 1;
      if (complete) len[(used ? one : 0) ? 0 : 1] = 1;
    }
    cx.sync();
    return true;
  }
  const int32_t full = 1 << maxbits;
  int32_t K = 0;  // Kraft sum in units of 2^-maxbits
  for (uint32_t s = 0; s < nsym; s++)
    if (len[s]) K += 1 << (maxbits - len[s]);
  cx.sync();  // every thread has summed before an owner changes a length
  const uint32_t guard_max = 16 * nsym;
  for (uint32_t it = 0; K != full; it++) {
    if (it == guard_max) return false;
    const bool shrink = K > full;
    const int32_t gap = full - K;
    uint32_t key = 0;  // count (or its complement) << 13 | symbol << 4 | length
    for (uint32_t s = cx.tid; s < nsym; s += cx.width) {
      uint32_t l = len[s];  // only this thread writes len[s]
      if (!l) continue;
      uint32_t k = 0;
      if (shrink) {
        if (l < maxbits) k = (0xFFFFu - hist[s]) << 13 | s << 4 | l;
      } else if (l > 1 && (1 << (maxbits - l)) <= gap) {
        k = hist[s] << 13 | s << 4 | l;
      }
      if (k > key) key = k;
    }
    key = cx.group_max(key, cells, it);
    if (!key) return false;
#if !defined(__HIP_DEVICE_COMPILE__)
    if (steps) steps->steps++, steps->shrink += shrink;
#endif
    uint32_t pick = (key >> 4) & 511u, l = key & 15u;
    if (shrink) K -= 1 << (maxbits - l - 1);
    else K += 1 << (maxbits - l);
    if (pick % cx.width == cx.tid) len[pick] = static_cast<uint8_t>(shrink ? l + 1 : l - 1);
  }
  cx.sync();
  return true;
}

MX_HD inline uint32_t bit_reverse(uint32_t v, uint32_t nbits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < nbits; i++) r |= ((v >> i) & 1u) << (nbits - 1 - i);
  return r;
}

// Canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first writer.
// One thread.
MX_HD inline void assign_codes(const uint8_t* len, uint32_t nsym, uint16_t* code) {
  uint32_t count[16] = {}, next[16] = {};
  for (uint32_t s = 0; s < nsym; s++) count[len[s]]++;
  count[0] = 0;
  for (uint32_t l = 1; l < 16; l++) next[l] = (next[l - 1] + count[l - 1]) << 1;
  for (uint32_t s = 0; s < nsym; s++)
    code[s] = len[s] ? static_cast<uint16_t>(bit_reverse(next[len[s]]++, len[s])) : 0;
}

// ---- bit writer -------------------------------------------------------------

// ORs the low nb (<= 48) bits of v into the zeroed image at bit `pos`,
// LSB first. Device threads share words, so they OR atomically.
MX_HD inline void or_word(uint32_t* w, uint32_t v) {
  if (!v) return;
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(w, v);
#else
  *w |= v;
#endif
}
MX_HD inline void put_bits(uint32_t* img, uint32_t pos, uint64_t v, uint32_t nb) {
  uint32_t w = pos >> 5, sh = pos & 31u;
  uint64_t lo = v << sh;
  or_word(img + w, static_cast<uint32_t>(lo));
  or_word(img + w + 1, static_cast<uint32_t>(lo >> 32));
  if (sh + nb > 64) or_word(img + w + 2, static_cast<uint32_t>(v >> (64 - sh)));
}

// Code and extra bits of a token: the bits in *v, their count returned.
MX_HD inline uint32_t token_bits(const Trees& t, uint32_t tok, uint64_t* v) {
  if (!(tok & kTokMatch)) {
    *v = t.code_ll[tok];
    return t.len_ll[tok];
  }
  uint32_t len3 = (tok >> 16) & 0xFFu, dist1 = tok & 0x7FFFu;
  uint32_t lc = len_code(len3), dc = dist_code(dist1);
  uint32_t le = len_extra_bits(lc), de = dist_extra_bits(dc);
  uint64_t bits = t.code_ll[257 + lc];
  uint32_t nb = t.len_ll[257 + lc];
  // the extra value is the low bits of len3 (code 28 has none)
  bits |= (uint64_t)(len3 & ((1u << le) - 1u)) << nb;
  nb += le;
  bits |= (uint64_t)t.code_d[dc] << nb;
  nb += t.len_d[dc];
  bits |= (uint64_t)(dist1 & ((1u << de) - 1u)) << nb;
  *v = bits;
  return nb + de;
}

MX_HD inline void count_token(uint32_t tok, uint32_t* ll_sym, uint32_t* d_sym) {
  *ll_sym = (tok & kTokMatch) ? 257 + len_code((tok >> 16) & 0xFFu) : tok;
  *d_sym = dist_code(tok & 0x7FFFu);
}

// ---- block header -----------------------------------------------------------

constexpr uint8_t kCLOrder[kNumCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct HeaderShape {
  uint32_t nll, nd, ncl;  // HLIT + 257, HDIST + 1, HCLEN + 4
};

MX_HD inline HeaderShape header_shape(const Trees& t) {
  HeaderShape h{257, 1, 4};
  for (uint32_t s = 257; s < kNumLL; s++)
    if (t.len_ll[s]) h.nll = s + 1;
  for (uint32_t s = 1; s < kNumD; s++)
    if (t.len_d[s]) h.nd = s + 1;
  return h;
}

// Histogram of the code lengths the header sends. One thread.
MX_HD inline void count_code_lengths(Trees& t, const HeaderShape& h) {
  for (uint32_t s = 0; s < kNumCL; s++) t.hist_cl[s] = 0;
  for (uint32_t s = 0; s < h.nll; s++) t.hist_cl[t.len_ll[s]]++;
  for (uint32_t s = 0; s < h.nd; s++) t.hist_cl[t.len_d[s]]++;
}

MX_HD inline uint32_t trim_hclen(const Trees& t) {
  uint32_t ncl = 4;
  for (uint32_t i = 4; i < kNumCL; i++)
    if (t.len_cl[kCLOrder[i]]) ncl = i + 1;
  return ncl;
}

MX_HD inline uint32_t header_bit_count(const Trees& t, const HeaderShape& h) {
  uint32_t bits = 3 + 5 + 5 + 4 + 3 * h.ncl;
  for (uint32_t s = 0; s < 16; s++) bits += t.hist_cl[s] * t.len_cl[s];
  return bits;
}

// Bits of the tokens and the end-of-block symbol.
MX_HD inline uint32_t body_bit_count(const Trees& t) {
  uint32_t bits = 0;
  for (uint32_t s = 0; s < kNumLL; s++)
    bits += t.hist_ll[s] * (t.len_ll[s] + (s >= 257 ? len_extra_bits(s - 257) : 0));
  for (uint32_t s = 0; s < kNumD; s++) bits += t.hist_d[s] * (t.len_d[s] + dist_extra_bits(s));
  return bits;
}

// Writes the header of a BTYPE=10, BFINAL=0 block at bit 0; returns the bit
// after it. One thread.
MX_HD inline uint32_t write_header(const Trees& t, const HeaderShape& h, uint32_t* img) {
  uint32_t pos = 0;
  put_bits(img, pos, 4 /* BFINAL=0, BTYPE=10 */, 3), pos += 3;
  put_bits(img, pos, h.nll - 257, 5), pos += 5;
  put_bits(img, pos, h.nd - 1, 5), pos += 5;
  put_bits(img, pos, h.ncl - 4, 4), pos += 4;
  for (uint32_t i = 0; i < h.ncl; i++) put_bits(img, pos, t.len_cl[kCLOrder[i]], 3), pos += 3;
  for (uint32_t s = 0; s < h.nll; s++) {
    uint32_t l = t.len_ll[s];
    put_bits(img, pos, t.code_cl[l], t.len_cl[l]), pos += t.len_cl[l];
  }
  for (uint32_t s = 0; s < h.nd; s++) {
    uint32_t l = t.len_d[s];
    put_bits(img, pos, t.code_cl[l], t.len_cl[l]), pos += t.len_cl[l];
  }
  return pos;
}

// The empty stored block that ends a chunk on a byte boundary, written at
// bit `pos` (just after the end-of-block symbol); returns the chunk's bytes.
MX_HD inline uint32_t write_sync(uint32_t* img, uint32_t pos, bool last) {
  put_bits(img, pos, last ? 1 : 0, 3);  // BFINAL, BTYPE=00
  uint32_t at = (pos + 3 + 7) / 8;      // LEN=0000 is already there
  put_bits(img, at * 8 + 16, 0xFFFFu, 16);
  return at + 4;
}
MX_HD inline uint32_t huffman_bytes(uint32_t block_bits) { return (block_bits + 3 + 7) / 8 + 4; }

MX_HD inline void stored_header(uint8_t* out, uint32_t n, bool last) {
  out[0] = last ? 1 : 0;
  out[1] = static_cast<uint8_t>(n);
  out[2] = static_cast<uint8_t>(n >> 8);
  out[3] = static_cast<uint8_t>(~n);
  out[4] = static_cast<uint8_t>(~n >> 8);
}

// All three trees from the lit/len and distance counts, with the header's
// shape and the block's bit count. Every thread of the group calls it; false
// if a tree could not be built. `steps`, if given, is three BuildSteps (lit/len,
// distance, code lengths), filled on the host.
template <class Ctx>
MX_HD inline bool build_trees(const Ctx& cx, Trees& t, HeaderShape* shape, uint32_t* block_bits,
                              BuildSteps* steps = nullptr) {
  BuildSteps* const st_ll = steps;
  BuildSteps* const st_d = steps ? steps + 1 : nullptr;
  BuildSteps* const st_cl = steps ? steps + 2 : nullptr;
  if (!build_lengths(cx, t.hist_ll, kNumLL, kLLBits, true, t.len_ll, t.cells, st_ll)) return false;
  if (!build_lengths(cx, t.hist_d, kNumD, kLLBits, false, t.len_d, t.cells, st_d)) return false;
  HeaderShape h = header_shape(t);
  if (cx.tid == 0) {
    assign_codes(t.len_ll, kNumLL, t.code_ll);
    assign_codes(t.len_d, kNumD, t.code_d);
    count_code_lengths(t, h);
  }
  cx.sync();
  if (!build_lengths(cx, t.hist_cl, kNumCL, kCLBits, true, t.len_cl, t.cells, st_cl)) return false;
  if (cx.tid == 0) assign_codes(t.len_cl, kNumCL, t.code_cl);
  cx.sync();
  h.ncl = trim_hclen(t);
  *shape = h;
  *block_bits = header_bit_count(t, h) + body_bit_count(t);
  return true;
}

// ---- host model -------------------------------------------------------------

// Tokens of one chunk, with the lit/len and distance counts in t.
inline void parse_chunk(const uint8_t* b, uint32_t n, std::vector<uint32_t>& tokens, Trees& t) {
  std::vector<uint32_t> table(1u << kHashBits, 0);
  std::memset(t.hist_ll, 0, sizeof t.hist_ll);
  std::memset(t.hist_d, 0, sizeof t.hist_d);
  tokens.clear();
  uint32_t next = 0;
  for (uint32_t base = 0; base < n; base += kRound) {
    uint32_t end = base + kRound < n ? base + kRound : n;
    uint32_t m[kRound] = {};
    for (uint32_t p = base; p < end; p++)
      if (p >= next && p + 4 <= n) m[p - base] = find_match(b, n, p, table[hash32(load32(b, p))]);
    for (uint32_t p = base; p < end; p++)
      if (p + 4 <= n) {
        uint32_t& e = table[hash32(load32(b, p))];
        if (e < p + 1) e = p + 1;
      }
    for (uint32_t p = next > base ? next : base; p < end;) {
      uint32_t len = m[p - base] >> 16;
      uint32_t tok = len ? make_match(len, m[p - base] & 0xFFFFu) : b[p];
      uint32_t ll, d;
      count_token(tok, &ll, &d);
      t.hist_ll[ll]++;
      if (len) t.hist_d[d]++;
      tokens.push_back(tok);
      p += len ? len : 1;
      next = p;
    }
  }
  t.hist_ll[256] = 1;
}

// One chunk (1 <= n <= kChunkBytes) appended to `out`.
inline void compress_chunk(const uint8_t* b, uint32_t n, bool last, std::vector<uint8_t>& out) {
  Trees t{};
  std::vector<uint32_t> tokens;
  parse_chunk(b, n, tokens, t);
  HeaderShape shape;
  uint32_t block_bits = 0;
  bool ok = build_trees(HostCtx{}, t, &shape, &block_bits);
  if (!ok || huffman_bytes(block_bits) >= chunk_bound(n)) {
    uint8_t hdr[kStoredOverhead];
    stored_header(hdr, n, last);
    out.insert(out.end(), hdr, hdr + sizeof hdr);
    out.insert(out.end(), b, b + n);
    return;
  }
  std::vector<uint32_t> img(huffman_bytes(block_bits) / 4 + 4, 0);
  uint32_t pos = write_header(t, shape, img.data());
  for (uint32_t tok : tokens) {
    uint64_t v;
    uint32_t nb = token_bits(t, tok, &v);
    put_bits(img.data(), pos, v, nb);
    pos += nb;
  }
  put_bits(img.data(), pos, t.code_ll[256], t.len_ll[256]);
  pos += t.len_ll[256];
  uint32_t bytes = write_sync(img.data(), pos, last);
  const uint8_t* p = reinterpret_cast<const uint8_t*>(img.data());  // little-endian words
  out.insert(out.end(), p, p + bytes);
}

// Which paths compress_chunk takes on one chunk, for tests that must prove an
// input reaches the edge it was built for. The token figures are those of the
// Huffman form and stay zero for a stored chunk, whose tokens are not written.
struct ChunkStats {
  uint32_t tokens, matches;
  bool trees_ok, stored;
  uint32_t used_ll, used_d;           // symbols with a count
  uint32_t nll, nd, ncl;              // HLIT + 257, HDIST + 1, HCLEN + 4
  uint32_t max_ll_len, max_d_len;     // longest code of a used symbol
  uint32_t max_dist, max_dist_code;   // over the matches
  uint32_t len258;                    // matches of kMaxMatch
  uint32_t max_token_bits;            // code and extra bits of the widest token
  uint32_t three_word_puts;           // tokens with (pos & 31) + bits > 64
  uint32_t three_word_nonzero;        // ... whose bits in the third word are not all zero
  BuildSteps builder[3];              // lit/len, distance, code lengths
  uint32_t builder_steps_max;
};

// One chunk (1 <= n <= kChunkBytes) through the parse, the builder and the
// token walk of compress_chunk, writing nothing.
inline ChunkStats chunk_stats(const uint8_t* b, uint32_t n) {
  ChunkStats st{};
  Trees t{};
  std::vector<uint32_t> tokens;
  parse_chunk(b, n, tokens, t);
  st.tokens = static_cast<uint32_t>(tokens.size());
  for (uint32_t tok : tokens) {
    if (!(tok & kTokMatch)) continue;
    uint32_t len = ((tok >> 16) & 0xFFu) + 3, dist = (tok & 0x7FFFu) + 1;
    st.matches++;
    st.len258 += len == kMaxMatch;
    if (dist > st.max_dist) st.max_dist = dist, st.max_dist_code = dist_code(dist - 1);
  }
  for (uint32_t s = 0; s < kNumLL; s++) st.used_ll += t.hist_ll[s] != 0;
  for (uint32_t s = 0; s < kNumD; s++) st.used_d += t.hist_d[s] != 0;
  HeaderShape shape{};
  uint32_t block_bits = 0;
  st.trees_ok = build_trees(HostCtx{}, t, &shape, &block_bits, st.builder);
  for (const BuildSteps& bs : st.builder)
    if (bs.steps > st.builder_steps_max) st.builder_steps_max = bs.steps;
  st.stored = !st.trees_ok || huffman_bytes(block_bits) >= chunk_bound(n);
  if (!st.trees_ok) return st;
  st.nll = shape.nll, st.nd = shape.nd, st.ncl = shape.ncl;
  for (uint32_t s = 0; s < kNumLL; s++)
    if (t.hist_ll[s] && t.len_ll[s] > st.max_ll_len) st.max_ll_len = t.len_ll[s];
  for (uint32_t s = 0; s < kNumD; s++)
    if (t.hist_d[s] && t.len_d[s] > st.max_d_len) st.max_d_len = t.len_d[s];
  if (st.stored) return st;
  uint32_t pos = header_bit_count(t, shape);
  for (uint32_t tok : tokens) {
    uint64_t v;
    uint32_t nb = token_bits(t, tok, &v);
    if (nb > st.max_token_bits) st.max_token_bits = nb;
    if ((pos & 31u) + nb > 64) {
      st.three_word_puts++;
      st.three_word_nonzero += (v >> (64 - (pos & 31u))) != 0;
    }
    pos += nb;
  }
  return st;
}

inline void gzip_trailer(uint8_t* out, uint32_t crc, uint64_t size) {
  for (int i = 0; i < 4; i++) out[i] = static_cast<uint8_t>(crc >> (8 * i));
  for (int i = 0; i < 4; i++) out[4 + i] = static_cast<uint8_t>(size >> (8 * i));
}

inline std::vector<uint8_t> gzip_compress(const uint8_t* data, uint64_t size) {
  std::vector<uint8_t> out(kGzipHeader, kGzipHeader + kGzipHeaderBytes);
  if (size == 0) {
    uint8_t hdr[kStoredOverhead];
    stored_header(hdr, 0, true);
    out.insert(out.end(), hdr, hdr + sizeof hdr);
  }
  uint64_t chunks = chunk_count(size);
  for (uint64_t c = 0; c < chunks; c++) {
    uint64_t off = c * kChunkBytes;
    uint32_t n = static_cast<uint32_t>(size - off < kChunkBytes ? size - off : kChunkBytes);
    compress_chunk(data + off, n, c + 1 == chunks, out);
  }
  uint8_t tr[kGzipTrailerBytes];
  gzip_trailer(tr, crc32::update(crc32::kInit, data, size) ^ crc32::kInit, size);
  out.insert(out.end(), tr, tr + sizeof tr);
  return out;
}

}  // namespace deflate
}  // namespace modelx
