// Span-parallel inflate of one gzip member (RFC 1951/1952), defined once for
// host and device: the header parse, the bit reader, the decode tables, the
// span decoder, the chain walk and the host model. The kernels
// (core/hip/inflate.hip) run this file with a wave as the group; the host
// model runs it with a group of one, and the two give the same span records
// and the same bytes.
//
// Why a member can be decoded in pieces. deflate_core.hpp compresses every
// 32 KiB chunk on its own and ends each Huffman chunk with an empty stored
// block, the byte-aligned 00 00 FF FF that Z_SYNC_FLUSH leaves; pigz -i and
// Z_FULL_FLUSH streams have the same shape. Wherever no match reaches back
// past such a marker, the stream after it decodes without the bytes before it.
//
// Candidate: the first deflate byte after the gzip header, or a position i
// with bytes[i-4..i) == 00 00 FF FF.
//
// Span: decoded from a candidate block by block (stored, fixed, dynamic; code
// length symbols 16-18). It ends at the byte after the first EMPTY stored block
// it consumes, or, when a block carries BFINAL, at the next byte boundary
// after that block (kFinal is then set). Its record is {end, out_bytes,
// status}:
//   corrupt    block type 3, an over-subscribed or incomplete code (zlib's
//              rules: a lone 1-bit code and an empty distance code may be
//              incomplete), no end-of-block code, LEN != ~NLEN, a bad repeat,
//              a symbol above 285 or 29, an unassigned code, running past the
//              stream
//   dependent  a distance that reaches before the span's own first byte
//   too-long   more than kSpanMaxCoded bytes of Huffman blocks (headers
//              included, counted token by token) in one span; stored blocks
//              do not count. A stock, unflushed stream ends the attempt here
//              after bounded work.
//
// Chain: from the first candidate follow `end`; every end that is not final
// is a candidate by construction. The member is eligible when every span on
// the chain is ok, the final span ends exactly at the trailer, and the
// out_bytes sum to ISIZE mod 2^32. Otherwise the status names the first
// reason: a span's own, `trailing` (bytes between the final block and the
// trailer: a second member, say), `corrupt` (ISIZE, and in the host model
// the CRC-32), `header` (no gzip header within kHeaderMax bytes, or no room
// for the trailer), `too-large` (4 GiB and above). Candidates off the chain
// are false markers and are ignored.
//
// A stream without markers is `too-long` or `dependent` by these rules; the
// section "search" at the end of this file decodes it from found block starts.
//
// Group. decode_span is called by every thread of a group with the same
// arguments, like deflate::build_lengths. Thread 0 owns the bit reader and
// decodes; what the others need it leaves in Work::ctl. The group fills the
// decode tables side by side: one code length per thread for the sorted
// symbol list, then one table entry per thread per trip, each entry found by
// the canonical first-code walk over the per-length counts, the same walk
// that serves codes longer than the primary lookup. Tokens are those of
// deflate_core.hpp; the sink takes them a batch at a time.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "modelx/deflate_core.hpp"

namespace modelx {
namespace inflate {

constexpr uint32_t kSpanMaxCoded = 256u << 10;
constexpr uint32_t kHeaderMax = 4096;
constexpr uint32_t kLLBits = 10, kDBits = 8, kCLBits = 7;  // primary lookups
constexpr uint32_t kMaxLL = 288, kMaxD = 32;               // the fixed code's alphabets
constexpr uint32_t kBatch = 64;
constexpr uint32_t kMarker = 0xFFFF0000u;  // 00 00 FF FF read as a little-endian word

enum Status : uint32_t {
  kOk = 0,
  kCorrupt = 1,
  kDependent = 2,
  kTooLong = 3,
  kHeader = 4,
  kTrailing = 5,
  kTooLarge = 6,
};
constexpr uint32_t kStatusMask = 0xFFu, kFinal = 0x100u;

inline const char* status_name(uint32_t s) {
  static const char* const names[] = {"ok", "corrupt", "dependent", "too-long",
                                      "header", "trailing", "too-large"};
  return names[(s & kStatusMask) <= kTooLarge ? (s & kStatusMask) : kCorrupt];
}

struct SpanRec {
  uint64_t out_bytes;
  uint32_t end;
  uint32_t status;  // Status | kFinal
};

// Block search (gunzip of streams without markers; see "search" below). A
// candidate is key << 1 | kind: kind 0 a block header whose first bit is at
// bit position `key`, kind 1 a stored block whose LEN field is at byte key / 8.
// A span that ends at a candidate leaves the candidate's byte in `end` and its
// low four bits (bit in the byte, kind) in the status from kEndShift up.
constexpr uint32_t kWindow = 32768;      // deflate's history
constexpr uint32_t kUnknown = 0x8000u;   // | k: byte k of the window a span was not given
constexpr uint32_t kCutHere = 0x80u;     // thread 0 -> group inside decode_span only
constexpr uint32_t kEndShift = 16;
constexpr uint64_t kNoCand = ~0ull;

MX_HD inline uint64_t make_cand(uint64_t bit, bool stored) { return bit << 1 | (stored ? 1u : 0u); }
MX_HD inline uint64_t end_cand(const SpanRec& rec) {
  return static_cast<uint64_t>(rec.end) << 4 | ((rec.status >> kEndShift) & 15u);
}

struct MarkerCut {
  static constexpr bool kSearch = false;
  MX_HD bool hit(uint64_t) { return false; }
};
// Ends the span at the first candidate of the sorted list, from `cur` on, that
// a block of the span's own chain starts at; the ones it passes are not on it.
struct ListCut {
  static constexpr bool kSearch = true;
  const uint64_t* cand;
  uint32_t n, cur;
  MX_HD bool hit(uint64_t c) {
    while (cur < n && cand[cur] < c) cur++;
    return cur < n && cand[cur] == c;
  }
};
// Ends the span where the plan says the next one starts.
struct EndCut {
  static constexpr bool kSearch = true;
  uint64_t end;
  MX_HD bool hit(uint64_t c) const { return c == end; }
};

// One span of the chain, as the emitting kernel takes it. In a search plan
// pad_ holds the low four bits of the span's candidate (in_start its byte).
struct PlanSpan {
  uint64_t out_offset;
  uint64_t out_bytes;
  uint32_t in_start;
  uint32_t pad_;
};

MX_HD inline uint64_t plan_cand(const PlanSpan& sp) {
  return static_cast<uint64_t>(sp.in_start) << 4 | (sp.pad_ & 15u);
}

// One span of a search's chain, as the window kernel takes it: which ring, and
// out_bytes % kWindow, where the window behind the span starts in it.
struct ChainLink {
  uint32_t ring, rot;
};

// Tokens that are neither literal nor match.
constexpr uint32_t kTokEnd = 0x40000000u, kTokBad = 0x40000001u;

// ---- gzip header ------------------------------------------------------------

// Length of the gzip header at b (n bytes visible, at most kHeaderMax of the
// member), or 0 if there is none that ends within them.
inline uint32_t parse_header(const uint8_t* b, uint64_t n) {
  if (n > kHeaderMax) n = kHeaderMax;
  if (n < deflate::kGzipHeaderBytes || b[0] != 0x1f || b[1] != 0x8b || b[2] != 8 || (b[3] & 0xE0u))
    return 0;
  const uint8_t flg = b[3];
  uint64_t p = deflate::kGzipHeaderBytes;
  if (flg & 4u) {  // FEXTRA
    if (p + 2 > n) return 0;
    p += 2 + (b[p] | (uint32_t)b[p + 1] << 8);
  }
  for (uint32_t bit = 8; bit <= 16; bit <<= 1)  // FNAME, FCOMMENT
    if (flg & bit) {
      while (p < n && b[p]) p++;
      p++;
    }
  if (flg & 2u) p += 2;  // FHCRC
  return p <= n ? static_cast<uint32_t>(p) : 0;
}

// ---- bit reader -------------------------------------------------------------

// LSB-first reader over cx.byte(pos), pos < limit; past the limit it reads
// zeros and past() turns true. `pos` is the next byte to load: fill() loads at
// most 8 bytes and leaves at least 57 bits.
struct BitReader {
  uint64_t buf, pos, limit;
  uint32_t cnt;
  MX_HD void init(uint64_t at, uint64_t lim) { buf = 0, cnt = 0, pos = at, limit = lim; }
  template <class Ctx>
  MX_HD void fill(const Ctx& cx) {
    while (cnt <= 56) {
      uint64_t b = pos < limit ? cx.byte(pos) : 0;
      buf |= b << cnt;
      cnt += 8, pos++;
    }
  }
  MX_HD uint32_t peek(uint32_t n) const { return static_cast<uint32_t>(buf) & ((1u << n) - 1u); }
  MX_HD void drop(uint32_t n) { buf >>= n, cnt -= n; }
  MX_HD uint32_t take(uint32_t n) {
    uint32_t v = peek(n);
    drop(n);
    return v;
  }
  MX_HD uint64_t bit_pos() const { return pos * 8 - cnt; }
  MX_HD bool past() const { return bit_pos() > limit * 8; }
};

// ---- decode tables ----------------------------------------------------------

// What a group needs to decode one block.
struct Tables {
  uint16_t ll[1u << kLLBits];  // symbol << 4 | length, 0: not in the lookup
  uint16_t d[1u << kDBits];    // the code length code's lookup while a header is read
  uint16_t sorted_ll[kMaxLL];  // symbols by length, then by value
  uint16_t sorted_d[kMaxD];
  uint16_t count_ll[16], count_d[16];  // codes per length
  uint8_t len[kMaxLL + kMaxD];
};

struct Work {
  Tables t;
  uint32_t tok[kBatch];
  uint32_t ctl[8];  // thread 0 -> group
};

enum CodeKind { kCodeLengths, kCodeLL, kCodeD };

// Counts per length of the n lengths, and whether they make a code inflate
// accepts. One thread.
MX_HD inline bool count_lengths(const uint8_t* len, uint32_t n, uint16_t* count, CodeKind kind) {
  for (uint32_t l = 0; l < 16; l++) count[l] = 0;
  for (uint32_t s = 0; s < n; s++) count[len[s] & 15u]++;
  count[0] = 0;
  int32_t left = 1;
  uint32_t used = 0, maxl = 0;
  for (uint32_t l = 1; l < 16; l++) {
    left = left * 2 - count[l];
    if (left < 0) return false;  // over-subscribed
    used += count[l];
    if (count[l]) maxl = l;
  }
  if (left == 0) return true;
  if (used == 0) return kind == kCodeD;    // a block of literals only
  return kind != kCodeLengths && maxl == 1;  // one 1-bit code
}

// Thread `l` of 1..15 puts the symbols of length l, ascending, where the
// canonical order has them.
MX_HD inline void sort_length(const uint8_t* len, uint32_t n, const uint16_t* count, uint32_t l,
                              uint16_t* sorted) {
  if (!count[l]) return;
  uint32_t at = 0;
  for (uint32_t k = 1; k < l; k++) at += count[k];
  for (uint32_t s = 0; s < n; s++)
    if (len[s] == l) sorted[at++] = static_cast<uint16_t>(s);
}

// The symbol whose code is the low bits of `bits`, first bit lowest, if it is
// at most maxlen long: symbol << 4 | length, else 0.
MX_HD inline uint32_t walk(const uint16_t* count, const uint16_t* sorted, uint32_t bits,
                           uint32_t maxlen) {
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l <= maxlen; l++) {
    code |= bits & 1u;
    bits >>= 1;
    uint32_t c = count[l];
    if (code - first < c) return static_cast<uint32_t>(sorted[index + code - first]) << 4 | l;
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return 0;
}

// The sorted list and the 2^bits lookup entries of a counted code, by the group.
template <class Ctx>
MX_HD inline void fill_table(const Ctx& cx, const uint8_t* len, uint32_t n, const uint16_t* count,
                             uint16_t* sorted, uint16_t* tab, uint32_t bits) {
  for (uint32_t l = 1 + cx.tid; l < 16; l += cx.width) sort_length(len, n, count, l, sorted);
  cx.sync();
  for (uint32_t i = cx.tid; i < (1u << bits); i += cx.width)
    tab[i] = static_cast<uint16_t>(walk(count, sorted, i, bits));
  cx.sync();
}

// One symbol off a reader with 15 bits filled; 0xFFFF for an unassigned code.
MX_HD inline uint32_t decode_symbol(BitReader& r, const uint16_t* tab, uint32_t bits,
                                    const uint16_t* count, const uint16_t* sorted) {
  uint32_t e = tab[r.peek(bits)];
  if (!e) e = walk(count, sorted, r.peek(15), 15);
  if (!e) return 0xFFFFu;
  r.drop(e & 15u);
  return e >> 4;
}

MX_HD inline uint32_t len_base(uint32_t code) {
  if (code < 8) return 3 + code;
  if (code == 28) return 258;
  return 3 + ((4 + (code & 3u)) << ((code >> 2) - 1));
}
MX_HD inline uint32_t dist_base(uint32_t code) {
  return code < 4 ? 1 + code : 1 + ((2 + (code & 1u)) << ((code >> 1) - 1));
}

// One token (at most 48 bits) off a filled reader.
MX_HD inline uint32_t decode_token(BitReader& r, const Tables& t) {
  uint32_t s = decode_symbol(r, t.ll, kLLBits, t.count_ll, t.sorted_ll);
  if (s < 256) return s;
  if (s == 256) return kTokEnd;
  if (s >= 257 + 29) return kTokBad;
  uint32_t lc = s - 257;
  uint32_t len = len_base(lc) + r.take(deflate::len_extra_bits(lc));
  uint32_t dc = decode_symbol(r, t.d, kDBits, t.count_d, t.sorted_d);
  if (dc >= 30) return kTokBad;
  uint32_t dist = dist_base(dc) + r.take(deflate::dist_extra_bits(dc));
  return deflate::make_match(len, dist);
}

MX_HD inline void fixed_lengths(uint8_t* len) {
  for (uint32_t s = 0; s < kMaxLL; s++) len[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
  for (uint32_t s = 0; s < kMaxD; s++) len[kMaxLL + s] = 5;
}

// Progress through the code lengths of a dynamic header.
struct LenState {
  uint32_t nll, nd, idx;
};

// Reads code lengths with the lookup in t.d until all are read (1), the
// reader has loaded to within 8 bytes of `safe` (0: call again after a
// refill), or they are bad (2). One thread.
template <class Ctx>
MX_HD inline uint32_t read_lengths(const Ctx& cx, BitReader& r, Tables& t, LenState& st,
                                   uint64_t safe) {
  const uint32_t total = st.nll + st.nd;
  while (st.idx < total) {
    if (r.pos + 8 > safe) return 0;
    r.fill(cx);
    uint32_t s = decode_symbol(r, t.d, kCLBits, t.count_d, t.sorted_d);
    if (s > 18 || r.past()) return 2;
    if (s < 16) {
      t.len[st.idx++] = static_cast<uint8_t>(s);
      continue;
    }
    uint32_t rep, v = 0;
    if (s == 16) {
      if (!st.idx) return 2;
      v = t.len[st.idx - 1];
      rep = 3 + r.take(2);
    } else {
      rep = s == 17 ? 3 + r.take(3) : 11 + r.take(7);
    }
    if (st.idx + rep > total) return 2;
    while (rep--) t.len[st.idx++] = static_cast<uint8_t>(v);
  }
  return r.past() ? 2 : 1;
}

// ---- span -------------------------------------------------------------------

// Ctx: tid, width, sync(), byte(pos), and refill(pos): the group makes the
// stream from byte `pos` on readable and returns the position up to which it
// is (thread 0 loads no byte at or past it before the next refill; at least
// 512 bytes on, or everything). Sink: stored(cx, at, len, out) copies a stored
// block's bytes, tokens(cx, tok, n, &out) takes a batch, adds what it
// produces to `out` and returns a status; `out` counts the span's bytes.
//
// The span starts at the candidate `start` (make_cand: a block header at a bit
// position, or the LEN field of a stored block whose header is taken as
// BFINAL=0). Cut says where it ends short of BFINAL. MarkerCut: after an empty
// stored block, as above. A searching Cut (kSearch) is asked by thread 0, with
// the candidate that every later block without BFINAL would start as, in
// stream order; the first hit ends the span before that block, and empty
// stored blocks are blocks like any other.
template <class Ctx, class Sink, class Cut>
MX_HD inline SpanRec decode_span(Ctx& cx, Work& w, Sink& sink, uint64_t start, uint64_t limit,
                                 Cut& cut) {
  const uint64_t start_bit = start >> 1;
  const bool at_len = (start & 1u) != 0;
  BitReader r;  // thread 0's
  r.init(start_bit >> 3, limit);
  uint64_t out = 0, coded = 0, at = start_bit >> 3, end = 0;
  uint32_t status = kOk;
  bool first = true, cut_here = false;
  for (;;) {
    uint64_t safe = cx.refill(at);
    LenState ls{kMaxLL, kMaxD, 0};
    uint64_t block_start = 0;
    if (cx.tid == 0) {
      r.fill(cx);
      if (first) r.drop(static_cast<uint32_t>(start_bit & 7u));
      block_start = r.bit_pos();
      uint32_t bfinal = 0, btype = 0, st = kOk, n = 0;
      uint64_t p = 0;
      if (!(first && at_len)) {
        bfinal = r.take(1), btype = r.take(2);
        if (Cut::kSearch && !first && !bfinal) {
          const uint64_t c = btype == 0 ? make_cand((r.bit_pos() + 7) / 8 * 8, true)
                                        : make_cand(block_start, false);
          if (cut.hit(c)) st = kCutHere, p = c;
        }
      }
      if (st) {  // the span ends before this block
      } else if (btype == 0) {
        r.drop(r.cnt & 7u);
        r.fill(cx);
        n = r.take(16);
        uint32_t nn = r.take(16);
        p = r.bit_pos() / 8;
        if (r.past() || n != (~nn & 0xFFFFu) || p + n > limit) st = kCorrupt;
        else r.init(p + n, limit);
      } else if (btype == 1) {
        fixed_lengths(w.t.len);
      } else if (btype == 2) {
        ls.nll = 257 + r.take(5), ls.nd = 1 + r.take(5);
        uint32_t ncl = 4 + r.take(4);
        for (uint32_t i = 0; i < deflate::kNumCL; i++) w.t.len[i] = 0;
        for (uint32_t i = 0; i < ncl; i++) {
          r.fill(cx);
          w.t.len[deflate::kCLOrder[i]] = static_cast<uint8_t>(r.take(3));
        }
        if (r.past() || ls.nll > deflate::kNumLL || ls.nd > deflate::kNumD ||
            !count_lengths(w.t.len, deflate::kNumCL, w.t.count_d, kCodeLengths))
          st = kCorrupt;
      } else {
        st = kCorrupt;
      }
      w.ctl[0] = st, w.ctl[1] = btype, w.ctl[2] = bfinal, w.ctl[3] = n;
      w.ctl[4] = static_cast<uint32_t>(p), w.ctl[5] = static_cast<uint32_t>(p >> 32);
      w.ctl[6] = static_cast<uint32_t>(r.pos), w.ctl[7] = static_cast<uint32_t>(r.pos >> 32);
    }
    cx.sync();
    status = w.ctl[0];
    const uint32_t btype = w.ctl[1], bfinal = w.ctl[2];
    if (status == kCutHere) {
      end = w.ctl[4] | static_cast<uint64_t>(w.ctl[5]) << 32;
      status = kOk, cut_here = true;
      break;
    }
    if (status) break;
    first = false;
    at = w.ctl[6] | static_cast<uint64_t>(w.ctl[7]) << 32;
    if (btype == 0) {
      const uint32_t n = w.ctl[3];
      const uint64_t p = w.ctl[4] | static_cast<uint64_t>(w.ctl[5]) << 32;
      cx.sync();  // ctl is read before thread 0 writes it again
      if (n) {
        status = sink.stored(cx, p, n, out);
        if (status) break;
        out += n;
      }
      if ((!Cut::kSearch && !n) || bfinal) {
        end = p + n;
        if (bfinal) status = kFinal;
        break;
      }
      continue;
    }
    if (btype == 2) {
      fill_table(cx, w.t.len, deflate::kNumCL, w.t.count_d, w.t.sorted_d, w.t.d, kCLBits);
      uint32_t rc = 0;
      while (!rc) {
        if (cx.tid == 0) {
          rc = read_lengths(cx, r, w.t, ls, safe);
          w.ctl[0] = rc;
          w.ctl[6] = static_cast<uint32_t>(r.pos), w.ctl[7] = static_cast<uint32_t>(r.pos >> 32);
        }
        cx.sync();
        rc = w.ctl[0];
        at = w.ctl[6] | static_cast<uint64_t>(w.ctl[7]) << 32;
        cx.sync();
        if (!rc) safe = cx.refill(at);
      }
      if (rc == 2) {
        status = kCorrupt;
        break;
      }
    }
    if (cx.tid == 0) {
      bool ok = w.t.len[256] != 0 && count_lengths(w.t.len, ls.nll, w.t.count_ll, kCodeLL) &&
                count_lengths(w.t.len + ls.nll, ls.nd, w.t.count_d, kCodeD);
      w.ctl[0] = ok ? kOk : kCorrupt;
      w.ctl[1] = ls.nll, w.ctl[2] = ls.nd;
    }
    cx.sync();
    status = w.ctl[0];
    const uint32_t nll = w.ctl[1], nd = w.ctl[2];
    cx.sync();
    if (status) break;
    fill_table(cx, w.t.len, nll, w.t.count_ll, w.t.sorted_ll, w.t.ll, kLLBits);
    fill_table(cx, w.t.len + nll, nd, w.t.count_d, w.t.sorted_d, w.t.d, kDBits);
    for (;;) {  // batches of tokens
      safe = cx.refill(at);
      if (cx.tid == 0) {
        uint32_t n = 0, flag = kOk;
        while (n < kBatch && r.pos + 8 <= safe) {
          r.fill(cx);
          uint32_t tok = decode_token(r, w.t);
          if (coded + (r.bit_pos() - block_start) > 8ull * kSpanMaxCoded) flag = kTooLong;
          else if (r.past() || tok == kTokBad) flag = kCorrupt;
          else if (tok == kTokEnd) flag = kTokEnd;
          if (flag) break;
          w.tok[n++] = tok;
        }
        w.ctl[0] = flag, w.ctl[1] = n;
        w.ctl[6] = static_cast<uint32_t>(r.pos), w.ctl[7] = static_cast<uint32_t>(r.pos >> 32);
      }
      cx.sync();
      const uint32_t flag = w.ctl[0], n = w.ctl[1];
      at = w.ctl[6] | static_cast<uint64_t>(w.ctl[7]) << 32;
      status = sink.tokens(cx, w.tok, n, &out);  // ends with a sync: tok and ctl are free
      if (!status && flag != kTokEnd) status = flag;
      if (status || flag == kTokEnd) break;
    }
    if (status) break;
    if (cx.tid == 0) {
      coded += r.bit_pos() - block_start;
      uint64_t e = (r.bit_pos() + 7) / 8;
      w.ctl[4] = static_cast<uint32_t>(e), w.ctl[5] = static_cast<uint32_t>(e >> 32);
    }
    cx.sync();
    const uint64_t e = w.ctl[4] | static_cast<uint64_t>(w.ctl[5]) << 32;
    cx.sync();
    if (bfinal) {
      end = e;
      status = e > limit ? kCorrupt : kFinal;
      break;
    }
  }
  if (status & kStatusMask) return SpanRec{0, 0, status};
  if (cut_here)  // `end` is the candidate the next span starts at
    return SpanRec{out, static_cast<uint32_t>(end >> 4),
                   static_cast<uint32_t>(end & 15u) << kEndShift};
  return SpanRec{out, static_cast<uint32_t>(end), status};
}

template <class Ctx, class Sink>
MX_HD inline SpanRec decode_span(Ctx& cx, Work& w, Sink& sink, uint64_t start, uint64_t limit) {
  MarkerCut cut;
  return decode_span(cx, w, sink, make_cand(start * 8, false), limit, cut);
}

// ---- chain ------------------------------------------------------------------

struct ChainResult {
  uint32_t status;
  uint32_t spans;
  uint64_t out_bytes;
};

// Follows the chain from `first`: span_at(pos) gives the record of the span
// that starts at the candidate pos, or nullptr if there is none; on_span(pos,
// rec, out_offset) sees every ok span of the chain in order.
template <class SpanAt, class OnSpan, class EndOf>
inline ChainResult walk_chain(uint64_t first, uint64_t limit, uint32_t isize, SpanAt span_at,
                              OnSpan on_span, EndOf end_of) {
  ChainResult cr{kOk, 0, 0};
  for (uint64_t pos = first;;) {
    const SpanRec* rec = span_at(pos);
    uint32_t st = rec ? rec->status & kStatusMask : kCorrupt;
    if (!st && end_of(*rec) <= pos) st = kCorrupt;  // a span consumes at least one block
    if (st) return ChainResult{st, 0, 0};
    on_span(pos, *rec, cr.out_bytes);
    cr.spans++;
    cr.out_bytes += rec->out_bytes;
    if (rec->status & kFinal) {
      if (rec->end != limit) return ChainResult{kTrailing, 0, 0};
      break;
    }
    pos = end_of(*rec);
  }
  if (static_cast<uint32_t>(cr.out_bytes) != isize) return ChainResult{kCorrupt, 0, 0};
  return cr;
}

// The chain over byte positions (markers); with search_end as EndOf the same
// walk runs over the candidates of a search.
template <class SpanAt, class OnSpan>
inline ChainResult walk_chain(uint64_t first, uint64_t limit, uint32_t isize, SpanAt span_at,
                              OnSpan on_span) {
  return walk_chain(first, limit, isize, span_at, on_span,
                    [](const SpanRec& rec) -> uint64_t { return rec.end; });
}

// Header length, stream limit and trailer of a member of `size` bytes whose
// first min(size, kHeaderMax) bytes are at head and last 8 at tail.
struct Member {
  uint32_t status, first;
  uint64_t limit;
  uint32_t crc, isize;
};
inline Member parse_member(const uint8_t* head, const uint8_t* tail, uint64_t size) {
  Member m{kOk, 0, 0, 0, 0};
  if (size >= (1ull << 32)) return m.status = kTooLarge, m;
  m.first = parse_header(head, size);
  if (!m.first || size < m.first + deflate::kGzipTrailerBytes) return m.status = kHeader, m;
  m.limit = size - deflate::kGzipTrailerBytes;
  m.crc = deflate::load32(tail, 0);
  m.isize = deflate::load32(tail, 4);
  return m;
}

// ---- host model -------------------------------------------------------------

struct HostCtx {
  static constexpr uint32_t tid = 0, width = 1;
  const uint8_t* data;
  void sync() const {}
  uint8_t byte(uint64_t pos) const { return data[pos]; }
  uint64_t refill(uint64_t) const { return ~0ull; }
};

struct HostSink {
  std::vector<uint8_t>& out;
  size_t base;  // the span's first byte in `out`
  uint32_t stored(const HostCtx& cx, uint64_t at, uint32_t n, uint64_t) {
    out.insert(out.end(), cx.data + at, cx.data + at + n);
    return kOk;
  }
  uint32_t tokens(const HostCtx&, const uint32_t* tok, uint32_t n, uint64_t* produced) {
    for (uint32_t i = 0; i < n; i++) {
      if (!(tok[i] & deflate::kTokMatch)) {
        out.push_back(static_cast<uint8_t>(tok[i]));
        continue;
      }
      uint32_t len = ((tok[i] >> 16) & 0xFFu) + 3, dist = (tok[i] & 0x7FFFu) + 1;
      if (dist > out.size() - base) return kDependent;
      for (uint32_t k = 0; k < len; k++) out.push_back(out[out.size() - dist]);
    }
    *produced = out.size() - base;
    return kOk;
  }
};

struct InflateResult {
  uint32_t status, spans;
  std::vector<uint8_t> bytes;
};

inline InflateResult gzip_inflate_spans(const uint8_t* data, uint64_t size) {
  InflateResult res{kOk, 0, {}};
  Member m = parse_member(data, size >= 8 ? data + size - 8 : data, size);
  if (m.status) return res.status = m.status, res;
  Work w;
  SpanRec rec;
  ChainResult cr = walk_chain(
      m.first, m.limit, m.isize,
      [&](uint64_t pos) {
        HostCtx cx{data};
        HostSink sink{res.bytes, res.bytes.size()};
        rec = decode_span(cx, w, sink, pos, m.limit);
        return &rec;
      },
      [](uint64_t, const SpanRec&, uint64_t) {});
  res.status = cr.status, res.spans = cr.spans;
  if (!res.status &&
      (deflate::crc32::update(deflate::crc32::kInit, res.bytes.data(), res.bytes.size()) ^
       deflate::crc32::kInit) != m.crc)
    res.status = kCorrupt;
  if (res.status) res.spans = 0, res.bytes.clear();
  return res;
}

// ---- search -----------------------------------------------------------------
//
// A stream without markers (stock gzip, Z_SYNC_FLUSH) is cut at a fixed stride
// after its first byte: boundary k is first + k * stride, k >= 1, and stride k
// runs from it to the next boundary or the stream end. In every stride the
// first position of each kind that can start a block becomes a candidate:
//   dynamic  a bit position with BFINAL=0, BTYPE=2, HLIT and HDIST <= 29, an
//            exactly complete code length code (dynamic_plausible: 17 header
//            bits and the Kraft sum of up to 19 three-bit lengths, one
//            position per thread), and then lengths that read without a bad
//            repeat or an overrun, an end-of-block code and two codes that
//            count_lengths accepts (dynamic_confirm, by the group, with the
//            functions decode_span itself uses)
//   stored   a byte p with LEN == ~NLEN at p, the top three bits of byte p-1
//            zero, and one hop: byte p+4+LEN is inside the stream, holds a
//            block type other than 3, and if that block is stored too its
//            LEN and NLEN agree
// Fixed blocks are not searched for; the span that reaches one decodes it.
// The sorted list starts with the stream's first bit and holds at most two
// candidates per stride.
//
// A span of a search decodes into a ring of kWindow uint16 entries instead of
// nowhere: entry k starts as kUnknown | k, "byte k of the window before my
// first byte" (k = kWindow - distance), literals and stored bytes are plain
// values, a match copies entries, so what a span takes from before its start
// stays symbolic and nothing is `dependent`. Byte o of the span lies at
// ring[o % kWindow]. In the span at the stream start a distance beyond its own
// output is corrupt. ListCut ends a span at the first candidate its own chain
// of blocks reaches; a candidate it passes is not on the chain (a false
// candidate never is: a key that a block of the chain starts at with the
// candidate's kind is a block start).
//
// Resolve, in chain order: R[0] is empty, and with T[j][k] = ring j's entry
// (out_bytes j + k) % kWindow, the window behind span j,
//   R[j+1][k] = T[j][k] plain ? T[j][k] : R[j][T[j][k] & 0x7FFF].
// The emitting pass decodes span j again with EndCut and reads a match that
// reaches d bytes before its first output byte from R[j][kWindow - d]. The
// CRC-32 and ISIZE decide as before.

// The 80 bits from bit position `bit` on: [0] the first 64, [1] the rest.
template <class Ctx>
MX_HD inline void load_bits80(const Ctx& cx, uint64_t bit, uint64_t limit, uint64_t* v) {
  const uint64_t p = bit >> 3;
  const uint32_t s = static_cast<uint32_t>(bit & 7u);
  uint64_t lo = 0, hi = 0;
  for (uint32_t i = 0; i < 8; i++)
    if (p + i < limit) lo |= static_cast<uint64_t>(cx.byte(p + i)) << (8 * i);
  for (uint32_t i = 0; i < 3; i++)
    if (p + 8 + i < limit) hi |= static_cast<uint64_t>(cx.byte(p + 8 + i)) << (8 * i);
  v[0] = s ? lo >> s | hi << (64 - s) : lo;
  v[1] = hi >> s;
}

// The cheap part of the dynamic test. One thread, registers only.
template <class Ctx>
MX_HD inline bool dynamic_plausible(const Ctx& cx, uint64_t bit, uint64_t limit) {
  uint64_t v[2];
  load_bits80(cx, bit, limit, v);
  if ((v[0] & 7u) != 4u) return false;  // BFINAL=0, BTYPE=2
  if (((v[0] >> 3) & 31u) > 29u || ((v[0] >> 8) & 31u) > 29u) return false;
  const uint32_t ncl = 4 + static_cast<uint32_t>((v[0] >> 13) & 15u);
  if (bit + 17 + 3 * ncl > limit * 8) return false;
  uint64_t lens = v[0] >> 17 | v[1] << 47;  // 57 bits of lengths at most
  uint32_t kraft = 0;
  for (uint32_t i = 0; i < ncl; i++, lens >>= 3)
    if (lens & 7u) kraft += 128u >> (lens & 7u);
  return kraft == 128u;
}

// The whole dynamic test at a plausible position, by the group. cx.byte must
// serve the 576 bytes from the position's byte on (the longest header is 4498
// bits, and the reader loads 8 bytes ahead).
template <class Ctx>
MX_HD inline bool dynamic_confirm(Ctx& cx, Work& w, uint64_t bit, uint64_t limit) {
  BitReader r;  // thread 0's
  LenState ls{0, 0, 0};
  r.init(bit >> 3, limit);
  if (cx.tid == 0) {
    r.fill(cx);
    r.drop(static_cast<uint32_t>(bit & 7u) + 3);
    ls.nll = 257 + r.take(5), ls.nd = 1 + r.take(5);
    const uint32_t ncl = 4 + r.take(4);
    for (uint32_t i = 0; i < deflate::kNumCL; i++) w.t.len[i] = 0;
    for (uint32_t i = 0; i < ncl; i++) {
      r.fill(cx);
      w.t.len[deflate::kCLOrder[i]] = static_cast<uint8_t>(r.take(3));
    }
    w.ctl[0] = !r.past() && ls.nll <= deflate::kNumLL && ls.nd <= deflate::kNumD &&
               count_lengths(w.t.len, deflate::kNumCL, w.t.count_d, kCodeLengths);
  }
  cx.sync();
  bool ok = w.ctl[0] != 0;
  cx.sync();
  if (!ok) return false;
  fill_table(cx, w.t.len, deflate::kNumCL, w.t.count_d, w.t.sorted_d, w.t.d, kCLBits);
  if (cx.tid == 0)
    w.ctl[0] = read_lengths(cx, r, w.t, ls, ~0ull) == 1 && w.t.len[256] != 0 &&
               count_lengths(w.t.len, ls.nll, w.t.count_ll, kCodeLL) &&
               count_lengths(w.t.len + ls.nll, ls.nd, w.t.count_d, kCodeD);
  cx.sync();
  ok = w.ctl[0] != 0;
  cx.sync();
  return ok;
}

// LEN == ~NLEN at p and the byte before: `near` serves bytes p-1 .. p+3.
template <class Near>
MX_HD inline bool stored_plausible(const Near& near, uint64_t p, uint64_t limit) {
  if (p == 0 || p + 4 > limit) return false;
  const uint32_t len = near.byte(p) | static_cast<uint32_t>(near.byte(p + 1)) << 8;
  const uint32_t nlen = near.byte(p + 2) | static_cast<uint32_t>(near.byte(p + 3)) << 8;
  return len == (~nlen & 0xFFFFu) && !(near.byte(p - 1) & 0xE0u);
}
// The hop: `far` serves any byte below limit.
template <class Far>
MX_HD inline bool stored_confirm(const Far& far, uint64_t p, uint64_t limit) {
  const uint64_t q = p + 4 + (far.byte(p) | static_cast<uint32_t>(far.byte(p + 1)) << 8);
  if (q >= limit) return false;
  const uint32_t btype = (far.byte(q) >> 1) & 3u;
  if (btype == 3) return false;
  if (btype != 0) return true;
  if (q + 5 > limit) return false;
  const uint32_t len = far.byte(q + 1) | static_cast<uint32_t>(far.byte(q + 2)) << 8;
  const uint32_t nlen = far.byte(q + 3) | static_cast<uint32_t>(far.byte(q + 4)) << 8;
  return len == (~nlen & 0xFFFFu);
}

MX_HD inline uint64_t search_strides(uint64_t first, uint64_t limit, uint64_t stride) {
  return limit > first ? (limit - first - 1) / stride : 0;
}

// Ring entry k of the window behind a span of `out` bytes, resolved against
// the window `prev` behind the span before it.
MX_HD inline uint8_t resolve_entry(const uint16_t* ring, uint64_t out, uint32_t k,
                                   const uint8_t* prev) {
  const uint32_t e = ring[(out + k) & (kWindow - 1)];
  return static_cast<uint8_t>(e & kUnknown ? prev[e & (kWindow - 1)] : e);
}

// The sorted candidates of the stream [first, limit) of data. Group of one.
inline std::vector<uint64_t> search_candidates(const uint8_t* data, uint64_t first, uint64_t limit,
                                               uint64_t stride) {
  std::vector<uint64_t> cand{make_cand(first * 8, false)};
  HostCtx cx{data};
  Work w;
  for (uint64_t k = 1, n = search_strides(first, limit, stride); k <= n; k++) {
    const uint64_t from = first + k * stride, to = from + stride < limit ? from + stride : limit;
    uint64_t dyn = kNoCand, sto = kNoCand;
    for (uint64_t bit = from * 8; bit < to * 8 && dyn == kNoCand; bit++)
      if (dynamic_plausible(cx, bit, limit) && dynamic_confirm(cx, w, bit, limit))
        dyn = make_cand(bit, false);
    for (uint64_t p = from; p < to && sto == kNoCand; p++)
      if (stored_plausible(cx, p, limit) && stored_confirm(cx, p, limit)) sto = make_cand(p * 8, true);
    if (dyn > sto) std::swap(dyn, sto);
    if (dyn != kNoCand) cand.push_back(dyn);
    if (sto != kNoCand) cand.push_back(sto);
  }
  return cand;
}

// What end_of of walk_chain takes from a record of a search.
inline uint64_t search_end(const SpanRec& rec) {
  return rec.status & kFinal ? make_cand(static_cast<uint64_t>(rec.end) * 8, false) : end_cand(rec);
}

// Measuring sink of a search: the symbolic ring.
struct HostRingSink {
  uint16_t* ring;
  bool at_stream_start;
  uint32_t stored(const HostCtx& cx, uint64_t at, uint32_t n, uint64_t out) {
    for (uint32_t k = 0; k < n; k++) ring[(out + k) & (kWindow - 1)] = cx.data[at + k];
    return kOk;
  }
  uint32_t tokens(const HostCtx&, const uint32_t* tok, uint32_t n, uint64_t* produced) {
    uint64_t o = *produced;
    for (uint32_t i = 0; i < n; i++) {
      if (!(tok[i] & deflate::kTokMatch)) {
        ring[o++ & (kWindow - 1)] = static_cast<uint8_t>(tok[i]);
        continue;
      }
      uint32_t len = ((tok[i] >> 16) & 0xFFu) + 3, dist = (tok[i] & 0x7FFFu) + 1;
      if (at_stream_start && dist > o) return kCorrupt;
      for (uint32_t k = 0; k < len; k++, o++) ring[o & (kWindow - 1)] = ring[(o - dist) & (kWindow - 1)];
    }
    *produced = o;
    return kOk;
  }
};

// Emitting sink of a search: matches that reach before the span read `win`.
struct HostWindowSink {
  std::vector<uint8_t>& out;
  size_t base;
  const uint8_t* win;  // nullptr at the stream start
  uint32_t stored(const HostCtx& cx, uint64_t at, uint32_t n, uint64_t) {
    out.insert(out.end(), cx.data + at, cx.data + at + n);
    return kOk;
  }
  uint32_t tokens(const HostCtx&, const uint32_t* tok, uint32_t n, uint64_t* produced) {
    for (uint32_t i = 0; i < n; i++) {
      if (!(tok[i] & deflate::kTokMatch)) {
        out.push_back(static_cast<uint8_t>(tok[i]));
        continue;
      }
      uint32_t len = ((tok[i] >> 16) & 0xFFu) + 3, dist = (tok[i] & 0x7FFFu) + 1;
      if (!win && dist > out.size() - base) return kCorrupt;
      for (uint32_t k = 0; k < len; k++) {
        const size_t have = out.size() - base;
        out.push_back(dist > have ? win[kWindow - (dist - have)] : out[out.size() - dist]);
      }
    }
    *produced = out.size() - base;
    return kOk;
  }
};

// The host model of a search: candidates, one symbolic ring per span of the
// chain, the chain walk, then resolve and emit span by span.
inline InflateResult gzip_inflate_search(const uint8_t* data, uint64_t size, uint64_t stride) {
  InflateResult res{kOk, 0, {}};
  Member m = parse_member(data, size >= 8 ? data + size - 8 : data, size);
  if (m.status) return res.status = m.status, res;
  const std::vector<uint64_t> cand = search_candidates(data, m.first, m.limit, stride);
  struct Link {
    uint64_t start, out_bytes;
    std::vector<uint16_t> ring;
  };
  std::vector<Link> chain;
  Work w;
  SpanRec rec;
  HostCtx cx{data};
  std::vector<uint16_t> ring(kWindow);
  ChainResult cr = walk_chain(
      cand[0], m.limit, m.isize,
      [&](uint64_t pos) -> const SpanRec* {
        auto it = std::lower_bound(cand.begin(), cand.end(), pos);
        if (it == cand.end() || *it != pos) return nullptr;
        for (uint32_t k = 0; k < kWindow; k++) ring[k] = static_cast<uint16_t>(kUnknown | k);
        HostRingSink sink{ring.data(), pos == cand[0]};
        ListCut cut{cand.data(), static_cast<uint32_t>(cand.size()),
                    static_cast<uint32_t>(it - cand.begin()) + 1};
        rec = decode_span(cx, w, sink, pos, m.limit, cut);
        return &rec;
      },
      [&](uint64_t pos, const SpanRec& r, uint64_t) { chain.push_back({pos, r.out_bytes, ring}); },
      search_end);
  res.status = cr.status, res.spans = cr.spans;
  std::vector<uint8_t> win(kWindow, 0), next(kWindow);
  for (size_t j = 0; j < chain.size() && !res.status; j++) {
    HostWindowSink sink{res.bytes, res.bytes.size(), j ? win.data() : nullptr};
    EndCut cut{j + 1 < chain.size() ? chain[j + 1].start : kNoCand};
    rec = decode_span(cx, w, sink, chain[j].start, m.limit, cut);
    if ((rec.status & kStatusMask) || rec.out_bytes != chain[j].out_bytes) res.status = kCorrupt;
    for (uint32_t k = 0; k < kWindow; k++)
      next[k] = resolve_entry(chain[j].ring.data(), chain[j].out_bytes, k, win.data());
    win.swap(next);
  }
  if (!res.status &&
      (deflate::crc32::update(deflate::crc32::kInit, res.bytes.data(), res.bytes.size()) ^
       deflate::crc32::kInit) != m.crc)
    res.status = kCorrupt;
  if (res.status) res.spans = 0, res.bytes.clear();
  return res;
}

}  // namespace inflate
}  // namespace modelx
