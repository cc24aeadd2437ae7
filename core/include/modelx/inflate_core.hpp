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
// Group. decode_span is called by every thread of a group with the same
// arguments, like deflate::build_lengths. Thread 0 owns the bit reader and
// decodes; what the others need it leaves in Work::ctl. The group fills the
// decode tables side by side: one code length per thread for the sorted
// symbol list, then one table entry per thread per trip, each entry found by
// the canonical first-code walk over the per-length counts, the same walk
// that serves codes longer than the primary lookup. Tokens are those of
// deflate_core.hpp; the sink takes them a batch at a time.
#pragma once

#include <cstddef>
#include <cstdint>
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

// One span of the chain, as the emitting kernel takes it.
struct PlanSpan {
  uint64_t out_offset;
  uint64_t out_bytes;
  uint32_t in_start;
  uint32_t pad_;
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
template <class Ctx, class Sink>
MX_HD inline SpanRec decode_span(Ctx& cx, Work& w, Sink& sink, uint64_t start, uint64_t limit) {
  BitReader r;  // thread 0's
  r.init(start, limit);
  uint64_t out = 0, coded = 0, at = start, end = 0;
  uint32_t status = kOk;
  for (;;) {
    uint64_t safe = cx.refill(at);
    LenState ls{kMaxLL, kMaxD, 0};
    uint64_t block_start = 0;
    if (cx.tid == 0) {
      r.fill(cx);
      block_start = r.bit_pos();
      uint32_t bfinal = r.take(1), btype = r.take(2), st = kOk, n = 0;
      uint64_t p = 0;
      if (btype == 0) {
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
    if (status) break;
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
      if (!n || bfinal) {
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
  return SpanRec{out, static_cast<uint32_t>(end), status};
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
template <class SpanAt, class OnSpan>
inline ChainResult walk_chain(uint64_t first, uint64_t limit, uint32_t isize, SpanAt span_at,
                              OnSpan on_span) {
  ChainResult cr{kOk, 0, 0};
  for (uint64_t pos = first;;) {
    const SpanRec* rec = span_at(pos);
    uint32_t st = rec ? rec->status & kStatusMask : kCorrupt;
    if (!st && rec->end <= pos) st = kCorrupt;  // a span consumes at least one block
    if (st) return ChainResult{st, 0, 0};
    on_span(pos, *rec, cr.out_bytes);
    cr.spans++;
    cr.out_bytes += rec->out_bytes;
    if (rec->status & kFinal) {
      if (rec->end != limit) return ChainResult{kTrailing, 0, 0};
      break;
    }
    pos = rec->end;
  }
  if (static_cast<uint32_t>(cr.out_bytes) != isize) return ChainResult{kCorrupt, 0, 0};
  return cr;
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

}  // namespace inflate
}  // namespace modelx
