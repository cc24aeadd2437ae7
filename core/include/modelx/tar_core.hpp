// The tar header walk, compiled for host and device alike: the numeric-field
// parse, the header checksum, and the single step "given the header at `off`,
// produce the entry and the next `off`, or an error code". tar_index_kernel
// (core/hip/tar.hip) and the host model (tar_host.hpp, _core.tar_index_host)
// run this same code, so the GPU index can be compared with a host run of the
// same rules and the rules themselves run under host sanitizers.
//
// Python's tarfile is the reference reader. Where it is laxer (it quietly ends
// a listing at a bad header past offset 0) the walk reports an error instead:
// the bytes come from a registry, and a listing that silently stops short is
// worse than a refused pull.
//
// No read goes past tar_len: a header is read only when all 512 bytes of it
// lie inside the archive, and a payload is never read here at all.
#pragma once

#include <cstdint>

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
namespace tarcore {

constexpr uint64_t kBlock = 512;

struct Entry {
  uint64_t header_off;   // offset of the 512 B header block
  uint64_t payload_off;  // offset of file data
  uint64_t size;         // bytes stored after the header (0 for links, dirs, devices)
  uint32_t typeflag;     // '0'/'\0'/'7' regular, '5' dir, 'L' GNU longname, ...
  uint32_t mode;         // decoded
};

// What a walk leaves behind, host or device.
struct WalkResult {
  uint32_t count;      // entries written
  uint32_t error;      // kOk, or the first error met
  uint64_t error_off;  // header offset the error belongs to
};

enum Status : uint32_t {
  kOk = 0,
  kEnd = 1,              // zero block, or fewer than 512 bytes left: not an error
  kErrTooManyEntries = 2,
  kErrChecksum = 3,      // non-zero block whose checksum field matches neither sum
  kErrSizeField = 4,     // neither octal nor base-256
  kErrSizeNegative = 5,  // base-256 with the sign bit set
  kErrSizeTooLarge = 6,  // base-256 value that does not fit 63 bits
  kErrModeField = 7,
  kErrPayloadPastEnd = 8,  // payload plus padding extends past tar_len
  // found by the name resolution on the host (tar_host.hpp)
  kErrPaxRecord = 9,   // PAX record with a malformed length
  kErrPaxSize = 10,    // PAX size= record: overrides the size the walk used
  kErrPaxSparse = 11,  // GNU.sparse.* records: member data is a sparse map
};

inline const char* status_text(uint32_t s) {
  switch (s) {
    case kOk: return "ok";
    case kEnd: return "end of archive";
    case kErrTooManyEntries: return "too many entries";
    case kErrChecksum: return "bad header checksum";
    case kErrSizeField: return "size field is neither octal nor base-256";
    case kErrSizeNegative: return "negative base-256 size";
    case kErrSizeTooLarge: return "base-256 size does not fit 63 bits";
    case kErrModeField: return "bad mode field";
    case kErrPayloadPastEnd: return "entry extends past the end of the archive";
    case kErrPaxRecord: return "malformed PAX record";
    case kErrPaxSize: return "PAX size= record is not supported";
    case kErrPaxSparse: return "GNU sparse member is not supported";
    default: return "unknown error";
  }
}

MX_HD inline bool is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// A numeric header field of n bytes, read as tarfile's nti() reads it.
// Octal: the bytes before the first NUL, surrounding white space dropped,
// then octal digits only (none at all is 0). Base-256 (GNU, legal for any
// value, used from 8 GiB up): first byte 0x80..0xBF, the remaining bits
// big-endian; 0xC0..0xFF is a negative number. Returns kOk or one of the three
// size errors; *out is below 2^63 on kOk.
MX_HD inline uint32_t parse_numeric(const uint8_t* p, int n, uint64_t* out) {
  *out = 0;
  if (p[0] & 0x80u) {
    if (p[0] & 0x40u) return kErrSizeNegative;
    uint64_t v = p[0] & 0x3fu;
    for (int i = 1; i < n; i++) {
      if (v >> 55) return kErrSizeTooLarge;
      v = (v << 8) | p[i];
    }
    *out = v;  // v < 2^55 before every shift, so v < 2^63 here
    return kOk;
  }
  int end = 0;
  while (end < n && p[end] != 0) end++;
  int beg = 0;
  while (beg < end && is_space(p[beg])) beg++;
  while (end > beg && is_space(p[end - 1])) end--;
  uint64_t v = 0;
  for (int i = beg; i < end; i++) {  // at most 12 digits: 36 bits
    if (p[i] < '0' || p[i] > '7') return kErrSizeField;
    v = (v << 3) | static_cast<uint64_t>(p[i] - '0');
  }
  *out = v;
  return kOk;
}

MX_HD inline uint32_t load_le32(const uint8_t* p, bool aligned) {
  if (aligned) {  // one dword load; archives in HBM start 16 B aligned
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    return v;
  }
  return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 |
         static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
}

MX_HD inline uint32_t popcount32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<uint32_t>(__popc(v));
#else
  return static_cast<uint32_t>(__builtin_popcount(v));
#endif
}

// Both checksums of one header block, the 8 checksum bytes counted as
// spaces: the sum of unsigned bytes (POSIX) and of signed bytes (old Sun
// tars; they differ once a byte is >= 0x80). Returns false for an all-zero
// block. One pass of 128 words, unrolled so that the one device thread that
// walks has all of a header's loads in flight at once instead of paying a
// memory round trip per trip of the loop.
MX_HD inline bool header_sums(const uint8_t* hdr, uint32_t* usum, int32_t* ssum) {
  bool aligned = (reinterpret_cast<uintptr_t>(hdr) & 3u) == 0;
  uint32_t any = 0, sum = 0, high = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int w = 0; w < 128; w++) {
    uint32_t v = load_le32(hdr + 4 * w, aligned);
    any |= v;
    if (w == 37 || w == 38) v = 0x20202020u;  // bytes 148..155
    sum += (v & 0x00ff00ffu) + ((v >> 8) & 0x00ff00ffu);
    high += popcount32(v & 0x80808080u);
  }
  sum = (sum & 0xffffu) + (sum >> 16);
  *usum = sum;
  *ssum = static_cast<int32_t>(sum) - 256 * static_cast<int32_t>(high);
  return any != 0;
}

MX_HD inline uint64_t pad_block(uint64_t n) { return (n + kBlock - 1) & ~(kBlock - 1); }

// One step of the walk. kOk: *e is the entry whose header is at `off` and
// *next the offset of the header after it, with every byte in between inside
// the archive. kEnd: the listing ends here. Anything else: the archive is
// refused, and neither *e nor *next means anything.
MX_HD inline uint32_t walk_step(const uint8_t* tar, uint64_t tar_len, uint64_t off, Entry* e,
                                uint64_t* next) {
  if (off > tar_len || tar_len - off < kBlock) return kEnd;
  const uint8_t* hdr = tar + off;
  uint32_t usum;
  int32_t ssum;
  if (!header_sums(hdr, &usum, &ssum)) return kEnd;
  uint64_t chk, size, mode;
  if (parse_numeric(hdr + 148, 8, &chk) != kOk) return kErrChecksum;
  if (chk != usum && !(ssum >= 0 && chk == static_cast<uint64_t>(ssum))) return kErrChecksum;
  uint32_t rc = parse_numeric(hdr + 124, 12, &size);
  if (rc != kOk) return rc;
  if (parse_numeric(hdr + 100, 8, &mode) != kOk || mode > 0xffffffffull) return kErrModeField;
  uint32_t typeflag = hdr[156];
  // links, devices, directories and fifos store nothing, whatever the size
  // field says (tarfile and libarchive agree)
  if (typeflag >= '1' && typeflag <= '6') size = 0;
  uint64_t padded = pad_block(size);  // size < 2^63: no wrap
  if (padded > tar_len - off - kBlock) return kErrPayloadPastEnd;
  *e = Entry{off, off + kBlock, size, typeflag, static_cast<uint32_t>(mode)};
  *next = off + kBlock + padded;
  return kOk;
}

// The whole walk: the steps from offset 0 until the end or the first error.
// On an error count is what came before it; callers return nothing then.
MX_HD inline void walk(const uint8_t* tar, uint64_t tar_len, Entry* entries,
                       uint32_t max_entries, WalkResult* res) {
  uint64_t off = 0;
  uint32_t n = 0, error = kOk;
  for (;;) {
    Entry e;
    uint64_t next;
    uint32_t rc = walk_step(tar, tar_len, off, &e, &next);
    if (rc == kEnd) break;
    if (rc == kOk && n == max_entries) rc = kErrTooManyEntries;
    if (rc != kOk) {
      error = rc;
      break;
    }
    entries[n++] = e;
    off = next;
  }
  res->count = n;
  res->error = error;
  res->error_off = error ? off : 0;
}

}  // namespace tarcore
}  // namespace modelx
