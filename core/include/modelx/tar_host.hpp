// Host-side tar writer layout: POSIX ustar headers for an ordered member
// list, every header's and payload's offset, and the total archive length.
// Pure C++ (no HIP) so the CPU suite and a sanitizer self-test can run it;
// the GPU pack kernel (core/hip/tar.hip) only moves bytes to the offsets
// computed here.
//
// Headers are deterministic (mode 0644, uid/gid/mtime 0, no user/group
// names): equal members give equal archives, equal digests, and HEAD-dedup
// on push. Names follow the rules GpuEngine::tar_index reads back: name
// field, then the ustar prefix field, then a PAX 'x' header with one path=
// record.
//
// The second half is the read side: what GpuEngine::tar_index does with the
// entry table once the kernel has walked the headers (see "index side").
#pragma once

#include <cstdint>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "modelx/tar_core.hpp"

namespace modelx {
namespace tarhost {

constexpr uint64_t kBlock = 512;
constexpr size_t kNameLen = 100;
constexpr size_t kPrefixLen = 155;
// 11 octal digits: the largest size the pack side writes is 8 GiB - 1. (The
// index side also reads GNU base-256 size fields, tar_core.hpp; the writer
// keeps to the octal field every reader understands.)
constexpr uint64_t kMaxMemberSize = (8ull << 30) - 1;
// Header entries GpuEngine::tar_index reads back from one archive; a member
// with a PAX header costs two. A pack that needs more is rejected.
constexpr uint32_t kMaxIndexEntries = 65536;

struct PackEntry {
  uint64_t header_off;   // first header block of this member (PAX or ustar)
  uint64_t header_len;   // 512, or 1024 + padded PAX payload
  uint64_t payload_off;  // header_off + header_len
  uint64_t size;
};

struct PackLayout {
  std::string headers;             // all header regions, concatenated in member order
  std::vector<PackEntry> entries;  // one per member, in member order
  uint64_t total = 0;              // archive length incl. the two trailing zero blocks
};

inline uint64_t pad512(uint64_t n) { return (n + kBlock - 1) & ~(kBlock - 1); }

inline void validate_name(const std::string& name) {
  if (name.empty()) throw std::invalid_argument("tar member name is empty");
  if (name.find('\0') != std::string::npos)
    throw std::invalid_argument("tar member name contains NUL");
  if (name[0] == '/') throw std::invalid_argument("tar member name is absolute: " + name);
  // components: none empty (so no "a//b" and no trailing '/', which tar
  // readers take for a directory), none "." or ".."
  size_t pos = 0;
  while (pos <= name.size()) {
    size_t slash = name.find('/', pos);
    if (slash == std::string::npos) slash = name.size();
    size_t n = slash - pos;
    if (n == 0) throw std::invalid_argument("tar member name has an empty component: " + name);
    if (name[pos] == '.' && (n == 1 || (n == 2 && name[pos + 1] == '.')))
      throw std::invalid_argument("tar member name has a '.' or '..' component: " + name);
    pos = slash + 1;
  }
}

// Split for the ustar prefix field: the last '/' that leaves a prefix of
// <= 155 bytes; usable when the remainder fits the name field. A later
// slash only shortens the remainder, so this one choice decides it.
inline bool split_prefix(const std::string& name, std::string* prefix, std::string* rest) {
  size_t slash = name.rfind('/', kPrefixLen);
  if (slash == std::string::npos || slash == 0) return false;
  size_t rest_len = name.size() - slash - 1;
  if (rest_len == 0 || rest_len > kNameLen) return false;
  *prefix = name.substr(0, slash);
  *rest = name.substr(slash + 1);
  return true;
}

inline void put_octal(char* field, size_t digits, uint64_t v) {
  for (size_t i = 0; i < digits; i++) {
    field[digits - 1 - i] = static_cast<char>('0' + (v & 7));
    v >>= 3;
  }
  field[digits] = '\0';
}

// One 512 B ustar header block appended to `out`.
inline void append_header(std::string* out, const std::string& name, const std::string& prefix,
                          uint64_t size, char typeflag) {
  char h[kBlock];
  std::memset(h, 0, sizeof h);
  std::memcpy(h, name.data(), name.size() < kNameLen ? name.size() : kNameLen);
  put_octal(h + 100, 7, 0644);  // mode
  put_octal(h + 108, 7, 0);     // uid
  put_octal(h + 116, 7, 0);     // gid
  put_octal(h + 124, 11, size);
  put_octal(h + 136, 11, 0);  // mtime
  std::memset(h + 148, ' ', 8);
  h[156] = typeflag;
  std::memcpy(h + 257, "ustar", 6);  // magic incl. NUL
  h[263] = '0';
  h[264] = '0';
  std::memcpy(h + 345, prefix.data(), prefix.size() < kPrefixLen ? prefix.size() : kPrefixLen);
  uint32_t sum = 0;
  for (size_t i = 0; i < kBlock; i++) sum += static_cast<unsigned char>(h[i]);
  put_octal(h + 148, 6, sum);  // 6 digits, NUL, then the space left in place
  h[155] = ' ';
  out->append(h, sizeof h);
}

// "<len> path=<name>\n" where <len> counts the whole record, itself included.
inline std::string pax_path_record(const std::string& name) {
  size_t body = 1 + 5 + name.size() + 1;  // ' ' "path=" name '\n'
  size_t len = body + 1;
  for (;;) {
    size_t digits = std::to_string(len).size();
    if (body + digits == len) break;
    len = body + digits;
  }
  return std::to_string(len) + " path=" + name + "\n";
}

inline PackLayout pack_layout(const std::vector<std::pair<std::string, uint64_t>>& members) {
  PackLayout lay;
  std::set<std::string> seen;
  for (const auto& m : members) {
    validate_name(m.first);
    if (m.second > kMaxMemberSize)
      throw std::invalid_argument("tar member " + m.first +
                                  " is 8 GiB or larger: does not fit the ustar size field");
    if (!seen.insert(m.first).second)
      throw std::invalid_argument("duplicate tar member name: " + m.first);
  }
  uint64_t off = 0, index_entries = 0;
  lay.entries.reserve(members.size());
  for (const auto& m : members) {
    const std::string& name = m.first;
    size_t before = lay.headers.size();
    std::string prefix, rest;
    if (name.size() <= kNameLen) {
      append_header(&lay.headers, name, "", m.second, '0');
    } else if (split_prefix(name, &prefix, &rest)) {
      append_header(&lay.headers, rest, prefix, m.second, '0');
    } else {
      std::string rec = pax_path_record(name);
      append_header(&lay.headers, "././@PaxHeader", "", rec.size(), 'x');
      lay.headers.append(rec);
      lay.headers.append(pad512(rec.size()) - rec.size(), '\0');
      append_header(&lay.headers, name.substr(0, kNameLen), "", m.second, '0');
    }
    uint64_t header_len = lay.headers.size() - before;
    index_entries += header_len == kBlock ? 1 : 2;
    if (index_entries > kMaxIndexEntries)
      throw std::invalid_argument("too many tar members: the archive would need more than " +
                                  std::to_string(kMaxIndexEntries) + " header entries");
    lay.entries.push_back({off, header_len, off + header_len, m.second});
    off += header_len + pad512(m.second);
  }
  lay.total = off + 2 * kBlock;
  return lay;
}

// ------------------------------------------------------------- index side --
//
// The read side of GpuEngine::tar_index, without the GPU: the entry table's
// check against tar_len, the entry-to-name resolution, and index_host, which
// runs the walk of tar_core.hpp and both of these on host bytes. The engine
// runs the walk in a kernel and copies bytes; everything else is here, so
// the CPU suite and a sanitizer self-test can run it.
//
// The reference reader is Python's tarfile: the result is its regular-file
// members (isfile()), in order, under its naming rules. Unlike tarfile, which
// quietly ends a listing at a bad header past offset 0, every damaged or
// unsupported construct is an IndexError naming the cause and the header's
// offset, and no entry is returned.

struct IndexedFile {
  std::string name;
  uint64_t offset;  // of the payload
  uint64_t size;
  uint32_t mode;
};

class IndexError : public std::runtime_error {
 public:
  IndexError(uint32_t code, uint64_t header_off)
      : std::runtime_error(std::string("tar_index: ") + tarcore::status_text(code) +
                           " at header offset " + std::to_string(header_off)),
        code(code), header_off(header_off) {}
  uint32_t code;
  uint64_t header_off;
};

// The entry table against tar_len, on the host: headers chained from offset
// 0 without gaps, every payload with its padding inside the archive. The
// walk has checked the same; this does not take its word for it, because
// what follows reads and allocates by these numbers.
inline void validate_entries(const std::vector<tarcore::Entry>& entries, uint64_t tar_len) {
  uint64_t expect = 0;
  for (const tarcore::Entry& e : entries) {
    if (e.header_off != expect || e.header_off > tar_len || tar_len - e.header_off < kBlock ||
        e.payload_off != e.header_off + kBlock || e.size >> 63 ||
        pad512(e.size) > tar_len - e.payload_off)
      throw IndexError(tarcore::kErrPayloadPastEnd, e.header_off);
    expect = e.payload_off + pad512(e.size);
  }
}

inline std::string field_string(const char* p, size_t n) { return std::string(p, strnlen(p, n)); }

// The records of one PAX extended header, "<len> key=value\n" each with
// <len> counting the whole record. Every payload byte must belong to a
// well-formed record. Sets *path from the last path= record. size= (it
// overrides the size the walk has already used) and GNU.sparse.* (the member
// data would be a sparse map) are refused, not half-supported.
inline bool parse_pax(const std::string& px, uint64_t header_off, std::string* path) {
  bool has_path = false;
  size_t pos = 0, n = px.size();
  while (pos < n) {
    size_t p = pos;
    uint64_t len = 0;
    while (p < n && px[p] >= '0' && px[p] <= '9' && p - pos < 18) len = len * 10 + (px[p++] - '0');
    if (p == pos || p >= n || px[p] != ' ' || len == 0 || len > n - pos)
      throw IndexError(tarcore::kErrPaxRecord, header_off);
    size_t end = pos + static_cast<size_t>(len), key = p + 1;
    if (end < key + 3 || px[end - 1] != '\n') throw IndexError(tarcore::kErrPaxRecord, header_off);
    size_t eq = px.find('=', key);
    if (eq == std::string::npos || eq == key || eq >= end - 1)
      throw IndexError(tarcore::kErrPaxRecord, header_off);
    std::string keyword = px.substr(key, eq - key);
    if (keyword == "size") throw IndexError(tarcore::kErrPaxSize, header_off);
    if (keyword.compare(0, 11, "GNU.sparse.") == 0)
      throw IndexError(tarcore::kErrPaxSparse, header_off);
    if (keyword == "path") {
      *path = px.substr(eq + 1, end - 1 - (eq + 1));
      while (!path->empty() && path->back() == '/') path->pop_back();
      has_path = true;
    }
    pos = end;
  }
  return has_path;
}

// Entries to named regular files. `headers` holds the entries' header
// blocks back to back (entries.size() * 512 bytes); read_payload(entry)
// returns the entry's `size` payload bytes and is called for 'L', 'x', 'X'
// and 'g' entries only, after validate_entries has passed.
//
// Names, as tarfile resolves them: a GNU 'L' payload or a PAX path= names
// the next entry that is none of 'L', 'K', 'x', 'X', 'g', whatever its type
// (a skipped directory consumes the name); when both precede an entry the
// first one wins; a 'g' path= names every later entry that has neither;
// otherwise the name field, behind the prefix field and a '/' if that is not
// empty. Regular is typeflag '0', NUL or '7', except NUL under a name field
// ending in '/' (a V7 directory).
template <class ReadPayload>
std::vector<IndexedFile> resolve_names(const std::vector<tarcore::Entry>& entries,
                                       const char* headers, ReadPayload&& read_payload,
                                       uint64_t tar_len) {
  validate_entries(entries, tar_len);
  std::vector<IndexedFile> out;
  std::string pending, global_path;
  bool has_pending = false, has_global = false;
  for (size_t i = 0; i < entries.size(); i++) {
    const tarcore::Entry& e = entries[i];
    const char* hdr = headers + i * kBlock;
    uint32_t tf = e.typeflag;
    if (tf == 'L') {
      std::string ln = read_payload(e);
      ln.resize(strnlen(ln.data(), ln.size()));
      if (!has_pending) pending = ln;
      has_pending = true;
      continue;
    }
    if (tf == 'K') continue;  // GNU long link target: names nothing
    if (tf == 'x' || tf == 'X' || tf == 'g') {
      std::string path;
      if (parse_pax(read_payload(e), e.header_off, &path)) {
        if (tf == 'g') {
          global_path = path;
          has_global = true;
        } else if (!has_pending) {
          pending = path;
          has_pending = true;
        }
      }
      continue;
    }
    std::string field = field_string(hdr, kNameLen);
    bool regular = tf == '0' || tf == '7' || (tf == 0 && (field.empty() || field.back() != '/'));
    std::string name;
    if (has_pending) {
      name = pending;
      has_pending = false;
    } else if (has_global) {
      name = global_path;
    } else {
      std::string prefix = field_string(hdr + 345, kPrefixLen);
      name = prefix.empty() ? field : prefix + "/" + field;
    }
    if (regular) out.push_back({name, e.payload_off, e.size, e.mode});
  }
  return out;
}

// tar_index on host bytes: the model the GPU result is compared with.
inline std::vector<IndexedFile> index_host(const uint8_t* data, uint64_t tar_len) {
  std::vector<tarcore::Entry> entries(kMaxIndexEntries);
  tarcore::WalkResult res;
  tarcore::walk(data, tar_len, entries.data(), kMaxIndexEntries, &res);
  if (res.error) throw IndexError(res.error, res.error_off);
  entries.resize(res.count);
  std::string headers(static_cast<size_t>(res.count) * kBlock, '\0');
  for (size_t i = 0; i < entries.size(); i++)
    std::memcpy(&headers[i * kBlock], data + entries[i].header_off, kBlock);
  auto read_payload = [&](const tarcore::Entry& e) {
    return std::string(reinterpret_cast<const char*>(data) + e.payload_off,
                       static_cast<size_t>(e.size));
  };
  return resolve_names(entries, headers.data(), read_payload, tar_len);
}

}  // namespace tarhost
}  // namespace modelx
