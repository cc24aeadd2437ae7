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
#pragma once

#include <cstdint>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace modelx {
namespace tarhost {

constexpr uint64_t kBlock = 512;
constexpr size_t kNameLen = 100;
constexpr size_t kPrefixLen = 155;
// 11 octal digits: the largest size the ustar field (and the index
// kernel's parse_octal) can carry is 8 GiB - 1
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

}  // namespace tarhost
}  // namespace modelx
