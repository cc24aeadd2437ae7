// Stand-alone self-test of the host-side tar layout builder
// (core/include/modelx/tar_host.hpp). Meant to be built with
//   g++ -std=c++17 -fsanitize=address,undefined -Icore/include
// so the header-only code runs its edge names and sizes under ASan/UBSan in a
// process of its own. Exit status 0 and no output on stderr mean success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "modelx/tar_host.hpp"

using modelx::tarhost::pack_layout;
using modelx::tarhost::pad512;
using modelx::tarhost::PackLayout;

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                          \
    }                                                                      \
  } while (0)

uint64_t octal(const char* p, size_t n) {
  uint64_t v = 0;
  for (size_t i = 0; i < n && p[i] >= '0' && p[i] <= '7'; i++) v = (v << 3) | (p[i] - '0');
  return v;
}

// One ustar block: magic, NUL-terminated numeric fields, checksum.
void check_block(const char* h, char typeflag, uint64_t size) {
  CHECK(std::string(h + 257, 6) == std::string("ustar\0", 6));
  CHECK(h[263] == '0' && h[264] == '0');
  CHECK(h[156] == typeflag);
  CHECK(octal(h + 100, 8) == 0644 && h[107] == '\0');
  CHECK(octal(h + 108, 8) == 0 && h[115] == '\0');
  CHECK(octal(h + 116, 8) == 0 && h[123] == '\0');
  CHECK(octal(h + 124, 12) == size && h[135] == '\0');
  CHECK(octal(h + 136, 12) == 0 && h[147] == '\0');
  for (int i = 157; i < 257; i++) CHECK(h[i] == '\0');  // linkname
  for (int i = 265; i < 345; i++) CHECK(h[i] == '\0');  // uname, gname, dev*
  for (int i = 500; i < 512; i++) CHECK(h[i] == '\0');
  uint32_t sum = 0;
  for (int i = 0; i < 512; i++)
    sum += (i >= 148 && i < 156) ? static_cast<unsigned char>(' ')
                                 : static_cast<unsigned char>(h[i]);
  CHECK(octal(h + 148, 6) == sum && h[154] == '\0' && h[155] == ' ');
}

std::string field(const char* p, size_t n) {
  size_t len = 0;
  while (len < n && p[len]) len++;
  return std::string(p, len);
}

void check_layout(const std::vector<std::pair<std::string, uint64_t>>& members) {
  PackLayout lay = pack_layout(members);
  CHECK(lay.entries.size() == members.size());
  uint64_t off = 0, hoff = 0;
  for (size_t i = 0; i < members.size(); i++) {
    const auto& e = lay.entries[i];
    const std::string& name = members[i].first;
    CHECK(e.header_off == off);
    CHECK(e.payload_off == off + e.header_len);
    CHECK(e.size == members[i].second);
    CHECK(e.header_len % 512 == 0);
    CHECK(hoff + e.header_len <= lay.headers.size());
    if (hoff + e.header_len > lay.headers.size()) return;
    const char* h = lay.headers.data() + hoff;
    const char* last = h + e.header_len - 512;
    check_block(last, '0', e.size);
    std::string resolved;
    if (e.header_len == 512) {
      std::string prefix = field(h + 345, 155);
      resolved = prefix.empty() ? field(h, 100) : prefix + "/" + field(h, 100);
    } else {
      uint64_t rec_len = octal(h + 124, 12);
      check_block(h, 'x', rec_len);
      CHECK(e.header_len == 1024 + pad512(rec_len));
      std::string rec(h + 512, rec_len);
      size_t sp = rec.find(' ');
      CHECK(sp != std::string::npos);
      CHECK(std::strtoull(rec.c_str(), nullptr, 10) == rec_len);
      CHECK(rec.compare(sp + 1, 5, "path=") == 0);
      CHECK(rec.back() == '\n');
      resolved = rec.substr(sp + 6, rec.size() - sp - 7);
      for (uint64_t k = rec_len; k < pad512(rec_len); k++) CHECK(h[512 + k] == '\0');
      CHECK(field(last, 100) == name.substr(0, 100));
      CHECK(field(last + 345, 155).empty());
    }
    CHECK(resolved == name);
    hoff += e.header_len;
    off += e.header_len + pad512(e.size);
  }
  CHECK(hoff == lay.headers.size());
  CHECK(lay.total == off + 1024);
  CHECK(lay.total % 512 == 0);
}

template <class F>
void expect_reject(F&& f, const char* what) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return;
  }
  std::fprintf(stderr, "not rejected: %s\n", what);
  failures++;
}

}  // namespace

int main() {
  const std::string s(1, '/');
  std::vector<std::pair<std::string, uint64_t>> members = {
      {"a", 0},
      {std::string(99, 'b'), 1},
      {std::string(100, 'c'), 511},
      {std::string(101, 'd'), 512},
      {"dir/" + std::string(97, 'e'), 513},
      {std::string(256, 'f'), (4u << 20) + 1},
      {std::string(160, 'g') + s + std::string(20, 'h'), (8ull << 30) - 1},
      {std::string(155, 'i') + s + std::string(100, 'j'), 7},    // both fields full
      {std::string(156, 'k') + s + std::string(100, 'l'), 7},    // prefix one too long
      {std::string(155, 'm') + s + std::string(101, 'n'), 7},    // name one too long
      {std::string(50, 'o') + s + std::string(50, 'p') + s + std::string(60, 'q'), 7},
      {std::string(887, 'r') + s + std::string(101, 's'), 7},    // 999-byte PAX record
      {std::string(888, 't') + s + std::string(101, 'u'), 7},    // 1001-byte PAX record
      {"a..b/..c/d..", 3},
  };
  check_layout(members);
  check_layout({});
  for (const auto& m : members) check_layout({m});

  PackLayout a = pack_layout(members), b = pack_layout(members);
  CHECK(a.headers == b.headers && a.total == b.total);

  expect_reject([] { pack_layout({{"", 1}}); }, "empty name");
  expect_reject([] { pack_layout({{"/abs", 1}}); }, "absolute name");
  expect_reject([] { pack_layout({{"a/../b", 1}}); }, "'..' component");
  expect_reject([] { pack_layout({{"..", 1}}); }, "'..' alone");
  expect_reject([] { pack_layout({{"a/..", 1}}); }, "trailing '..'");
  expect_reject([] { pack_layout({{"dir/", 1}}); }, "trailing slash");
  expect_reject([] { pack_layout({{"a//b", 1}}); }, "empty component");
  expect_reject([] { pack_layout({{"./a", 1}}); }, "'.' component");
  expect_reject([] {
    std::vector<std::pair<std::string, uint64_t>> many;
    for (int i = 0; i < 32769; i++) many.push_back({std::string(200, 'L') + std::to_string(i), 0});
    pack_layout(many);
  }, "more header entries than the index reads");
  expect_reject([] { pack_layout({{std::string("nul\0name", 8), 1}}); }, "embedded NUL");
  expect_reject([] { pack_layout({{"dup", 1}, {"x", 2}, {"dup", 3}}); }, "duplicate");
  expect_reject([] { pack_layout({{"big", 8ull << 30}}); }, "8 GiB member");

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("tar_pack_selftest ok\n");
  return 0;
}
