// Stand-alone self-test of the tar index's host model: the header walk of
// core/include/modelx/tar_core.hpp (the code tar_index_kernel runs) and the
// name resolution of tar_host.hpp. Meant to be built with
//   g++ -std=c++17 -fsanitize=address,undefined -Icore/include
// Every archive is indexed from a heap buffer of exactly tar_len bytes, so a
// read past the end of the archive is an ASan report. Exit status 0 and no
// output on stderr mean success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "modelx/tar_host.hpp"

namespace th = modelx::tarhost;
namespace tc = modelx::tarcore;

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                          \
    }                                                                      \
  } while (0)

using Members = std::vector<std::pair<std::string, uint64_t>>;

// index_host over a buffer allocated at exactly the archive's length
std::vector<th::IndexedFile> index_exact(const std::string& archive) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[archive.size()]);
  if (!archive.empty()) std::memcpy(buf.get(), archive.data(), archive.size());
  return th::index_host(buf.get(), archive.size());
}

// The archive pack_layout describes; member i's payload is filled with 'a' + i.
std::string build(const Members& members, bool end_marker = true) {
  th::PackLayout lay = th::pack_layout(members);
  std::string out;
  size_t hoff = 0;
  for (size_t i = 0; i < members.size(); i++) {
    const th::PackEntry& e = lay.entries[i];
    out.append(lay.headers, hoff, e.header_len);
    hoff += e.header_len;
    out.append(e.size, static_cast<char>('a' + i % 26));
    out.append(th::pad512(e.size) - e.size, '\0');
  }
  if (end_marker) out.append(1024, '\0');
  return out;
}

void fix_checksum(std::string* a, size_t off) {
  std::memset(&(*a)[off + 148], ' ', 8);
  uint32_t sum = 0;
  for (size_t i = 0; i < 512; i++) sum += static_cast<unsigned char>((*a)[off + i]);
  th::put_octal(&(*a)[off + 148], 6, sum);
  (*a)[off + 155] = ' ';
}

void set_size_field(std::string* a, size_t off, const std::string& field) {
  CHECK(field.size() == 12);
  std::memcpy(&(*a)[off + 124], field.data(), 12);
  fix_checksum(a, off);
}

std::string octal_field(uint64_t v) {
  char f[13];
  th::put_octal(f, 11, v);
  return std::string(f, 12);
}

std::string base256_field(unsigned char first, uint64_t low) {
  std::string f(12, '\0');
  f[0] = static_cast<char>(first);
  for (int i = 0; i < 8; i++) f[11 - i] = static_cast<char>(low >> (8 * i));
  return f;
}

// One PAX member: 'x' (or 'g') header with `payload`, then a 700-byte file.
std::string pax_archive(const std::string& payload, char typeflag = 'x') {
  std::string a;
  th::append_header(&a, "PaxHeader", "", payload.size(), typeflag);
  a.append(payload);
  a.append(th::pad512(payload.size()) - payload.size(), '\0');
  a.append(build({{"m1", 700}}));
  return a;
}

void expect_files(const std::string& archive, const Members& members, const char* what) {
  try {
    std::vector<th::IndexedFile> got = index_exact(archive);
    CHECK(got.size() == members.size());
    for (size_t i = 0; i < got.size() && i < members.size(); i++) {
      CHECK(got[i].name == members[i].first);
      CHECK(got[i].size == members[i].second);
      CHECK(got[i].mode == 0644);
      CHECK(got[i].offset + got[i].size <= archive.size());
      if (got[i].size) CHECK(archive[got[i].offset] == static_cast<char>('a' + i % 26));
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s: unexpected error: %s\n", what, e.what());
    failures++;
  }
}

void expect_reject(const std::string& archive, uint32_t code, uint64_t header_off,
                   const char* what) {
  try {
    index_exact(archive);
  } catch (const th::IndexError& e) {
    if (e.code != code || e.header_off != header_off) {
      std::fprintf(stderr, "%s: rejected with \"%s\", expected code %u at %llu\n", what, e.what(),
                   code, static_cast<unsigned long long>(header_off));
      failures++;
    }
    return;
  }
  std::fprintf(stderr, "not rejected: %s\n", what);
  failures++;
}

}  // namespace

int main() {
  const std::string s(1, '/');
  Members members = {
      {"a", 0},
      {std::string(99, 'b'), 1},
      {std::string(100, 'c'), 511},
      {std::string(101, 'd'), 512},  // PAX path=
      {"dir/" + std::string(97, 'e'), 513},
      {std::string(256, 'f'), 70001},
      {std::string(155, 'i') + s + std::string(100, 'j'), 7},  // both fields full
      {std::string(887, 'r') + s + std::string(101, 't'), 7},  // 999-byte PAX record
  };
  expect_files(build(members), members, "pack_layout archive");
  expect_files(build(members, false), members, "no end marker");
  expect_files(build({}), {}, "end marker only");
  expect_files("", {}, "empty archive");
  for (const auto& m : members) expect_files(build({m}), {m}, "single member");

  // ragged lengths: whatever is cut off, no read past the end; the result
  // is a shorter listing or a refusal
  const Members two = {{"m1", 700}, {"m2", 513}};
  const std::string good = build(two, false);  // header, 1024, header, 1024
  const size_t h2 = 1536;
  CHECK(good.size() == 3072);
  for (size_t cut = 0; cut <= good.size(); cut++) {
    size_t whole = cut >= 3072 ? 2 : cut >= 1536 ? 1 : 0;
    bool partial_header = cut - whole * 1536 < 512;
    try {
      std::vector<th::IndexedFile> got = index_exact(good.substr(0, cut));
      CHECK(partial_header && got.size() == whole);
    } catch (const th::IndexError& e) {
      CHECK(!partial_header && e.code == tc::kErrPayloadPastEnd &&
            e.header_off == whole * 1536);
    }
  }
  std::string x_member = build({{std::string(200, 'n'), 513}}, false);
  for (size_t cut = 0; cut < x_member.size(); cut += 37) {
    try {
      CHECK(index_exact(x_member.substr(0, cut)).empty());
    } catch (const th::IndexError& e) {
      CHECK(e.code == tc::kErrPayloadPastEnd);
    }
  }

  // sizes against the archive
  std::string a = good;
  set_size_field(&a, h2, octal_field(1024 + 1));
  expect_reject(a, tc::kErrPayloadPastEnd, h2, "size overruns by 1 byte");
  set_size_field(&a, h2, octal_field(1024 + (1u << 20)));
  expect_reject(a, tc::kErrPayloadPastEnd, h2, "size overruns by 1 MiB");
  set_size_field(&a, h2, octal_field(th::kMaxMemberSize));
  expect_reject(a, tc::kErrPayloadPastEnd, h2, "size of 8 GiB - 1");
  set_size_field(&a, h2, octal_field(1024));
  expect_files(a, {{"m1", 700}, {"m2", 1024}}, "size fills the archive exactly");
  expect_reject(x_member.substr(0, 512 + 100), tc::kErrPayloadPastEnd, 0, "'x' truncated");
  std::string l_member = x_member;
  l_member[156] = 'L';
  fix_checksum(&l_member, 0);
  expect_reject(l_member.substr(0, 512 + 100), tc::kErrPayloadPastEnd, 0, "'L' truncated");
  {  // the 'L' payload (here the PAX record's text) names the member
    std::vector<th::IndexedFile> got = index_exact(l_member);
    CHECK(got.size() == 1 && got[0].name == th::pax_path_record(std::string(200, 'n')));
  }
  std::string g_member = x_member;
  g_member[156] = 'g';
  fix_checksum(&g_member, 0);
  expect_reject(g_member.substr(0, 512 + 100), tc::kErrPayloadPastEnd, 0, "'g' truncated");

  // base-256 sizes
  a = good;
  set_size_field(&a, h2, base256_field(0x80, 513));
  expect_files(a, two, "base-256 size 513");
  set_size_field(&a, h2, base256_field(0x80, 1025));
  expect_reject(a, tc::kErrPayloadPastEnd, h2, "base-256 size overruns by 1 byte");
  set_size_field(&a, h2, base256_field(0xff, ~0ull));
  expect_reject(a, tc::kErrSizeNegative, h2, "base-256 -1");
  set_size_field(&a, h2, base256_field(0xc0, 513));
  expect_reject(a, tc::kErrSizeNegative, h2, "base-256 sign bit");
  set_size_field(&a, h2, base256_field(0x80, 1ull << 63));
  expect_reject(a, tc::kErrSizeTooLarge, h2, "base-256 2^63");
  set_size_field(&a, h2, base256_field(0x80, ~0ull));
  expect_reject(a, tc::kErrSizeTooLarge, h2, "base-256 2^64 - 1");
  set_size_field(&a, h2, base256_field(0x81, 513));
  expect_reject(a, tc::kErrSizeTooLarge, h2, "base-256 above 2^88");
  {
    std::string f = base256_field(0x80, 513);
    f[2] = 1;  // 2^72
    set_size_field(&a, h2, f);
    expect_reject(a, tc::kErrSizeTooLarge, h2, "base-256 2^72");
  }
  set_size_field(&a, h2, (std::string("0000000z001") + '\0'));
  expect_reject(a, tc::kErrSizeField, h2, "size with a letter");
  set_size_field(&a, h2, "       1001 ");
  expect_files(a, two, "size with leading spaces and a trailing space");
  set_size_field(&a, h2, std::string(12, ' '));
  expect_reject(a, tc::kErrChecksum, h2 + 512, "blank size: the payload is taken for a header");

  // checksums
  a = good;
  a[h2 + 1] ^= 1;
  expect_reject(a, tc::kErrChecksum, h2, "flipped name byte");
  a = good.substr(0, h2) + std::string(512, '\x5a') + good.substr(h2);
  expect_reject(a, tc::kErrChecksum, h2, "garbage block");
  a = good;
  std::memcpy(&a[h2 + 148], "zzzzzz\0 ", 8);
  expect_reject(a, tc::kErrChecksum, h2, "checksum field is no number");
  {  // the sum of signed bytes is accepted too
    a = build({{"\xc3\xa9\xc3\xa8", 700}});
    std::memset(&a[148], ' ', 8);
    int32_t sum = 0;
    for (size_t i = 0; i < 512; i++) sum += static_cast<signed char>(a[i]);
    th::put_octal(&a[148], 6, static_cast<uint64_t>(sum));
    a[155] = ' ';
    expect_files(a, {{"\xc3\xa9\xc3\xa8", 700}}, "signed checksum");
  }
  a = good;
  std::memcpy(&a[h2 + 100], "0000z44", 7);
  fix_checksum(&a, h2);
  expect_reject(a, tc::kErrModeField, h2, "mode with a letter");

  // PAX records
  expect_files(pax_archive("12 path=abc\n"), {{"abc", 700}}, "PAX path=");
  expect_files(pax_archive("13 mtime=1.5\n12 path=abc\n11 uid=100\n"), {{"abc", 700}},
               "PAX path= among others");
  expect_files(pax_archive(""), {{"m1", 700}}, "empty PAX header");
  expect_files(pax_archive("15 comment=abc\n", 'g'), {{"m1", 700}}, "PAX global header");
  expect_reject(pax_archive("12 path=abc\n12 size=700\n"), tc::kErrPaxSize, 0, "PAX size=");
  expect_reject(pax_archive("12 size=700\n", 'g'), tc::kErrPaxSize, 0, "PAX global size=");
  expect_reject(pax_archive("0 path=abc\n"), tc::kErrPaxRecord, 0, "PAX record length 0");
  expect_reject(pax_archive("99 path=abc\n"), tc::kErrPaxRecord, 0, "PAX length past payload");
  expect_reject(pax_archive("path=abc\n"), tc::kErrPaxRecord, 0, "PAX record without length");
  expect_reject(pax_archive("12"), tc::kErrPaxRecord, 0, "PAX record of digits only");
  expect_reject(pax_archive("3 \n"), tc::kErrPaxRecord, 0, "PAX record without keyword");
  expect_reject(pax_archive("4 =\n\n"), tc::kErrPaxRecord, 0, "PAX record with empty keyword");
  expect_reject(pax_archive("11 path=abc"), tc::kErrPaxRecord, 0, "PAX record without newline");
  expect_reject(pax_archive("11 pathabc\n"), tc::kErrPaxRecord, 0, "PAX record without '='");
  expect_reject(pax_archive("99999999999999999999 path=abc\n"), tc::kErrPaxRecord, 0,
                "PAX length of 20 digits");
  expect_reject(pax_archive(std::string("12 path=abc\n\0\0", 14)), tc::kErrPaxRecord, 0,
                "PAX trailing NULs");
  expect_reject(pax_archive("22 GNU.sparse.major=1\n"), tc::kErrPaxSparse, 0, "GNU sparse");

  // the entry table's limit
  {
    std::string one;
    th::append_header(&one, "m", "", 0, '0');
    std::string many;
    many.reserve(512 * (th::kMaxIndexEntries + 1) + 1024);
    for (uint32_t i = 0; i < th::kMaxIndexEntries; i++) many.append(one);
    try {
      CHECK(index_exact(many).size() == th::kMaxIndexEntries);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "65536 members: unexpected error: %s\n", e.what());
      failures++;
    }
    many.append(one);
    expect_reject(many, tc::kErrTooManyEntries, 512ull * th::kMaxIndexEntries,
                  "65537 members");
  }

  // the host-side table check does not take the walk's word
  {
    std::vector<tc::Entry> table = {{0, 512, 700, '0', 0644}, {1536, 2048, 513, '0', 0644}};
    th::validate_entries(table, 3072);
    auto bad = [&](std::vector<tc::Entry> t, uint64_t len, const char* what) {
      try {
        th::validate_entries(t, len);
      } catch (const th::IndexError&) {
        return;
      }
      std::fprintf(stderr, "table not refused: %s\n", what);
      failures++;
    };
    bad(table, 3071, "archive one byte short");
    bad({{0, 512, 1025, '0', 0644}, {1536, 2048, 513, '0', 0644}}, 3072, "gap in the chain");
    bad({{0, 512, ~0ull, '0', 0644}}, 3072, "size of 2^64 - 1");
    bad({{0, 512, (1ull << 63) - 1, '0', 0644}}, 3072, "size of 2^63 - 1");
    bad({{0, 1024, 700, '0', 0644}}, 3072, "payload not behind its header");
    bad({{512, 1024, 0, '0', 0644}}, 3072, "first header not at 0");
    bad({{0, 512, 0, '0', 0644}}, 511, "header past the end");
  }

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("tar_index_selftest ok\n");
  return 0;
}
