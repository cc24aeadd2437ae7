// Self-test for the strict seek-table parser (zstdhost::parse_seek_footer /
// parse_seek_entries) — the host-side validation between a stored blob's
// tail and the frame offsets the GPU decode kernel is launched with. Feeds
// it the way the engine does (a 17-byte footer copy, then an exactly
// table_bytes-long tail copy, each in its own heap buffer so a sanitizer
// sees any read past either), over a fixed corrupt set and seeded random
// tails. Links only zstd_cpu.cpp: no GPU, no Python.
//
// Build and run (one line; also run it without the -fsanitize flags):
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Icore/include core/src/zstd_cpu.cpp tools/seek_table_selftest.cpp
//       -o /tmp/seek_table_selftest -pthread && /tmp/seek_table_selftest
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "modelx/zstd_host.hpp"

using namespace modelx::zstdhost;
typedef std::vector<uint8_t> Bytes;

// The engine's two-copy protocol. Returns true and fills *out when the tail
// is accepted; false when either step throws.
static bool strict_parse(const Bytes& blob, std::vector<SeekEntry>* out) {
  try {
    Bytes foot(kSeekFooterBytes, 0);
    if (blob.size() >= kSeekFooterBytes)
      memcpy(foot.data(), blob.data() + blob.size() - kSeekFooterBytes, kSeekFooterBytes);
    SeekFooter f = parse_seek_footer(foot.data(), blob.size());
    Bytes table(blob.end() - f.table_bytes, blob.end());
    parse_seek_entries(table.data(), f, blob.size(), out);
    return true;
  } catch (const std::runtime_error&) {
    return false;
  }
}

static void put32(Bytes& b, size_t pos, uint32_t v) {
  for (int i = 0; i < 4; i++) b[pos + i] = (uint8_t)(v >> (8 * i));
}
static uint32_t get32(const Bytes& b, size_t pos) {
  return b[pos] | (b[pos + 1] << 8) | (b[pos + 2] << 16) | ((uint32_t)b[pos + 3] << 24);
}

int main() {
  int fails = 0;
  auto check = [&](bool ok, const char* what) {
    if (!ok) {
      printf("FAIL %s\n", what);
      fails++;
    }
  };

  Bytes data(10 << 10);
  for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)(i * 7 + i / 251);
  const Bytes good = compress_seekable(data.data(), data.size(), 4 << 10);
  const size_t tbl = good.size() - (8 + 3 * 8 + 9);

  std::vector<SeekEntry> ref;
  check(strict_parse(good, &ref) && ref.size() == 3, "good blob parses to 3 frames");
  check(ref.size() == 3 && ref[2].c_off + ref[2].c_size == tbl &&
            ref[2].d_off + ref[2].d_size == data.size(),
        "good blob spans");
  for (size_t n : {0ul, 1ul}) {
    Bytes b = compress_seekable(data.data(), n, 4 << 10);
    std::vector<SeekEntry> t;
    check(strict_parse(b, &t) && t.size() == 1 && t[0].d_size == n, "tiny blob parses");
  }

  // the fixed corrupt set (same cases as tests/util_seek.py)
  std::vector<std::pair<const char*, Bytes>> bad;
  bad.push_back({"truncated-16", Bytes(good.begin(), good.begin() + 16)});
  {
    Bytes b = good;
    b.back() ^= 0xFF;
    bad.push_back({"footer-magic", b});
  }
  {
    Bytes b = good;
    put32(b, b.size() - 9, (uint32_t)b.size());
    bad.push_back({"nframes-exceeds-blob", b});
  }
  {
    Bytes b = good;
    b[tbl] ^= 0xFF;
    bad.push_back({"envelope-magic", b});
  }
  {
    Bytes b = good;
    put32(b, tbl + 4, get32(b, tbl + 4) + 1);
    bad.push_back({"envelope-length", b});
  }
  {
    Bytes b = good;
    put32(b, tbl + 8, get32(b, tbl + 8) + 1);
    bad.push_back({"entry-csize", b});
  }
  for (auto& [name, b] : bad) {
    std::vector<SeekEntry> t;
    check(!strict_parse(b, &t), name);
    check(t.empty(), "rejected tail leaves the output vector as it was");
    check(parse_seek_table(b.data(), b.size()).empty(), "lenient wrapper returns empty");
  }

  // seeded random tails: whatever is accepted must describe spans that lie
  // inside the blob and tile the frame region exactly
  std::mt19937 rng(20240611);
  int accepted = 0;
  for (int iter = 0; iter < 4000; iter++) {
    Bytes b;
    switch (iter % 4) {
      case 0:  // pure noise, short lengths included
        b.resize(rng() % 96);
        for (auto& x : b) x = (uint8_t)rng();
        break;
      case 1:  // good blob, 1-3 random tail bytes replaced
        b = good;
        for (int k = 1 + rng() % 3; k > 0; k--) b[tbl + rng() % (b.size() - tbl)] = (uint8_t)rng();
        break;
      case 2:  // good blob, random truncation
        b.assign(good.begin(), good.begin() + rng() % (good.size() + 1));
        break;
      default: {  // valid footer magic, everything before it random
        b.resize(17 + rng() % 200);
        for (auto& x : b) x = (uint8_t)rng();
        put32(b, b.size() - 4, 0x8F92EAB1u);
        if (rng() % 2) put32(b, b.size() - 9, rng() % 32);
        break;
      }
    }
    std::vector<SeekEntry> t;
    if (!strict_parse(b, &t)) continue;
    accepted++;
    uint64_t c = 0, d = 0;
    for (auto& e : t) {
      check(e.c_off == c && e.d_off == d, "accepted entries are contiguous");
      c += e.c_size;
      d += e.d_size;
    }
    check(c <= b.size(), "accepted entries stay inside the blob");
  }
  printf("random tails: %d of 4000 accepted\n", accepted);

  printf(fails ? "SEEK TABLE SELFTEST FAILED: %d\n" : "seek table selftest ok (%d)\n", fails);
  return fails ? 1 : 0;
}
