// Stand-alone self-test of the byte-plane host model
// (core/include/modelx/byteplane_host.hpp). Meant to be built with
//   g++ -std=c++17 -fsanitize=address,undefined -Icore/include
// so the header-only code runs its edge sizes under ASan/UBSan in a process
// of its own: every buffer is allocated at exactly `size` bytes, so one read
// or write outside the blob is a sanitizer report. Exit status 0 and no
// output on stderr mean success.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "modelx/byteplane_host.hpp"

namespace bp = modelx::byteplane;

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                          \
    }                                                                      \
  } while (0)

// The definition, evaluated per destination byte: independent of the
// plane-by-plane loops of the header.
uint8_t planar_at(const std::vector<uint8_t>& raw, uint64_t j, uint64_t elem, uint64_t group) {
  uint64_t k = j / group;
  uint64_t base = k * group;
  uint64_t n = raw.size() - base < group ? raw.size() - base : group;
  uint64_t m = n / elem;
  uint64_t r = j - base;
  if (r >= m * elem) return raw[j];
  uint64_t p = r / m, i = r % m;
  return raw[base + i * elem + p];
}

void check(uint64_t size, uint32_t elem, uint64_t group) {
  std::vector<uint8_t> raw(size), planar(size), back(size);
  uint32_t x = 0x9E3779B9u ^ static_cast<uint32_t>(size * 31 + elem);
  for (auto& b : raw) {
    x = x * 1664525u + 1013904223u;
    b = static_cast<uint8_t>(x >> 24);
  }
  bp::split(raw.data(), planar.data(), size, elem, group);
  bool ok = true;
  for (uint64_t j = 0; j < size && ok; j++) ok = planar[j] == planar_at(raw, j, elem, group);
  CHECK(ok);
  bp::merge(planar.data(), back.data(), size, elem, group);
  CHECK(back == raw);
  // a permutation: the byte histogram is unchanged
  uint64_t ha[256] = {0}, hb[256] = {0};
  for (uint64_t j = 0; j < size; j++) {
    ha[raw[j]]++;
    hb[planar[j]]++;
  }
  for (int v = 0; v < 256; v++) ok = ok && ha[v] == hb[v];
  CHECK(ok);
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
  for (uint32_t elem : {2u, 4u, 8u}) {
    const uint64_t e = elem;
    const uint64_t groups[] = {e, 16 * e, 24 * e, e * (128u << 10)};
    for (uint64_t group : groups) {
      const uint64_t sizes[] = {0,         1,         e - 1,            e,
                                elem + 1,  group - 1, group,            group + 1,
                                group + elem + 1,     3 * group + 5,    2 * group};
      for (uint64_t size : sizes) check(size, elem, group);
    }
  }
  // null buffers are fine for an empty blob
  bp::split(nullptr, nullptr, 0, 2, 2);
  bp::merge(nullptr, nullptr, 0, 8, 64);

  uint8_t a[8] = {0}, b[8] = {0};
  expect_reject([&] { bp::split(a, b, 8, 3, 96); }, "elem 3");
  expect_reject([&] { bp::split(a, b, 8, 0, 8); }, "elem 0");
  expect_reject([&] { bp::split(a, b, 8, 1, 8); }, "elem 1");
  expect_reject([&] { bp::split(a, b, 8, 16, 64); }, "elem 16");
  expect_reject([&] { bp::merge(a, b, 8, 2, 0); }, "group 0");
  expect_reject([&] { bp::merge(a, b, 8, 2, 7); }, "group 7 with elem 2");
  expect_reject([&] { bp::merge(a, b, 8, 8, 12); }, "group 12 with elem 8");

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("byteplane_selftest ok\n");
  return 0;
}
