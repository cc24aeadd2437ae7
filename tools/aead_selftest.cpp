// Stand-alone self-test of the ChaCha20-Poly1305 host model
// (core/include/modelx/aead_core.hpp). Meant to be built with
//   g++ -std=c++17 -fsanitize=address,undefined -Icore/include
// so the header-only code runs its edge lengths under ASan/UBSan in a process
// of its own: every buffer is allocated at exactly its size, so one read or
// write outside it is a sanitizer report. Pins the RFC 8439 section 2.8.2 text
// with empty AAD, then seals and opens the lengths of the GPU test at the
// default segment and at 2048. Exit status 0 and no output on stderr mean
// success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "modelx/aead_core.hpp"

namespace ae = modelx::aead;

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                          \
    }                                                                      \
  } while (0)

void rfc_vector() {
  uint8_t kb[32];
  for (int i = 0; i < 32; i++) kb[i] = static_cast<uint8_t>(0x80 + i);
  const ae::Key key = ae::key_from_bytes(kb);
  const char* text =
      "Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the "
      "future, sunscreen would be it.";
  const size_t n = std::strlen(text);
  CHECK(n == 114);
  // nonce 07000000 4041424344454647 as the three state words
  const uint32_t nonce[3] = {7u, 0x43424140u, 0x47464544u};
  uint32_t ks[16];
  ae::chacha_block(key, 1, nonce, ks);
  const uint8_t first[4] = {0xd3, 0x1a, 0x8d, 0x34};
  for (int i = 0; i < 4; i++)
    CHECK((static_cast<uint8_t>(text[i]) ^ static_cast<uint8_t>(ks[0] >> (8 * i))) == first[i]);
}

void round_trips(uint64_t seg) {
  const uint64_t S = seg;
  const uint64_t lengths[] = {1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025,
                              S - 1, S, S + 1, 3 * S + 1041};
  uint8_t kb[32];
  for (int i = 0; i < 32; i++) kb[i] = static_cast<uint8_t>(7 * i + 1);
  const ae::Key key = ae::key_from_bytes(kb);
  for (uint64_t n : lengths) {
    std::vector<uint8_t> plain(n);
    for (uint64_t i = 0; i < n; i++) plain[i] = static_cast<uint8_t>(i * 131 + (i >> 8));
    std::vector<uint8_t> sealed(ae::sealed_size(n, seg));
    ae::seal_blob(key, plain.data(), n, seg, sealed.data());
    std::vector<uint8_t> back(n);
    CHECK(ae::open_blob(key, sealed.data(), n, seg, back.data()) == -1);
    CHECK(back == plain);
    // in place, and a flipped bit in the last segment's ciphertext and tag
    std::vector<uint8_t> inplace = sealed;
    CHECK(ae::open_blob(key, inplace.data(), n, seg, inplace.data()) == -1);
    CHECK(std::memcmp(inplace.data(), plain.data(), n) == 0);
    const int64_t last = static_cast<int64_t>(ae::segment_count(n, seg)) - 1;
    std::vector<uint8_t> bent = sealed;
    bent[n - 1] ^= 0x10;
    CHECK(ae::open_blob(key, bent.data(), n, seg, back.data()) == last);
    bent = sealed;
    bent[sealed.size() - 1] ^= 0x01;
    CHECK(ae::open_blob(key, bent.data(), n, seg, back.data()) == last);
  }
}

}  // namespace

int main() {
  rfc_vector();
  round_trips(ae::kDefaultSegmentBytes);
  round_trips(2048);
  if (failures) return 1;
  std::printf("aead_selftest ok\n");
  return 0;
}
