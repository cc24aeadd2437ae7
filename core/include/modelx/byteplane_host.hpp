// Byte-plane transform of a tensor blob: the normative host model.
//
// A little-endian float stream alternates statistically different bytes
// (bf16: a near-random mantissa byte, a strongly skewed sign/exponent byte).
// Storing each byte position of the element as its own plane makes every
// zstd frame homogeneous, so its one Huffman table fits.
//
// For a blob of `size` bytes, element size E and group size G (G > 0,
// G % E == 0), group k covers [kG, min((k+1)G, size)); it has length n and
// m = n / E whole elements:
//
//   planar[kG + p*m + i] = raw[kG + i*E + p]      0 <= i < m, 0 <= p < E
//
// and the n - m*E trailing bytes (only the last group can have any) keep
// their offsets. `merge` is the inverse. Both are permutations of
// [0, size): no parameter choice reads or writes outside the blob.
//
// Pure C++ (no HIP) so the CPU client, the CPU suite and a sanitizer
// self-test run it; the kernels in core/hip/byteplane.hip are tested
// against it.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>

namespace modelx {
namespace byteplane {

inline bool valid_elem(uint64_t elem) { return elem == 2 || elem == 4 || elem == 8; }

// Throws std::invalid_argument unless elem is 2, 4 or 8 and group is a
// positive multiple of it.
inline void validate(uint64_t elem, uint64_t group) {
  if (!valid_elem(elem))
    throw std::invalid_argument("byte planes: element size " + std::to_string(elem) +
                                " is not 2, 4 or 8");
  if (group == 0 || group % elem != 0)
    throw std::invalid_argument("byte planes: group size " + std::to_string(group) +
                                " is not a positive multiple of the element size " +
                                std::to_string(elem));
}

namespace detail {

template <bool kMerge>
inline void run(const uint8_t* src, uint8_t* dst, uint64_t size, uint32_t elem, uint64_t group) {
  validate(elem, group);
  for (uint64_t base = 0; base < size;) {
    uint64_t n = size - base < group ? size - base : group;
    uint64_t m = n / elem;
    const uint8_t* s = src + base;
    uint8_t* d = dst + base;
    for (uint32_t p = 0; p < elem; p++) {
      if (kMerge) {
        const uint8_t* plane = s + p * m;
        for (uint64_t i = 0; i < m; i++) d[i * elem + p] = plane[i];
      } else {
        uint8_t* plane = d + p * m;
        for (uint64_t i = 0; i < m; i++) plane[i] = s[i * elem + p];
      }
    }
    for (uint64_t j = m * elem; j < n; j++) d[j] = s[j];
    base += n;
  }
}

}  // namespace detail

// raw -> planar. The buffers must not overlap.
inline void split(const uint8_t* raw, uint8_t* planar, uint64_t size, uint32_t elem,
                  uint64_t group) {
  detail::run<false>(raw, planar, size, elem, group);
}

// planar -> raw. The buffers must not overlap.
inline void merge(const uint8_t* planar, uint8_t* raw, uint64_t size, uint32_t elem,
                  uint64_t group) {
  detail::run<true>(planar, raw, size, elem, group);
}

}  // namespace byteplane
}  // namespace modelx
