// CDNA4 byte-plane kernels (gfx950): split a tensor blob into one plane per
// byte position of its element, and merge the planes back.
//
// The transform and its parameters are defined by the host model
// (modelx/byteplane_host.hpp): per group of G bytes holding m = G/E
// elements, planar[p*m + i] = raw[i*E + p]. It is a pure permutation, so the
// kernels are bandwidth-bound; a device-to-device copy of the same size is
// their ceiling.
//
// Fast path (full group, m a multiple of 16, both buffers 16 B aligned): one
// lane owns 16 consecutive elements. Split reads their E*16 contiguous bytes
// as E 16 B loads, transposes bytes in registers (v_perm_b32) and issues one
// 16 B store per plane; across a wave every plane store is 1 KiB contiguous.
// Merge is the mirror image. Everything else — the short last group, its
// n % E tail, unaligned buffers, a group whose planes are not 16 B
// multiples — goes bytewise.
//
// The grid walks a flattened (group, tile) index with a grid stride, so one
// group and a 100 GiB blob both spread over the chip. All offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/device_abi.hpp"

namespace {

constexpr int kThreads = 256;
constexpr uint64_t kUnitElems = 16;                      // elements per lane per trip
constexpr uint64_t kTileElems = kThreads * kUnitElems;   // elements per workgroup per trip
constexpr uint32_t kMaxBlocks = 2048;                    // 8 per CU; the rest grid-strides

// One 16 B load or store in the IR (see the note in tar.hip).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Byte i of the result is byte sel.byte[i] of the 8-byte value {hi:lo}
// (0..3 pick from lo, 4..7 from hi).
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
  return __builtin_amdgcn_perm(hi, lo, sel);
}

// 4x4 byte transpose: byte c of input row r becomes byte r of output row c.
// Its own inverse.
__device__ __forceinline__ void transpose4(uint32_t a, uint32_t b, uint32_t c, uint32_t d,
                                           uint32_t& o0, uint32_t& o1, uint32_t& o2,
                                           uint32_t& o3) {
  uint32_t t0 = perm(b, a, 0x05010400u);  // a0 b0 a1 b1
  uint32_t t1 = perm(b, a, 0x07030602u);  // a2 b2 a3 b3
  uint32_t t2 = perm(d, c, 0x05010400u);  // c0 d0 c1 d1
  uint32_t t3 = perm(d, c, 0x07030602u);  // c2 d2 c3 d3
  o0 = perm(t2, t0, 0x05040100u);         // a0 b0 c0 d0
  o1 = perm(t2, t0, 0x07060302u);         // a1 b1 c1 d1
  o2 = perm(t3, t1, 0x05040100u);
  o3 = perm(t3, t1, 0x07060302u);
}

// raw[4*E] holds 16 elements of E bytes; plane[p][k] receives byte p of
// elements 4k..4k+3.
template <int E>
__device__ __forceinline__ void split_unit(const uint32_t* raw, u32x4* plane) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (E == 2) {
      plane[0][k] = perm(raw[2 * k + 1], raw[2 * k], 0x06040200u);
      plane[1][k] = perm(raw[2 * k + 1], raw[2 * k], 0x07050301u);
    } else {
      // element j of the four is dwords (E/4)*j .. of this k's E dwords;
      // each dword position h is one 4x4 transpose
#pragma unroll
      for (int h = 0; h < E / 4; h++) {
        const uint32_t* r = raw + E * k + h;
        uint32_t o0, o1, o2, o3;
        transpose4(r[0], r[E / 4], r[2 * (E / 4)], r[3 * (E / 4)], o0, o1, o2, o3);
        plane[4 * h + 0][k] = o0;
        plane[4 * h + 1][k] = o1;
        plane[4 * h + 2][k] = o2;
        plane[4 * h + 3][k] = o3;
      }
    }
  }
}

// The inverse of split_unit.
template <int E>
__device__ __forceinline__ void merge_unit(const u32x4* plane, uint32_t* raw) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (E == 2) {
      raw[2 * k] = perm(plane[1][k], plane[0][k], 0x05010400u);
      raw[2 * k + 1] = perm(plane[1][k], plane[0][k], 0x07030602u);
    } else {
#pragma unroll
      for (int h = 0; h < E / 4; h++) {
        uint32_t* r = raw + E * k + h;
        transpose4(plane[4 * h + 0][k], plane[4 * h + 1][k], plane[4 * h + 2][k],
                   plane[4 * h + 3][k], r[0], r[E / 4], r[2 * (E / 4)], r[3 * (E / 4)]);
      }
    }
  }
}

// Shared body. Tile T of the flattened index is tile T % tiles_per_group of
// group T / tiles_per_group; a tile is kTileElems elements of its group (the
// short last group simply has empty tiles). `vec_ok` says the buffers are
// 16 B aligned and a full group's planes are 16 B multiples.
template <int E, bool kMerge>
__device__ __forceinline__ void byte_planes_body(const uint8_t* __restrict__ src,
                                                 uint8_t* __restrict__ dst, uint64_t size,
                                                 uint64_t group, uint64_t tiles_per_group,
                                                 uint64_t ntiles, bool vec_ok) {
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint64_t g = tile / tiles_per_group;
    uint64_t t = tile - g * tiles_per_group;
    uint64_t base = g * group;  // < size: the host sizes ntiles by ceil(size / group)
    uint64_t n = size - base < group ? size - base : group;
    uint64_t m = n / E;
    const uint8_t* s = src + base;
    uint8_t* d = dst + base;
    if (vec_ok && n == group) {
      uint64_t i = t * kTileElems + threadIdx.x * kUnitElems;  // first element of this lane
      if (i < m) {  // m % 16 == 0: the whole unit is inside the group
        uint32_t raw[4 * E];
        u32x4 plane[E];
        if (kMerge) {
#pragma unroll
          for (int p = 0; p < E; p++) plane[p] = *reinterpret_cast<const u32x4*>(s + p * m + i);
          merge_unit<E>(plane, raw);
          u32x4* out = reinterpret_cast<u32x4*>(d + i * E);
#pragma unroll
          for (int j = 0; j < E; j++) {
            u32x4 v = {raw[4 * j], raw[4 * j + 1], raw[4 * j + 2], raw[4 * j + 3]};
            out[j] = v;
          }
        } else {
          const u32x4* in = reinterpret_cast<const u32x4*>(s + i * E);
#pragma unroll
          for (int j = 0; j < E; j++) {
            u32x4 v = in[j];
            raw[4 * j] = v.x;
            raw[4 * j + 1] = v.y;
            raw[4 * j + 2] = v.z;
            raw[4 * j + 3] = v.w;
          }
          split_unit<E>(raw, plane);
#pragma unroll
          for (int p = 0; p < E; p++) *reinterpret_cast<u32x4*>(d + p * m + i) = plane[p];
        }
      }
    } else {
      uint64_t end = (t + 1) * kTileElems < m ? (t + 1) * kTileElems : m;
      for (uint64_t i = t * kTileElems + threadIdx.x; i < end; i += kThreads) {
#pragma unroll
        for (int p = 0; p < E; p++) {
          if (kMerge) d[i * E + p] = s[p * m + i];
          else d[p * m + i] = s[i * E + p];
        }
      }
      // the n % E trailing bytes keep their offsets
      uint64_t j = m * E + threadIdx.x;
      if (t == 0 && j < n) d[j] = s[j];
    }
  }
}

template <int E>
__global__ __launch_bounds__(kThreads) void byte_planes_split_kernel(
    const uint8_t* __restrict__ raw, uint8_t* __restrict__ planar, uint64_t size, uint64_t group,
    uint64_t tiles_per_group, uint64_t ntiles, bool vec_ok) {
  byte_planes_body<E, false>(raw, planar, size, group, tiles_per_group, ntiles, vec_ok);
}

template <int E>
__global__ __launch_bounds__(kThreads) void byte_planes_merge_kernel(
    const uint8_t* __restrict__ planar, uint8_t* __restrict__ raw, uint64_t size, uint64_t group,
    uint64_t tiles_per_group, uint64_t ntiles, bool vec_ok) {
  byte_planes_body<E, true>(planar, raw, size, group, tiles_per_group, ntiles, vec_ok);
}

template <int E>
hipError_t launch(const uint8_t* src, uint8_t* dst, uint64_t size, uint64_t group, bool merge,
                  hipStream_t stream) {
  uint64_t m = group / E;  // elements of a full group
  // tiles cover the longest group there is (a blob shorter than one group
  // has only its short one); at least one, which also carries the tail
  uint64_t span = (group < size ? group : size) / E;
  uint64_t tiles_per_group = span ? (span - 1) / kTileElems + 1 : 1;
  uint64_t ngroups = (size - 1) / group + 1;  // size > 0
  uint64_t ntiles = ngroups * tiles_per_group;
  bool vec_ok = m % kUnitElems == 0 &&
                ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  uint32_t blocks = static_cast<uint32_t>(ntiles < kMaxBlocks ? ntiles : kMaxBlocks);
  if (merge)
    hipLaunchKernelGGL(byte_planes_merge_kernel<E>, dim3(blocks), dim3(kThreads), 0, stream, src,
                       dst, size, group, tiles_per_group, ntiles, vec_ok);
  else
    hipLaunchKernelGGL(byte_planes_split_kernel<E>, dim3(blocks), dim3(kThreads), 0, stream, src,
                       dst, size, group, tiles_per_group, ntiles, vec_ok);
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t modelx_byte_planes(const void* src, void* dst, uint64_t size, uint32_t elem,
                                         uint64_t group, int merge, hipStream_t stream) {
  if (group == 0 || (elem != 2 && elem != 4 && elem != 8) || group % elem != 0)
    return hipErrorInvalidValue;
  if (size == 0) return hipSuccess;
  const uint8_t* s = static_cast<const uint8_t*>(src);
  uint8_t* d = static_cast<uint8_t*>(dst);
  switch (elem) {
    case 2: return launch<2>(s, d, size, group, merge != 0, stream);
    case 4: return launch<4>(s, d, size, group, merge != 0, stream);
    default: return launch<8>(s, d, size, group, merge != 0, stream);
  }
}
