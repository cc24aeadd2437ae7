// CDNA4 content-defined chunking: every candidate position of a device range
// (modelx/cdc_core.hpp defines the gear table, the rolling hash and the
// candidate test; the sequential boundary selection over the candidates stays
// on the host).
//
// Replaces (reference): nothing — the reference dedups whole blobs only
// (pkg/client/push.go:169-177); this feeds the shift-tolerant chunk dedup.
//
// Work split. A workgroup of 256 lanes owns a tile of kTileBytes on the 16 B
// grid of the range's first byte (tile k starts at (ptr & ~15) + k*kTileBytes),
// so every global load of the body is one aligned 16 B load. It stages the
// tile and the 32 bytes before it into LDS, then each lane rolls the hash
// serially over its own run of kRunBytes, starting 32 bytes early with h = 0:
// after 32 steps the value is exact whatever came before (cdc_core.hpp).
//
// LDS layout. Lane t reads dwords t*kRunBytes/4 + j. At a power-of-two run
// length all 64 lanes of a wave would sit on one bank, so one pad dword
// follows every kRunBytes of data: logical byte o lives in dword
// o/4 + o/kRunBytes, lane t's j-th dword at t*(kRunBytes/4 + 1) + j — an odd
// stride, conflict-free at 32 and at 64 banks. The 1 KiB gear table is in LDS
// too; its reads are data-dependent, so their conflicts are random.
//
// Inner loop. Per byte: one bit-field extract, one LDS gear read, one
// v_lshl_add_u32. The candidate test is taken once per dword on the minimum
// of its four hashes (hits are one per 2^bits bytes), so the rare branch
// costs a compare per four bytes.
//
// Edges. Only the first tile can hold bytes before the range and only the
// last one bytes after it. A lane whose run (with warm-up) is not wholly
// inside the range rolls bytewise from the range's first byte with h = 0 —
// bytes before offset 0 contribute nothing — and stops at its end. Staging
// loads the partial first and last 16 B word bytewise: no byte outside
// [ptr, ptr + len) is read.
//
// Output. Hits go through an LDS counter into an LDS list, then to the tile's
// slice of a global list (cap entries, unordered) with the true count beside
// it. A tile whose count exceeds cap is recomputed by the engine on the host,
// so the result never depends on cap.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/cdc_core.hpp"
#include "modelx/device_abi.hpp"

namespace {

namespace cdc = modelx::cdc;

constexpr int kThreads = 256;
constexpr uint32_t kTile = modelx::abi::kCdcTileBytes;
constexpr uint32_t kRun = kTile / kThreads;            // bytes a lane owns
constexpr uint32_t kHalo = cdc::kWindow;               // staged before the tile
constexpr uint32_t kLogical = kTile + kHalo;           // staged bytes
constexpr uint32_t kRunDwords = kRun / 4;
constexpr uint32_t kDataDwords = kLogical / 4 + kLogical / kRun + 1;
constexpr uint32_t kMaxCap = modelx::abi::kCdcMaxTileCap;
constexpr uint32_t kStageVecs = kLogical / 16;

static_assert(kRun % 16 == 0 && kRun >= 64, "a 16 B vector must not straddle a pad dword");
static_assert(kTile <= 65536, "tile offsets are stored as uint16_t");
static_assert(kHalo == 32 && kHalo % 16 == 0, "the halo is two 16 B vectors");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// dword index of logical byte o (o % 4 == 0) in the padded LDS tile
__device__ __forceinline__ uint32_t padded_dword(uint32_t o) { return o / 4 + o / kRun; }

struct Hits {
  uint16_t* list;   // LDS, kMaxCap entries
  uint32_t* count;  // LDS
  uint32_t cap;
  __device__ __forceinline__ void emit(uint32_t tile_off) {
    uint32_t at = atomicAdd(count, 1u);
    if (at < cap) list[at] = static_cast<uint16_t>(tile_off);
  }
};

__global__ __launch_bounds__(kThreads) void cdc_candidates_kernel(
    const uint8_t* __restrict__ ptr, uint64_t len, uint32_t bits, uint32_t ntiles, uint32_t cap,
    uint32_t* __restrict__ counts, uint16_t* __restrict__ lists) {
  __shared__ uint32_t s_gear[256];
  __shared__ uint32_t s_data[kDataDwords];
  __shared__ uint16_t s_list[kMaxCap];
  __shared__ uint32_t s_count;

  const uint32_t t = threadIdx.x;
  s_gear[t] = cdc::gear(t);  // kThreads == 256
  const uint32_t thr = cdc::threshold(bits);
  const uintptr_t begin = reinterpret_cast<uintptr_t>(ptr);
  const uintptr_t end = begin + len;
  const uintptr_t grid0 = begin & ~static_cast<uintptr_t>(15);
  Hits hits{s_list, &s_count, cap};

  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // logical byte o of the staged tile is the byte at address org + o
    const uintptr_t org = grid0 + static_cast<uint64_t>(tile) * kTile - kHalo;
    // valid logical bytes are [lo, hi)
    const uint32_t lo = begin > org ? static_cast<uint32_t>(begin - org) : 0u;
    const uint32_t hi = end - org < kLogical ? static_cast<uint32_t>(end - org) : kLogical;
    if (t == 0) s_count = 0;

    // ---- stage [org, org + kLogical) into the padded LDS tile ----
    if (lo == 0 && hi == kLogical) {
      const u32x4* vs = reinterpret_cast<const u32x4*>(org);
      constexpr uint32_t kFull = kStageVecs / kThreads;  // trips with every lane loading
#pragma unroll 4
      for (uint32_t i = 0; i < kFull; i++) {
        uint32_t v = i * kThreads + t;
        u32x4 x = vs[v];
        uint32_t* d = s_data + padded_dword(16 * v);
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
      }
      uint32_t v = kFull * kThreads + t;
      if (v < kStageVecs) {
        u32x4 x = vs[v];
        uint32_t* d = s_data + padded_dword(16 * v);
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
      }
    } else {
      for (uint32_t v = t; v < kStageVecs; v += kThreads) {
        uint32_t o = 16 * v;
        if (o + 16 <= lo || o >= hi) continue;  // nothing valid: never read below
        u32x4 x;
        if (o >= lo && o + 16 <= hi) {
          x = *reinterpret_cast<const u32x4*>(org + o);
        } else {
          uint32_t w[4] = {0, 0, 0, 0};
          for (uint32_t k = 0; k < 16; k++)
            if (o + k >= lo && o + k < hi)
              w[k / 4] |= static_cast<uint32_t>(*reinterpret_cast<const uint8_t*>(org + o + k))
                          << (8 * (k % 4));
          x.x = w[0]; x.y = w[1]; x.z = w[2]; x.w = w[3];
        }
        uint32_t* d = s_data + padded_dword(o);
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
      }
    }
    __syncthreads();

    // ---- roll: lane t warms up on [t*kRun, t*kRun + 32), owns the kRun after ----
    const uint32_t run0 = t * kRun;
    if (run0 >= lo && run0 + kHalo + kRun <= hi) {
      const uint32_t* w = s_data + t * (kRunDwords + 1);
      uint32_t h = 0;
#pragma unroll
      for (uint32_t j = 0; j < kHalo / 4; j++) {
        uint32_t d = w[j];
        h = cdc::roll(h, s_gear[d & 0xffu]);
        h = cdc::roll(h, s_gear[(d >> 8) & 0xffu]);
        h = cdc::roll(h, s_gear[(d >> 16) & 0xffu]);
        h = cdc::roll(h, s_gear[d >> 24]);
      }
#pragma unroll 8
      for (uint32_t j = kHalo / 4; j < kHalo / 4 + kRunDwords; j++) {
        uint32_t d = w[j + (j >= kRunDwords ? 1u : 0u)];  // past the pad dword
        uint32_t h0 = cdc::roll(h, s_gear[d & 0xffu]);
        uint32_t h1 = cdc::roll(h0, s_gear[(d >> 8) & 0xffu]);
        uint32_t h2 = cdc::roll(h1, s_gear[(d >> 16) & 0xffu]);
        uint32_t h3 = cdc::roll(h2, s_gear[d >> 24]);
        h = h3;
        uint32_t m01 = h0 < h1 ? h0 : h1, m23 = h2 < h3 ? h2 : h3;
        if ((m01 < m23 ? m01 : m23) < thr) {
          uint32_t off = run0 + 4 * j - kHalo;  // tile offset of the dword's first byte
          if (h0 < thr) hits.emit(off);
          if (h1 < thr) hits.emit(off + 1);
          if (h2 < thr) hits.emit(off + 2);
          if (h3 < thr) hits.emit(off + 3);
        }
      }
    } else {
      const uint8_t* bytes = reinterpret_cast<const uint8_t*>(s_data);
      uint32_t o = run0 > lo ? run0 : lo;
      uint32_t stop = run0 + kHalo + kRun < hi ? run0 + kHalo + kRun : hi;
      uint32_t h = 0;
      for (; o < stop; o++) {
        h = cdc::roll(h, s_gear[bytes[4 * padded_dword(o & ~3u) + (o & 3u)]]);
        if (h < thr && o >= run0 + kHalo) hits.emit(o - kHalo);
      }
    }
    __syncthreads();

    // ---- publish the tile's hits ----
    uint32_t n = s_count;
    uint32_t keep = n < cap ? n : cap;
    uint16_t* out = lists + static_cast<uint64_t>(tile) * cap;
    for (uint32_t i = t; i < keep; i += kThreads) out[i] = s_list[i];
    if (t == 0) counts[tile] = n;
    __syncthreads();  // s_count, s_list and s_data are reused by the next tile
  }
}

}  // namespace

extern "C" {

hipError_t modelx_cdc_candidates(const void* ptr, uint64_t len, uint32_t bits, uint32_t ntiles,
                                 uint32_t cap, uint32_t* counts_dev, uint16_t* lists_dev,
                                 hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  if (!cdc::valid_bits(bits) || cap == 0 || cap > kMaxCap) return hipErrorInvalidValue;
  if (ntiles != modelx::abi::cdc_tile_count(reinterpret_cast<uintptr_t>(ptr), len))
    return hipErrorInvalidValue;
  // grid-stride: a few resident workgroups per CU cover any size in one launch
  uint32_t blocks = ntiles < modelx::abi::kCdcMaxBlocks ? ntiles : modelx::abi::kCdcMaxBlocks;
  hipLaunchKernelGGL(cdc_candidates_kernel, dim3(blocks), dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(ptr), len, bits, ntiles, cap, counts_dev,
                     lists_dev);
  return hipGetLastError();
}

}  // extern "C"
