// CDNA4 CRC-32C kernels (gfx950): the checksum of many (device address,
// length) ranges in one launch, one 32-bit value per range. The arithmetic is
// modelx/crc32c_core.hpp's, shared with the host; this file is how the work
// is split and how the bytes move.
//
// A CRC register started at 0 is linear over GF(2) in the message, so a range
// is cut into pieces that are folded independently and joined afterwards by
// "advance through n zero bytes", a multiplication by x^(8n) mod P.
//
// Step 1, crc32c_segments_kernel. A range is its unaligned head (< 16 B), then
// an aligned body cut into segments of kSegmentBytes. One wave owns one
// segment; the grid is capped and strides over the flattened (range, segment)
// index, found by a wave-uniform binary search over the ranges' first-segment
// numbers. In each trip the 64 lanes load one 16 B word each
// (global_load_dwordx4), 1 KiB contiguous per wave, so the hot loop is
// coalesced without staging through LDS. A lane keeps FOUR raw registers, one
// per dword of its load, and for each new dword computes s = A(s) ^ w, where
// A is "advance through 1024 zero bytes": every dword position of a lane
// recurs at the same 1 KiB stride, so one set of four 256-entry tables serves
// all four chains (four LDS reads per dword, the cost of slicing-by-4), and
// the four chains are independent, which hides LDS latency. Two registers
// with two table sets (strides 8 and 1016) would halve the state and double
// the LDS footprint for no fewer lookups. At the end of the segment a lane
// folds its four registers into one (they are the raw CRC of a 16 B word),
// multiplies it by x^(8*16*(63-lane)), the bytes after its last word, taken
// from a 64-entry table, and the wave XOR-reduces with __shfl_xor. The rows
// after the last full 1 KiB trip go the same way, one 16 B piece per lane, and
// the last < 16 bytes bytewise.
//
// Choices, and why:
//  - Segment 128 KiB: a lane's end-of-segment work (two 32-step
//    multiplications, sixteen byte steps) is about 5% of its 512 hot-loop
//    dwords, and 1 GiB is still 8192 waves, 64 MiB still 512.
//  - One 16 B word per lane per trip, the loop unrolled four times so four
//    loads are in flight per lane.
//  - Tables not replicated in LDS: the indexes are pseudo-random bytes, so a
//    replica changes which address a lane reads, not how the 64 reads spread
//    over the banks. 4 KiB of stride tables + 1 KiB byte table + 256 B of lane
//    multipliers per workgroup, copied from constant data built at compile
//    time.
//  - No matrix instructions: the work is integer, LDS lookups and xors.
//
// Step 2, crc32c_finish_kernel, one workgroup per range (grid-strided): the
// head bytes start a conventional register at 0xFFFFFFFF, which carries the
// initial-value term mul_xn(0xFFFFFFFF, len) through everything that follows;
// each thread Horner-folds a block of consecutive full segments with the
// constant x^(8*kSegmentBytes), advances its partial over the segments that
// follow, the workgroup XORs the partials, and the last (short) segment and
// the final xor are applied. Nothing but the 32-bit results goes back.
//
// No byte outside [ptr, ptr + len) of a range is read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/crc32c_core.hpp"
#include "modelx/device_abi.hpp"

namespace {

namespace cc = modelx::crc32c;
using modelx::abi::CrcRange;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kMaxBlocks = 2048;  // 8 per CU; the rest grid-strides
constexpr uint64_t kSeg = cc::kSegmentBytes;
constexpr uint64_t kRow = cc::kRowBytes;
static_assert(kSeg % kRow == 0, "a segment is whole rows");
static_assert(kSeg == modelx::abi::kCrc32cSegmentBytes, "ABI constant");

// One 16 B load in the IR (see the note in tar.hip). The ranges arrive as
// integers, so the loads say themselves that they are global: a flat load
// would also count against the LDS wait counter the hot loop lives on.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4* GlobalVec;
typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;

// x^(8*16*m) for m = 0..63: lane multipliers at the end of a segment.
struct LaneMul {
  uint32_t v[64];
};
constexpr LaneMul make_lane_mul() {
  LaneMul lm{};
  for (int m = 0; m < 64; m++) lm.v[m] = cc::xpow8n(16u * m);
  return lm;
}

__device__ const cc::StrideTables kStrideTables = cc::make_stride_tables(kRow);
__device__ const cc::ByteTable kByteTable = cc::make_byte_table();
__device__ const LaneMul kLaneMul = make_lane_mul();
__device__ const cc::PowTable kPow = cc::make_pow_table();
constexpr uint32_t kXSeg = cc::xpow8n(kSeg);

struct Lds {
  uint32_t adv[4][256];  // stride tables
  uint32_t byte[256];
  uint32_t lane_mul[64];
};

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
  return v;
}

// s advanced through kRow zero bytes.
__device__ __forceinline__ uint32_t advance_row(const Lds& l, uint32_t s) {
  return l.adv[0][s & 0xFFu] ^ l.adv[1][(s >> 8) & 0xFFu] ^ l.adv[2][(s >> 16) & 0xFFu] ^
         l.adv[3][s >> 24];
}

__device__ __forceinline__ uint32_t advance4(const Lds& l, uint32_t s) {
#pragma unroll
  for (int i = 0; i < 4; i++) s = l.byte[s & 0xFFu] ^ (s >> 8);
  return s;
}

// Raw CRC of the 16 bytes whose dwords are w (equally: four registers at
// consecutive dword positions folded into one, at the end of the last).
__device__ __forceinline__ uint32_t fold16(const Lds& l, u32x4 w) {
  uint32_t s = advance4(l, w.x) ^ w.y;
  s = advance4(l, s) ^ w.z;
  s = advance4(l, s) ^ w.w;
  return advance4(l, s);
}

// The range that owns flattened segment `seg`: the last one whose seg_base is
// <= seg and that has a segment. Ranges without segments share their
// successor's seg_base and sort before it, so "last with seg_base <= seg" is
// the owner.
__device__ __forceinline__ uint32_t owner_of(const CrcRange* ranges, uint32_t nranges,
                                             uint32_t seg) {
  uint32_t lo = 0, hi = nranges;  // answer in [lo, hi)
  while (hi - lo > 1) {
    uint32_t mid = lo + (hi - lo) / 2;
    if (ranges[mid].seg_base <= seg) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void crc32c_segments_kernel(
    const CrcRange* __restrict__ ranges, uint32_t nranges, uint32_t total_segments,
    uint32_t* __restrict__ seg_vals) {
  __shared__ Lds lds;
  for (int i = threadIdx.x; i < 4 * 256; i += kThreads)
    lds.adv[i >> 8][i & 255] = kStrideTables.t[i >> 8][i & 255];
  lds.byte[threadIdx.x] = kByteTable.t[threadIdx.x];
  if (threadIdx.x < 64) lds.lane_mul[threadIdx.x] = kLaneMul.v[threadIdx.x];
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t seg = blockIdx.x * kWaves + wave; seg < total_segments;
       seg += gridDim.x * kWaves) {
    const CrcRange r = ranges[owner_of(ranges, nranges, seg)];
    const uint64_t head = cc::head_bytes(r.ptr, r.len);
    const uint64_t off = static_cast<uint64_t>(seg - r.seg_base) * kSeg;  // within the body
    const uint64_t body = r.len - head;
    const uint64_t seg_len = body - off < kSeg ? body - off : kSeg;
    const uint64_t base = r.ptr + head + off;  // 16 B aligned

    // full rows: four chains per lane at a 1 KiB stride
    const uint32_t trips = static_cast<uint32_t>(seg_len / kRow);
    GlobalVec p = (GlobalVec)base + lane;
    u32x4 s = {0, 0, 0, 0};
#pragma unroll 4
    for (uint32_t t = 0; t < trips; t++) {
      u32x4 w = p[static_cast<size_t>(t) * 64];
      s.x = advance_row(lds, s.x) ^ w.x;
      s.y = advance_row(lds, s.y) ^ w.y;
      s.z = advance_row(lds, s.z) ^ w.z;
      s.w = advance_row(lds, s.w) ^ w.w;
    }
    // a lane's last word is followed by the words of lanes lane+1..63
    uint32_t v = cc::gf_mul(fold16(lds, s), lds.lane_mul[63u - lane]);

    // the rows that remain: q whole 16 B pieces, one per lane, then < 16 bytes
    const uint32_t tail = static_cast<uint32_t>(seg_len % kRow);
    const uint32_t q = tail / 16u;
    const uint64_t tp = base + static_cast<uint64_t>(trips) * kRow;
    if (q) {
      v = cc::gf_mul(v, lds.lane_mul[q]);
      if (lane < q) {
        u32x4 w = ((GlobalVec)tp)[lane];
        v ^= cc::gf_mul(fold16(lds, w), lds.lane_mul[q - 1u - lane]);
      }
    }
    v = wave_xor(v);
    for (uint32_t i = q * 16u; i < tail; i++) v = lds.byte[(v ^ ((GlobalBytes)tp)[i]) & 0xFFu] ^ (v >> 8);
    if (lane == 0) seg_vals[seg] = v;
  }
}

__global__ __launch_bounds__(kThreads) void crc32c_finish_kernel(
    const CrcRange* __restrict__ ranges, uint32_t nranges, const uint32_t* __restrict__ seg_vals,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t partial[kWaves];
  for (uint32_t ri = blockIdx.x; ri < nranges; ri += gridDim.x) {
    const CrcRange r = ranges[ri];
    const uint64_t head = cc::head_bytes(r.ptr, r.len);
    const uint64_t nseg = cc::segment_count(r.ptr, r.len);
    const uint64_t full = nseg ? nseg - 1 : 0;  // segments before the last, all kSeg long
    const uint32_t* sv = seg_vals + r.seg_base;

    // thread 0 starts from the head's conventional register; its block of
    // segments is the first, so the register is advanced over all that follows
    uint32_t s = 0;
    if (threadIdx.x == 0) {
      s = cc::kInit;
      GlobalBytes hp = (GlobalBytes)r.ptr;
      for (uint64_t i = 0; i < head; i++) s = cc::update_byte(s, hp[i]);
    }
    const uint64_t per = (full + kThreads - 1) / kThreads;
    uint64_t j0 = threadIdx.x * per < full ? threadIdx.x * per : full;
    uint64_t j1 = j0 + per < full ? j0 + per : full;
    for (uint64_t j = j0; j < j1; j++) s = cc::gf_mul(s, kXSeg) ^ sv[j];
    // over the full segments after this thread's block
    if (s) s = cc::mul_xn(s, full - j1, kPow.v + 17);
    s = wave_xor(s);
    __syncthreads();  // the previous range's partials have been read
    if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      s = 0;
      for (int w = 0; w < kWaves; w++) s ^= partial[w];
      if (nseg) {
        uint64_t last_len = r.len - head - full * kSeg;
        s = cc::mul_xn(s, last_len, kPow.v) ^ sv[full];
      }
      out[ri] = s ^ cc::kInit;
    }
  }
}

}  // namespace

static_assert(modelx::crc32c::kSegmentBytes == (1u << 17), "kPow.v + 17 is x^(8*kSegmentBytes)");

extern "C" hipError_t modelx_crc32c_ranges(const CrcRange* ranges_dev, uint32_t nranges,
                                           uint32_t total_segments, uint32_t* seg_vals_dev,
                                           uint32_t* out_dev, hipStream_t stream) {
  if (nranges == 0) return hipSuccess;
  if (total_segments) {
    uint32_t want = (total_segments + kWaves - 1) / kWaves;
    uint32_t blocks = want < kMaxBlocks ? want : kMaxBlocks;
    hipLaunchKernelGGL(crc32c_segments_kernel, dim3(blocks), dim3(kThreads), 0, stream,
                       ranges_dev, nranges, total_segments, seg_vals_dev);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  uint32_t blocks = nranges < kMaxBlocks ? nranges : kMaxBlocks;
  hipLaunchKernelGGL(crc32c_finish_kernel, dim3(blocks), dim3(kThreads), 0, stream, ranges_dev,
                     nranges, seg_vals_dev, out_dev);
  return hipGetLastError();
}
