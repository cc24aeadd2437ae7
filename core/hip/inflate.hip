// CDNA4 inflate kernels (gfx950): one gzip member in HBM decoded span by
// span. What a candidate, a span and the chain are, the bit reader, the decode
// tables and the block decoder itself are modelx/inflate_core.hpp's, shared
// with the host model; this file is how the work is split and how the bytes
// move.
//
// inflate_scan_kernel<kWrite>: one workgroup of 256 threads per 16 KiB tile
// on the 16 B grid of the source, four rows of 4 KiB. A thread loads one 16 B
// word and the dword before it and tests the sixteen four-byte windows that
// end in its word against 00 00 FF FF, so a marker that straddles two tiles
// belongs to the tile it ends in. The counting instance leaves one count per
// tile; the host prefix-sums them. The writing instance ranks a hit by the
// counts of the lanes below it (ballot of the lanes that hit, popcount of
// their masks), the counts of the waves below it (four LDS words) and the
// rows before it, and stores the positions in ascending order: a sorted
// uint32 list, no atomics on global memory. Entry 0 is the first deflate byte.
//
// inflate_spans_kernel<kEmit>: one wave per span, four spans per workgroup,
// no workgroup barrier: waves share nothing but the launch. The wave is the
// group of inflate::decode_span. Lane 0 owns the bit reader and decodes; the
// 64 lanes refill the ring, build the tables (one code length per lane for the
// sorted list, sixteen lookup entries per lane) and take each batch of up to
// 64 tokens: an inclusive scan of the token lengths gives every token its
// output offset and every match its distance check. The measuring instance
// writes nothing but the span record. The emitting instance stores the
// literals from their lanes, then copies each match in order with all lanes,
// out[p + k] = out[p - dist + k % dist], from the wave's own earlier output in
// global memory, a workgroup-scope fence between a token's stores and the
// loads that may read them. Nonempty stored blocks are copied by the wave
// with the window of copy_shifted.hpp, whatever the phases. It never writes
// outside [out_offset, out_offset + out_bytes) of its span and never reads
// before out_offset.
//
// LDS of a wave (4896 B; 19.1 KiB a workgroup, eight workgroups or 32 waves
// to a CU's 160 KiB, so LDS does not limit occupancy):
//   ll      2 KiB    1024 lit/len lookup entries (10 bits)
//   d       512 B    256 distance entries (8 bits); the code length code's
//   sorted  640 B    symbols in canonical order, both alphabets
//   count   64 B     codes per length, both alphabets
//   len     320 B    the code lengths lane 0 read
//   tok     256 B    a batch of tokens
//   ctl     32 B     lane 0 -> wave
//   ring    1 KiB    stored bytes, indexed by address mod 1 KiB, refilled in
//                    halves by all lanes with 8 B loads when fewer than 512
//                    bytes lie ahead of the reader, so the decoding lane
//                    never loads from HBM
//
// crc32_pieces_kernel: one workgroup per 32 KiB piece of the output, staged
// into LDS with 16 B loads; every thread folds 132 bytes, advances its raw
// value over the bytes behind it and the workgroup XORs them (the scheme of
// deflate.hip). The host joins the pieces with mul_xn.
//
// Every loop is bounded by the stream end, the span's measured size, the
// alphabet size or kSpanMaxCoded.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/copy_shifted.hpp"
#include "modelx/device_abi.hpp"
#include "modelx/inflate_core.hpp"

namespace {

namespace df = modelx::deflate;
namespace inf = modelx::inflate;
using modelx::abi::kInflateScanTile;
using modelx::devcopy::PackWindow;
using modelx::devcopy::u32x4;

constexpr uint32_t kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr uint32_t kRing = 1024;
constexpr uint32_t kScanRow = kThreads * 16;
static_assert(kInflateScanTile % kScanRow == 0, "a tile is whole rows");
static_assert(inf::kBatch == kWave, "one token per lane");

struct WaveLds {
  inf::Work w;
  alignas(16) uint8_t ring[kRing];
};
static_assert(sizeof(WaveLds) * kWaves * 8 <= 160u << 10, "32 waves to a CU");

__device__ const df::crc32::PowTable kPow = df::crc32::make_pow_table();

// ---- scan -------------------------------------------------------------------

// base16 is the source's first byte moved down to its 16 B word, `phase` the
// bytes between; a_end is phase + size rounded up to 16. Candidates are the
// positions i of (first + 4 .. limit] with the marker in bytes[i-4..i).
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void inflate_scan_kernel(
    const uint8_t* __restrict__ base16, uint32_t phase, uint64_t a_end, uint64_t first,
    uint64_t limit, uint32_t* __restrict__ counts, const uint32_t* __restrict__ tile_base,
    uint32_t* __restrict__ cand, uint32_t ncand) {
  __shared__ uint32_t wave_cnt[kWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t run = kWrite ? tile_base[blockIdx.x] : 0;
  for (uint32_t row = 0; row < kInflateScanTile / kScanRow; row++) {
    const uint64_t a = static_cast<uint64_t>(blockIdx.x) * kInflateScanTile + row * kScanRow + tid * 16;
    uint32_t d[5] = {0, 0, 0, 0, 0};
    if (a < a_end) {
      u32x4 v = *reinterpret_cast<const u32x4*>(base16 + a);
      d[1] = v.x, d[2] = v.y, d[3] = v.z, d[4] = v.w;
      if (a) d[0] = *reinterpret_cast<const uint32_t*>(base16 + a - 4);
    }
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t e = 0; e < 16; e++) {  // the window that ends in byte e of the word
      const uint32_t j = e >> 2, s = e & 3u;
      const uint32_t win = s == 3 ? d[j + 1] : __builtin_amdgcn_alignbyte(d[j + 1], d[j], s + 1);
      const uint64_t i = a + e + 1 - phase;  // wraps only where the test below fails
      if (win == inf::kMarker && a + e + 1 >= phase + first + 4 && i <= limit) mask |= 1u << e;
    }
    const uint32_t cnt = __popc(mask);
    uint32_t below = 0, wave_total = 0;
    for (uint64_t hit = __ballot(mask != 0); hit; hit &= hit - 1) {
      const int l = __ffsll(static_cast<unsigned long long>(hit)) - 1;
      const uint32_t c = __shfl(cnt, l, kWave);
      if (lane > static_cast<uint32_t>(l)) below += c;
      wave_total += c;
    }
    if (lane == 0) wave_cnt[wave] = wave_total;
    __syncthreads();
    uint32_t before = 0, row_total = 0;
    for (uint32_t v = 0; v < kWaves; v++) {
      const uint32_t c = wave_cnt[v];
      if (v < wave) before += c;
      row_total += c;
    }
    if (kWrite) {
      for (uint32_t at = run + before + below; mask; mask &= mask - 1, at++)
        if (at < ncand) cand[at] = static_cast<uint32_t>(a + __ffs(mask) - phase);
    }
    run += row_total;
    __syncthreads();  // wave_cnt is read before the next row writes it
  }
  if (!kWrite && tid == 0) counts[blockIdx.x] = run;
  if (kWrite && blockIdx.x == 0 && tid == 0) cand[0] = static_cast<uint32_t>(first);
}

// ---- spans ------------------------------------------------------------------

// The wave as the group of inflate::decode_span.
struct WaveCtx {
  static constexpr uint32_t width = kWave;
  uint32_t tid;
  const uint8_t* base16;
  uint32_t phase;
  uint64_t a_end, limit;
  uint8_t* ring;
  uint64_t hi;  // the ring holds addresses [hi - kRing, hi) of base16
  __device__ __forceinline__ void sync() const { __threadfence_block(); }
  __device__ __forceinline__ uint8_t byte(uint64_t pos) const {
    return ring[(phase + pos) & (kRing - 1)];
  }
  __device__ __forceinline__ uint64_t refill(uint64_t pos) {
    const uint64_t a = phase + pos;
    if (a >= hi) hi = a & ~15ull;  // the first fill, or the reader jumped a stored block
    while (hi <= a + kRing / 2) {  // the half this overwrites lies behind the reader
      const uint64_t w = hi + 8 * tid;
      uint2 v = make_uint2(0, 0);
      if ((w & ~15ull) < a_end) v = *reinterpret_cast<const uint2*>(base16 + w);
      *reinterpret_cast<uint2*>(ring + (w & (kRing - 1))) = v;
      hi += kRing / 2;
    }
    sync();
    return hi >= phase + limit ? ~0ull : hi - phase;
  }
};

template <int Q>
__device__ __forceinline__ void wave_body_shifted(const uint32_t* __restrict__ ws,
                                                  u32x4* __restrict__ vd, uint32_t nvec,
                                                  uint32_t b, uint32_t lane) {
  for (uint32_t k = lane; k < nvec; k += kWave) {
    PackWindow<Q> win;
    win.load(ws + 4 * k);
    vd[k] = win.shifted(b);
  }
}

// copy_to_aligned_grid of copy_shifted.hpp at the width of a wave: the
// destination decides the 16 B grid, the shifted body reads the aligned words
// that hold a source byte and no others.
__device__ __forceinline__ void wave_copy(const uint8_t* __restrict__ src,
                                          uint8_t* __restrict__ dst, uint32_t len, uint32_t lane) {
  uint32_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  if (head > len) head = len;
  if (lane < head) dst[lane] = src[lane];
  const uint32_t nvec = (len - head) / 16;
  if (nvec) {
    u32x4* vd = reinterpret_cast<u32x4*>(dst + head);
    const uintptr_t s = reinterpret_cast<uintptr_t>(src + head);
    const uint32_t phase = static_cast<uint32_t>(s & 15u), b = phase & 3u;
    if (phase == 0) {
      const u32x4* vs = reinterpret_cast<const u32x4*>(s);
      for (uint32_t k = lane; k < nvec; k += kWave) vd[k] = vs[k];
    } else {
      const uint32_t* ws = reinterpret_cast<const uint32_t*>(s - phase);
      switch (phase >> 2) {  // uniform across the wave
        case 0: wave_body_shifted<0>(ws, vd, nvec, b, lane); break;
        case 1: wave_body_shifted<1>(ws, vd, nvec, b, lane); break;
        case 2: wave_body_shifted<2>(ws, vd, nvec, b, lane); break;
        default: wave_body_shifted<3>(ws, vd, nvec, b, lane); break;
      }
    }
  }
  const uint32_t k = head + nvec * 16 + lane;
  if (k < len) dst[k] = src[k];
}

template <bool kEmit>
struct WaveSink {
  const uint8_t* src;
  uint8_t* dst;   // the span's first output byte
  uint64_t cap;   // the span's measured size

  __device__ __forceinline__ uint32_t stored(WaveCtx& cx, uint64_t at, uint32_t n, uint64_t out) {
    if (kEmit) {
      if (out + n > cap) return inf::kCorrupt;
      wave_copy(src + at, dst + out, n, cx.tid);
    }
    return inf::kOk;
  }

  __device__ __forceinline__ uint32_t tokens(WaveCtx& cx, const uint32_t* tok, uint32_t n,
                                             uint64_t* out) {
    const uint32_t lane = cx.tid;
    const uint32_t t = lane < n ? tok[lane] : 0;
    const bool match = (t & df::kTokMatch) != 0;
    const uint32_t len = lane < n ? (match ? ((t >> 16) & 0xFFu) + 3 : 1) : 0;
    const uint32_t dist = (t & 0x7FFFu) + 1;
    uint32_t inc = len;
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
      const uint32_t v = __shfl_up(inc, d, kWave);
      if (lane >= d) inc += v;
    }
    const uint32_t total = __shfl(inc, kWave - 1, kWave);
    const uint32_t before = inc - len;  // of this batch
    const uint64_t base = *out;
    uint32_t status = inf::kOk;
    if (__ballot(match && dist > base + before)) status = inf::kDependent;
    else if (kEmit && base + total > cap) status = inf::kCorrupt;
    if (kEmit && !status) {
      uint8_t* o = dst + base;
      if (lane < n && !match) o[before] = static_cast<uint8_t>(t);
      for (uint64_t mm = __ballot(match); mm; mm &= mm - 1) {
        const int l = __ffsll(static_cast<unsigned long long>(mm)) - 1;
        const uint32_t p = __shfl(before, l, kWave), ml = __shfl(len, l, kWave),
                       md = __shfl(dist, l, kWave);
        __threadfence_block();  // the bytes before p are stored before they are loaded
        const uint8_t* from = o + p - md;  // >= dst: md <= base + p
        for (uint32_t k = lane; k < ml; k += kWave) o[p + k] = from[md >= ml ? k : k % md];
      }
    }
    if (!status) *out = base + total;
    cx.sync();  // tok is read before lane 0 writes the next batch
    return status;
  }
};

// kEmit == false: span i starts at cand[i] and leaves recs[i]. kEmit == true:
// span i is plan[i], written at dst + out_offset; a span that does not decode
// to exactly out_bytes sets *err.
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void inflate_spans_kernel(
    const uint8_t* __restrict__ src, uint64_t size, uint64_t limit,
    const uint32_t* __restrict__ cand, const inf::PlanSpan* __restrict__ plan, uint32_t nspans,
    inf::SpanRec* __restrict__ recs, uint8_t* dst, uint32_t* __restrict__ err) {
  __shared__ WaveLds lds[kWaves];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t span = blockIdx.x * kWaves + wave;
  if (span >= nspans) return;  // a whole wave: no barrier follows
  WaveLds& my = lds[wave];
  const uint32_t phase = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src) & 15u);
  WaveCtx cx{lane, src - phase, phase, (phase + size + 15) & ~15ull, limit, my.ring, 0};
  uint64_t start, out_offset = 0, cap = 0;
  if (kEmit) start = plan[span].in_start, out_offset = plan[span].out_offset, cap = plan[span].out_bytes;
  else start = cand[span];
  inf::SpanRec rec{0, 0, inf::kCorrupt};
  if (start <= limit) {
    WaveSink<kEmit> sink{src, dst + out_offset, cap};
    rec = inf::decode_span(cx, my.w, sink, start, limit);
  }
  if (lane == 0) {
    if (kEmit) {
      if ((rec.status & inf::kStatusMask) || rec.out_bytes != cap) *err = 1;
    } else {
      recs[span] = rec;
    }
  }
}

// ---- crc --------------------------------------------------------------------

constexpr uint32_t kCrcPiece = modelx::abi::kInflateCrcPiece;
constexpr uint32_t kCrcFold = 132;  // 33 dwords: the lanes of a wave start in 32 banks
static_assert(kCrcFold * kThreads >= kCrcPiece, "the folds cover a piece");

struct CrcLds {
  alignas(16) uint8_t buf[kCrcPiece + 32];
  uint32_t tab[256];
  uint32_t pow[16];
  uint32_t crc;
};

__global__ __launch_bounds__(kThreads) void crc32_pieces_kernel(const uint8_t* __restrict__ data,
                                                                uint64_t total,
                                                                uint32_t* __restrict__ out) {
  __shared__ CrcLds lds;
  const uint32_t tid = threadIdx.x;
  const uint64_t off = static_cast<uint64_t>(blockIdx.x) * kCrcPiece;
  const uint32_t n = static_cast<uint32_t>(total - off < kCrcPiece ? total - off : kCrcPiece);
  const uint8_t* p = data + off;
  const uint32_t ph = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p) & 15u);
  const u32x4* words = reinterpret_cast<const u32x4*>(p - ph);
  for (uint32_t k = tid; k < (ph + n + 15) / 16; k += kThreads)
    reinterpret_cast<u32x4*>(lds.buf)[k] = words[k];
  lds.tab[tid] = df::crc32::table_entry(tid);
  if (tid < 16) lds.pow[tid] = kPow.v[tid];
  if (tid == 0) lds.crc = 0;
  __syncthreads();
  const uint32_t a = tid * kCrcFold < n ? tid * kCrcFold : n;
  const uint32_t b = a + kCrcFold < n ? a + kCrcFold : n;
  if (a < b) {
    uint32_t s = 0;
    for (uint32_t i = a; i < b; i++) s = lds.tab[(s ^ lds.buf[ph + i]) & 0xFFu] ^ (s >> 8);
    if (s) atomicXor(&lds.crc, df::crc32::mul_xn(s, n - b, lds.pow));
  }
  __syncthreads();
  if (tid == 0) out[blockIdx.x] = lds.crc;
}

}  // namespace

extern "C" hipError_t modelx_inflate_scan(const void* src, uint64_t size, uint64_t first,
                                          uint64_t limit, uint32_t ntiles, uint32_t* counts_dev,
                                          const uint32_t* tile_base_dev, uint32_t* cand_dev,
                                          uint32_t ncand, hipStream_t stream) {
  if (!src || first > limit || limit > size || size >= (1ull << 32) ||
      ntiles != modelx::abi::inflate_scan_tiles(reinterpret_cast<uintptr_t>(src), size))
    return hipErrorInvalidValue;
  const uint32_t phase = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src) & 15u);
  const uint8_t* base16 = static_cast<const uint8_t*>(src) - phase;
  const uint64_t a_end = (phase + size + 15) & ~15ull;
  if (cand_dev)
    hipLaunchKernelGGL(inflate_scan_kernel<true>, dim3(ntiles), dim3(kThreads), 0, stream, base16,
                       phase, a_end, first, limit, nullptr, tile_base_dev, cand_dev, ncand);
  else
    hipLaunchKernelGGL(inflate_scan_kernel<false>, dim3(ntiles), dim3(kThreads), 0, stream, base16,
                       phase, a_end, first, limit, counts_dev, nullptr, nullptr, 0u);
  return hipGetLastError();
}

extern "C" hipError_t modelx_inflate_measure(const void* src, uint64_t size, uint64_t limit,
                                             const uint32_t* cand_dev, uint32_t ncand,
                                             modelx::inflate::SpanRec* recs_dev,
                                             hipStream_t stream) {
  if (!src || limit > size || size >= (1ull << 32) || !ncand) return hipErrorInvalidValue;
  hipLaunchKernelGGL(inflate_spans_kernel<false>, dim3((ncand + kWaves - 1) / kWaves),
                     dim3(kThreads), 0, stream, static_cast<const uint8_t*>(src), size, limit,
                     cand_dev, nullptr, ncand, recs_dev, nullptr, nullptr);
  return hipGetLastError();
}

extern "C" hipError_t modelx_inflate_emit(const void* src, uint64_t size, uint64_t limit,
                                          const modelx::inflate::PlanSpan* plan_dev,
                                          uint32_t nspans, void* dst, uint32_t* err_dev,
                                          hipStream_t stream) {
  if (!src || !dst || limit > size || size >= (1ull << 32) || !nspans) return hipErrorInvalidValue;
  hipLaunchKernelGGL(inflate_spans_kernel<true>, dim3((nspans + kWaves - 1) / kWaves),
                     dim3(kThreads), 0, stream, static_cast<const uint8_t*>(src), size, limit,
                     nullptr, plan_dev, nspans, nullptr, static_cast<uint8_t*>(dst), err_dev);
  return hipGetLastError();
}

extern "C" hipError_t modelx_crc32_pieces(const void* data, uint64_t total, uint32_t* out_dev,
                                          hipStream_t stream) {
  if (!total) return hipSuccess;
  if (!data) return hipErrorInvalidValue;
  const uint64_t pieces = (total + kCrcPiece - 1) / kCrcPiece;
  if (pieces > 0x7FFFFFFFu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(crc32_pieces_kernel, dim3(static_cast<uint32_t>(pieces)), dim3(kThreads), 0,
                     stream, static_cast<const uint8_t*>(data), total, out_dev);
  return hipGetLastError();
}
