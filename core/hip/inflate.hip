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
// Streams without markers (inflate_core.hpp, "search") take four more kernels,
// each described where it stands: inflate_search_kernel (one workgroup per
// 64 KiB stride, one bit position per lane against a staged tile in LDS, the
// survivors confirmed by the wave as a group), inflate_compact_kernel (the
// sorted candidate list, ranked like the scan), inflate_search_spans_kernel
// (the span kernel with a symbolic ring in HBM as the measuring sink and a
// resolved window behind the emitting sink) and inflate_windows_kernel (one
// workgroup, the chain in order, two 32 KiB windows in LDS).
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

// ---- search -----------------------------------------------------------------

constexpr uint32_t kStride = modelx::abi::kInflateSearchStride;
constexpr uint32_t kTile = modelx::abi::kInflateSearchTile;
constexpr uint32_t kSeg = kTile / kWaves;  // a wave's bytes of a tile
constexpr uint32_t kSlack = 640;           // the longest dynamic header, 8 bytes of read-ahead
constexpr uint32_t kStaged = kTile + kSlack + 32;
constexpr uint32_t kWinMask = inf::kWindow - 1;
static_assert(kSeg % kWave == 0 && kSlack >= 576 + 16, "whole steps; a header fits the slack");

struct SearchLds {
  alignas(16) uint8_t buf[kStaged];
  inf::Work w[kWaves];
  uint64_t dyn[kWaves], sto[kWaves];
};
static_assert(sizeof(SearchLds) <= 32u << 10, "five workgroups to a CU");

// The staged bytes [a0, a0 + kStaged) of base16 as the stream; anything else
// reads as zero.
struct TileCtx {
  static constexpr uint32_t width = kWave;
  uint32_t tid;
  const uint8_t* buf;
  uint64_t a0;  // of base16, 16 B aligned
  uint32_t phase;
  __device__ __forceinline__ void sync() const { __threadfence_block(); }
  __device__ __forceinline__ uint8_t byte(uint64_t pos) const {
    const uint64_t i = phase + pos - a0;  // wraps below a0: the test fails
    return i < kStaged ? buf[i] : 0;
  }
};

struct GlobalBytes {
  const uint8_t* src;
  __device__ __forceinline__ uint8_t byte(uint64_t pos) const { return src[pos]; }
};

// One workgroup per stride, a tile at a time: 16 B loads stage the tile, the
// byte before it and the slack behind it; wave v owns bytes [v * kSeg, (v + 1)
// * kSeg) of the tile. Dynamic: 64 bit positions a step, one per lane
// (dynamic_plausible on LDS), the survivors confirmed in ballot order by the
// wave as a group until one holds. Stored: 64 byte positions a step, the hop
// straight from HBM. After a tile the workgroup takes the lowest hit of each
// kind and stops looking for that kind. slots[2 * (k - 1)] and the word after
// it get stride k's candidates in ascending order, kNoCand for none.
__global__ __launch_bounds__(kThreads) void inflate_search_kernel(
    const uint8_t* __restrict__ base16, uint32_t phase, uint64_t a_end, uint64_t first,
    uint64_t limit, uint64_t* __restrict__ slots) {
  __shared__ SearchLds lds;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t from = first + (static_cast<uint64_t>(blockIdx.x) + 1) * kStride;
  const uint64_t to = from + kStride < limit ? from + kStride : limit;
  uint64_t dyn = inf::kNoCand, sto = inf::kNoCand;
  for (uint64_t t0 = from; t0 < to && (dyn == inf::kNoCand || sto == inf::kNoCand); t0 += kTile) {
    const uint64_t a0 = (phase + t0 - 1) & ~15ull;
    for (uint32_t k = tid; k < kStaged / 16; k += kThreads) {
      u32x4 v = {0, 0, 0, 0};
      if (a0 + 16ull * k < a_end) v = *reinterpret_cast<const u32x4*>(base16 + a0 + 16ull * k);
      reinterpret_cast<u32x4*>(lds.buf)[k] = v;
    }
    __syncthreads();
    TileCtx cx{lane, lds.buf, a0, phase};
    const uint64_t seg = t0 + wave * kSeg;
    uint64_t hit = inf::kNoCand;
    if (dyn == inf::kNoCand)
      for (uint32_t step = 0; step < kSeg * 8 / kWave && hit == inf::kNoCand; step++) {
        const uint64_t bit = seg * 8 + step * kWave + lane;
        uint64_t live = __ballot(bit < to * 8 && inf::dynamic_plausible(cx, bit, limit));
        for (; live && hit == inf::kNoCand; live &= live - 1) {
          const uint64_t b = seg * 8 + step * kWave + __ffsll(static_cast<unsigned long long>(live)) - 1;
          if (inf::dynamic_confirm(cx, lds.w[wave], b, limit)) hit = inf::make_cand(b, false);
        }
      }
    if (lane == 0) lds.dyn[wave] = hit;
    hit = inf::kNoCand;
    if (sto == inf::kNoCand)
      for (uint32_t step = 0; step < kSeg / kWave && hit == inf::kNoCand; step++) {
        const uint64_t p = seg + step * kWave + lane;
        const bool ok = p < to && inf::stored_plausible(cx, p, limit) &&
                        inf::stored_confirm(GlobalBytes{base16 + phase}, p, limit);
        const uint64_t live = __ballot(ok);
        if (live)
          hit = inf::make_cand((seg + step * kWave + __ffsll(static_cast<unsigned long long>(live)) - 1) * 8, true);
      }
    if (lane == 0) lds.sto[wave] = hit;
    __syncthreads();
    for (uint32_t v = 0; v < kWaves; v++) {  // ascending positions: the first hit is the lowest
      if (dyn == inf::kNoCand) dyn = lds.dyn[v];
      if (sto == inf::kNoCand) sto = lds.sto[v];
    }
    __syncthreads();  // buf and the hits are read before the next tile writes them
  }
  if (tid == 0) {
    slots[2ull * blockIdx.x] = dyn < sto ? dyn : sto;
    slots[2ull * blockIdx.x + 1] = dyn < sto ? sto : dyn;
  }
}

// One workgroup packs the slots, 256 a row, into the sorted list behind entry
// 0, ranked as inflate_scan_kernel ranks its hits: the lanes below by ballot,
// the waves below by four LDS words, the rows before by a running count.
__global__ __launch_bounds__(kThreads) void inflate_compact_kernel(
    const uint64_t* __restrict__ slots, uint32_t nslots, uint64_t start,
    uint64_t* __restrict__ cand, uint32_t* __restrict__ ncand) {
  __shared__ uint32_t wave_cnt[kWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t run = 1;
  for (uint32_t row = 0; row < nslots; row += kThreads) {
    const uint64_t v = row + tid < nslots ? slots[row + tid] : inf::kNoCand;
    const uint64_t have = __ballot(v != inf::kNoCand);
    if (lane == 0) wave_cnt[wave] = __popcll(have);
    __syncthreads();
    uint32_t before = 0, row_total = 0;
    for (uint32_t u = 0; u < kWaves; u++) {
      if (u < wave) before += wave_cnt[u];
      row_total += wave_cnt[u];
    }
    if (v != inf::kNoCand) cand[run + before + __popcll(have & ((1ull << lane) - 1))] = v;
    run += row_total;
    __syncthreads();
  }
  if (tid == 0) cand[0] = start, *ncand = run;
}

// The measuring sink of a search: the span's bytes as entries of its symbolic
// ring in HBM (inflate_core.hpp). A write at byte o replaces byte o - 32768,
// which an earlier token of the same batch may still copy from, so the batch
// goes in order: the literals up to a match from their lanes, then the match
// with all lanes, entry by entry as the emitting sink copies bytes.
struct RingSink {
  const uint8_t* src;
  uint16_t* ring;
  bool at_stream_start;

  __device__ __forceinline__ uint32_t stored(WaveCtx& cx, uint64_t at, uint32_t n, uint64_t out) {
    for (uint32_t k = (n > inf::kWindow ? n - inf::kWindow : 0) + cx.tid; k < n; k += kWave)
      ring[(out + k) & kWinMask] = src[at + k];
    __threadfence_block();
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
    const uint32_t before = inc - len;
    const uint64_t base = *out;
    uint32_t status = inf::kOk;
    if (at_stream_start && __ballot(match && dist > base + before)) status = inf::kCorrupt;
    if (!status) {
      uint32_t done = 0;  // lanes below it have stored
      for (uint64_t mm = __ballot(match);; mm &= mm - 1) {
        const uint32_t l = mm ? __ffsll(static_cast<unsigned long long>(mm)) - 1 : kWave;
        if (lane >= done && lane < l && lane < n) ring[(base + before) & kWinMask] = t & 0xFFu;
        if (!mm) break;
        const uint64_t p = base + __shfl(before, l, kWave);
        const uint32_t ml = __shfl(len, l, kWave), md = __shfl(dist, l, kWave);
        __threadfence_block();  // the entries before p are stored before they are loaded
        for (uint32_t k = lane; k < ml; k += kWave)
          ring[(p + k) & kWinMask] = ring[(p - md + (md >= ml ? k : k % md)) & kWinMask];
        done = l + 1;
      }
      *out = base + total;
    }
    cx.sync();
    return status;
  }
};

// The emitting sink of a search: WaveSink<true>, but a match that reaches
// before the span's first byte takes those bytes from the resolved window.
struct WindowSink {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t cap;
  const uint8_t* win;  // nullptr at the stream start

  __device__ __forceinline__ uint32_t stored(WaveCtx& cx, uint64_t at, uint32_t n, uint64_t out) {
    if (out + n > cap) return inf::kCorrupt;
    wave_copy(src + at, dst + out, n, cx.tid);
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
    const uint32_t before = inc - len;
    const uint64_t base = *out;
    uint32_t status = inf::kOk;
    if (!win && __ballot(match && dist > base + before)) status = inf::kCorrupt;
    else if (base + total > cap) status = inf::kCorrupt;
    if (!status) {
      uint8_t* o = dst + base;
      if (lane < n && !match) o[before] = static_cast<uint8_t>(t);
      for (uint64_t mm = __ballot(match); mm; mm &= mm - 1) {
        const int l = __ffsll(static_cast<unsigned long long>(mm)) - 1;
        const uint32_t p = __shfl(before, l, kWave), ml = __shfl(len, l, kWave),
                       md = __shfl(dist, l, kWave);
        __threadfence_block();
        const int64_t from = static_cast<int64_t>(base + p) - md;  // in the span; < 0: the window
        for (uint32_t k = lane; k < ml; k += kWave) {
          const int64_t at = from + (md >= ml ? k : k % md);
          o[p + k] = at < 0 ? win[inf::kWindow + at] : dst[at];  // at >= -32768: md <= 32768
        }
      }
      *out = base + total;
    }
    cx.sync();
    return status;
  }
};

// One wave per span, as inflate_spans_kernel. kEmit == false: span i starts at
// cand[i], fills rings + i * kWindow (set to kUnknown | k by the wave first)
// and leaves recs[i]. kEmit == true: span i is plan[i] with windows + i *
// kWindow behind it and ends where plan[i + 1] starts.
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void inflate_search_spans_kernel(
    const uint8_t* __restrict__ src, uint64_t size, uint64_t limit,
    const uint64_t* __restrict__ cand, const inf::PlanSpan* __restrict__ plan, uint32_t nspans,
    uint16_t* rings, const uint8_t* __restrict__ windows, inf::SpanRec* __restrict__ recs,
    uint8_t* dst, uint32_t* __restrict__ err) {
  __shared__ WaveLds lds[kWaves];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t span = blockIdx.x * kWaves + wave;
  if (span >= nspans) return;  // a whole wave: no barrier follows
  WaveLds& my = lds[wave];
  const uint32_t phase = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src) & 15u);
  WaveCtx cx{lane, src - phase, phase, (phase + size + 15) & ~15ull, limit, my.ring, 0};
  inf::SpanRec rec{0, 0, inf::kCorrupt};
  if (kEmit) {
    const uint64_t start = inf::plan_cand(plan[span]), cap = plan[span].out_bytes;
    if ((start >> 4) <= limit) {
      WindowSink sink{src, dst + plan[span].out_offset, cap,
                      span ? windows + static_cast<uint64_t>(span) * inf::kWindow : nullptr};
      inf::EndCut cut{span + 1 < nspans ? inf::plan_cand(plan[span + 1]) : inf::kNoCand};
      rec = inf::decode_span(cx, my.w, sink, start, limit, cut);
    }
    if (lane == 0 && ((rec.status & inf::kStatusMask) || rec.out_bytes != cap)) *err = 1;
  } else {
    uint16_t* ring = rings + static_cast<uint64_t>(span) * inf::kWindow;
    for (uint32_t k = lane * 2; k < inf::kWindow; k += kWave * 2)
      *reinterpret_cast<uint32_t*>(ring + k) = (inf::kUnknown | k) | (inf::kUnknown | (k + 1)) << 16;
    __threadfence_block();
    RingSink sink{src, ring, span == 0};
    inf::ListCut cut{cand, nspans, span + 1};
    rec = inf::decode_span(cx, my.w, sink, cand[span], limit, cut);
    if (lane == 0) recs[span] = rec;
  }
}

// One workgroup of 1024 threads, the chain in order: the window behind the
// spans so far is in LDS (32 KiB), span j's is written out, then the next is
// resolved from span j's ring into the other 32 KiB: 64 KiB of a CU's 160.
constexpr uint32_t kWinThreads = 1024;
__global__ __launch_bounds__(kWinThreads) void inflate_windows_kernel(
    const uint16_t* __restrict__ rings, const inf::ChainLink* __restrict__ chain, uint32_t nspans,
    uint8_t* __restrict__ windows) {
  __shared__ alignas(16) uint8_t win[2][inf::kWindow];
  const uint32_t tid = threadIdx.x;
  for (uint32_t k = tid; k < inf::kWindow / 16; k += kWinThreads)
    reinterpret_cast<u32x4*>(win[0])[k] = u32x4{0, 0, 0, 0};
  __syncthreads();
  for (uint32_t j = 0; j < nspans; j++) {
    const uint8_t* cur = win[j & 1u];
    uint8_t* next = win[(j + 1) & 1u];
    u32x4* out = reinterpret_cast<u32x4*>(windows + static_cast<uint64_t>(j) * inf::kWindow);
    for (uint32_t k = tid; k < inf::kWindow / 16; k += kWinThreads)
      out[k] = reinterpret_cast<const u32x4*>(cur)[k];
    if (j + 1 < nspans) {
      const uint16_t* ring = rings + static_cast<uint64_t>(chain[j].ring) * inf::kWindow;
      const uint32_t rot = chain[j].rot;
      for (uint32_t k = tid; k < inf::kWindow; k += kWinThreads)
        next[k] = inf::resolve_entry(ring, rot, k, cur);
    }
    __syncthreads();
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

extern "C" hipError_t modelx_inflate_search(const void* src, uint64_t size, uint64_t first,
                                            uint64_t limit, uint32_t nstrides,
                                            uint64_t* slots_dev, uint64_t* cand_dev,
                                            uint32_t* ncand_dev, hipStream_t stream) {
  if (!src || !cand_dev || !ncand_dev || first > limit || limit > size || size >= (1ull << 32) ||
      nstrides != inf::search_strides(first, limit, kStride) || (nstrides && !slots_dev))
    return hipErrorInvalidValue;
  const uint32_t phase = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src) & 15u);
  const uint8_t* base16 = static_cast<const uint8_t*>(src) - phase;
  const uint64_t a_end = (phase + size + 15) & ~15ull;
  if (nstrides)
    hipLaunchKernelGGL(inflate_search_kernel, dim3(nstrides), dim3(kThreads), 0, stream, base16,
                       phase, a_end, first, limit, slots_dev);
  hipLaunchKernelGGL(inflate_compact_kernel, dim3(1), dim3(kThreads), 0, stream, slots_dev,
                     2 * nstrides, inf::make_cand(first * 8, false), cand_dev, ncand_dev);
  return hipGetLastError();
}

extern "C" hipError_t modelx_inflate_measure_search(const void* src, uint64_t size, uint64_t limit,
                                                    const uint64_t* cand_dev, uint32_t ncand,
                                                    uint16_t* rings_dev,
                                                    modelx::inflate::SpanRec* recs_dev,
                                                    hipStream_t stream) {
  if (!src || !cand_dev || !rings_dev || !recs_dev || limit > size || size >= (1ull << 32) || !ncand)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(inflate_search_spans_kernel<false>, dim3((ncand + kWaves - 1) / kWaves),
                     dim3(kThreads), 0, stream, static_cast<const uint8_t*>(src), size, limit,
                     cand_dev, nullptr, ncand, rings_dev, nullptr, recs_dev, nullptr, nullptr);
  return hipGetLastError();
}

extern "C" hipError_t modelx_inflate_windows(const uint16_t* rings_dev,
                                             const modelx::inflate::ChainLink* chain_dev,
                                             uint32_t nspans, uint8_t* windows_dev,
                                             hipStream_t stream) {
  if (!rings_dev || !chain_dev || !windows_dev || !nspans) return hipErrorInvalidValue;
  hipLaunchKernelGGL(inflate_windows_kernel, dim3(1), dim3(kWinThreads), 0, stream, rings_dev,
                     chain_dev, nspans, windows_dev);
  return hipGetLastError();
}

extern "C" hipError_t modelx_inflate_emit_search(const void* src, uint64_t size, uint64_t limit,
                                                 const modelx::inflate::PlanSpan* plan_dev,
                                                 uint32_t nspans, const uint8_t* windows_dev,
                                                 void* dst, uint32_t* err_dev,
                                                 hipStream_t stream) {
  if (!src || !dst || !windows_dev || limit > size || size >= (1ull << 32) || !nspans)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(inflate_search_spans_kernel<true>, dim3((nspans + kWaves - 1) / kWaves),
                     dim3(kThreads), 0, stream, static_cast<const uint8_t*>(src), size, limit,
                     nullptr, plan_dev, nspans, nullptr, windows_dev, nullptr,
                     static_cast<uint8_t*>(dst), err_dev);
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
