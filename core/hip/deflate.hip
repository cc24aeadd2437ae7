// CDNA4 DEFLATE kernels (gfx950): a device buffer compressed into the chunks
// of one gzip member. Format, parse rules, Huffman builder and bit layout are
// modelx/deflate_core.hpp's, shared with the host model, and the bytes this
// file produces equal the host model's. This file is how the work is split
// and how the bytes move.
//
// deflate_chunks_kernel: one workgroup of 256 threads per 32 KiB chunk, the
// grid capped at kDeflateMaxBlocks and strided over the chunks. Per chunk:
//  1. stage: the chunk goes into LDS with 16 B loads whatever the 16 B phase
//     of the source (copy_shifted.hpp), while the hash table and the
//     histograms are cleared.
//  2. crc: every thread folds 132 consecutive bytes of the staged chunk (33
//     dwords, so that the 64 lanes of a wave start in 32 different banks),
//     advances its raw value over the bytes that follow and the workgroup
//     XORs the values: one raw CRC-32 per chunk, joined on the host. The
//     input is read from HBM once for both compression and checksum.
//  3. parse: wave 0 walks the rounds of 64 positions. A lane looks up its
//     position in the LDS hash table, the wave then inserts with atomicMax,
//     walks the round with readlane to find which positions start a token,
//     and the chosen lanes write their tokens side by side (rank by popcount
//     of the selection mask) into the workgroup's slice of global scratch
//     and count their symbols with LDS atomics. Waves 1-3 wait at the barrier
//     after the parse; nothing waits on another workgroup.
//  4. trees: deflate::build_trees across the workgroup, its arg-max steps
//     through an LDS word and one barrier each.
//  5. encode: the chunk in LDS is dead (tokens carry the literals), so the
//     same region becomes the zeroed output image. A thread owns a
//     consecutive run of tokens, sums their bits, thread 0 scans the 256
//     sums, and every thread ORs its codes into the image (atomicOr: runs
//     share words). Thread 0 adds the header, end-of-block and the empty
//     stored block. The image is flushed to the chunk's slot with 16 B stores.
//  6. out[chunk] = {bytes (| kStoredFlag), raw crc}. A chunk whose Huffman
//     form is not smaller writes nothing else: the gather copies it from the
//     source.
//
// LDS of a workgroup (53.7 KiB of the 64 KiB it may have; three workgroups
// fit a CU's 160 KiB):
//   buf    32 KiB + 64   the chunk, then the output image
//   table  16 KiB        4096 hash entries (position + 1)
//   trees  2.4 KiB       counts, lengths and codes of the three alphabets
//   crc    1 KiB + 64    byte table, x^(8 * 2^k) for k < 16
//   scan   1 KiB         bit counts of the 256 token runs
//
// Every loop is bounded by the chunk length, the token count, the alphabet
// size or the builder's guard.
//
// deflate_gather_kernel: one workgroup per chunk copies the chunk's bytes to
// their final address: from its slot, or for a stored chunk the five header
// bytes and the source bytes. Any phase of source and destination
// (copy_shifted.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/copy_shifted.hpp"
#include "modelx/deflate_core.hpp"
#include "modelx/deflate_wg.hpp"
#include "modelx/device_abi.hpp"

namespace {

namespace df = modelx::deflate;
using modelx::abi::DeflateChunkOut;
using modelx::devcopy::u32x4;

constexpr uint32_t kThreads = 256;
static_assert(kThreads == modelx::devcopy::kPackThreads, "copy_shifted.hpp's workgroup");
constexpr uint32_t kChunk = df::kChunkBytes;
constexpr uint32_t kCrcPiece = 132;
static_assert(kCrcPiece * kThreads >= kChunk, "the pieces cover a chunk");
static_assert(modelx::abi::kDeflateSlotStride >= kChunk + 16 &&
                  modelx::abi::kDeflateSlotStride % 16 == 0,
              "a slot holds an image rounded up to 16 B");

__device__ const df::crc32::PowTable kPow = df::crc32::make_pow_table();

struct Lds {
  alignas(16) uint8_t buf[kChunk + 64];
  uint32_t table[1u << df::kHashBits];
  df::Trees t;
  uint32_t crc_tab[256];
  uint32_t pow[16];
  uint32_t scan[kThreads];
  uint32_t ntok;
  uint32_t crc;
};
static_assert(sizeof(Lds) <= 64u << 10, "LDS of one workgroup");

using modelx::deflate_wg::WgCtx;  // shared with deflate_lengths.hip, the tests' way in
static_assert(kThreads == modelx::deflate_wg::kThreads, "deflate_wg.hpp's workgroup");

// Wave 0: tokens of the staged chunk into `tokens`, symbol counts into lds.t.
__device__ __forceinline__ void parse_wave(Lds& lds, uint32_t n, uint32_t* __restrict__ tokens) {
  const uint32_t lane = threadIdx.x;
  uint32_t next = 0, ntok = 0;
  for (uint32_t base = 0; base < n; base += df::kRound) {
    const uint32_t p = base + lane;
    const bool can = p + 4 <= n;
    uint32_t h = 0, m = 0;
    if (can) {
      h = df::hash32(df::load32(lds.buf, p));
      if (p >= next) m = df::find_match(lds.buf, n, p, lds.table[h]);
    }
    __threadfence_block();  // every lane has looked up before any inserts
    if (can) atomicMax(&lds.table[h], p + 1);
    const uint32_t end = base + df::kRound < n ? base + df::kRound : n;
    uint64_t sel = 0;
    uint32_t q = __builtin_amdgcn_readfirstlane(next > base ? next : base);
    while (q < end) {
      uint32_t i = q - base;
      uint32_t len = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(m), i)) >> 16;
      sel |= 1ull << i;
      q += len ? len : 1;
    }
    next = q;
    if (p < end && ((sel >> lane) & 1u)) {
      uint32_t rank = __popcll(sel & ((1ull << lane) - 1));
      uint32_t len = m >> 16;
      uint32_t tok = len ? df::make_match(len, m & 0xFFFFu) : lds.buf[p];
      tokens[ntok + rank] = tok;
      uint32_t ll, d;
      df::count_token(tok, &ll, &d);
      atomicAdd(&lds.t.hist_ll[ll], 1u);
      if (len) atomicAdd(&lds.t.hist_d[d], 1u);
    }
    ntok += __popcll(sel);
    __threadfence_block();  // the inserts land before the next round looks up
  }
  if (lane == 0) lds.ntok = ntok;
}

__global__ __launch_bounds__(kThreads) void deflate_chunks_kernel(
    const uint8_t* __restrict__ src, uint64_t size, uint64_t first_chunk, uint32_t nchunks,
    uint64_t total_chunks, uint32_t* __restrict__ token_scratch, uint8_t* __restrict__ slots,
    DeflateChunkOut* __restrict__ out) {
  __shared__ Lds lds;
  const uint32_t tid = threadIdx.x;
  const WgCtx cx{tid};
  lds.crc_tab[tid] = df::crc32::table_entry(tid);
  if (tid < 16) lds.pow[tid] = kPow.v[tid];
  uint32_t* tokens = token_scratch + static_cast<uint64_t>(blockIdx.x) * kChunk;
  uint32_t* img = reinterpret_cast<uint32_t*>(lds.buf);

  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const uint64_t g = first_chunk + chunk;
    const uint64_t off = g * kChunk;
    const uint32_t n = static_cast<uint32_t>(size - off < kChunk ? size - off : kChunk);
    const bool last = g + 1 == total_chunks;
    __syncthreads();  // the previous chunk's image has been flushed

    // 1. stage and clear
    modelx::devcopy::copy_to_aligned_grid(src + off, lds.buf, n);
    for (uint32_t i = tid; i < (1u << df::kHashBits); i += kThreads) lds.table[i] = 0;
    for (uint32_t i = tid; i < 288; i += kThreads) lds.t.hist_ll[i] = i == 256 ? 1u : 0u;
    if (tid < 32) lds.t.hist_d[tid] = 0;
    if (tid == 0) lds.crc = 0;
    __syncthreads();

    // 2. raw CRC-32 of the chunk
    {
      uint32_t a = tid * kCrcPiece;
      if (a < n) {
        uint32_t b = a + kCrcPiece < n ? a + kCrcPiece : n;
        uint32_t s = 0;
        for (uint32_t i = a; i < b; i++) s = lds.crc_tab[(s ^ lds.buf[i]) & 0xFFu] ^ (s >> 8);
        if (s) atomicXor(&lds.crc, df::crc32::mul_xn(s, n - b, lds.pow));
      }
    }

    // 3. parse
    if (tid < 64) parse_wave(lds, n, tokens);
    __syncthreads();  // tokens (global), counts, ntok and crc are visible
    const uint32_t ntok = lds.ntok;
    const uint32_t crc = lds.crc;

    // 4. trees
    df::HeaderShape shape;
    uint32_t block_bits = 0;
    const bool ok = df::build_trees(cx, lds.t, &shape, &block_bits);
    const uint32_t bytes = df::huffman_bytes(block_bits);
    if (!ok || bytes >= df::chunk_bound(n)) {  // uniform
      if (tid == 0) out[chunk] = {df::chunk_bound(n) | df::kStoredFlag, crc};
      continue;
    }

    // 5. encode into the image
    const uint32_t nvec = (bytes + 15) / 16;
    for (uint32_t i = tid; i < nvec * 4 + 4; i += kThreads) img[i] = 0;
    const uint32_t per = (ntok + kThreads - 1) / kThreads;
    const uint32_t a = tid * per < ntok ? tid * per : ntok;
    const uint32_t b = a + per < ntok ? a + per : ntok;
    uint32_t my_bits = 0;
    for (uint32_t i = a; i < b; i++) {
      uint64_t v;
      my_bits += df::token_bits(lds.t, tokens[i], &v);
    }
    lds.scan[tid] = my_bits;
    __syncthreads();
    if (tid == 0) {
      uint32_t run = df::header_bit_count(lds.t, shape);
      for (uint32_t i = 0; i < kThreads; i++) {
        uint32_t v = lds.scan[i];
        lds.scan[i] = run;
        run += v;
      }
    }
    __syncthreads();
    uint32_t pos = lds.scan[tid];
    for (uint32_t i = a; i < b; i++) {
      uint64_t v;
      uint32_t nb = df::token_bits(lds.t, tokens[i], &v);
      df::put_bits(img, pos, v, nb);
      pos += nb;
    }
    if (tid == 0) {
      df::write_header(lds.t, shape, img);
      df::put_bits(img, block_bits - lds.t.len_ll[256], lds.t.code_ll[256], lds.t.len_ll[256]);
      df::write_sync(img, block_bits, last);
    }
    __syncthreads();
    u32x4* vd = reinterpret_cast<u32x4*>(slots + static_cast<uint64_t>(chunk) *
                                                     modelx::abi::kDeflateSlotStride);
    const u32x4* vs = reinterpret_cast<const u32x4*>(lds.buf);
    for (uint32_t k = tid; k < nvec; k += kThreads) vd[k] = vs[k];
    if (tid == 0) out[chunk] = {bytes, crc};
  }
}

__global__ __launch_bounds__(kThreads) void deflate_gather_kernel(
    const uint8_t* __restrict__ src, uint64_t size, uint64_t first_chunk, uint32_t nchunks,
    uint64_t total_chunks, const uint8_t* __restrict__ slots,
    const DeflateChunkOut* __restrict__ out, const uint64_t* __restrict__ dst_addr) {
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const uint32_t sz = out[chunk].size;
    uint8_t* dst = reinterpret_cast<uint8_t*>(dst_addr[chunk]);
    if (sz & df::kStoredFlag) {
      const uint64_t g = first_chunk + chunk;
      const uint64_t off = g * kChunk;
      const uint32_t n = static_cast<uint32_t>(size - off < kChunk ? size - off : kChunk);
      uint8_t hdr[df::kStoredOverhead];
      df::stored_header(hdr, n, g + 1 == total_chunks);
      if (threadIdx.x < df::kStoredOverhead) dst[threadIdx.x] = hdr[threadIdx.x];
      modelx::devcopy::copy_to_aligned_grid(src + off, dst + df::kStoredOverhead, n);
    } else {
      modelx::devcopy::copy_to_aligned_grid(
          slots + static_cast<uint64_t>(chunk) * modelx::abi::kDeflateSlotStride, dst, sz);
    }
  }
}

}  // namespace

extern "C" hipError_t modelx_deflate_chunks(const void* src, uint64_t size, uint64_t first_chunk,
                                            uint32_t nchunks, void* token_scratch, void* slots,
                                            DeflateChunkOut* out_dev, hipStream_t stream) {
  const uint64_t total = df::chunk_count(size);
  if (nchunks == 0 || first_chunk + nchunks > total) return hipErrorInvalidValue;
  uint32_t blocks = nchunks < modelx::abi::kDeflateMaxBlocks ? nchunks
                                                             : modelx::abi::kDeflateMaxBlocks;
  hipLaunchKernelGGL(deflate_chunks_kernel, dim3(blocks), dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(src), size, first_chunk, nchunks, total,
                     static_cast<uint32_t*>(token_scratch), static_cast<uint8_t*>(slots),
                     out_dev);
  return hipGetLastError();
}

extern "C" hipError_t modelx_deflate_gather(const void* src, uint64_t size, uint64_t first_chunk,
                                            uint32_t nchunks, const void* slots,
                                            const DeflateChunkOut* out_dev,
                                            const uint64_t* dst_addr_dev, hipStream_t stream) {
  const uint64_t total = df::chunk_count(size);
  if (nchunks == 0 || first_chunk + nchunks > total) return hipErrorInvalidValue;
  uint32_t blocks = nchunks < 2048u ? nchunks : 2048u;
  hipLaunchKernelGGL(deflate_gather_kernel, dim3(blocks), dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(src), size, first_chunk, nchunks, total,
                     static_cast<const uint8_t*>(slots), out_dev, dst_addr_dev);
  return hipGetLastError();
}
