// The host<->kernel ABI, declared once: the POD structs that cross the
// launch boundary in device memory and the extern "C" launchers of
// core/hip/*.hip. Each .hip file includes this header, so the compiler checks
// every launcher definition against the prototype the engine calls. The
// decode kernel's frame descriptor is zstdhost::SeekEntry itself: the engine
// uploads the parsed seek table as-is.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/aead_core.hpp"
#include "modelx/crc32c_core.hpp"
#include "modelx/deflate_core.hpp"
#include "modelx/inflate_core.hpp"
#include "modelx/tar_core.hpp"
#include "modelx/zstd_host.hpp"

namespace modelx {
namespace abi {

// One indexed header and the outcome of a header walk: tar_core.hpp's, which
// the index kernel and the host model share.
using TarEntry = tarcore::Entry;
using TarWalkResult = tarcore::WalkResult;

// Scatter segment: copies src[src_off..src_off+len) -> dst_ptr.
struct CopySeg {
  uint64_t src_off;
  uint64_t dst_ptr;  // device address
  uint64_t len;
};

// Pack segment: copies len bytes from the absolute device address src_ptr to
// tar + dst_off, then writes zero_len zero bytes after them.
struct PackSeg {
  uint64_t src_ptr;
  uint64_t dst_off;
  uint64_t len;
  uint64_t zero_len;
};

struct ChunkLeavesDesc {
  const uint8_t* data;
  uint8_t* leaves;
  uint64_t total;
  uint64_t chunk_size;
  uint32_t chunk_base;  // chunks in all preceding buffers
  uint32_t pad_;
};

// Linear-probe window of the chunk-dedup table (core/hip/dedup.hip): the
// smallest table capacity the engine accepts.
constexpr uint32_t kDedupMaxProbes = 64;

// One range of modelx_crc32c_ranges (core/hip/crc32c.hip): `len` bytes at the
// device address `ptr`. The kernel cuts the range's 16 B aligned body into
// segments of kCrc32cSegmentBytes (crc32c::segment_count of them); seg_base
// is the number of segments of all preceding ranges.
struct CrcRange {
  uint64_t ptr;
  uint64_t len;
  uint32_t seg_base;
  uint32_t pad_;
};

constexpr uint64_t kCrc32cSegmentBytes = crc32c::kSegmentBytes;

// Candidate kernel (core/hip/cdc.hip). A workgroup owns kCdcTileBytes on the
// 16 B grid of the range's first byte: tile k covers the addresses
// [(ptr & ~15) + k * kCdcTileBytes, ... + kCdcTileBytes) that lie in the range.
// 32 KiB keeps tile, halo, gear table and hit list under 40 KiB of LDS, four
// workgroups to a CU (profiles/cdc_kernel.md).
constexpr uint32_t kCdcTileBytes = 32u << 10;
constexpr uint32_t kCdcMaxTileCap = 2048;  // hit-list entries a tile can keep
constexpr uint32_t kCdcMaxBlocks = 256 * 8;

inline uint64_t cdc_tile_phase(uint64_t ptr) { return ptr & 15u; }

inline uint64_t cdc_tile_count(uint64_t ptr, uint64_t len) {
  return len ? (cdc_tile_phase(ptr) + len + kCdcTileBytes - 1) / kCdcTileBytes : 0;
}

// Hit-list capacity per tile at `bits`: four times the expected count of
// random data plus slack, so only periodic data or a tiny `bits` overflows.
inline uint32_t cdc_tile_cap(uint32_t bits) {
  uint64_t want = 32 + 4 * (static_cast<uint64_t>(kCdcTileBytes) >> bits);
  return want < kCdcMaxTileCap ? static_cast<uint32_t>(want) : kCdcMaxTileCap;
}

// One chunk of the off-grid dedup kernels (core/hip/dedup.hip). insert: `at`
// is the chunk's device address; probe: `at` is unused; gather: `at` is the
// chunk's byte offset in the destination.
struct DedupRange {
  uint64_t at;
  uint64_t len;
};

// One launch of modelx_aead_segments (core/hip/aead.hip): seal (open == 0) or
// open the n bytes at the device address src into dst, cut into nseg ==
// aead::segment_count(n, seg_bytes) segments (modelx/aead_core.hpp), with tag
// i at tags + 16 * i. dst is 16 B aligned; src may equal dst and may otherwise
// have any alignment; tags may have any alignment.
struct AeadJob {
  aead::Key key;
  uint64_t src;
  uint64_t dst;
  uint64_t tags;
  uint64_t n;
  uint64_t seg_bytes;
  uint64_t nseg;
  uint32_t open;
  uint32_t pad_;
};

// One chunk of modelx_deflate_chunks (core/hip/deflate.hip): the bytes the
// chunk becomes, with deflate::kStoredFlag set when it is stored (its slot is
// then not written), and the raw CRC-32 of its input bytes.
struct DeflateChunkOut {
  uint32_t size;
  uint32_t crc_raw;
};

// Workgroups of the chunk kernel (three per CU); each owns
// deflate::kChunkBytes tokens of scratch. A chunk's slot holds its output
// image rounded up to 16 B.
constexpr uint32_t kDeflateMaxBlocks = 768;
constexpr uint64_t kDeflateSlotStride = deflate::kChunkBytes + 16;

// Marker scan of core/hip/inflate.hip: a workgroup owns kInflateScanTile bytes
// on the 16 B grid of the member's first byte, as the candidate kernel's
// tiles above. The CRC kernel takes the output in pieces of kInflateCrcPiece.
constexpr uint32_t kInflateScanTile = 16u << 10;
constexpr uint32_t kInflateCrcPiece = 32u << 10;
// Block search of core/hip/inflate.hip: the deflate stream is cut every
// kInflateSearchStride bytes after its first byte, one workgroup per stride,
// which it stages kInflateSearchTile bytes at a time.
constexpr uint32_t kInflateSearchStride = 64u << 10;
constexpr uint32_t kInflateSearchTile = 4u << 10;
static_assert(kInflateSearchStride % kInflateSearchTile == 0, "a stride is whole tiles");

inline uint32_t inflate_scan_tiles(uint64_t ptr, uint64_t size) {
  return static_cast<uint32_t>(((ptr & 15u) + size + kInflateScanTile - 1) / kInflateScanTile);
}

}  // namespace abi
}  // namespace modelx

extern "C" {

hipError_t modelx_sha256_chunk_leaves(const void* data, uint64_t total, uint64_t chunk_size,
                                      void* leaves, uint32_t nchunks, hipStream_t stream);
hipError_t modelx_sha256_chunk_leaves_many(const modelx::abi::ChunkLeavesDesc* descs_dev,
                                           uint32_t nbuf, uint32_t total_chunks,
                                           hipStream_t stream);
hipError_t modelx_sha256_multibuf(const void* const* buffers, const uint64_t* lengths,
                                  uint32_t nbuf, void* digests, hipStream_t stream);
// Walks the headers of the archive at `tar` (tarcore::walk): up to
// max_entries entries and the count, error code and error offset in
// *result_dev. Reads no byte at or past tar + tar_len.
hipError_t modelx_tar_index(const void* tar, uint64_t tar_len, modelx::abi::TarEntry* entries,
                            uint32_t max_entries, modelx::abi::TarWalkResult* result_dev,
                            hipStream_t stream);
hipError_t modelx_tar_scatter(const void* tar, const modelx::abi::CopySeg* segs, uint32_t nsegs,
                              hipStream_t stream);
hipError_t modelx_tar_pack(void* tar, const modelx::abi::PackSeg* segs, uint32_t nsegs,
                           hipStream_t stream);
hipError_t modelx_zstd_decompress_frames(const void* src,
                                         const modelx::zstdhost::SeekEntry* frames_dev,
                                         uint32_t nframes, void* dst, void* lit_scratch,
                                         int64_t* rc_dev, uint32_t flags, hipStream_t stream);
hipError_t modelx_zstd_compress_frames(const void* src, uint64_t srclen, uint32_t frame_raw,
                                       uint32_t first_frame, uint32_t nframes, void* dst_scratch,
                                       uint64_t stride, void* seq_scratch, uint32_t max_seqs,
                                       int64_t* out_sizes_dev, uint32_t flags,
                                       hipStream_t stream);
// leaves_dev: `nleaves` digests, pairwise distinct; chunk_idx_dev[i] is the
// chunk of the blob that leaf i digests.
hipError_t modelx_dedup_insert(const void* leaves_dev, const uint32_t* chunk_idx_dev,
                               uint32_t nleaves, uint64_t base, uint64_t chunk_size,
                               uint64_t total, void* table, uint64_t cap,
                               uint32_t* dropped_dev, hipStream_t stream);
hipError_t modelx_dedup_probe(const void* leaves_dev, uint32_t nchunks, uint64_t chunk_size,
                              uint64_t total, const void* table, uint64_t cap,
                              uint64_t* src_addr_dev, uint64_t* src_len_dev, hipStream_t stream);
hipError_t modelx_dedup_gather(const uint64_t* src_addr_dev, const uint64_t* src_len_dev,
                               uint32_t nchunks, uint64_t dst_base, uint64_t chunk_size,
                               hipStream_t stream);
// The same table for chunks off the grid: entry i is (digest i, ranges_dev[i]).
// insert: digests pairwise distinct. probe: src_addr_dev[i] is the address of a
// resident chunk with digest i and length ranges_dev[i].len, or 0. gather: one
// workgroup per chunk with src_addr_dev[i] != 0 copies it to
// dst_base + ranges_dev[i].at, whatever the 16 B phases of the two.
hipError_t modelx_dedup_insert_ranges(const void* digests_dev,
                                      const modelx::abi::DedupRange* ranges_dev, uint32_t n,
                                      void* table, uint64_t cap, uint32_t* dropped_dev,
                                      hipStream_t stream);
hipError_t modelx_dedup_probe_ranges(const void* digests_dev,
                                     const modelx::abi::DedupRange* ranges_dev, uint32_t n,
                                     const void* table, uint64_t cap, uint64_t* src_addr_dev,
                                     hipStream_t stream);
hipError_t modelx_dedup_gather_ranges(const uint64_t* src_addr_dev,
                                      const modelx::abi::DedupRange* ranges_dev, uint32_t n,
                                      uint64_t dst_base, hipStream_t stream);
// Candidate positions (modelx/cdc_core.hpp) of the `len` bytes at `ptr`, per
// tile: counts_dev[k] is tile k's true count, lists_dev[k * cap ...] holds
// min(count, cap) of its hits in no order, each as the offset from the tile's
// first grid address. ntiles must be cdc_tile_count(ptr, len), cap at most
// kCdcMaxTileCap. Reads no byte outside the range.
hipError_t modelx_cdc_candidates(const void* ptr, uint64_t len, uint32_t bits, uint32_t ntiles,
                                 uint32_t cap, uint32_t* counts_dev, uint16_t* lists_dev,
                                 hipStream_t stream);
// Byte-plane split (merge == 0) or merge of `size` bytes, src -> dst, which
// must not overlap (modelx/byteplane_host.hpp defines the transform).
// hipErrorInvalidValue unless elem is 2, 4 or 8 and group a positive
// multiple of it.
hipError_t modelx_byte_planes(const void* src, void* dst, uint64_t size, uint32_t elem,
                              uint64_t group, int merge, hipStream_t stream);
// CRC-32C of `nranges` device ranges, out_dev[i] for ranges_dev[i]. Ranges may
// be empty or overlap. seg_vals_dev is scratch of total_segments values, the
// sum of the ranges' segment counts. Reads no byte outside a range.
hipError_t modelx_crc32c_ranges(const modelx::abi::CrcRange* ranges_dev, uint32_t nranges,
                                uint32_t total_segments, uint32_t* seg_vals_dev,
                                uint32_t* out_dev, hipStream_t stream);
// ChaCha20-Poly1305 over every segment of `job`. Seal writes the ciphertext
// and the tags. Open writes the plaintext, compares every tag and leaves in
// *bad_dev (which the caller sets to 0xFFFFFFFF) the lowest segment index
// whose tag differs. hipErrorInvalidValue for a job that breaks AeadJob's
// rules. Reads no byte outside [src, src + n) and the tags.
hipError_t modelx_aead_segments(modelx::abi::AeadJob job, uint32_t* bad_dev,
                                hipStream_t stream);
// DEFLATE chunks [first_chunk, first_chunk + nchunks) of the `size` bytes at
// src (modelx/deflate_core.hpp). token_scratch holds min(nchunks,
// kDeflateMaxBlocks) * deflate::kChunkBytes 32-bit tokens; slots holds nchunks
// * kDeflateSlotStride bytes, 16 B aligned; out_dev[i] describes chunk
// first_chunk + i. Reads no byte outside the 16 B aligned words of the source.
hipError_t modelx_deflate_chunks(const void* src, uint64_t size, uint64_t first_chunk,
                                 uint32_t nchunks, void* token_scratch, void* slots,
                                 modelx::abi::DeflateChunkOut* out_dev, hipStream_t stream);
// Copies every chunk of such a launch to dst_addr_dev[i] (any alignment): its
// slot's bytes, or for a stored chunk the block header and the source bytes.
hipError_t modelx_deflate_gather(const void* src, uint64_t size, uint64_t first_chunk,
                                 uint32_t nchunks, const void* slots,
                                 const modelx::abi::DeflateChunkOut* out_dev,
                                 const uint64_t* dst_addr_dev, hipStream_t stream);
// deflate::build_lengths of the nsym (2..286) counts at hist_dev, each below
// 2^16, to at most maxbits (1..15) bits, by one workgroup: the nsym lengths in
// len_dev and the builder's return value in *ok_dev.
hipError_t modelx_deflate_code_lengths(const uint32_t* hist_dev, uint32_t nsym, uint32_t maxbits,
                                       int complete, uint8_t* len_dev, uint32_t* ok_dev,
                                       hipStream_t stream);
// Candidates (modelx/inflate_core.hpp) of the gzip member of `size` bytes
// (below 4 GiB) at src whose deflate stream is [first, limit). With cand_dev
// null: counts_dev[k] is the number of markers that end in tile k. Otherwise
// cand_dev[0] = first and tile k's positions, ascending, follow from
// cand_dev[tile_base_dev[k]]; nothing is written at or past ncand. ntiles
// must be inflate_scan_tiles(src, size). Reads no byte outside the 16 B
// aligned words of the member.
hipError_t modelx_inflate_scan(const void* src, uint64_t size, uint64_t first, uint64_t limit,
                               uint32_t ntiles, uint32_t* counts_dev,
                               const uint32_t* tile_base_dev, uint32_t* cand_dev, uint32_t ncand,
                               hipStream_t stream);
// inflate::decode_span from each of the ncand candidates, writing nothing but
// recs_dev[i].
hipError_t modelx_inflate_measure(const void* src, uint64_t size, uint64_t limit,
                                  const uint32_t* cand_dev, uint32_t ncand,
                                  modelx::inflate::SpanRec* recs_dev, hipStream_t stream);
// Decodes span i of the plan into [dst + out_offset, ... + out_bytes) and
// nowhere else, whatever the plan says; *err_dev (which the caller clears)
// becomes nonzero if a span does not decode to exactly its out_bytes.
hipError_t modelx_inflate_emit(const void* src, uint64_t size, uint64_t limit,
                               const modelx::inflate::PlanSpan* plan_dev, uint32_t nspans,
                               void* dst, uint32_t* err_dev, hipStream_t stream);
// Block search (modelx/inflate_core.hpp, "search") of the same member:
// slots_dev takes two words per stride, nstrides = inflate::search_strides at
// kInflateSearchStride; cand_dev (1 + 2 * nstrides words) takes the sorted
// candidates, the stream's first bit as entry 0, and *ncand_dev their number.
// Reads no byte outside the 16 B aligned words of the member.
hipError_t modelx_inflate_search(const void* src, uint64_t size, uint64_t first, uint64_t limit,
                                 uint32_t nstrides, uint64_t* slots_dev, uint64_t* cand_dev,
                                 uint32_t* ncand_dev, hipStream_t stream);
// inflate::decode_span with ListCut from each candidate into its symbolic ring,
// rings_dev + i * kWindow (uint16 entries), leaving recs_dev[i].
hipError_t modelx_inflate_measure_search(const void* src, uint64_t size, uint64_t limit,
                                         const uint64_t* cand_dev, uint32_t ncand,
                                         uint16_t* rings_dev, modelx::inflate::SpanRec* recs_dev,
                                         hipStream_t stream);
// Resolves the windows of the nspans chain spans in order: windows_dev + j *
// kWindow is what span j reads before its first byte (zeros for span 0).
hipError_t modelx_inflate_windows(const uint16_t* rings_dev,
                                  const modelx::inflate::ChainLink* chain_dev, uint32_t nspans,
                                  uint8_t* windows_dev, hipStream_t stream);
// modelx_inflate_emit for a search plan: span i starts at the candidate in
// in_start and pad_, ends where span i + 1 starts, and reads matches that
// reach before it from windows_dev + i * kWindow.
hipError_t modelx_inflate_emit_search(const void* src, uint64_t size, uint64_t limit,
                                      const modelx::inflate::PlanSpan* plan_dev, uint32_t nspans,
                                      const uint8_t* windows_dev, void* dst, uint32_t* err_dev,
                                      hipStream_t stream);
// Raw CRC-32 (deflate::crc32) of every kInflateCrcPiece bytes of data, the
// last piece short. Reads the 16 B aligned words that hold a byte of data.
hipError_t modelx_crc32_pieces(const void* data, uint64_t total, uint32_t* out_dev,
                               hipStream_t stream);

}  // extern "C"
