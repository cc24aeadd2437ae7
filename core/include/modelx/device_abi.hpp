// The host<->kernel ABI, declared once: the POD structs that cross the
// launch boundary in device memory and the extern "C" launchers of
// core/hip/*.hip. Each .hip file includes this header, so the compiler checks
// every launcher definition against the prototype the engine calls. The
// decode kernel's frame descriptor is zstdhost::SeekEntry itself: the engine
// uploads the parsed seek table as-is.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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
// Byte-plane split (merge == 0) or merge of `size` bytes, src -> dst, which
// must not overlap (modelx/byteplane_host.hpp defines the transform).
// hipErrorInvalidValue unless elem is 2, 4 or 8 and group a positive
// multiple of it.
hipError_t modelx_byte_planes(const void* src, void* dst, uint64_t size, uint32_t elem,
                              uint64_t group, int merge, hipStream_t stream);

}  // extern "C"
