// Host-side zstd container helpers: seekable multi-frame blobs.
//
// Blob layout = N standard zstd frames (each <= frame_raw decompressed bytes)
// concatenated, followed by one skippable frame holding the
// zstd-seekable-format seek table. Stock `zstd -d` decodes the blob (it
// ignores skippable frames); the GPU kernels use the table to decode all
// frames in parallel (one workgroup per frame).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace modelx {
namespace zstdhost {

struct SeekEntry {
  uint64_t c_off, c_size;  // compressed span within the blob
  uint64_t d_off, d_size;  // decompressed span
};

// The seek-table format, in two strict steps over host bytes: a caller whose
// blob lives elsewhere (the GPU engine) fetches the fixed-size footer, learns
// the table's length from it, then fetches exactly that tail. Both steps throw
// std::runtime_error on malformed input.
constexpr size_t kSeekFooterBytes = 17;

struct SeekFooter {
  uint32_t nframes;
  uint32_t entry_bytes;  // 8, or 12 with per-frame checksums
  uint64_t table_bytes;  // whole skippable frame: 8 + nframes*entry_bytes + 9
};

// tail17 = the blob's last kSeekFooterBytes (unread if blob_len is shorter).
SeekFooter parse_seek_footer(const uint8_t* tail17, uint64_t blob_len);

// table = the blob's last f.table_bytes. Appends one entry per frame to *out
// and returns the decompressed total.
uint64_t parse_seek_entries(const uint8_t* table, const SeekFooter& f, uint64_t blob_len,
                            std::vector<SeekEntry>* out);

// Parse the seek table from a full blob. Returns empty vector if the blob
// has no valid seek table (caller falls back to sequential frame walking).
std::vector<SeekEntry> parse_seek_table(const uint8_t* blob, size_t len);

// Walk frames sequentially (no seek table needed); returns entries or empty
// on malformed input. Skips skippable frames.
std::vector<SeekEntry> walk_frames(const uint8_t* blob, size_t len);

// Serialize the seekable skippable frame for the given entries.
std::vector<uint8_t> build_seek_table(const std::vector<SeekEntry>& entries);

// CPU compress src into a seekable multi-frame blob (threads over frames).
// `flags` are EncTables::flags (zstd_enc.hpp): 4 = literals-only.
std::vector<uint8_t> compress_seekable(const uint8_t* src, size_t len, uint32_t frame_raw,
                                       uint32_t flags = 0);

// CPU decompress a seekable (or plain multi-frame) blob.
// Returns decompressed bytes; throws std::runtime_error on corrupt input.
std::vector<uint8_t> decompress(const uint8_t* blob, size_t len);

// Total decompressed size from the table (or walk).
uint64_t content_size(const uint8_t* blob, size_t len);

}  // namespace zstdhost
}  // namespace modelx
