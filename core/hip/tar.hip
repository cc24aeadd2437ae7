// CDNA4 tar kernels: index a tar archive resident in HBM and scatter file
// payloads to per-file device buffers.
//
// Replaces the reference's CPU UnTGZ extract loop (pkg/client/helper.go:
// 55-79) for archives landed in HBM by the pinned-ring engine. The header
// walk is inherently sequential (each header's size field locates the next),
// so one device thread builds the entry table (hundreds of 512 B headers —
// microseconds); the payload scatter is the bulk work and runs as a grid of
// 256-thread workgroups, one per ≤4 MiB segment, uint4-vectorized.
//
// The pack kernel is the inverse: it writes a whole archive (headers, payload
// pieces, padding, end marker) from a segment table laid out on the host
// (modelx/tar_host.hpp), again one workgroup per ≤4 MiB segment.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/copy_shifted.hpp"
#include "modelx/device_abi.hpp"

using modelx::abi::CopySeg;
using modelx::abi::PackSeg;
using modelx::abi::TarEntry;
using modelx::abi::TarWalkResult;

namespace {

constexpr int kIndexThreads = 64;  // one wave; only its first lane works

// Single-thread sequential header walk: tarcore::walk, the same steps the
// host model runs (modelx/tar_core.hpp). entries sized by the caller. The
// launch bound gives the one wave the registers to hold a whole header, so
// the checksum's loads are all in flight together.
__global__ __launch_bounds__(kIndexThreads) void tar_index_kernel(
    const uint8_t* __restrict__ tar, uint64_t tar_len, TarEntry* __restrict__ entries,
    uint32_t max_entries, TarWalkResult* __restrict__ result) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  TarWalkResult res;
  modelx::tarcore::walk(tar, tar_len, entries, max_entries, &res);
  *result = res;
}

constexpr int kScatterThreads = 256;

// Scatter segments: seg i copies src[src_off..src_off+len) -> dst_ptr.
__global__ __launch_bounds__(kScatterThreads) void tar_scatter_kernel(
    const uint8_t* __restrict__ tar, const CopySeg* __restrict__ segs, uint32_t nsegs) {
  uint32_t seg_idx = blockIdx.x;
  if (seg_idx >= nsegs) return;
  CopySeg seg = segs[seg_idx];
  const uint8_t* src = tar + seg.src_off;
  uint8_t* dst = reinterpret_cast<uint8_t*>(seg.dst_ptr);
  uint64_t len = seg.len;
  // vector main body when both sides share 16-byte phase
  uint64_t i = threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
    uintptr_t mis = reinterpret_cast<uintptr_t>(src) & 15u;
    uint64_t head = mis ? (16 - mis) : 0;
    if (head > len) head = len;
    for (uint64_t k = threadIdx.x; k < head; k += kScatterThreads) dst[k] = src[k];
    uint64_t body = (len - head) / 16;
    const uint4* vs = reinterpret_cast<const uint4*>(src + head);
    uint4* vd = reinterpret_cast<uint4*>(dst + head);
    for (uint64_t k = threadIdx.x; k < body; k += kScatterThreads) vd[k] = vs[k];
    for (uint64_t k = head + body * 16 + threadIdx.x; k < len; k += kScatterThreads)
      dst[k] = src[k];
  } else {
    for (uint64_t k = i; k < len; k += kScatterThreads) dst[k] = src[k];
  }
}

using modelx::devcopy::copy_to_aligned_grid;
using modelx::devcopy::kPackThreads;

// Pack segments: seg i copies len bytes from the absolute address src_ptr to
// tar + dst_off, then writes zero_len zero bytes. The destination decides the
// vector grid (the engine keeps every dst_off 16 B aligned); whatever phase
// the source has against it, the body stores full uint4 words built from two
// adjacent aligned source words. Only the <16 B head and tail go bytewise.
__global__ __launch_bounds__(kPackThreads) void tar_pack_kernel(
    uint8_t* __restrict__ tar, const PackSeg* __restrict__ segs, uint32_t nsegs) {
  uint32_t seg_idx = blockIdx.x;
  if (seg_idx >= nsegs) return;
  PackSeg seg = segs[seg_idx];
  const uint8_t* src = reinterpret_cast<const uint8_t*>(seg.src_ptr);
  uint8_t* dst = tar + seg.dst_off;
  uint64_t len = seg.len;
  if (len) copy_to_aligned_grid(src, dst, len);
  uint64_t zlen = seg.zero_len;
  if (zlen) {
    uint8_t* z = dst + len;
    uint64_t head = (16 - (reinterpret_cast<uintptr_t>(z) & 15u)) & 15u;
    if (head > zlen) head = zlen;
    for (uint64_t k = threadIdx.x; k < head; k += kPackThreads) z[k] = 0;
    uint64_t nvec = (zlen - head) / 16;
    uint4* vz = reinterpret_cast<uint4*>(z + head);
    for (uint64_t k = threadIdx.x; k < nvec; k += kPackThreads) vz[k] = make_uint4(0, 0, 0, 0);
    for (uint64_t k = head + nvec * 16 + threadIdx.x; k < zlen; k += kPackThreads) z[k] = 0;
  }
}

}  // namespace

extern "C" {

hipError_t modelx_tar_index(const void* tar, uint64_t tar_len, TarEntry* entries,
                            uint32_t max_entries, TarWalkResult* result_dev,
                            hipStream_t stream) {
  hipLaunchKernelGGL(tar_index_kernel, dim3(1), dim3(kIndexThreads), 0, stream,
                     static_cast<const uint8_t*>(tar), tar_len,
                     entries, max_entries, result_dev);
  return hipGetLastError();
}

hipError_t modelx_tar_scatter(const void* tar, const CopySeg* segs, uint32_t nsegs,
                              hipStream_t stream) {
  if (nsegs == 0) return hipSuccess;
  hipLaunchKernelGGL(tar_scatter_kernel, dim3(nsegs), dim3(kScatterThreads), 0, stream,
                     static_cast<const uint8_t*>(tar), segs, nsegs);
  return hipGetLastError();
}

hipError_t modelx_tar_pack(void* tar, const PackSeg* segs, uint32_t nsegs, hipStream_t stream) {
  if (nsegs == 0) return hipSuccess;
  hipLaunchKernelGGL(tar_pack_kernel, dim3(nsegs), dim3(kPackThreads), 0, stream,
                     static_cast<uint8_t*>(tar), segs, nsegs);
  return hipGetLastError();
}

}  // extern "C"
