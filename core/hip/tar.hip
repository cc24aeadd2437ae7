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

constexpr int kPackThreads = 256;
// 16 B vectors per thread per trip, all loaded before the first is stored.
// Measured flat between 4 and 16 on aligned sources (profiles/tar_pack.md).
constexpr int kPackUnroll = 8;
// The shifted body loads two pieces per vector. Measured on 1 GiB at source
// phase 1: 2 vectors per trip 2055-2107 GiB/s, 4 vectors 1723-1759, 8 vectors
// 1729 (profiles/tar_pack.md); the aligned body measures the same at 4, 8, 16.
constexpr int kPackShiftUnroll = 2;

// Native vector type for the body: a load of it is one 16 B load in the IR.
// (A uint4 struct copy is a memcpy, and load-then-store pairs of those fold
// into one memcpy each — a load/wait/store chain with one load in flight.)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Dword vectors of 1..4 elements at dword alignment, for the shifted body.
template <int N>
struct PackDwords {
  typedef uint32_t type __attribute__((ext_vector_type(N), aligned(4)));
};

// The five dwords Q..Q+4 of the aligned word pair at p: the tail of the first
// word and the head of the second, each loaded at exactly its width. (Loading
// both words whole leaves dead lanes that the register allocator hands to the
// next load, and the write-after-write wait that follows drains the queue.)
template <int Q>
struct PackWindow {
  typename PackDwords<4 - Q>::type a;
  typename PackDwords<Q + 1>::type b;
  __device__ __forceinline__ void load(const uint32_t* __restrict__ p) {
    a = *reinterpret_cast<const typename PackDwords<4 - Q>::type*>(p + Q);
    b = *reinterpret_cast<const typename PackDwords<Q + 1>::type*>(p + 4);
  }
  __device__ __forceinline__ uint32_t dword(int i) const {  // i = 0..4, constant
    return i < 4 - Q ? a[i < 4 - Q ? i : 0] : b[i < 4 - Q ? 0 : i - (4 - Q)];
  }
  // 16 source bytes starting 4*Q + s bytes into the pair: alignbyte(h, l, s)
  // is bytes s..s+3 of the 8-byte value {h:l}.
  __device__ __forceinline__ u32x4 shifted(uint32_t s) const {
    u32x4 r;
    r.x = __builtin_amdgcn_alignbyte(dword(1), dword(0), s);
    r.y = __builtin_amdgcn_alignbyte(dword(2), dword(1), s);
    r.z = __builtin_amdgcn_alignbyte(dword(3), dword(2), s);
    r.w = __builtin_amdgcn_alignbyte(dword(4), dword(3), s);
    return r;
  }
};

// Body of a misaligned-source copy: vd[k] = 16 bytes at byte offset
// 16*k + 4*Q + b of the aligned words at ws (4 dwords each). Touches words
// 0..nvec inclusive and nothing outside them; the caller guarantees
// 4*Q + b > 0, so word nvec still holds a source byte.
template <int Q>
__device__ __forceinline__ void pack_body_shifted(const uint32_t* __restrict__ ws,
                                                  u32x4* __restrict__ vd, uint64_t nvec,
                                                  uint32_t b) {
  constexpr uint64_t kStep = static_cast<uint64_t>(kPackThreads) * kPackShiftUnroll;
  uint64_t k = threadIdx.x;
  for (; k + kStep - kPackThreads < nvec; k += kStep) {
    PackWindow<Q> win[kPackShiftUnroll];
#pragma unroll
    for (int u = 0; u < kPackShiftUnroll; u++) win[u].load(ws + 4 * (k + u * kPackThreads));
#pragma unroll
    for (int u = 0; u < kPackShiftUnroll; u++) vd[k + u * kPackThreads] = win[u].shifted(b);
  }
  for (; k < nvec; k += kPackThreads) {
    PackWindow<Q> win;
    win.load(ws + 4 * k);
    vd[k] = win.shifted(b);
  }
}

__device__ __forceinline__ void pack_body_aligned(const u32x4* __restrict__ vs,
                                                  u32x4* __restrict__ vd, uint64_t nvec) {
  constexpr uint64_t kStep = static_cast<uint64_t>(kPackThreads) * kPackUnroll;
  uint64_t k = threadIdx.x;
  for (; k + kStep - kPackThreads < nvec; k += kStep) {
    u32x4 v[kPackUnroll];
#pragma unroll
    for (int u = 0; u < kPackUnroll; u++) v[u] = vs[k + u * kPackThreads];
#pragma unroll
    for (int u = 0; u < kPackUnroll; u++) vd[k + u * kPackThreads] = v[u];
  }
  for (; k < nvec; k += kPackThreads) vd[k] = vs[k];
}

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
  if (len) {
    uint64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    if (head > len) head = len;
    for (uint64_t k = threadIdx.x; k < head; k += kPackThreads) dst[k] = src[k];
    uint64_t nvec = (len - head) / 16;
    if (nvec) {
      u32x4* vd = reinterpret_cast<u32x4*>(dst + head);
      uintptr_t s = reinterpret_cast<uintptr_t>(src + head);
      uint32_t phase = static_cast<uint32_t>(s & 15u);
      uint32_t b = phase & 3u;
      if (phase == 0) {
        pack_body_aligned(reinterpret_cast<const u32x4*>(s), vd, nvec);
      } else {
        const uint32_t* ws = reinterpret_cast<const uint32_t*>(s - phase);
        switch (phase >> 2) {  // uniform across the workgroup
          case 0: pack_body_shifted<0>(ws, vd, nvec, b); break;
          case 1: pack_body_shifted<1>(ws, vd, nvec, b); break;
          case 2: pack_body_shifted<2>(ws, vd, nvec, b); break;
          default: pack_body_shifted<3>(ws, vd, nvec, b); break;
        }
      }
    }
    for (uint64_t k = head + nvec * 16 + threadIdx.x; k < len; k += kPackThreads)
      dst[k] = src[k];
  }
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
