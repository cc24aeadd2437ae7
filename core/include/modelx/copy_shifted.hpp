// Device-side body of a workgroup copy onto a 16 B aligned destination grid,
// whatever 16 B phase the source has against it: full 16 B stores built from
// two adjacent aligned source words. Shared by the tar pack kernel
// (core/hip/tar.hip) and the off-grid dedup gather (core/hip/dedup.hip).
// Device code only; every function expects a workgroup of kPackThreads.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace modelx {
namespace devcopy {

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

// Copies len bytes src -> dst with the whole workgroup. The destination
// decides the vector grid; only the <16 B head and tail go bytewise. The
// shifted body reads the aligned 16 B words that hold the first and the last
// source byte of the body whole, so a few bytes beside the source are read
// (never past the aligned word a source byte lives in).
__device__ __forceinline__ void copy_to_aligned_grid(const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst, uint64_t len) {
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

}  // namespace devcopy
}  // namespace modelx
