// How a workgroup of 256 threads runs deflate_core.hpp's Huffman builder: the
// group context of core/hip/deflate.hip's chunk kernel, and of the one-workgroup
// launcher in core/hip/deflate_lengths.hip through which the tests reach the
// builder alone. Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace modelx {
namespace deflate_wg {

constexpr uint32_t kThreads = 256;

struct WgCtx {
  uint32_t tid;
  static constexpr uint32_t width = kThreads;
  __device__ void sync() const { __syncthreads(); }
  // Call `iter` uses cell iter % 3; thread 0 clears the cell of call iter + 2
  // behind this call's barrier, after its last readers (call iter - 1) and a
  // barrier before its next writers.
  __device__ uint32_t group_max(uint32_t v, uint32_t* cells, uint32_t iter) const {
    uint32_t* c = cells + iter % 3;
    if (v) atomicMax(c, v);
    __syncthreads();
    uint32_t r = *c;
    if (tid == 0) cells[(iter + 2) % 3] = 0;
    return r;
  }
};

}  // namespace deflate_wg
}  // namespace modelx
