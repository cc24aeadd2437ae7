// The DEFLATE kernel's Huffman builder alone (gfx950), for the tests. One
// workgroup of 256 threads stages a histogram into a deflate::Trees in LDS,
// where the chunk kernel (deflate.hip) keeps its lit/len counts, runs
// deflate::build_lengths with the chunk kernel's group context
// (modelx/deflate_wg.hpp) and writes back the lengths and the return value.
// The tests hold that to the builder on the host on histograms no chunk
// produces: the Kraft sum above one, keys with the top bits set, the filler
// codes. Nothing in the engine's data path launches it. It is a file of its
// own so that the chunk kernel compiles exactly as it does without it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/deflate_core.hpp"
#include "modelx/deflate_wg.hpp"
#include "modelx/device_abi.hpp"

namespace {

namespace df = modelx::deflate;
using modelx::deflate_wg::kThreads;
using modelx::deflate_wg::WgCtx;

__global__ __launch_bounds__(kThreads) void deflate_code_lengths_kernel(
    const uint32_t* __restrict__ hist, uint32_t nsym, uint32_t maxbits, uint32_t complete,
    uint8_t* __restrict__ len_out, uint32_t* __restrict__ ok_out) {
  __shared__ df::Trees t;
  const uint32_t tid = threadIdx.x;
  const WgCtx cx{tid};
  for (uint32_t i = tid; i < 288; i += kThreads) {
    t.hist_ll[i] = i < nsym ? hist[i] : 0u;
    t.len_ll[i] = 0;
  }
  __syncthreads();
  const bool ok =
      df::build_lengths(cx, t.hist_ll, nsym, maxbits, complete != 0, t.len_ll, t.cells);
  __syncthreads();  // a failed build returns without its last barrier
  for (uint32_t i = tid; i < nsym; i += kThreads) len_out[i] = t.len_ll[i];
  if (tid == 0) *ok_out = ok ? 1u : 0u;
}

}  // namespace

extern "C" hipError_t modelx_deflate_code_lengths(const uint32_t* hist_dev, uint32_t nsym,
                                                  uint32_t maxbits, int complete,
                                                  uint8_t* len_dev, uint32_t* ok_dev,
                                                  hipStream_t stream) {
  if (!hist_dev || !len_dev || !ok_dev || nsym < 2 || nsym > df::kNumLL || maxbits < 1 ||
      maxbits > df::kLLBits)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(deflate_code_lengths_kernel, dim3(1), dim3(kThreads), 0, stream, hist_dev,
                     nsym, maxbits, complete ? 1u : 0u, len_dev, ok_dev);
  return hipGetLastError();
}
