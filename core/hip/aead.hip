// CDNA4 ChaCha20-Poly1305 kernel (gfx950): seals or opens every segment of a
// sealed blob (modelx/aead_core.hpp defines the layout and the arithmetic,
// shared with the host) in one launch, HBM to HBM. One kernel serves both
// directions; AeadJob::open selects which side of the xor is MAC'd and
// whether tags are written or compared.
//
// One wave owns one segment; four waves to a workgroup, the grid capped and
// striding over the segments. 1 GiB at the default 128 KiB segment is 8192
// waves.
//
// Bytes. A row is 1 KiB; lane L owns bytes [16L, 16L + 16) of every row and
// does one global_load_dwordx4 and one global_store_dwordx4 per row: fully
// coalesced, nothing staged through LDS, and src == dst is safe because a
// lane only ever rewrites what it read. The pointers arrive as integers and
// the accesses say themselves that they are global.
//
// Keystream. A quad of lanes computes one 64-byte ChaCha20 block, so the 16
// quads of a wave cover the 16 blocks of a row; the quad (L >> 2) of row t
// has block counter 1 + 16t + (L >> 2). Lane j of a quad holds column j of
// the 4x4 state (a, b, c, d = rows 0..3): the column round is lane-local,
// and the diagonal round is the same quarter round after b, c, d have been
// rotated by 1, 2, 3 lanes within the quad (DPP quad_perm, no LDS), then
// rotated back. After the 20 rounds and the feed-forward a 4x4 transpose
// within the quad (a lane-local rotate by j, three quad_perm moves, a
// rotate back) leaves lane j with keystream words 4j..4j+3: exactly the 16
// bytes it loaded. A block per lane would need 64 B per lane per trip and
// strided accesses; it was not built.
//
// MAC. Poly1305 is a Horner evaluation in r, sequential as written. Here
// lane L keeps its own accumulator and absorbs its own 16-byte ciphertext
// word each row, A = A * R + (word + 2^128) with R = r^64 the same for all
// lanes: one mulmod (25 32x32->64 multiply-adds and a carry) per 16 bytes,
// the same as the sequential form, with no traffic between lanes. With T full
// rows and q blocks in the last, short row (the final one zero-padded to 16
// bytes, which is the AEAD's pad16 rule, so it too carries 2^128), the state
// before the length block is
//   sum_L A_L * r^(64 + q - L)  +  sum_{L < q} tail_L * r^(q - L),
// so each lane multiplies by two powers of its own, the wave adds the limbs
// with shuffles (64-bit sums: 64 loose limbs pass 32 bits), and every lane
// finishes alike: + length block, * r, full carry, + s. All lanes hold the
// tag, so its bytes are stored or compared one per lane.
//
// Per segment set-up: all quads compute block 0 (one row's worth of rounds)
// and r, s are read from lanes 0 and 1; each lane derives R and its two
// powers by square-and-multiply on its own (8 squarings, about 8 multiplies:
// some 20 mulmods against 128 in the hot loop at 128 KiB, which is why the
// default segment is not 64 KiB).
//
// Tags. Seal stores tag i at tags + 16i, which follows n and may be
// unaligned: four dword stores when it is 4 B aligned, else sixteen byte
// stores; plain vector stores either way. Open recomputes the tag, compares
// all 16 bytes with no early exit and on a mismatch does atomicMin of the
// segment index into *bad (the host sets 0xFFFFFFFF first). The plaintext of
// a segment is written before its tag is known; the host hands out nothing
// from a buffer whose open reported a mismatch.
//
// Alignment. dst is 16 B aligned (the engine refuses anything else). A source
// that is not takes the same lane layout through sixteen byte loads per lane
// and row: a view pushed at an odd offset is slower, never different. The
// short last row goes the same way for its final, partial word.
//
// No byte outside [src, src + n) is read; none outside [dst, dst + n) and the
// tag array is written (open reads the tag array and writes only *bad
// besides).
//
// No matrix instructions: the work is 32-bit add/rotate/xor and 26-bit
// multiply-accumulate. No LDS. Compiled without packed fp32 (setup_ext.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modelx/aead_core.hpp"
#include "modelx/device_abi.hpp"

namespace {

namespace ae = modelx::aead;
using modelx::abi::AeadJob;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kMaxBlocks = 2048;  // 8 per CU; the rest grid-strides
constexpr uint64_t kRow = ae::kRowBytes;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4* GlobalVec;
typedef __attribute__((address_space(1))) u32x4* GlobalVecOut;
typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
typedef __attribute__((address_space(1))) uint8_t* GlobalBytesOut;
typedef __attribute__((address_space(1))) uint32_t* GlobalWordOut;

__device__ __forceinline__ uint32_t pick4(uint32_t j, uint32_t v0, uint32_t v1, uint32_t v2,
                                          uint32_t v3) {
  return j == 0 ? v0 : j == 1 ? v1 : j == 2 ? v2 : v3;
}

// Lane j of every quad reads lane (j + s) & 3 of its quad.
template <int kShift>
__device__ __forceinline__ uint32_t quad_rotate(uint32_t v) {
  constexpr int ctrl = kShift == 1 ? 0x39 : kShift == 2 ? 0x4E : 0x93;  // quad_perm
  return static_cast<uint32_t>(
      __builtin_amdgcn_mov_dpp(static_cast<int>(v), ctrl, 0xF, 0xF, true));
}

// out[m] = v[(m + j) & 3], j the lane's own.
__device__ __forceinline__ void rotate_own(uint32_t (&v)[4], uint32_t j) {
  const bool one = j & 1u, two = j & 2u;
  uint32_t a0 = one ? v[1] : v[0], a1 = one ? v[2] : v[1], a2 = one ? v[3] : v[2],
           a3 = one ? v[0] : v[3];
  v[0] = two ? a2 : a0;
  v[1] = two ? a3 : a1;
  v[2] = two ? a0 : a2;
  v[3] = two ? a1 : a3;
}

// The lane's 16 bytes of the ChaCha20 block its quad computes; (a, b, c, d)
// is the lane's column of the input state. All 64 lanes must be active.
__device__ __forceinline__ u32x4 quad_keystream(uint32_t a0, uint32_t b0, uint32_t c0,
                                                uint32_t d0, uint32_t j) {
  uint32_t a = a0, b = b0, c = c0, d = d0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    ae::quarter_round(a, b, c, d);
    b = quad_rotate<1>(b);
    c = quad_rotate<2>(c);
    d = quad_rotate<3>(d);
    ae::quarter_round(a, b, c, d);
    b = quad_rotate<3>(b);
    c = quad_rotate<2>(c);
    d = quad_rotate<1>(d);
  }
  // v[k] is word 4k + j of the block; lane j wants words 4j + k
  uint32_t v[4] = {a + a0, b + b0, c + c0, d + d0};
  rotate_own(v, j);
  uint32_t t[4] = {v[0], quad_rotate<1>(v[3]), quad_rotate<2>(v[2]), quad_rotate<3>(v[1])};
  rotate_own(t, (4u - j) & 3u);
  return u32x4{t[0], t[1], t[2], t[3]};
}

// `count` <= 16 bytes at p as a zero-padded word.
__device__ __forceinline__ u32x4 load_bytes(uint64_t addr, uint32_t count) {
  GlobalBytes p = (GlobalBytes)addr;
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
  for (uint32_t i = 0; i < 16; i++)
    if (i < count) w[i >> 2] |= static_cast<uint32_t>(p[i]) << (8u * (i & 3u));
  return u32x4{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ void store_bytes(uint64_t addr, u32x4 v, uint32_t count) {
  GlobalBytesOut p = (GlobalBytesOut)addr;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t i = 0; i < 16; i++)
    if (i < count) p[i] = static_cast<uint8_t>(w[i >> 2] >> (8u * (i & 3u)));
}

// Mask of the bytes of word w (0..3) that lie in the first `count` of 16.
__device__ __forceinline__ uint32_t word_mask(uint32_t count, uint32_t w) {
  return count >= 4 * w + 4 ? 0xFFFFFFFFu : count <= 4 * w ? 0u : (1u << (8u * (count - 4 * w))) - 1u;
}

template <bool kSrcAligned>
__device__ __forceinline__ u32x4 load_word(uint64_t addr) {
  if constexpr (kSrcAligned) return *(GlobalVec)addr;
  else return load_bytes(addr, 16);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
    v += static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(v), d, 64));
  return v;
}

__device__ __forceinline__ uint32_t broadcast(uint32_t v, int lane) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), lane));
}

template <bool kSrcAligned>
__global__ __launch_bounds__(kThreads) void aead_segments_kernel(const AeadJob job,
                                                                 uint32_t* bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t j = lane & 3u;
  // the lane's column of the state rows that do not change
  const uint32_t col_a = pick4(j, ae::kSigma0, ae::kSigma1, ae::kSigma2, ae::kSigma3);
  const uint32_t col_b = pick4(j, job.key.w[0], job.key.w[1], job.key.w[2], job.key.w[3]);
  const uint32_t col_c = pick4(j, job.key.w[4], job.key.w[5], job.key.w[6], job.key.w[7]);
  const bool open = job.open != 0;

  for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; seg < job.nseg;
       seg += static_cast<uint64_t>(gridDim.x) * kWaves) {
    const uint64_t off = seg * job.seg_bytes;
    const uint64_t len = job.n - off < job.seg_bytes ? job.n - off : job.seg_bytes;
    uint32_t nonce[3];
    ae::segment_nonce(seg, seg == job.nseg - 1, nonce);
    const uint32_t col_d = pick4(j, 0, nonce[0], nonce[1], nonce[2]);  // counter 0

    // block 0: r from words 0..3 (lane 0 of a quad), s from words 4..7 (lane 1)
    const u32x4 k0 = quad_keystream(col_a, col_b, col_c, col_d, j);
    const ae::Fe r = ae::fe_clamped_r(broadcast(k0.x, 0), broadcast(k0.y, 0),
                                      broadcast(k0.z, 0), broadcast(k0.w, 0));
    const uint32_t s[4] = {broadcast(k0.x, 1), broadcast(k0.y, 1), broadcast(k0.z, 1),
                           broadcast(k0.w, 1)};

    const uint32_t trips = static_cast<uint32_t>(len / kRow);
    const uint32_t tail = static_cast<uint32_t>(len % kRow);
    const uint32_t q_full = tail / 16u, rem = tail % 16u;
    const uint32_t q = q_full + (rem ? 1u : 0u);  // blocks of the short row, <= 64

    // R = r^64 and the lane's powers r^(64 + q - lane), r^(q - lane)
    const uint32_t e_rows = 64u + q - lane;
    const uint32_t e_tail = lane < q ? q - lane : 0u;
    ae::Fe base = r, p_rows = ae::fe_one(), p_tail = ae::fe_one(), R = r;
    for (uint32_t k = 0; k < 8; k++) {
      const ae::Fe5 base5 = ae::fe_times5(base);
      if (k == 6) R = base;
      if ((e_rows >> k) & 1u) p_rows = ae::fe_mulmod(p_rows, base, base5);
      if ((e_tail >> k) & 1u) p_tail = ae::fe_mulmod(p_tail, base, base5);
      if (k < 7) base = ae::fe_mulmod(base, base, base5);
    }
    const ae::Fe5 R5 = ae::fe_times5(R);

    const uint64_t src = job.src + off + 16u * lane;
    const uint64_t dst = job.dst + off + 16u * lane;
    const uint32_t quad = lane >> 2;
    ae::Fe acc{{0, 0, 0, 0, 0}};
    for (uint32_t t = 0; t < trips; t++) {
      const uint32_t counter = 1u + 16u * t + quad;
      const u32x4 ks = quad_keystream(col_a, col_b, col_c, j == 0 ? counter : col_d, j);
      const u32x4 in = load_word<kSrcAligned>(src + static_cast<uint64_t>(t) * kRow);
      const u32x4 out = in ^ ks;
      *(GlobalVecOut)(dst + static_cast<uint64_t>(t) * kRow) = out;
      const u32x4 m = open ? in : out;
      acc = ae::fe_add(ae::fe_mulmod(acc, R, R5), ae::fe_from_words(m.x, m.y, m.z, m.w, 1));
    }

    ae::Fe part = ae::fe_mulmod(acc, p_rows);
    if (tail) {  // wave-uniform
      const uint32_t counter = 1u + 16u * trips + quad;
      const u32x4 ks = quad_keystream(col_a, col_b, col_c, j == 0 ? counter : col_d, j);
      if (lane < q) {
        const uint64_t at = static_cast<uint64_t>(trips) * kRow;
        const bool whole = lane < q_full;
        const uint32_t count = whole ? 16u : rem;
        u32x4 in;
        if (whole) in = load_word<kSrcAligned>(src + at);
        else in = load_bytes(src + at, rem);
        // the MAC sees the ciphertext zero-padded: no keystream past the end
        const u32x4 out = in ^ (ks & u32x4{word_mask(count, 0), word_mask(count, 1),
                                           word_mask(count, 2), word_mask(count, 3)});
        if (whole) *(GlobalVecOut)(dst + at) = out;
        else store_bytes(dst + at, out, rem);
        const u32x4 m = open ? in : out;
        part = ae::fe_add(part, ae::fe_mulmod(ae::fe_from_words(m.x, m.y, m.z, m.w, 1), p_tail));
      }
    }

    // the wave's sum, the length block, the last multiplication, the tag
    const ae::Fe sum = ae::fe_carry(wave_sum(part.v[0]), wave_sum(part.v[1]),
                                    wave_sum(part.v[2]), wave_sum(part.v[3]),
                                    wave_sum(part.v[4]));
    const ae::Fe h = ae::fe_mulmod(ae::fe_add(sum, ae::fe_length_block(len)), r);
    uint32_t tag[4];
    ae::fe_tag(h, s, tag);

    const uint64_t tag_at = job.tags + ae::kTagBytes * seg;
    const uint32_t my_word = pick4((lane >> 2) & 3u, tag[0], tag[1], tag[2], tag[3]);
    const uint32_t my_byte = (my_word >> (8u * (lane & 3u))) & 0xFFu;  // byte `lane` of the tag
    if (!open) {
      if ((tag_at & 3u) == 0) {
        if (lane < 4) ((GlobalWordOut)tag_at)[lane] = pick4(lane, tag[0], tag[1], tag[2], tag[3]);
      } else if (lane < 16) {
        ((GlobalBytesOut)tag_at)[lane] = static_cast<uint8_t>(my_byte);
      }
    } else {
      uint32_t diff = 0;
      if (lane < 16) diff = ((GlobalBytes)tag_at)[lane] ^ my_byte;
      if (__ballot(diff != 0) != 0 && lane == 0) atomicMin(bad, static_cast<uint32_t>(seg));
    }
  }
}

}  // namespace

extern "C" hipError_t modelx_aead_segments(AeadJob job, uint32_t* bad_dev, hipStream_t stream) {
  if (job.nseg == 0) return hipSuccess;
  if (!ae::valid_segment(job.seg_bytes) || job.n == 0 ||
      job.nseg != ae::segment_count(job.n, job.seg_bytes) || job.nseg >= UINT32_MAX ||
      (job.dst & 15u) || (job.open && !bad_dev))
    return hipErrorInvalidValue;
  const uint64_t want = (job.nseg + kWaves - 1) / kWaves;
  const uint32_t blocks = want < kMaxBlocks ? static_cast<uint32_t>(want) : kMaxBlocks;
  if (job.src & 15u)
    hipLaunchKernelGGL(aead_segments_kernel<false>, dim3(blocks), dim3(kThreads), 0, stream,
                       job, bad_dev);
  else
    hipLaunchKernelGGL(aead_segments_kernel<true>, dim3(blocks), dim3(kThreads), 0, stream, job,
                       bad_dev);
  return hipGetLastError();
}
