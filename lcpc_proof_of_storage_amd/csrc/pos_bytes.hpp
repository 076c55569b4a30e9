// pos_bytes.hpp -- device helpers of the kernels that read a WriteableFt63 file image directly
// (pos.hip, pos_eval.hip): 7 little-endian data bytes per element, moved as 56-byte runs of 8
// elements (7 aligned u64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace lcpc {

// a block of the LDS-staged byte kernels covers 2048 elements (14336 bytes, a multiple of 16)
constexpr int PACK_EL = 2048, PACK_BYTES = 7 * PACK_EL;

// element k = bits [56k, 56k + 56) of the 448-bit little-endian run q
__device__ __forceinline__ uint64_t pack7_elem(const uint64_t q[7], int k) {
  const int bit = 56 * k, wi = bit >> 6, sh = bit & 63;
  uint64_t v = q[wi] >> sh;
  if (sh > 8 && wi + 1 < 7) v |= q[wi + 1] << (64 - sh);
  return v & 0x00ffffffffffffffull;
}

// the 56-byte run at byte offset off (a multiple of 8; bytes 8-byte aligned) of an image of
// n_bytes bytes, zero padded past its end
__device__ __forceinline__ void pack7_load_run(const uint8_t *__restrict__ bytes, size_t n_bytes, size_t off,
                                               uint64_t q[7]) {
  if (off + 56 <= n_bytes) {
    const uint64_t *w = reinterpret_cast<const uint64_t *>(bytes + off);
#pragma unroll
    for (int i = 0; i < 7; i++) q[i] = w[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 7; i++) {  // (static indices: q stays in registers)
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const size_t b = off + 8 * i + j;
      if (b < n_bytes) w |= (uint64_t)bytes[b] << (8 * j);
    }
    q[i] = w;
  }
}

}  // namespace lcpc
