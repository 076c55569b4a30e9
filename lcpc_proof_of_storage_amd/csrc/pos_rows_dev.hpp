// pos_rows_dev.hpp -- the device code the grouped ingest, scrub and repair kernels share:
// a workgroup's rows in LDS and the radix-2 stages over them, forward (k_group_encode,
// k_group_repair_rows) and inverse (k_group_scrub_rows, k_group_repair_rows), the Merkle levels over a
// job's leaves (k_group_ingest_trees, k_group_repair_trees) and the table lookup of a chunk wave.
// Everything is __forceinline__: a kernel that calls these is the kernel that spelled them out.
#pragma once
#include "blake3_dev.hpp"
#include "field.hpp"
#include "pos.hpp"

namespace lcpc {

__device__ __forceinline__ int bitrev_bits(int x, int bits) {
  return (int)(__builtin_bitreverse32((uint32_t)x) >> (32 - bits));
}
// The slot of a row's LDS that k_group_encode stores at position c of the stored row, and the stored
// position whose word goes to slot c on the way back: the map is its own inverse.
__device__ __forceinline__ int row_slot(int c, int log_enc) {
  return LCPC_FFT_OUTPUT_BITREV ? c : bitrev_bits(c, log_enc);
}
// element (tile slot t, row r of the tile, point i) of a workgroup's LDS: POS_INGEST_TILE_ROWS = 8
// rows of 2^log_enc points per tile slot
__device__ __forceinline__ int row_elem(int t, int r, int i, int log_enc) {
  return (t << (3 + log_enc)) + (r << log_enc) + i;
}

// k_ntt_small's radix-2 DIF stages over the `total` elements of a workgroup of 256 threads, rows of
// 2^log_enc points: gap = 2^lg, w_enc^(enc / (2 gap) j) = tw[j << (MAX_LOG - 1 - lg)].  A barrier
// before every stage and one after the last.  NT: the workgroup's threads where they are not 256
// (k_group_locate_bm: one wave over its one row).
template <class F, int NT = 256>
__device__ __forceinline__ void rows_forward_stages(Fe<F> *buf, int log_enc, int total, const uint32_t *__restrict__ tw) {
  const int enc = 1 << log_enc;
  for (int lg = log_enc - 1; lg >= 0; lg--) {
    __syncthreads();
    const int gap = 1 << lg;
    for (int idx = threadIdx.x; idx < total / 2; idx += NT) {
      const int row = idx >> (log_enc - 1), i = idx & (enc / 2 - 1);
      const int j = i & (gap - 1);
      const int base = (row << log_enc) + ((i >> lg) << (lg + 1));
      const Fe<F> a = buf[base + j], b = buf[base + j + gap];
      buf[base + j] = fe_add<F>(a, b);
      buf[base + j + gap] = j ? fe_mul<F>(fe_sub_lazy<F>(a, b), fe_load<F>(tw, (size_t)j << (POS_INGEST_MAX_LOG_ENC - 1 - lg)))
                              : fe_sub<F>(a, b);
    }
  }
  __syncthreads();
}

// The same stages undone, in reverse order with the inverse twiddles w^-j = tw[TW_N - (j << ..)], each
// (A, B) -> (A + B w^-j, A - B w^-j) = 2 (a, b): the factor 2 per stage stays in (pos_scrub.hip, THE
// ROW CHECK).  A barrier before every stage and one after the last.
template <class F>
__device__ __forceinline__ void rows_inverse_stages(Fe<F> *buf, int log_enc, int total, const uint32_t *__restrict__ tw) {
  constexpr int TW_N = 1 << POS_INGEST_MAX_LOG_ENC;
  const int enc = 1 << log_enc;
  for (int lg = 0; lg < log_enc; lg++) {
    __syncthreads();
    const int gap = 1 << lg;
    for (int idx = threadIdx.x; idx < total / 2; idx += 256) {
      const int row = idx >> (log_enc - 1), i = idx & (enc / 2 - 1);
      const int j = i & (gap - 1);
      const int base = (row << log_enc) + ((i >> lg) << (lg + 1));
      const Fe<F> a = buf[base + j];
      Fe<F> b = buf[base + j + gap];
      if (j) b = fe_mul<F>(b, fe_load<F>(tw, (size_t)(TW_N - (j << (POS_INGEST_MAX_LOG_ENC - 1 - lg)))));
      buf[base + j] = fe_add<F>(a, b);
      buf[base + j + gap] = fe_sub<F>(a, b);
    }
  }
  __syncthreads();
}

// The tree over the enc leaves at tree[0, 32 enc): every level is hashed from the one below it
// (MerkleTree::to_bytes: leaves || parents, root last); a barrier orders a level's stores -- and, before
// the first level, the leaves' -- before the next level's loads, all by this workgroup of 256 threads.
__device__ __forceinline__ void merkle_levels(uint8_t *tree, uint32_t enc) {
  size_t in = 0;
  for (uint32_t n = enc; n > 1; n >>= 1) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n / 2; i += 256) {
      uint32_t msg[16], o[8];
      b3::load8(reinterpret_cast<const uint32_t *>(tree + 32 * (in + 2 * i)), msg);
      b3::load8(reinterpret_cast<const uint32_t *>(tree + 32 * (in + 2 * i + 1)), msg + 8);
      b3::hash64(msg, o);
      b3::store8(reinterpret_cast<uint32_t *>(tree + 32 * (in + n + i)), o);
    }
    in += n;
  }
}

// A chunk kernel's workgroup is four waves and wave w of the launch reads waves[w] (wave-uniform: no
// search).  false: the launch has no such wave.
__device__ __forceinline__ bool chunk_wave(const PosIngestWave *__restrict__ waves, uint32_t n_waves, uint32_t &wave,
                                           PosIngestWave &wv) {
  wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t w = blockIdx.x * 4 + wave;
  if (w >= n_waves) return false;
  wv = waves[w];
  return true;
}

}  // namespace lcpc
