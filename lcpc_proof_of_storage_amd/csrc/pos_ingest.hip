// pos_ingest.hip -- many small files turned into stored files in one pass.  A server that
// takes uploads of small files, or a client that needs the root of every file it hands over, pays per
// file about ten launches, four copies and two round trips for an encode of a few dozen short rows.
// Here the host packs the raw images of a whole staging group into one arena with tables (pos.hpp:
// PosIngestJob / Tile / Wg / Wave) and this unit does the group's work in three launches:
//
//   k_group_encode         a workgroup holds tiles of up to 8 whole rows of one length in LDS.  An element
//                          is 7 bytes of the image, read through the two aligned 8-byte words that hold it,
//                          clipped to the image's own end (pack7_elem's bit arithmetic at any element
//                          index; the raw limb is the element, as k_pack7 leaves it), rows zero padded to
//                          enc.  The rows go through k_ntt_small's radix-2 DIF stages -- the same
//                          butterfly, the same field calls in the same order -- with one twiddle table of
//                          2^10 points read by stride, so one launch covers every enc of a group, and
//                          leave canonical (fe_from_mont) and column-major: a full tile's column segment
//                          is one 64-byte store.  With LCPC_FFT_OUTPUT_BITREV = 0 the store reads the
//                          bit-reversed position, which is ntt_rows' reordering pass.
//   k_group_ingest_chunks  a wave per (job, 64 columns, 1-KiB chunk): blake3_dev.hpp's column-major chunk
//                          pass on the canonical words (k_group_leaf_dot without the dot).
//   k_group_ingest_trees   a workgroup per job: a lane per column folds the column's chaining values to
//                          its leaf with a register stack (leaf_fold_stack: selects, no dynamic index),
//                          then the 2 enc - 1 digests are built level by level behind workgroup barriers.
//
// Control flow is uniform over a workgroup in the first kernel (its tiles share enc) and over a wave in
// the other two (a wave's lanes share a job).  No atomics.
#include "kernels.hpp"
#include "pos_rows_dev.hpp"
#include "prof.hpp"

namespace lcpc {

hipError_t ntt_tw_table_ft63(uint32_t *, int, bool, hipStream_t);  // ntt_ft63.hip: the table every Ft63 plan builds

namespace {

using namespace b3;

// element at byte offset b (= 7 x its index) of an image of n_bytes bytes that starts 8-byte aligned
// and is zero past its end: bits [8 (b & 7), +56) of the aligned words b / 8 and b / 8 + 1, the second
// needed iff the shift exceeds 8 (pack7_elem).  A word is loaded only if the image reaches into it.
__device__ __forceinline__ uint64_t ingest_elem(const uint64_t *__restrict__ img, size_t n_bytes, size_t b) {
  auto word = [&](size_t w) -> uint64_t {
    const size_t o = 8 * w;
    if (o >= n_bytes) return 0;
    const uint64_t v = img[w];
    return o + 8 > n_bytes ? v & (~(uint64_t)0 >> (8 * (o + 8 - n_bytes))) : v;
  };
  const size_t w = b >> 3;
  const int sh = (int)(b & 7) * 8;
  uint64_t v = word(w) >> sh;
  if (sh > 8) v |= word(w + 1) << (64 - sh);
  return v & 0x00ffffffffffffffull;
}

// workgroup b of the launch reads wgs[b]; element idx of its LDS is (tile slot, row of the tile, point)
template <class F>
__global__ __launch_bounds__(256) void k_group_encode(const uint8_t *__restrict__ arena,
                                                      const PosIngestJob *__restrict__ jobs,
                                                      const PosIngestTile *__restrict__ tiles,
                                                      const PosIngestWg *__restrict__ wgs,
                                                      const uint32_t *__restrict__ tw, uint8_t *__restrict__ enc_out) {
  static_assert(F::N == 2, "a stored file holds WriteableFt63 elements");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Fe<F> *buf = reinterpret_cast<Fe<F> *>(smem);
  const PosIngestWg wg = wgs[blockIdx.x];
  const int log_enc = (int)wg.log_enc, enc = 1 << log_enc;
  const int total = (int)wg.n_tiles << (3 + log_enc);
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int t = idx >> (3 + log_enc), r = (idx >> log_enc) & 7, i = idx & (enc - 1);
    const PosIngestTile tl = tiles[wg.tile0 + t];
    uint64_t v = 0;
    if ((uint32_t)r < tl.n_rows) {
      const PosIngestJob &jb = jobs[tl.job];
      const uint32_t pre = jb.pre;
      if ((uint32_t)i < pre)
        v = ingest_elem(reinterpret_cast<const uint64_t *>(arena + jb.base), jb.n_bytes,
                        7 * ((size_t)(tl.row_lo + r) * pre + i));
    }
    Fe<F> e;
    e.v[0] = (uint32_t)v;
    e.v[1] = (uint32_t)(v >> 32);
    buf[idx] = e;
  }
  rows_forward_stages<F>(buf, log_enc, total, tw);
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int r = idx & 7, c = (idx >> 3) & (enc - 1), t = idx >> (3 + log_enc);
    const PosIngestTile tl = tiles[wg.tile0 + t];
    if ((uint32_t)r >= tl.n_rows) continue;
    const PosIngestJob &jb = jobs[tl.job];
    const Fe<F> v = fe_from_mont<F>(buf[row_elem(t, r, row_slot(c, log_enc), log_enc)]);
    uint64_t *col = reinterpret_cast<uint64_t *>(enc_out + jb.enc_off) + (size_t)c * jb.rows_pad;
    col[tl.row_lo + r] = (uint64_t)v.v[0] | ((uint64_t)v.v[1] << 32);
  }
}

// a workgroup is four waves; wave w of the launch reads waves[w] (wave-uniform: no search)
template <class F>
__global__ __launch_bounds__(256) void k_group_ingest_chunks(const uint8_t *__restrict__ enc,
                                                             const PosIngestJob *__restrict__ jobs,
                                                             const PosIngestWave *__restrict__ waves, uint32_t n_waves,
                                                             uint32_t *__restrict__ cvs) {
  __shared__ uint4 stage[4][64][5];
  const uint32_t lane = threadIdx.x & 63;
  uint32_t wave;
  PosIngestWave wv;
  if (!chunk_wave(waves, n_waves, wave, wv)) return;
  const PosIngestJob jb = jobs[wv.job];
  const size_t n_cols = (size_t)1 << jb.log_enc;
  uint32_t cv[8];
  Fe<F> acc = fe_zero<F>();
  bool unused = false;
  cm_chunk_cv<F, true, true, false, false>(stage[wave], reinterpret_cast<const uint32_t *>(enc + jb.enc_off), jb.n_rows,
                                           n_cols, wv.col_lo, 2 * (size_t)jb.rows_pad, 8, (int)wv.chunk,
                                           (int)jb.n_chunks, nullptr, 0, cv, acc, unused);
  const size_t k = wv.col_lo + lane;
  if (k >= n_cols) return;
  store8(cvs + (jb.cv0 + (size_t)wv.chunk * n_cols + k) * 8, cv);
}

// workgroup j of the launch is job j.  The leaves go to the tree's first enc digests, then every
// level is hashed from the one below it (MerkleTree::to_bytes: leaves || parents, root last); a
// barrier orders a level's stores before the next level's loads, both by this workgroup.
template <int D>
__global__ __launch_bounds__(256) void k_group_ingest_trees(const PosIngestJob *__restrict__ jobs,
                                                            const uint32_t *__restrict__ cvs, uint8_t *trees) {
  const PosIngestJob jb = jobs[blockIdx.x];
  const uint32_t enc = 1u << jb.log_enc;
  uint8_t *tree = trees + 32 * jb.tree0;
  for (uint32_t c0 = 0; c0 < enc; c0 += 256) {
    const uint32_t c = c0 + threadIdx.x;
    if (c >= enc) continue;
    uint32_t leaf[8];
    leaf_fold_stack<D>(cvs + (jb.cv0 + c) * 8, enc, (int)jb.n_chunks, leaf);
    store8(reinterpret_cast<uint32_t *>(tree + 32 * (size_t)c), leaf);
  }
  merkle_levels(tree, enc);
}

}  // namespace

hipError_t pos_ingest_twiddles(uint32_t *tw, hipStream_t s) {
  return ntt_tw_table_ft63(tw, POS_INGEST_MAX_LOG_ENC, LCPC_FFT_OMEGA_INVERSE != 0, s);
}

hipError_t pos_group_ingest(const uint8_t *arena, const PosIngestJob *jobs, size_t n_jobs, const PosIngestTile *tiles,
                            const PosIngestWg *wgs, size_t n_wgs, size_t lds_bytes, const PosIngestWave *waves,
                            size_t n_waves, size_t max_chunks, const uint32_t *tw, uint8_t *enc, uint32_t *cvs,
                            uint8_t *trees, hipStream_t s) {
  if (!n_jobs || !n_waves || !max_chunks || max_chunks > POS_INGEST_MAX_CHUNKS) return hipErrorInvalidValue;
  const size_t blocks = (n_waves + 3) / 4;
  if (n_wgs >= ((size_t)1 << 24) || blocks >= ((size_t)1 << 24) || n_jobs >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  if (lds_bytes > (POS_INGEST_TILE_ROWS << POS_INGEST_MAX_LOG_ENC) * 8) return hipErrorInvalidValue;
  prof::Scope ps("pos_group_ingest", s);
  hipError_t e;
  if (n_wgs) {
    hipLaunchKernelGGL((k_group_encode<Ft63>), dim3((unsigned)n_wgs), dim3(256), lds_bytes, s, arena, jobs, tiles, wgs,
                       tw, enc);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_group_ingest_chunks<Ft63>), dim3((unsigned)blocks), dim3(256), 0, s, enc, jobs, waves,
                     (uint32_t)n_waves, cvs);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (max_chunks <= 256)
    hipLaunchKernelGGL((k_group_ingest_trees<8>), dim3((unsigned)n_jobs), dim3(256), 0, s, jobs, cvs, trees);
  else
    hipLaunchKernelGGL((k_group_ingest_trees<16>), dim3((unsigned)n_jobs), dim3(256), 0, s, jobs, cvs, trees);
  return hipGetLastError();
}

}  // namespace lcpc
