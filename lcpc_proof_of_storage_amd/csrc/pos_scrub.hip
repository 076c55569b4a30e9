// pos_scrub.hip -- many stored files scrubbed in one pass.  A scrubber walks its whole
// store and nearly every file it reads is clean; per file the single entries cost two uploads of the
// image and a dozen launches for a few dozen short rows.  Here the host packs the written rows of a
// whole staging group of images into one arena with tables (pos.hpp: PosScrubJob and the ingest's Tile
// / Wg / Wave) and this unit answers "which of these files has a finding" in three launches:
//
//   k_group_scrub_rows    a workgroup holds tiles of up to 8 whole stored rows of one length in LDS (a
//                         full tile's column segment is one 64-byte load) and runs k_group_encode
//                         backwards: dirty[row] = the row is not the encoding of pre coefficients.
//   k_group_scrub_chunks  a wave per (job, 64 columns, 1-KiB chunk): blake3_dev.hpp's column-major chunk
//                         pass on the canonical words, with its check that every word is < p; the flag
//                         goes to the (chunk, column)'s own byte.
//   k_group_scrub_leaves  a workgroup per job: a lane per column folds the chaining values to the leaf
//                         (leaf_fold_stack) and decides the column's status against the stored leaf; a
//                         lane per stored parent hashes its two stored children and compares (node
//                         enc + m of MerkleTree::to_bytes has the children 2 m and 2 m + 1, so no level
//                         waits for another); one lane compares the stored root with the expected one.
//
// THE ROW CHECK.  k_group_encode is E = S . D: the radix-2 DIF stages D over a row's LDS slots (stage
// lg, gap 2^lg, from lg = log_enc - 1 down to 0: (a, b) -> (a + b, (a - b) w^j), w^j = tw[j << (9 - lg)])
// and the store S, which puts slot c (LCPC_FFT_OUTPUT_BITREV = 1) or slot bitrev(c) (= 0) at stored
// position c.  Whether tw holds the powers of omega or of its inverse (LCPC_FFT_OMEGA_INVERSE) is the
// table's business: both kernels read the one pos_ingest_twiddles built.  This kernel applies S^-1 on
// the load -- stored position c goes to the slot the encode read it from, under the same switch -- and
// then undoes the stages in reverse order, lg = 0 up to log_enc - 1, each by
// (A, B) -> (A + B w^-j, A - B w^-j) = 2 (a, b), with w^-j = tw[1024 - (j << (9 - lg))] (tw[0] = 1 is
// never needed: j = 0 skips the product, as the encode does).  So slot k ends with enc times coefficient
// k of the polynomial the row evaluates, for either setting of either switch, and the row is a codeword
// iff the slots k >= pre are zero: what decode_row / ifft_oi test after their reordering and 1 / n
// scaling, and what the locator's syndrome scan tests at the bit-reversed positions of the plan's
// output.  The stored words are canonical; they are used as Montgomery residues as they are (the residue
// v stands for v / R) and the factor enc stays in: the map is linear, so both multiply every coefficient
// by one non-zero constant and leave the zero test alone.  A word that is not < p makes its row's answer
// meaningless (the host reports such a job as unchecked from the column flags); the field calls are
// straight-line code, so it neither faults nor loops.
//
// Control flow is uniform over a workgroup in the first kernel (its tiles share enc) and over a wave in
// the chunk kernel; the third is uniform over the workgroup but for the column and node bounds.  No
// atomics: every output byte has one writer.
#include "kernels.hpp"
#include "pos_rows_dev.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

using namespace b3;

// workgroup b of the launch reads wgs[b]; element idx of its LDS is (tile slot, row of the tile, slot)
template <class F>
__global__ __launch_bounds__(256) void k_group_scrub_rows(const uint8_t *__restrict__ arena,
                                                          const PosScrubJob *__restrict__ jobs,
                                                          const PosIngestTile *__restrict__ tiles,
                                                          const PosIngestWg *__restrict__ wgs,
                                                          const uint32_t *__restrict__ tw, uint8_t *__restrict__ dirty) {
  static_assert(F::N == 2, "a stored file holds WriteableFt63 elements");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Fe<F> *buf = reinterpret_cast<Fe<F> *>(smem);
  const PosIngestWg wg = wgs[blockIdx.x];
  const int log_enc = (int)wg.log_enc, enc = 1 << log_enc;
  const int total = (int)wg.n_tiles << (3 + log_enc);
  // S^-1: the rows of a tile are the fast index, so a full tile's column segment is 64 contiguous bytes
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int r = idx & 7, c = (idx >> 3) & (enc - 1), t = idx >> (3 + log_enc);
    const PosIngestTile tl = tiles[wg.tile0 + t];
    uint64_t v = 0;
    if ((uint32_t)r < tl.n_rows) {
      const PosScrubJob &jb = jobs[tl.job];
      const uint64_t *col = reinterpret_cast<const uint64_t *>(arena + jb.img) + (size_t)c * jb.rows_pad;
      v = col[tl.row_lo + r];
    }
    Fe<F> e;
    e.v[0] = (uint32_t)v;
    e.v[1] = (uint32_t)(v >> 32);
    buf[row_elem(t, r, row_slot(c, log_enc), log_enc)] = e;
  }
  // D^-1 (times 2 per stage): the encode's stages in reverse order with the inverse twiddles
  rows_inverse_stages<F>(buf, log_enc, total, tw);
  // a row is dirty iff a slot k >= pre is non-zero.  min(enc, 64) lanes share a row and OR through the
  // wave's ballot; the group's first lane stores the row's byte, 0 or 1: one writer per byte.
  const int log_g = log_enc < 6 ? log_enc : 6, g = 1 << log_g, rows_per_wave = 64 >> log_g;
  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n_rows_lds = (int)wg.n_tiles << 3;
  const uint64_t group_mask = g == 64 ? ~(uint64_t)0 : (((uint64_t)1 << g) - 1);
  for (int r0 = wave * rows_per_wave; r0 < n_rows_lds; r0 += 4 * rows_per_wave) {
    const int row = r0 + (lane >> log_g), li = lane & (g - 1);
    const bool in = row < n_rows_lds;
    PosIngestTile tl = {0, 0, 0, 0};
    int pre = enc;
    uint64_t row0 = 0;
    if (in) {
      tl = tiles[wg.tile0 + (row >> 3)];
      const PosScrubJob &jb = jobs[tl.job];
      pre = (int)jb.pre;
      row0 = jb.row0;
    }
    bool nz = false;
    for (int i = li; i < enc; i += g)
      if (in && i >= pre) nz |= !fe_is_zero<F>(buf[(row << log_enc) + i]);
    const uint64_t votes = __ballot(nz);
    const bool any = ((votes >> ((lane >> log_g) << log_g)) & group_mask) != 0;
    if (in && li == 0 && (uint32_t)(row & 7) < tl.n_rows) dirty[row0 + tl.row_lo + (row & 7)] = any ? 1 : 0;
  }
}

// a workgroup is four waves; wave w of the launch reads waves[w] (wave-uniform: no search)
template <class F>
__global__ __launch_bounds__(256) void k_group_scrub_chunks(const uint8_t *__restrict__ arena,
                                                            const PosScrubJob *__restrict__ jobs,
                                                            const PosIngestWave *__restrict__ waves, uint32_t n_waves,
                                                            uint32_t *__restrict__ cvs, uint8_t *__restrict__ cflags) {
  __shared__ uint4 stage[4][64][5];
  const uint32_t lane = threadIdx.x & 63;
  uint32_t wave;
  PosIngestWave wv;
  if (!chunk_wave(waves, n_waves, wave, wv)) return;
  const PosScrubJob jb = jobs[wv.job];
  const size_t n_cols = (size_t)1 << jb.log_enc;
  uint32_t cv[8];
  Fe<F> acc = fe_zero<F>();
  bool noncanon = false;
  cm_chunk_cv<F, true, true, true, false>(stage[wave], reinterpret_cast<const uint32_t *>(arena + jb.img), jb.n_rows,
                                          n_cols, wv.col_lo, 2 * (size_t)jb.rows_pad, 8, (int)wv.chunk,
                                          (int)jb.n_chunks, nullptr, 0, cv, acc, noncanon);
  const size_t k = wv.col_lo + lane;
  if (k >= n_cols) return;
  const size_t slot = jb.cv0 + (size_t)wv.chunk * n_cols + k;
  store8(cvs + slot * 8, cv);
  cflags[slot] = noncanon ? 1 : 0;
}

__device__ __forceinline__ bool differs8(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t o = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) o |= a[q] ^ b[q];
  return o != 0;
}

// workgroup j of the launch is job j
template <int D>
__global__ __launch_bounds__(256) void k_group_scrub_leaves(const uint8_t *__restrict__ arena,
                                                            const PosScrubJob *__restrict__ jobs,
                                                            const uint32_t *__restrict__ cvs,
                                                            const uint8_t *__restrict__ cflags,
                                                            uint8_t *__restrict__ flags, uint8_t *__restrict__ status,
                                                            uint8_t *__restrict__ digests) {
  const PosScrubJob jb = jobs[blockIdx.x];
  const uint32_t enc = 1u << jb.log_enc;
  const uint8_t *tree = arena + jb.tree;
  if (!jb.tree_only) {
    for (uint32_t c0 = 0; c0 < enc; c0 += 256) {
      const uint32_t c = c0 + threadIdx.x;
      if (c >= enc) continue;
      uint32_t leaf[8];
      leaf_fold_stack<D>(cvs + (jb.cv0 + c) * 8, enc, (int)jb.n_chunks, leaf);
      uint32_t bad = 0;
      for (uint32_t k = 0; k < jb.n_chunks; k++) bad |= cflags[jb.cv0 + (size_t)k * enc + c];
      uint8_t st = 0;
      if (bad) {  // a column with a word that is not < p has no digest
#pragma unroll
        for (int q = 0; q < 8; q++) leaf[q] = 0;
        st = 2;
      } else if (jb.tree_kind) {
        uint32_t stored[8];
        load8(reinterpret_cast<const uint32_t *>(tree + 32 * (size_t)c), stored);
        st = differs8(leaf, stored) ? 1 : 0;
      }
      store8(reinterpret_cast<uint32_t *>(digests + 32 * (jb.col0 + c)), leaf);
      status[jb.col0 + c] = st;
    }
  }
  // every stored parent against its two stored children: by induction from the leaves up this is
  // MerkleTree::new(leaves) == tree, with no level waiting for the one below it
  int bad_parent = 0;
  if (jb.tree_kind == 2) {
    for (uint32_t m = threadIdx.x; m < enc - 1; m += 256) {
      uint32_t msg[16], o[8], stored[8];
      load8(reinterpret_cast<const uint32_t *>(tree + 32 * (size_t)(2 * m)), msg);
      load8(reinterpret_cast<const uint32_t *>(tree + 32 * (size_t)(2 * m + 1)), msg + 8);
      hash64(msg, o);
      load8(reinterpret_cast<const uint32_t *>(tree + 32 * (size_t)(enc + m)), stored);
      bad_parent |= differs8(o, stored) ? 1 : 0;
    }
  }
  const int any_bad = __syncthreads_or(bad_parent);
  if (threadIdx.x == 0) {
    uint8_t consistent = POS_SCRUB_NOT_EVALUATED, root_ok = POS_SCRUB_NOT_EVALUATED;
    if (jb.tree_kind == 2) {
      consistent = any_bad ? 0 : 1;
      if (jb.has_root) {
        uint32_t a[8], b[8];
        load8(reinterpret_cast<const uint32_t *>(tree + 32 * (size_t)(2 * enc - 2)), a);
        load8(reinterpret_cast<const uint32_t *>(arena + jb.root), b);
        root_ok = differs8(a, b) ? 0 : 1;
      }
    }
    flags[2 * (size_t)blockIdx.x] = consistent;
    flags[2 * (size_t)blockIdx.x + 1] = root_ok;
  }
}

}  // namespace

hipError_t pos_group_scrub(const uint8_t *arena, const PosScrubJob *jobs, size_t n_jobs, const PosIngestTile *tiles,
                           const PosIngestWg *wgs, size_t n_wgs, size_t lds_bytes, const PosIngestWave *waves,
                           size_t n_waves, size_t max_chunks, const uint32_t *tw, uint32_t *cvs, uint8_t *cflags,
                           uint8_t *flags, uint8_t *status, uint8_t *dirty, uint8_t *digests, hipStream_t s) {
  if (!n_jobs || !max_chunks || max_chunks > POS_INGEST_MAX_CHUNKS) return hipErrorInvalidValue;
  const size_t blocks = (n_waves + 3) / 4;
  if (n_wgs >= ((size_t)1 << 24) || blocks >= ((size_t)1 << 24) || n_jobs >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  if (lds_bytes > (POS_INGEST_TILE_ROWS << POS_INGEST_MAX_LOG_ENC) * 8) return hipErrorInvalidValue;
  prof::Scope ps("pos_group_scrub", s);
  hipError_t e;
  if (n_wgs) {
    hipLaunchKernelGGL((k_group_scrub_rows<Ft63>), dim3((unsigned)n_wgs), dim3(256), lds_bytes, s, arena, jobs, tiles,
                       wgs, tw, dirty);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_waves) {
    hipLaunchKernelGGL((k_group_scrub_chunks<Ft63>), dim3((unsigned)blocks), dim3(256), 0, s, arena, jobs, waves,
                       (uint32_t)n_waves, cvs, cflags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (max_chunks <= 256)
    hipLaunchKernelGGL((k_group_scrub_leaves<8>), dim3((unsigned)n_jobs), dim3(256), 0, s, arena, jobs, cvs, cflags,
                       flags, status, digests);
  else
    hipLaunchKernelGGL((k_group_scrub_leaves<16>), dim3((unsigned)n_jobs), dim3(256), 0, s, arena, jobs, cvs, cflags,
                       flags, status, digests);
  return hipGetLastError();
}

}  // namespace lcpc
