// pos_verify_group.hip -- the client's check of many stored-file audit responses in one pass (DESIGN
// §5h).  An auditor that holds thousands of roots gets back, per file, a result vector and the opened
// columns with their Merkle paths; checked one response at a time that is six library calls and two
// uploads of the columns per file, all launch latency below a few MiB.  Here the host packs the
// columns, paths, roots and left vectors of a whole staging group into one arena with tables
// (pos.hpp: PosVerifyJob / PosVerifyWave) and this unit checks the group in two launches:
//
//   k_group_leaf_dot      a wave per (job, 64 columns, 1-KiB chunk): the column-major chunk pass of
//                         blake3_dev.hpp (cm_chunk_cv: four lanes load a column's 64-byte block, blocks
//                         handed over through LDS, the next block's loads in flight over the compress)
//                         on Montgomery words, hashing fe_repr_words of each element and, in the same
//                         pass, accumulating sum_r left[r] col[r] over the chunk's rows.  Every lane of a
//                         wave shares one job, so the row count is uniform and the weight loads scalar.
//   k_group_leaf_finish   a lane per (job, column): the column's chunk chaining values folded
//                         left-balanced (the register stack of blake3.hip's k_leaf_fold_stack, the chunk
//                         count now the job's), the chunk sums added, the Merkle path walked to the
//                         job's root with the job's path length, the sum compared with the job's
//                         re-encoded result at the column's index.
//
// The arithmetic is the single check's: fe_mul(left, element) summed with fe_add (k_column_checks) and
// compared word for word with the re-encoded result.  The left vector is reduced, so every product is
// in [0, p) whatever 64-bit word the column holds, and a sum of such values does not depend on its
// order: a job's split into chunks does not show in its verdict.
#include "blake3_dev.hpp"
#include "field.hpp"
#include "kernels.hpp"
#include "pos.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

using namespace b3;

// a workgroup is four waves; wave w of the launch reads waves[w] (wave-uniform: no search)
template <class F>
__global__ __launch_bounds__(256) void k_group_leaf_dot(const uint8_t *__restrict__ arena,
                                                        const PosVerifyJob *__restrict__ jobs,
                                                        const PosVerifyWave *__restrict__ waves, uint32_t n_waves,
                                                        const uint32_t *__restrict__ lefts,
                                                        uint32_t *__restrict__ cvs, uint32_t *__restrict__ partials) {
  static_assert(F::N == 2, "a stored file's columns hold WriteableFt63 elements");
  __shared__ uint4 stage[4][64][5];
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * 4 + wave;
  if (w >= n_waves) return;
  const PosVerifyWave wv = waves[w];
  const PosVerifyJob jb = jobs[wv.job];
  uint32_t cv[8];
  Fe<F> acc = fe_zero<F>();
  bool unused = false;
  cm_chunk_cv<F, false, true, false, true>(stage[wave], reinterpret_cast<const uint32_t *>(arena + jb.cols), jb.n_rows,
                                           jb.n_cols, wv.col_lo, jb.col_words, 8, (int)wv.chunk, (int)jb.n_chunks,
                                           lefts + 2 * jb.left, 0, cv, acc, unused);
  const uint32_t k = wv.col_lo + lane;
  if (k >= jb.n_cols) return;
  const size_t slot = jb.cv0 + (size_t)wv.chunk * jb.n_cols + k;
  store8(cvs + slot * 8, cv);
  fe_store<F>(partials, slot, acc);
}

// wave w of the launch: columns [col_lo, col_lo + 64) of fwaves[w].job, a lane each.  The fold is
// k_leaf_fold_stack's: level[k] = the root of a complete 2^k-chunk subtree, present iff bit k of the
// number of chunks taken so far is set; the last chunk merges with every level still present, lowest
// first, ROOT on the last parent (a one-chunk column's chaining value carries ROOT already).  The
// chunk index is uniform over the wave, so the stack is picked over by unrolled compares.
// n_chunks - 1 < 2^D.
template <class F, int D>
__global__ __launch_bounds__(256) void k_group_leaf_finish(const uint8_t *__restrict__ arena,
                                                           const PosVerifyJob *__restrict__ jobs,
                                                           const PosVerifyWave *__restrict__ fwaves, uint32_t n_fwaves,
                                                           const uint8_t *__restrict__ roots,
                                                           const uint64_t *__restrict__ idx,
                                                           const uint32_t *__restrict__ want,
                                                           const uint32_t *__restrict__ cvs,
                                                           const uint32_t *__restrict__ partials,
                                                           uint32_t *__restrict__ bits) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * 4 + wave;
  if (w >= n_fwaves) return;
  const PosVerifyWave wv = fwaves[w];
  const PosVerifyJob jb = jobs[wv.job];
  const uint32_t c = wv.col_lo + lane;
  if (c >= jb.n_cols) return;
  const int n_chunks = (int)jb.n_chunks;
  const size_t slot0 = jb.cv0 + c, stride = jb.n_cols;
  uint32_t level[D][8], cv[8], nxt[8];
  Fe<F> sum = fe_zero<F>();
  load8(cvs + slot0 * 8, nxt);
  for (int i = 0; i < n_chunks; i++) {
#pragma unroll
    for (int q = 0; q < 8; q++) cv[q] = nxt[q];
    if (i + 1 < n_chunks) load8(cvs + (slot0 + (size_t)(i + 1) * stride) * 8, nxt);  // in flight over the merges
    sum = fe_add<F>(sum, fe_load<F>(partials, slot0 + (size_t)i * stride));
    const bool last = i + 1 == n_chunks;
    for (int k = 0; k < D; k++) {
      const bool top = (i >> (k + 1)) == 0;  // no level above k is present
      if ((i >> k) & 1) {
        uint32_t l[8], o[8];
#pragma unroll
        for (int j = 0; j < D; j++)
          if (j == k) {
#pragma unroll
            for (int q = 0; q < 8; q++) l[q] = level[j][q];
          }
        parent_cv(l, cv, last && top, o);
#pragma unroll
        for (int q = 0; q < 8; q++) cv[q] = o[q];
      } else if (!last) {
#pragma unroll
        for (int j = 0; j < D; j++)
          if (j == k) {
#pragma unroll
            for (int q = 0; q < 8; q++) level[j][q] = cv[q];
          }
        break;
      }
      if (last && top) break;
    }
  }
  // the path from the leaf to the job's root (k_path_checks)
  uint32_t msg[16];
  size_t col = idx[jb.col0 + c];
  const uint8_t *path = arena + jb.paths + 32 * ((size_t)c * jb.path_len);
  for (uint32_t i = 0; i < jb.path_len; i++) {
    uint32_t p[8];
    load8(reinterpret_cast<const uint32_t *>(path + 32 * (size_t)i), p);
#pragma unroll
    for (int q = 0; q < 8; q++) {
      msg[q] = (col & 1) ? p[q] : cv[q];
      msg[8 + q] = (col & 1) ? cv[q] : p[q];
    }
    hash64(msg, cv);
    col >>= 1;
  }
  uint32_t rt[8];
  load8(reinterpret_cast<const uint32_t *>(roots + 32 * (size_t)wv.job), rt);
  uint32_t diff = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) diff |= cv[q] ^ rt[q];
  const bool value_ok = fe_eq<F>(sum, fe_load<F>(want, jb.col0 + c));
  bits[jb.col0 + c] = (diff == 0 ? 1u : 0u) | (value_ok ? 2u : 0u);
}

}  // namespace

hipError_t pos_group_verify(const uint8_t *arena, const PosVerifyJob *jobs, const PosVerifyWave *waves, size_t n_waves,
                            const PosVerifyWave *fwaves, size_t n_fwaves, size_t max_chunks, const uint32_t *lefts,
                            const uint8_t *roots, const uint64_t *idx, const uint32_t *want, uint32_t *cvs,
                            uint32_t *partials, uint32_t *bits, hipStream_t s) {
  if (!n_waves || !n_fwaves || !max_chunks || max_chunks > POS_VERIFY_MAX_CHUNKS) return hipErrorInvalidValue;
  const size_t blocks = (n_waves + 3) / 4, fblocks = (n_fwaves + 3) / 4;
  if (blocks >= ((size_t)1 << 24) || fblocks >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  prof::Scope ps("pos_group_verify", s);
  hipLaunchKernelGGL((k_group_leaf_dot<Ft63>), dim3((unsigned)blocks), dim3(256), 0, s, arena, jobs, waves,
                     (uint32_t)n_waves, lefts, cvs, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (max_chunks <= 256)
    hipLaunchKernelGGL((k_group_leaf_finish<Ft63, 8>), dim3((unsigned)fblocks), dim3(256), 0, s, arena, jobs, fwaves,
                       (uint32_t)n_fwaves, roots, idx, want, cvs, partials, bits);
  else
    hipLaunchKernelGGL((k_group_leaf_finish<Ft63, 16>), dim3((unsigned)fblocks), dim3(256), 0, s, arena, jobs, fwaves,
                       (uint32_t)n_fwaves, roots, idx, want, cvs, partials, bits);
  return hipGetLastError();
}

}  // namespace lcpc
