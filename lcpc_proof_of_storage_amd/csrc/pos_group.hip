// pos_group.hip -- k_left_mul_bytes (pos_eval.hip) over many file images in one launch: the grouped
// stored-file audit.  A server answers audits of many files, most of them small; one
// launch per file is all launch latency, so the host packs the (job, row range, run range) tiles of
// a whole staging group into waves (pos.hpp: PosGroupJob / Tile / Wave / Fold) and this unit runs
// them in one launch plus one fold launch for the jobs that were split in rows.
//
// The arithmetic is k_left_mul_bytes': raw 56-bit elements against Montgomery words, fe_dot_kmax
// rows per lazy reduction, the canonical word of each sum.  Field sums are exact, so a job's split
// does not show in its words: every job's output is bit for bit the single kernel's.
//
// Padding is per image: a tile reads through its own job's (base, n_bytes) only (pack7_load_run
// zero-fills past n_bytes), never the bytes that follow the image in the arena -- they belong to
// the next file.
#include "field.hpp"
#include "kernels.hpp"
#include "pos.hpp"
#include "pos_bytes.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

// a workgroup is four waves; wave w of the launch reads waves[w] (wave-uniform), lane l of it the
// tile tile0 + (l >> log_w): no search
template <class F>
__global__ __launch_bounds__(256) void k_group_left_mul(const uint8_t *__restrict__ arena,
                                                        const PosGroupJob *__restrict__ jobs,
                                                        const PosGroupTile *__restrict__ tiles,
                                                        const PosGroupWave *__restrict__ waves, uint32_t n_waves,
                                                        const uint32_t *__restrict__ lefts,
                                                        uint32_t *__restrict__ res) {
  static_assert(F::N == 2, "a file image holds WriteableFt63 elements");
  constexpr int K = fe_dot_kmax<F>() < 4 ? fe_dot_kmax<F>() : 4;
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_waves) return;
  const PosGroupWave wv = waves[w];
  const uint32_t lane = threadIdx.x & 63, ti = lane >> wv.log_w;
  if (ti >= wv.n_tiles) return;
  const PosGroupTile t = tiles[wv.tile0 + ti];
  const PosGroupJob jb = jobs[t.job];
  const uint8_t *bytes = arena + jb.base;
  const size_t n_bytes = jb.n_bytes, row_b = 7 * jb.pre;
  const uint32_t *left = lefts + 2 * jb.left_off;
  const size_t g = t.run_lo + (lane & ((1u << wv.log_w) - 1));
  const size_t r1 = (size_t)t.row_lo + wv.n_rows;
  Fe<F> acc[8];
#pragma unroll
  for (int k = 0; k < 8; k++) acc[k] = fe_zero<F>();
  size_t r = t.row_lo;
  for (; r + K <= r1; r += K) {
    uint64_t q[K][7];
    Fe<F> a[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      pack7_load_run(bytes, n_bytes, (r + j) * row_b + 56 * g, q[j]);
      a[j] = fe_load<F>(left, r + j);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      Fe<F> b[K];
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint64_t e = pack7_elem(q[j], k);
        b[j].v[0] = (uint32_t)e;
        b[j].v[1] = (uint32_t)(e >> 32);
      }
      acc[k] = fe_add<F>(acc[k], fe_dot<F, K>(a, b));
    }
  }
  for (; r < r1; r++) {
    uint64_t q[7];
    pack7_load_run(bytes, n_bytes, r * row_b + 56 * g, q);
    const Fe<F> a = fe_load<F>(left, r);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint64_t e = pack7_elem(q, k);
      Fe<F> b;
      b.v[0] = (uint32_t)e;
      b.v[1] = (uint32_t)(e >> 32);
      acc[k] = fe_add<F>(acc[k], fe_mul<F>(a, b));
    }
  }
#pragma unroll
  for (int k = 0; k < 8; k++) fe_store<F>(res, t.dst + 8 * g + k, acc[k]);
}

// wave w of the launch sums the partials of folds[w], a lane per column (the outputs and the
// partials are disjoint ranges of res)
template <class F>
__global__ __launch_bounds__(256) void k_group_fold(const PosGroupFold *__restrict__ folds, uint32_t n_folds,
                                                    uint32_t *res) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= n_folds) return;
  const PosGroupFold f = folds[w];
  if (lane >= f.n_cols) return;
  const size_t c = f.col0 + lane;
  Fe<F> v = fe_zero<F>();
  for (uint32_t y = 0; y < f.n_split; y++) v = fe_add<F>(v, fe_load<F>(res, f.part + (size_t)y * f.pre + c));
  fe_store<F>(res, f.out + c, v);
}

}  // namespace

hipError_t pos_group_left_mul(const uint8_t *arena, const PosGroupJob *jobs, const PosGroupTile *tiles,
                              const PosGroupWave *waves, size_t n_waves, const PosGroupFold *folds, size_t n_folds,
                              const uint32_t *lefts, uint32_t *res, hipStream_t s) {
  if (!n_waves) return hipErrorInvalidValue;
  const size_t blocks = (n_waves + 3) / 4, fold_blocks = (n_folds + 3) / 4;
  if (blocks >= ((size_t)1 << 24) || fold_blocks >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  prof::Scope ps("pos_group_left_mul", s);
  hipLaunchKernelGGL((k_group_left_mul<Ft63>), dim3((unsigned)blocks), dim3(256), 0, s, arena, jobs, tiles, waves,
                     (uint32_t)n_waves, lefts, res);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !n_folds) return e;
  hipLaunchKernelGGL((k_group_fold<Ft63>), dim3((unsigned)fold_blocks), dim3(256), 0, s, folds, (uint32_t)n_folds, res);
  return hipGetLastError();
}

}  // namespace lcpc
