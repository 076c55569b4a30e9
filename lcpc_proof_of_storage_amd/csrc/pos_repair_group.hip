// pos_repair_group.hip -- the damaged columns of many stored files recomputed in one pass.
// After a scrub every file with a finding went through lcpc_pos_repair_columns on its own: a locator
// build, ten allocations, a dozen launches and three synchronisations for a few dozen rows of a few
// hundred points.  Here the host packs the columns that are NOT listed of a whole staging group of images
// into one arena with tables (pos.hpp: PosRepairJob and the ingest's Tile / Wg / Wave) and this unit does
// the Reed-Solomon erasure decode of DESIGN §5b, a different erasure set E per job, in four launches:
//
//   k_group_repair_locators  a workgroup per job.  L(x) = prod_{j in E} (x - x_j): lambda_c = L(x_c) for
//                            c not in E, and for j in E the product without its own factor, L'(x_j),
//                            inverted on the device with the constants the row kernel leaves in.
//   k_group_repair_rows      a workgroup holds tiles of up to 8 whole rows of one length in LDS, the tiles
//                            of different jobs: masked load, k_group_scrub_rows' inverse stages, degree
//                            check, derivative, k_group_encode's forward stages, fill.
//   k_group_repair_chunks    a wave per (job, 64 repaired columns, 1-KiB chunk): cm_chunk_cv.
//   k_group_repair_trees     a workgroup per job: a lane per repaired column folds its leaf; with the
//                            job's leaves the 2 enc - 1 digests are built over them, the repaired ones in.
//
// THE POINTS.  Stored position c of a row of enc points holds f(x_c), x_c = tw[e(c) << (10 - log_enc)]
// with e(c) = bitrev(c) (LCPC_FFT_OUTPUT_BITREV = 1) or c (= 0), tw the one table pos_ingest_twiddles
// builds (which root it holds, LCPC_FFT_OMEGA_INVERSE, is the table's business): what k_group_encode's
// stages and store compute, and what lcpc_rs_domain_points states.
//
// THE ROW KERNEL'S CONSTANTS.  The stored canonical word y is used as a Montgomery residue as it is (it
// stands for y / R), and the inverse stages leave a factor enc in, as in k_group_scrub_rows: with g_c =
// y_c lambda_c at c not in E and 0 in E, slot k holds (enc / R) P_k, P = f L, deg P < pre + |E|.  A row
// passes iff the slots k >= pre + |E| are zero.  Instead of the shifted P' the slots keep their places
// and take the factor k, given as the canonical word k (one more 1 / R): slot k = (enc / R^2) k P_k, the
// coefficients of x P'(x).  No slot moves, so no lane reads what another writes.  The forward stages
// evaluate that at every x_c, and since P' = f' L + f L' with L(x_j) = 0,
//   f(x_j) = x_j P'(x_j) / (x_j L'(x_j)),   j in E.
// The locator kernel therefore stores T_j = to_mont(1 / (enc x_j L'(x_j))): the fill is the one product
// fe_mul(slot, T_j), which is fully reduced and is the canonical word of f(x_j).
//
// Listed columns are not in the arena at all: no kernel can read them.  Control flow is uniform over a
// workgroup in the row kernel (its tiles share enc) and over a wave elsewhere, but for bounds.  No
// atomics: every output byte has one writer.
#include "kernels.hpp"
#include "pos_rows_dev.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

using namespace b3;

// index in the table of 2^POS_INGEST_MAX_LOG_ENC points of x_c, c a stored position of a row of 2^log_enc
__device__ __forceinline__ size_t repair_point(int c, int log_enc) {
  const int e = LCPC_FFT_OUTPUT_BITREV ? bitrev_bits(c, log_enc) : c;
  return (size_t)e << (POS_INGEST_MAX_LOG_ENC - log_enc);
}

// workgroup j of the launch is job j
template <class F>
__global__ __launch_bounds__(256) void k_group_repair_locators(const uint8_t *__restrict__ arena,
                                                               const PosRepairJob *__restrict__ jobs,
                                                               const uint32_t *__restrict__ tw,
                                                               uint32_t *__restrict__ tabs) {
  constexpr int MAX_E = 1 << POS_INGEST_MAX_LOG_ENC;  // |E| <= enc - pre < 2^10
  __shared__ Fe<F> s_x[MAX_E];
  __shared__ uint32_t s_idx[MAX_E];
  const PosRepairJob jb = jobs[blockIdx.x];
  if (jb.tree_only) return;
  const int log_enc = (int)jb.log_enc, enc = 1 << log_enc, n_bad = (int)jb.n_bad;
  const uint32_t *bad = reinterpret_cast<const uint32_t *>(arena + jb.bad);
  const int32_t *cmap = reinterpret_cast<const int32_t *>(arena + jb.cmap);
  for (int k = threadIdx.x; k < n_bad && k < MAX_E; k += 256) {
    const uint32_t j = bad[k];
    s_idx[k] = j;
    s_x[k] = fe_load<F>(tw, repair_point((int)j, log_enc));
  }
  __syncthreads();
  Fe<F> enc_c = fe_zero<F>();
  enc_c.v[0] = (uint32_t)enc;
  const Fe<F> enc_m = fe_to_mont<F>(enc_c);
  for (int c = threadIdx.x; c < enc; c += 256) {
    const Fe<F> xc = fe_load<F>(tw, repair_point(c, log_enc));
    Fe<F> acc = fe_one<F>();
    for (int k = 0; k < n_bad; k++)
      if (s_idx[k] != (uint32_t)c) acc = fe_mul<F>(acc, fe_sub<F>(xc, s_x[k]));
    const int32_t m = cmap[c];
    if (m >= 0)
      fe_store<F>(tabs, jb.dinv0 + (size_t)m, fe_to_mont<F>(fe_inv_fermat<F>(fe_mul<F>(fe_mul<F>(acc, xc), enc_m))));
    else
      fe_store<F>(tabs, jb.lam0 + (size_t)c, acc);
  }
}

// workgroup b of the launch reads wgs[b]; element idx of its LDS is (tile slot, row of the tile, slot).
// A lane's loads are 256 elements apart, at most 32 of them (8192 elements): bit q of ncmask says that
// its q-th load was not < p.  The rows' lanes of the degree check are the lanes of the closing flag
// store, at most 8 rounds: bit q of degmask is the q-th round's verdict.
template <class F>
__global__ __launch_bounds__(256) void k_group_repair_rows(const uint8_t *__restrict__ arena,
                                                           const PosRepairJob *__restrict__ jobs,
                                                           const PosIngestTile *__restrict__ tiles,
                                                           const PosIngestWg *__restrict__ wgs,
                                                           const uint32_t *__restrict__ tw,
                                                           const uint32_t *__restrict__ tabs, uint8_t *__restrict__ rep,
                                                           uint8_t *__restrict__ flags) {
  static_assert(F::N == 2, "a stored file holds WriteableFt63 elements");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Fe<F> *buf = reinterpret_cast<Fe<F> *>(smem);
  const PosIngestWg wg = wgs[blockIdx.x];
  const int log_enc = (int)wg.log_enc, enc = 1 << log_enc;
  const int total = (int)wg.n_tiles << (3 + log_enc);
  // masked load: the rows of a tile are the fast index, so a full tile's column segment is 64 contiguous
  // bytes; a listed position gets zero and no address is formed for it
  uint32_t ncmask = 0;
  {
    int q = 0;
    for (int idx = threadIdx.x; idx < total; idx += 256, q++) {
      const int r = idx & 7, c = (idx >> 3) & (enc - 1), t = idx >> (3 + log_enc);
      const PosIngestTile tl = tiles[wg.tile0 + t];
      Fe<F> e = fe_zero<F>();
      if ((uint32_t)r < tl.n_rows) {
        const PosRepairJob &jb = jobs[tl.job];
        const int32_t m = reinterpret_cast<const int32_t *>(arena + jb.cmap)[c];
        if (m < 0) {
          const uint64_t *col = reinterpret_cast<const uint64_t *>(arena + jb.img) + (size_t)(-1 - m) * jb.rows_pad;
          const uint64_t v = col[tl.row_lo + r];
          Fe<F> y;
          y.v[0] = (uint32_t)v;
          y.v[1] = (uint32_t)(v >> 32);
          if (fe_is_canonical<F>(y))
            e = fe_mul<F>(y, fe_load<F>(tabs, jb.lam0 + (size_t)c));
          else
            ncmask |= 1u << q;
        }
      }
      buf[row_elem(t, r, row_slot(c, log_enc), log_enc)] = e;
    }
  }
  // k_group_scrub_rows' inverse stages (times 2 per stage)
  rows_inverse_stages<F>(buf, log_enc, total, tw);
  // degree check and x P'(x) in one sweep: min(enc, 64) lanes share a row and OR through the wave's ballot
  const int log_g = log_enc < 6 ? log_enc : 6, g = 1 << log_g, rows_per_wave = 64 >> log_g;
  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n_rows_lds = (int)wg.n_tiles << 3;
  const uint64_t group_mask = g == 64 ? ~(uint64_t)0 : (((uint64_t)1 << g) - 1);
  uint32_t degmask = 0;
  {
    int q = 0;
    for (int r0 = wave * rows_per_wave; r0 < n_rows_lds; r0 += 4 * rows_per_wave, q++) {
      const int row = r0 + (lane >> log_g), li = lane & (g - 1);
      const bool in = row < n_rows_lds;
      int deg = enc;
      if (in) {
        const PosRepairJob &jb = jobs[tiles[wg.tile0 + (row >> 3)].job];
        deg = (int)(jb.pre + jb.n_bad);
      }
      bool nz = false;
      for (int i = li; i < enc; i += g) {
        if (!in) continue;
        const Fe<F> v = buf[(row << log_enc) + i];
        if (i >= deg) nz |= !fe_is_zero<F>(v);
        Fe<F> kk = fe_zero<F>();
        kk.v[0] = (uint32_t)i;
        buf[(row << log_enc) + i] = fe_mul<F>(v, kk);
      }
      const uint64_t votes = __ballot(nz);
      if (((votes >> ((lane >> log_g) << log_g)) & group_mask) != 0) degmask |= 1u << q;
    }
  }
  // k_group_encode's forward stages
  rows_forward_stages<F>(buf, log_enc, total, tw);
  // fill, at the listed positions only: one product, canonical, column-major into the repaired arena
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int r = idx & 7, c = (idx >> 3) & (enc - 1), t = idx >> (3 + log_enc);
    const PosIngestTile tl = tiles[wg.tile0 + t];
    if ((uint32_t)r >= tl.n_rows) continue;
    const PosRepairJob &jb = jobs[tl.job];
    const int32_t m = reinterpret_cast<const int32_t *>(arena + jb.cmap)[c];
    if (m < 0) continue;
    const Fe<F> v = fe_mul<F>(buf[row_elem(t, r, row_slot(c, log_enc), log_enc)],
                              fe_load<F>(tabs, jb.dinv0 + (size_t)m));
    uint64_t *col = reinterpret_cast<uint64_t *>(rep + jb.rep) + (size_t)m * jb.rows_pad;
    col[tl.row_lo + r] = (uint64_t)v.v[0] | ((uint64_t)v.v[1] << 32);
  }
  // the rows' flags.  The LDS is free now: a byte per row takes the loads' verdicts (every lane that
  // stores to a byte stores 1), then the lane that closed a row's degree check stores the row's flag.
  __syncthreads();
  uint8_t *nc = reinterpret_cast<uint8_t *>(smem);
  for (int i = threadIdx.x; i < n_rows_lds; i += 256) nc[i] = 0;
  __syncthreads();
  for (int q = 0; q < 32; q++)
    if ((ncmask >> q) & 1u) {
      const int idx = (int)threadIdx.x + 256 * q;
      nc[((idx >> (3 + log_enc)) << 3) + (idx & 7)] = 1;
    }
  __syncthreads();
  {
    int q = 0;
    for (int r0 = wave * rows_per_wave; r0 < n_rows_lds; r0 += 4 * rows_per_wave, q++) {
      const int row = r0 + (lane >> log_g), li = lane & (g - 1);
      if (row >= n_rows_lds || li != 0) continue;
      const PosIngestTile tl = tiles[wg.tile0 + (row >> 3)];
      if ((uint32_t)(row & 7) >= tl.n_rows) continue;
      const uint8_t f = (uint8_t)((((degmask >> q) & 1u) ? POS_REPAIR_ROW_DEGREE : 0) | (nc[row] ? POS_REPAIR_ROW_NONCANON : 0));
      flags[jobs[tl.job].row0 + tl.row_lo + (row & 7)] = f;
    }
  }
}

// a workgroup is four waves; wave w of the launch reads waves[w] (wave-uniform: no search)
template <class F>
__global__ __launch_bounds__(256) void k_group_repair_chunks(const uint8_t *__restrict__ rep,
                                                             const PosRepairJob *__restrict__ jobs,
                                                             const PosIngestWave *__restrict__ waves, uint32_t n_waves,
                                                             uint32_t *__restrict__ cvs) {
  __shared__ uint4 stage[4][64][5];
  const uint32_t lane = threadIdx.x & 63;
  uint32_t wave;
  PosIngestWave wv;
  if (!chunk_wave(waves, n_waves, wave, wv)) return;
  const PosRepairJob jb = jobs[wv.job];
  const size_t n_cols = jb.n_bad;
  uint32_t cv[8];
  Fe<F> acc = fe_zero<F>();
  bool unused = false;
  cm_chunk_cv<F, true, true, false, false>(stage[wave], reinterpret_cast<const uint32_t *>(rep + jb.rep), jb.n_rows,
                                           n_cols, wv.col_lo, 2 * (size_t)jb.rows_pad, 8, (int)wv.chunk,
                                           (int)jb.n_chunks, nullptr, 0, cv, acc, unused);
  const size_t k = wv.col_lo + lane;
  if (k >= n_cols) return;
  store8(cvs + (jb.cv0 + (size_t)wv.chunk * n_cols + k) * 8, cv);
}

// workgroup j of the launch is job j.  A lane per repaired column folds its digest; with the job's
// leaves the tree's first enc digests are those leaves with the repaired digests in place (a digest
// has one writer: the lane of its repaired column, or the lane that copies its leaf), then every
// level is hashed from the one below it as in k_group_ingest_trees.
template <int D>
__global__ __launch_bounds__(256) void k_group_repair_trees(const uint8_t *__restrict__ arena,
                                                            const PosRepairJob *__restrict__ jobs,
                                                            const uint32_t *__restrict__ cvs,
                                                            uint8_t *__restrict__ digests, uint8_t *trees) {
  const PosRepairJob jb = jobs[blockIdx.x];
  const uint32_t enc = 1u << jb.log_enc, n_bad = jb.n_bad;
  const uint32_t *bad = reinterpret_cast<const uint32_t *>(arena + jb.bad);
  uint8_t *tree = trees + 32 * jb.tree0;
  for (uint32_t k0 = 0; k0 < n_bad; k0 += 256) {
    const uint32_t k = k0 + threadIdx.x;
    if (k >= n_bad) continue;
    uint32_t leaf[8];
    if (jb.tree_only) {
      load8(reinterpret_cast<const uint32_t *>(arena + jb.dig_in + 32 * (size_t)k), leaf);
    } else {
      leaf_fold_stack<D>(cvs + (jb.cv0 + k) * 8, n_bad, (int)jb.n_chunks, leaf);
      store8(reinterpret_cast<uint32_t *>(digests + 32 * (jb.dig0 + k)), leaf);
    }
    if (jb.has_tree) store8(reinterpret_cast<uint32_t *>(tree + 32 * (size_t)bad[k]), leaf);
  }
  if (!jb.has_tree) return;
  const int32_t *cmap = reinterpret_cast<const int32_t *>(arena + jb.cmap);
  for (uint32_t c = threadIdx.x; c < enc; c += 256) {
    if (cmap[c] >= 0) continue;
    uint32_t leaf[8];
    load8(reinterpret_cast<const uint32_t *>(arena + jb.leaves + 32 * (size_t)c), leaf);
    store8(reinterpret_cast<uint32_t *>(tree + 32 * (size_t)c), leaf);
  }
  merkle_levels(tree, enc);
}

}  // namespace

hipError_t pos_group_repair_locators(const uint8_t *arena, const PosRepairJob *jobs, size_t n_jobs, const uint32_t *tw,
                                     uint32_t *tabs, hipStream_t s) {
  if (!n_jobs || n_jobs >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_group_repair_locators<Ft63>), dim3((unsigned)n_jobs), dim3(256), 0, s, arena, jobs, tw, tabs);
  return hipGetLastError();
}

hipError_t pos_group_repair(const uint8_t *arena, const PosRepairJob *jobs, size_t n_jobs, const PosIngestTile *tiles,
                            const PosIngestWg *wgs, size_t n_wgs, size_t lds_bytes, const PosIngestWave *waves,
                            size_t n_waves, size_t max_chunks, bool tree_only_group, const uint32_t *tw, uint32_t *tabs,
                            uint8_t *rep, uint32_t *cvs, uint8_t *flags, uint8_t *digests, uint8_t *trees,
                            hipStream_t s) {
  if (!n_jobs || !max_chunks || max_chunks > POS_INGEST_MAX_CHUNKS) return hipErrorInvalidValue;
  const size_t blocks = (n_waves + 3) / 4;
  if (n_wgs >= ((size_t)1 << 24) || blocks >= ((size_t)1 << 24) || n_jobs >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  if (lds_bytes > (POS_INGEST_TILE_ROWS << POS_INGEST_MAX_LOG_ENC) * 8) return hipErrorInvalidValue;
  prof::Scope ps("pos_group_repair", s);
  hipError_t e;
  if (!tree_only_group) {
    hipLaunchKernelGGL((k_group_repair_locators<Ft63>), dim3((unsigned)n_jobs), dim3(256), 0, s, arena, jobs, tw, tabs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n_wgs) {
      hipLaunchKernelGGL((k_group_repair_rows<Ft63>), dim3((unsigned)n_wgs), dim3(256), lds_bytes, s, arena, jobs, tiles,
                         wgs, tw, tabs, rep, flags);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (n_waves) {
      hipLaunchKernelGGL((k_group_repair_chunks<Ft63>), dim3((unsigned)blocks), dim3(256), 0, s, rep, jobs, waves,
                         (uint32_t)n_waves, cvs);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  if (max_chunks <= 256)
    hipLaunchKernelGGL((k_group_repair_trees<8>), dim3((unsigned)n_jobs), dim3(256), 0, s, arena, jobs, cvs, digests,
                       trees);
  else
    hipLaunchKernelGGL((k_group_repair_trees<16>), dim3((unsigned)n_jobs), dim3(256), 0, s, arena, jobs, cvs, digests,
                       trees);
  return hipGetLastError();
}

}  // namespace lcpc
