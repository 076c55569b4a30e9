// pos_locate_group.hip -- the damaged columns of many stored files named by their own rows in one pass
// (DESIGN §5m).  lcpc_pos_locate_porenc pays, per file, a second upload of the image, the
// masked load, four transform launches, a flag read-back, a gather, Berlekamp-Massey, a forward
// transform, a zero scan and several synchronisations.  Here the host packs the columns that are NOT
// known to be bad of a whole staging group of images into one arena, with the grouped repair's tables
// (pos.hpp: PosRepairJob, PosLocateJob, the ingest's Tile / Wg), and this unit does §5c's location, a
// different erasure set E per job, in four launches:
//
//   k_group_repair_locators  (pos_repair_group.hip, as it is; skipped when no job lists a column)
//                            lambda_c = L(x_c), L(x) = prod_{j in E} (x - x_j).
//   k_group_locate_rows      k_group_repair_rows up to its degree sweep: masked load times lambda_c, the
//                            inverse stages.  Slot k of a row then holds (enc / R) P_k, and the slots
//                            k >= pre + |E| are the syndromes S_i of §5c, i = k - pre - |E| < N (one
//                            non-zero constant on all of them, which neither the shortest recurrence nor
//                            its roots notice).  Stored: the row's flag byte (bit 0 some S_i != 0, bit 1 a
//                            word not < p) and, for a dirty row, S_0 .. S_{N-1} to the row's own slot of
//                            the syndrome arena.  No atomics, no compaction.
//   k_group_locate_bm        a one-wave workgroup per row.  A clean row's wave stores status 0 and exits on
//                            the flag byte.  Else inversion-free Berlekamp-Massey as rs_locate.hip's k_bm
//                            (every value fully reduced, the discrepancy reduced across lanes only as far as
//                            L + 1 reaches, B double-buffered) with the whole sequence resident in LDS:
//                            N <= 1023, L <= 511.  Then the root search in the same workgroup: C
//                            zero-padded to enc, k_group_encode's forward stages, zeros read at stored
//                            positions through row_slot.  Located iff C_L != 0, 2 L <= N, L zeros, none on
//                            a listed column: §5c's conditions.  Stored: the row's status byte and its
//                            enc-bit position mask, in the row's own slot.
//   k_group_locate_cols      a workgroup per job, a lane per column: the OR of the column's bit over the
//                            job's located rows; 0, 1, or 3 for a listed column.
//
// Listed columns are not in the arena at all: no kernel can read them.  Every output byte has one writer
// and nothing is cleared first: what a recycled block held before cannot matter.
#include "kernels.hpp"
#include "pos_rows_dev.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

// workgroup b of the launch reads wgs[b]; the LDS, the masked load and ncmask / degmask are
// k_group_repair_rows' (pos_repair_group.hip)
template <class F>
__global__ __launch_bounds__(256) void k_group_locate_rows(const uint8_t *__restrict__ arena,
                                                           const PosRepairJob *__restrict__ jobs,
                                                           const PosLocateJob *__restrict__ ljobs,
                                                           const PosIngestTile *__restrict__ tiles,
                                                           const PosIngestWg *__restrict__ wgs,
                                                           const uint32_t *__restrict__ tw,
                                                           const uint32_t *__restrict__ tabs,
                                                           uint64_t *__restrict__ synd, uint8_t *__restrict__ flags) {
  static_assert(F::N == 2, "a stored file holds WriteableFt63 elements");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Fe<F> *buf = reinterpret_cast<Fe<F> *>(smem);
  const PosIngestWg wg = wgs[blockIdx.x];
  const int log_enc = (int)wg.log_enc, enc = 1 << log_enc;
  const int total = (int)wg.n_tiles << (3 + log_enc);
  // masked load.  A job that lists nothing has lambda = 1 (the Montgomery one: the product is y itself)
  // and no table: the locator launch may not have run.
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
            e = jb.n_bad ? fe_mul<F>(y, fe_load<F>(tabs, jb.lam0 + (size_t)c)) : y;
          else
            ncmask |= 1u << q;
        }
      }
      buf[row_elem(t, r, row_slot(c, log_enc), log_enc)] = e;
    }
  }
  rows_inverse_stages<F>(buf, log_enc, total, tw);
  // the syndrome sweep: min(enc, 64) lanes share a row and OR through the wave's ballot; the lanes of a
  // dirty row store its syndromes
  const int log_g = log_enc < 6 ? log_enc : 6, g = 1 << log_g, rows_per_wave = 64 >> log_g;
  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n_rows_lds = (int)wg.n_tiles << 3;
  const uint64_t group_mask = g == 64 ? ~(uint64_t)0 : (((uint64_t)1 << g) - 1);
  uint32_t degmask = 0;
  {
    int q = 0;
    for (int r0 = wave * rows_per_wave; r0 < n_rows_lds; r0 += 4 * rows_per_wave, q++) {
      const int row = r0 + (lane >> log_g), li = lane & (g - 1);
      bool in = row < n_rows_lds;
      int deg = enc;
      uint64_t *S = nullptr;
      if (in) {
        const PosIngestTile tl = tiles[wg.tile0 + (row >> 3)];
        in = (uint32_t)(row & 7) < tl.n_rows;
        if (in) {
          const PosRepairJob &jb = jobs[tl.job];
          deg = (int)(jb.pre + jb.n_bad);
          S = synd + ljobs[tl.job].synd0 + (size_t)(tl.row_lo + (row & 7)) * (size_t)(enc - deg);
        }
      }
      bool nz = false;
      if (in)
        for (int i = deg + li; i < enc; i += g) nz |= !fe_is_zero<F>(buf[(row << log_enc) + i]);
      const uint64_t votes = __ballot(nz);
      const bool dirty = ((votes >> ((lane >> log_g) << log_g)) & group_mask) != 0;
      if (dirty) degmask |= 1u << q;
      if (in && dirty)
        for (int i = li; i < enc - deg; i += g) {
          const Fe<F> v = buf[(row << log_enc) + deg + i];
          S[i] = (uint64_t)v.v[0] | ((uint64_t)v.v[1] << 32);
        }
    }
  }
  // the rows' flags, as k_group_repair_rows: a byte per row of the LDS takes the loads' verdicts, then the
  // lane that closed a row's sweep stores the row's flag
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

// The sum over the wave of one element per lane (every lane gets it).  Only the lanes below `active` (a
// power of two <= 64, uniform) hold a non-zero term: rs_locate.hip's block_sum for one wave.
template <class F>
__device__ __forceinline__ Fe<F> wave_sum(Fe<F> v, int active) {
  for (int off = 32; off >= 1; off >>= 1) {
    if (off >= active) continue;
    Fe<F> o;
#pragma unroll
    for (int i = 0; i < F::N; i++) o.v[i] = __shfl_xor(v.v[i], off, 64);
    v = fe_add<F>(v, o);
  }
#pragma unroll
  for (int i = 0; i < F::N; i++) v.v[i] = __builtin_amdgcn_readfirstlane(v.v[i]);
  return v;
}

// Workgroup b of the launch is row b & 7 of tile b >> 3 of the group's tile table: one wave.  LDS:
// [enc] the syndromes, later C zero-padded; [W] C, [W] B, [W] the next B, W = N / 2 + 1 <= enc / 2.
// Control flow is uniform over the wave (the discrepancy is broadcast), so the barriers are the wave's own.
template <class F>
__global__ __launch_bounds__(64) void k_group_locate_bm(const uint8_t *__restrict__ arena,
                                                        const PosRepairJob *__restrict__ jobs,
                                                        const PosLocateJob *__restrict__ ljobs,
                                                        const PosIngestTile *__restrict__ tiles,
                                                        const uint32_t *__restrict__ tw,
                                                        const uint64_t *__restrict__ synd,
                                                        const uint8_t *__restrict__ flags, uint8_t *__restrict__ rstat,
                                                        uint64_t *__restrict__ masks) {
  static_assert(F::N == 2, "a stored file holds WriteableFt63 elements");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const PosIngestTile tl = tiles[blockIdx.x >> 3];
  const uint32_t r = blockIdx.x & 7, tid = threadIdx.x;
  if (r >= tl.n_rows) return;
  const PosRepairJob &jb = jobs[tl.job];
  const PosLocateJob lj = ljobs[tl.job];
  const size_t jrow = (size_t)tl.row_lo + r, row = jb.row0 + jrow;
  if (!(flags[row] & POS_REPAIR_ROW_DEGREE)) {
    if (tid == 0) rstat[row] = 0;
    return;
  }
  const int log_enc = (int)jb.log_enc, enc = 1 << log_enc;
  const uint32_t N = (uint32_t)enc - jb.pre - jb.n_bad, l_max = N / 2, W = l_max + 1;
  Fe<F> *buf = reinterpret_cast<Fe<F> *>(smem);
  Fe<F> *Cc = buf + enc, *Bc = Cc + W, *Bn = Bc + W;
  const uint64_t *S = synd + lj.synd0 + jrow * N;
  for (uint32_t i = tid; i < N; i += 64) {
    const uint64_t v = S[i];
    Fe<F> e;
    e.v[0] = (uint32_t)v;
    e.v[1] = (uint32_t)(v >> 32);
    buf[i] = e;
  }
  for (uint32_t j = tid; j < W; j += 64) {
    Cc[j] = j ? fe_zero<F>() : fe_one<F>();
    Bc[j] = j ? fe_zero<F>() : fe_one<F>();
    Bn[j] = fe_zero<F>();
  }
  uint32_t L = 0, LB = 0, m = 1;  // LB: B_j = 0 for j > LB
  Fe<F> b = fe_one<F>();
  bool fail = false;
  __syncthreads();
  for (uint32_t i = 0; i < N; i++) {
    Fe<F> acc = fe_zero<F>();
    for (uint32_t j = tid; j <= L && j <= i; j += 64) acc = fe_add<F>(acc, fe_mul<F>(Cc[j], buf[i - j]));
    const uint32_t terms = L + 1 < 64 ? L + 1 : 64;
    const int active = terms <= 1 ? 1 : 1 << (32 - __builtin_clz(terms - 1));
    const Fe<F> dsc = wave_sum<F>(acc, active);
    if (fe_is_zero<F>(dsc)) {  // fully reduced: fe_add / fe_mul results are < p
      m++;
      continue;
    }
    const bool grow = 2 * L <= i;
    const uint32_t l_new = grow ? i + 1 - L : L;
    if (l_new > l_max) {  // L never shrinks: more wrong positions than the syndromes can name
      fail = true;
      break;
    }
    // C <- b C - d z^m B on [0, l_new]; deg z^m B <= l_new (the invariant of the algorithm)
    for (uint32_t j = tid; j <= l_new; j += 64) {
      const Fe<F> cj = Cc[j];
      Fe<F> v = fe_mul<F>(b, cj);
      if (j >= m && j - m <= LB) v = fe_sub<F>(v, fe_mul<F>(dsc, Bc[j - m]));
      Cc[j] = v;
      if (grow) Bn[j] = cj;
    }
    if (grow) {
      Fe<F> *t = Bc;
      Bc = Bn;
      Bn = t;
      LB = L;
      L = l_new;
      b = dsc;
      m = 1;
    } else {
      m++;
    }
    __syncthreads();
  }
  __syncthreads();
  if (!fail && (2 * L > N || L == 0 || fe_is_zero<F>(Cc[L]))) fail = true;
  if (fail) {
    if (tid == 0) rstat[row] = 2;
    return;
  }
  // the root search: C(x_c) at every stored position c
  for (int j = (int)tid; j < enc; j += 64) buf[j] = (uint32_t)j <= L ? Cc[j] : fe_zero<F>();
  rows_forward_stages<F, 64>(buf, log_enc, enc, tw);
  const int32_t *cmap = reinterpret_cast<const int32_t *>(arena + jb.cmap);
  uint64_t *mask = masks + lj.mask0 + jrow * (size_t)(enc > 64 ? enc >> 6 : 1);
  uint32_t n_zero = 0;
  bool on_listed = false;
  for (int c0 = 0; c0 < enc; c0 += 64) {
    const int c = c0 + (int)tid;
    bool z = false, lst = false;
    if (c < enc) {
      z = fe_is_zero<F>(buf[row_slot(c, log_enc)]);
      lst = z && cmap[c] >= 0;
    }
    const uint64_t zs = __ballot(z);
    n_zero += (uint32_t)__popcll(zs);
    on_listed |= __ballot(lst) != 0;
    if (tid == 0) mask[c0 >> 6] = zs;
  }
  if (tid == 0) rstat[row] = (n_zero == L && !on_listed) ? 1 : 2;
}

// workgroup j of the launch is job j; a lane per column
__global__ __launch_bounds__(256) void k_group_locate_cols(const uint8_t *__restrict__ arena,
                                                           const PosRepairJob *__restrict__ jobs,
                                                           const PosLocateJob *__restrict__ ljobs,
                                                           const uint8_t *__restrict__ rstat,
                                                           const uint64_t *__restrict__ masks,
                                                           uint8_t *__restrict__ col_status) {
  const PosRepairJob jb = jobs[blockIdx.x];
  const PosLocateJob lj = ljobs[blockIdx.x];
  const uint32_t enc = 1u << jb.log_enc, w64 = enc > 64 ? enc >> 6 : 1;
  const int32_t *cmap = reinterpret_cast<const int32_t *>(arena + jb.cmap);
  for (uint32_t c = threadIdx.x; c < enc; c += 256) {
    uint8_t st = 3;
    if (cmap[c] < 0) {
      uint64_t any = 0;
      for (uint32_t r = 0; r < jb.n_rows; r++)
        if (rstat[jb.row0 + r] == 1) any |= masks[lj.mask0 + (size_t)r * w64 + (c >> 6)];
      st = (uint8_t)((any >> (c & 63)) & 1);
    }
    col_status[lj.col0 + c] = st;
  }
}

}  // namespace

hipError_t pos_group_locate(const uint8_t *arena, const PosRepairJob *jobs, const PosLocateJob *ljobs, size_t n_jobs,
                            const PosIngestTile *tiles, size_t n_tiles, const PosIngestWg *wgs, size_t n_wgs,
                            size_t lds_rows, size_t lds_bm, bool any_listed, const uint32_t *tw, uint32_t *tabs,
                            uint64_t *synd, uint64_t *masks, uint8_t *flags, uint8_t *rstat, uint8_t *col_status,
                            hipStream_t s) {
  if (!n_jobs || n_jobs >= ((size_t)1 << 24) || n_wgs >= ((size_t)1 << 24) || n_tiles >= ((size_t)1 << 24))
    return hipErrorInvalidValue;
  if (lds_rows > (POS_INGEST_TILE_ROWS << POS_INGEST_MAX_LOG_ENC) * 8) return hipErrorInvalidValue;
  if (lds_bm > pos_locate_bm_lds((size_t)1 << POS_INGEST_MAX_LOG_ENC)) return hipErrorInvalidValue;
  prof::Scope ps("pos_group_locate", s);
  hipError_t e;
  if (any_listed && (e = pos_group_repair_locators(arena, jobs, n_jobs, tw, tabs, s)) != hipSuccess) return e;
  if (n_wgs && n_tiles) {
    hipLaunchKernelGGL((k_group_locate_rows<Ft63>), dim3((unsigned)n_wgs), dim3(256), lds_rows, s, arena, jobs, ljobs,
                       tiles, wgs, tw, tabs, synd, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((k_group_locate_bm<Ft63>), dim3((unsigned)(n_tiles * 8)), dim3(64), lds_bm, s, arena, jobs, ljobs,
                       tiles, tw, synd, flags, rstat, masks);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_group_locate_cols, dim3((unsigned)n_jobs), dim3(256), 0, s, arena, jobs, ljobs, rstat, masks,
                     col_status);
  return hipGetLastError();
}

}  // namespace lcpc
