// pos_repair_plan.hpp -- the host-only half of the grouped repair of stored files: how a
// queue of jobs is cut into staging groups, how a group's page-locked block is laid out, and how the
// columns that are not listed are packed into it.  No device call, no allocation on a device: the CPU
// tests (lcpc_pos_repair_plan) and tools/hostsan/pos_repair_san.cpp drive exactly this code;
// pos_repair_group_host.cpp adds the uploads and launches.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/lcpc_mi.h"
#include "pos.hpp"
#include "pos_image.hpp"

namespace lcpc_host {
namespace repair {

using lcpc::PosIngestTile;
using lcpc::PosIngestWave;
using lcpc::PosIngestWg;
using lcpc::PosRepairJob;
using lcpc::POS_INGEST_MAX_CHUNKS;
using lcpc::POS_INGEST_MAX_LOG_ENC;
using lcpc::POS_INGEST_TILE_ROWS;
using lcpc::POS_INGEST_WG_ELEMS;

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }
inline size_t rows_pad(size_t n_rows) { return align_up(n_rows, 2); }
inline size_t leaf_chunks(size_t n_rows) { return ceil_div(8 + 2 * n_rows, 256); }
// the written rows of n_cols columns, each column 16-byte aligned
inline size_t packed_bytes(size_t n_rows, size_t n_cols) { return rows_pad(n_rows) * n_cols * POS_WB; }
// tile slots of a workgroup of rows of enc points
inline size_t wg_slots(size_t enc) { return std::max<size_t>(1, POS_INGEST_WG_ELEMS / (POS_INGEST_TILE_ROWS * enc)); }
inline uint32_t log2_pow2(size_t v) { return (uint32_t)__builtin_ctzll((unsigned long long)v); }

static_assert(LCPC_POS_REPAIR_MAX_ENC == LCPC_POS_INGEST_MAX_ENC);
static_assert(LCPC_POS_REPAIR_TILE_ROWS == POS_INGEST_TILE_ROWS);
static_assert(sizeof(PosRepairJob) % 16 == 0);

struct Step {
  bool single = false;
  size_t job_lo = 0, job_hi = 0;
  // a staging group: jobs[i] is job job_lo + src[i] of the call (img = the packed image's offset in the
  // staged arena; the offsets of the maps, lists and leaves are set when the block is laid out); the
  // bytes of the packed images and of the repaired columns, the elements of the locator tables, the
  // chaining values, repaired digests, columns and rows of its jobs, the LDS of its row launch and the
  // largest chunk count
  std::vector<uint32_t> src;
  std::vector<size_t> col0;  // the first of jobs[i]'s enc columns among the group's
  std::vector<PosRepairJob> jobs;
  std::vector<PosIngestTile> tiles;
  std::vector<PosIngestWg> wgs;
  std::vector<PosIngestWave> waves;
  size_t image_bytes = 0, rep_bytes = 0, tab_elems = 0, cv_slots = 0, n_dig = 0, n_cols = 0, n_rows = 0, lds_bytes = 0,
         max_chunks = 1;
};

// Cuts the jobs, in order, into steps: a staging group of consecutive jobs (its tables built here) or
// one job for lcpc_pos_repair_columns (enc above LCPC_POS_REPAIR_MAX_ENC, an image above group_bytes,
// or more leaf chunks than the fold's stack holds).  A job with more listed columns than the code can
// restore is in no table: it does no device work and ends no group.
class Planner {
 public:
  Planner(const size_t *rows, const size_t *pre, const size_t *enc, const size_t *n_bad, size_t n_jobs,
          size_t group_bytes)
      : rows_(rows), pre_(pre), enc_(enc), n_bad_(n_bad), n_jobs_(n_jobs), gb_(group_bytes) {}

  // whether the code can restore the job's listed columns (else: no device work)
  bool works(size_t j) const { return n_bad_[j] <= enc_[j] - pre_[j]; }

  bool next(Step &st) {
    st = Step{};
    if (next_ >= n_jobs_) return false;
    const size_t lo = next_;
    st.job_lo = lo;
    if (!grouped(lo)) {
      st.single = true;
      st.job_hi = next_ = lo + 1;
      return true;
    }
    size_t hi = lo, n = 0, bytes = 0, rows = 0, tiles = 0, tree = 0;
    for (; hi < n_jobs_ && grouped(hi); hi++) {
      if (!works(hi)) continue;
      // the image on the device is the packed columns and the repaired ones: enc columns in all
      const size_t nr = rows_[hi], nb = packed_bytes(nr, enc_[hi]);
      const size_t nt = ceil_div(nr, POS_INGEST_TILE_ROWS), tb = (2 * enc_[hi] - 1) * 32;
      if (n && (bytes + nb > gb_ || n >= LCPC_POS_INGEST_MAX_JOBS || rows + nr > LCPC_POS_INGEST_MAX_ROWS ||
                tiles + nt > LCPC_POS_INGEST_MAX_TILES || tree + tb > LCPC_POS_INGEST_MAX_TREE_BYTES))
        break;
      n++, bytes += nb, rows += nr, tiles += nt, tree += tb;
    }
    st.job_hi = next_ = hi;
    build(st);
    return true;
  }

 private:
  bool grouped(size_t j) const {
    if (!works(j)) return true;
    const size_t nr = rows_[j];
    return enc_[j] <= LCPC_POS_REPAIR_MAX_ENC && nr <= LCPC_POS_INGEST_MAX_ROWS && packed_bytes(nr, enc_[j]) <= gb_ &&
           leaf_chunks(nr) <= POS_INGEST_MAX_CHUNKS && ceil_div(nr, POS_INGEST_TILE_ROWS) <= LCPC_POS_INGEST_MAX_TILES;
  }

  void build(Step &st) const {
    // tiles by row length, the longest rows first (their workgroups run longest), jobs in order
    std::vector<PosIngestTile> by_len[POS_INGEST_MAX_LOG_ENC + 1];
    size_t img = 0, rep = 0, tab = 0, cv0 = 0, dig0 = 0, col0 = 0, row0 = 0, max_enc = 2;
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      if (!works(j)) continue;
      const size_t pre = pre_[j], enc = enc_[j], nr = rows_[j], nb = n_bad_[j], nc = leaf_chunks(nr);
      const uint32_t le = log2_pow2(enc), ji = (uint32_t)st.jobs.size();
      PosRepairJob t{};
      t.img = img, t.lam0 = tab, t.dinv0 = tab + enc, t.rep = rep, t.cv0 = cv0, t.dig0 = dig0, t.row0 = row0;
      t.pre = (uint32_t)pre, t.log_enc = le, t.n_rows = (uint32_t)nr, t.rows_pad = (uint32_t)rows_pad(nr);
      t.n_chunks = (uint32_t)nc, t.n_bad = (uint32_t)nb;
      st.jobs.push_back(t);
      st.src.push_back((uint32_t)(j - st.job_lo));
      st.col0.push_back(col0);
      for (size_t r = 0; r < nr; r += POS_INGEST_TILE_ROWS)
        by_len[le].push_back(PosIngestTile{ji, (uint32_t)r, (uint32_t)std::min(POS_INGEST_TILE_ROWS, nr - r), 0});
      for (size_t c = 0; c < nc; c++)
        for (size_t k = 0; k < nb; k += 64) st.waves.push_back(PosIngestWave{ji, (uint32_t)k, (uint32_t)c, 0});
      if (nr) max_enc = std::max(max_enc, enc);
      st.max_chunks = std::max(st.max_chunks, nc);
      img += packed_bytes(nr, enc - nb);
      rep += packed_bytes(nr, nb);
      tab += enc + nb;
      cv0 += nc * nb;
      dig0 += nb;
      col0 += enc;
      row0 += nr;
    }
    st.image_bytes = img;
    st.rep_bytes = rep;
    st.tab_elems = tab;
    st.cv_slots = cv0;
    st.n_dig = dig0;
    st.n_cols = col0;
    st.n_rows = row0;
    st.lds_bytes = std::max(POS_INGEST_WG_ELEMS, POS_INGEST_TILE_ROWS * max_enc) * POS_WB;
    for (int le = POS_INGEST_MAX_LOG_ENC; le >= 1; le--) {
      const size_t slots = wg_slots((size_t)1 << le);
      for (const PosIngestTile &t : by_len[le]) {
        if (st.wgs.empty() || st.wgs.back().log_enc != (uint32_t)le || st.wgs.back().n_tiles == slots)
          st.wgs.push_back(PosIngestWg{(uint32_t)st.tiles.size(), 0, (uint32_t)le, 0});
        st.wgs.back().n_tiles++;
        st.tiles.push_back(t);
      }
    }
  }

  const size_t *rows_, *pre_, *enc_, *n_bad_;
  size_t n_jobs_, gb_, next_ = 0;
};

inline bool wants_tree(const lcpc_pos_repair_job &job) { return job.tree_out || job.root_out; }

// cmap of one job (pos.hpp): k >= 0 for the k-th listed column, -1 - q for packed column q
inline void column_map(const lcpc_pos_repair_job &job, int32_t *cmap) {
  for (size_t c = 0; c < job.enc; c++) cmap[c] = -1;
  for (size_t k = 0; k < job.n_bad; k++) cmap[job.bad_cols[k]] = (int32_t)k;
  int32_t q = 0;
  for (size_t c = 0; c < job.enc; c++)
    if (cmap[c] < 0) cmap[c] = -1 - q++;
}

// The block of a group: [packed images | leaves, single-path digests | maps, lists | jobs | tiles | wgs |
// waves] go up (in_bytes); [flags | digests | trees] (out_bytes, offsets within the device's output
// buffer) and, where a job wants them, [repaired columns] come back behind them.
struct Layout {
  size_t o_jobs = 0, o_tiles = 0, o_wgs = 0, o_waves = 0, in_bytes = 0, d_dig = 0, d_trees = 0, out_bytes = 0, total = 0;
  bool want_cols = false;
};

// Sets the offsets the planner left open in g.jobs.  tree_only: the step's one job went through
// lcpc_pos_repair_columns and only its tree is built here, from that call's digests.
inline Layout lay_out(Step &g, const lcpc_pos_repair_job *all, bool tree_only) {
  Layout L;
  const size_t n_jobs = g.jobs.size();
  size_t o = align_up(g.image_bytes, 32), n_tree_dig = 0;
  for (size_t i = 0; i < n_jobs; i++) {
    const lcpc_pos_repair_job &job = all[g.job_lo + g.src[i]];
    PosRepairJob &t = g.jobs[i];
    const size_t enc = (size_t)1 << t.log_enc;
    L.want_cols |= job.cols_out != nullptr && t.n_bad && t.n_rows && !tree_only;
    t.tree_only = tree_only;
    t.has_tree = job.leaves != nullptr && wants_tree(job);
    if (t.has_tree) {
      t.leaves = o;
      o += enc * 32;
      t.tree0 = n_tree_dig;
      n_tree_dig += 2 * enc - 1;
    }
    if (tree_only) {
      t.dig_in = o;
      o += (size_t)t.n_bad * 32;
    }
  }
  for (size_t i = 0; i < n_jobs; i++) {
    PosRepairJob &t = g.jobs[i];
    t.cmap = o;
    o += ((size_t)4 << t.log_enc);
    t.bad = o;
    o += (size_t)t.n_bad * 4;
  }
  L.o_jobs = align_up(o, 16);
  L.o_tiles = L.o_jobs + n_jobs * sizeof(PosRepairJob);
  L.o_wgs = L.o_tiles + g.tiles.size() * sizeof(PosIngestTile);
  L.o_waves = L.o_wgs + g.wgs.size() * sizeof(PosIngestWg);
  L.in_bytes = align_up(L.o_waves + g.waves.size() * sizeof(PosIngestWave), 256);
  L.d_dig = align_up(g.n_rows, 32);
  L.d_trees = L.d_dig + 32 * g.n_dig;
  L.out_bytes = align_up(L.d_trees + 32 * n_tree_dig + 1, 256);
  L.total = L.in_bytes + L.out_bytes + (L.want_cols ? g.rep_bytes : 0);
  return L;
}

// Fills the first in_bytes of the block h.  The maps come first: the packing reads them, and a listed
// column of an image is never addressed.  Per column only the written rows are copied: the slack up to
// row_capacity never crosses the bus.
inline void pack(const Step &g, const lcpc_pos_repair_job *all, const Layout &L, const uint8_t *single_digests,
                 uint8_t *h) {
  const size_t n_jobs = g.jobs.size();
  const bool tree_only = single_digests != nullptr;
  auto tables = [&](size_t i) {
    const PosRepairJob &t = g.jobs[i];
    const lcpc_pos_repair_job &job = all[g.job_lo + g.src[i]];
    column_map(job, reinterpret_cast<int32_t *>(h + t.cmap));
    uint32_t *bad = reinterpret_cast<uint32_t *>(h + t.bad);
    for (size_t c = 0; c < t.n_bad; c++) bad[c] = (uint32_t)job.bad_cols[c];
    if (t.has_tree) std::memcpy(h + t.leaves, job.leaves, ((size_t)32 << t.log_enc));
    if (tree_only && t.n_bad) std::memcpy(h + t.dig_in, single_digests, (size_t)t.n_bad * 32);
  };
  if (n_jobs < 64) {
    for (size_t i = 0; i < n_jobs; i++) tables(i);
  } else {
    parallel_for(n_jobs, tables);
  }
  auto pack_col = [&](size_t i, size_t c) {
    const PosRepairJob &t = g.jobs[i];
    const int32_t m = reinterpret_cast<const int32_t *>(h + t.cmap)[c];
    if (m >= 0) return;
    const lcpc_pos_repair_job &job = all[g.job_lo + g.src[i]];
    const size_t col = (size_t)t.rows_pad * POS_WB, n = (size_t)t.n_rows * POS_WB;
    uint8_t *dst = h + t.img + (size_t)(-1 - m) * col;
    std::memcpy(dst, job.porenc + c * job.row_capacity * POS_WB, n);
    if (n != col) std::memset(dst + n, 0, col - n);
  };
  // little to copy: this thread; else the group's columns, whatever job they belong to, over the host
  // threads in one pass (column gc of the group is column gc - col0 of the last job with col0 <= gc)
  const bool images = !tree_only && g.image_bytes;
  if (images && g.image_bytes < ((size_t)4 << 20)) {
    for (size_t i = 0; i < n_jobs; i++)
      for (size_t c = 0; g.jobs[i].n_rows && c < ((size_t)1 << g.jobs[i].log_enc); c++) pack_col(i, c);
  } else if (images) {
    parallel_for(g.n_cols, [&](size_t gc) {
      const size_t i = (size_t)(std::upper_bound(g.col0.begin(), g.col0.end(), gc) - g.col0.begin()) - 1;
      if (g.jobs[i].n_rows) pack_col(i, gc - g.col0[i]);
    });
  }
  std::memcpy(h + L.o_jobs, g.jobs.data(), n_jobs * sizeof(PosRepairJob));
  if (!g.tiles.empty()) std::memcpy(h + L.o_tiles, g.tiles.data(), g.tiles.size() * sizeof(PosIngestTile));
  if (!g.wgs.empty()) std::memcpy(h + L.o_wgs, g.wgs.data(), g.wgs.size() * sizeof(PosIngestWg));
  if (!g.waves.empty()) std::memcpy(h + L.o_waves, g.waves.data(), g.waves.size() * sizeof(PosIngestWave));
}

}  // namespace repair
}  // namespace lcpc_host
