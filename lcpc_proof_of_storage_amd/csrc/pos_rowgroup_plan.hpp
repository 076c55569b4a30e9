// pos_rowgroup_plan.hpp -- the host-only half of the grouped ingest, scrub and repair of stored files
// (DESIGN §5l): the arithmetic of a stored image, how a queue of jobs is cut into staging groups, the
// tile / workgroup / wave tables of a group's row and chunk launches, where the tables go in the
// group's page-locked block, how stored columns are packed into it, and the work list the three
// lcpc_pos_*_plan entries give.  No device call, no allocation on a device: the CPU tests and
// tools/hostsan/pos_rowgroup_san.cpp drive exactly this code; pos_ingest_host.cpp, pos_scrub_host.cpp
// and pos_repair_group_host.cpp add the uploads and launches (pos_rowgroup_stage.hpp).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/lcpc_mi.h"
#include "pos.hpp"
#include "pos_image.hpp"

namespace lcpc_host {

using lcpc::PosIngestJob;
using lcpc::PosIngestTile;
using lcpc::PosIngestWave;
using lcpc::PosIngestWg;
using lcpc::PosRepairJob;
using lcpc::PosScrubJob;
using lcpc::POS_INGEST_MAX_CHUNKS;
using lcpc::POS_INGEST_MAX_LOG_ENC;
using lcpc::POS_INGEST_TILE_ROWS;
using lcpc::POS_INGEST_WG_ELEMS;

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }
inline size_t job_rows(size_t n_bytes, size_t pre) { return ceil_div(ceil_div(n_bytes, POS_DB), pre); }
inline size_t rows_pad(size_t n_rows) { return align_up(n_rows, 2); }
inline size_t leaf_chunks(size_t n_rows) { return ceil_div(8 + 2 * n_rows, 256); }
// the written rows of n_cols columns, each column 16-byte aligned
inline size_t packed_bytes(size_t n_rows, size_t n_cols) { return rows_pad(n_rows) * n_cols * POS_WB; }
// tile slots of a workgroup of rows of enc points
inline size_t wg_slots(size_t enc) { return std::max<size_t>(1, POS_INGEST_WG_ELEMS / (POS_INGEST_TILE_ROWS * enc)); }
inline uint32_t log2_pow2(size_t v) { return (uint32_t)__builtin_ctzll((unsigned long long)v); }

static_assert(((size_t)1 << POS_INGEST_MAX_LOG_ENC) == LCPC_POS_INGEST_MAX_ENC);
static_assert(POS_INGEST_TILE_ROWS == LCPC_POS_INGEST_TILE_ROWS);
static_assert(LCPC_POS_SCRUB_MAX_ENC == LCPC_POS_INGEST_MAX_ENC && LCPC_POS_REPAIR_MAX_ENC == LCPC_POS_INGEST_MAX_ENC);
static_assert(LCPC_POS_SCRUB_TILE_ROWS == POS_INGEST_TILE_ROWS && LCPC_POS_REPAIR_TILE_ROWS == POS_INGEST_TILE_ROWS);
static_assert(sizeof(PosRepairJob) % 16 == 0);

// ---------------------------------------------------------------- a step and its tables
// What a step of any of the three entries is: one job for the single-file path, or a staging group of
// the consecutive jobs [job_lo, job_hi) with the tables of its row launch (tiles in workgroups) and of
// its chunk launch (waves), the LDS of the row launch and the largest chunk count.  The entry's own
// step adds its job table and totals.
struct RowGroup {
  bool single = false;
  size_t job_lo = 0, job_hi = 0;
  std::vector<PosIngestTile> tiles;
  std::vector<PosIngestWg> wgs;
  std::vector<PosIngestWave> waves;
  size_t lds_bytes = 0, max_chunks = 1;
  // the call's job behind entry i of the group's job table
  size_t job_of(uint32_t i) const { return job_lo + i; }
};

// Builds a group's tables: add() per job of the job table, in order, then finish().
class RowTables {
 public:
  explicit RowTables(RowGroup &g) : g_(g) {}

  // entry ji of the job table: n_rows rows of 2^log_enc points, wave_cols columns with chunk waves;
  // returns the chunks of a column's leaf message
  size_t add(uint32_t ji, uint32_t log_enc, size_t n_rows, size_t wave_cols) {
    const size_t nc = leaf_chunks(n_rows);
    for (size_t r = 0; r < n_rows; r += POS_INGEST_TILE_ROWS)
      by_len_[log_enc].push_back(PosIngestTile{ji, (uint32_t)r, (uint32_t)std::min(POS_INGEST_TILE_ROWS, n_rows - r), 0});
    for (size_t c = 0; c < nc; c++)
      for (size_t k = 0; k < wave_cols; k += 64) g_.waves.push_back(PosIngestWave{ji, (uint32_t)k, (uint32_t)c, 0});
    if (n_rows) max_enc_ = std::max(max_enc_, (size_t)1 << log_enc);
    g_.max_chunks = std::max(g_.max_chunks, nc);
    return nc;
  }

  // tiles by row length, the longest rows first (their workgroups run longest), jobs in order
  void finish() {
    g_.lds_bytes = std::max(POS_INGEST_WG_ELEMS, POS_INGEST_TILE_ROWS * max_enc_) * POS_WB;
    for (int le = POS_INGEST_MAX_LOG_ENC; le >= 1; le--) {
      const size_t slots = wg_slots((size_t)1 << le);
      for (const PosIngestTile &t : by_len_[le]) {
        if (g_.wgs.empty() || g_.wgs.back().log_enc != (uint32_t)le || g_.wgs.back().n_tiles == slots)
          g_.wgs.push_back(PosIngestWg{(uint32_t)g_.tiles.size(), 0, (uint32_t)le, 0});
        g_.wgs.back().n_tiles++;
        g_.tiles.push_back(t);
      }
    }
  }

 private:
  RowGroup &g_;
  std::vector<PosIngestTile> by_len_[POS_INGEST_MAX_LOG_ENC + 1];
  size_t max_enc_ = 2;
};

// ---------------------------------------------------------------- the cut
// What a job weighs in a group: the bytes it stages (against the group's size), a second byte count
// (ingest: its encoded matrix, against four times the group's size; else 0), its rows and row length.
struct JobCost {
  size_t bytes, bytes2, rows, enc;
};

// whether a job of this cost goes into a staging group at all (else: the single-file path)
inline bool fits_group(const JobCost &c, size_t group_bytes) {
  return c.enc <= LCPC_POS_INGEST_MAX_ENC && c.bytes <= group_bytes && c.bytes2 <= 4 * group_bytes &&
         leaf_chunks(c.rows) <= POS_INGEST_MAX_CHUNKS && c.rows <= LCPC_POS_INGEST_MAX_ROWS &&
         ceil_div(c.rows, POS_INGEST_TILE_ROWS) <= LCPC_POS_INGEST_MAX_TILES;
}

// The next step of p's queue from job `next` on: g.single with one job that fits no group, or the
// longest run of jobs that stays within the group's bytes and the tables' limits.  p.cost(j) is job j's
// cost; a job with !p.works(j) (repair: more listed columns than the code restores) does no device
// work: it joins whatever group is open, ends none and counts toward no limit.  false: no job is left.
template <class Planner>
bool cut_next(const Planner &p, size_t n_jobs, size_t group_bytes, size_t &next, RowGroup &g) {
  if (next >= n_jobs) return false;
  auto grouped = [&](size_t j) { return !p.works(j) || fits_group(p.cost(j), group_bytes); };
  const size_t lo = next;
  g.job_lo = lo;
  if (!grouped(lo)) {
    g.single = true;
    g.job_hi = next = lo + 1;
    return true;
  }
  size_t hi = lo, n = 0, bytes = 0, bytes2 = 0, rows = 0, tiles = 0, tree = 0;
  for (; hi < n_jobs && grouped(hi); hi++) {
    if (!p.works(hi)) continue;
    const JobCost c = p.cost(hi);
    const size_t nt = ceil_div(c.rows, POS_INGEST_TILE_ROWS), tb = (2 * c.enc - 1) * 32;
    if (n && (bytes + c.bytes > group_bytes || bytes2 + c.bytes2 > 4 * group_bytes || n >= LCPC_POS_INGEST_MAX_JOBS ||
              rows + c.rows > LCPC_POS_INGEST_MAX_ROWS || tiles + nt > LCPC_POS_INGEST_MAX_TILES ||
              tree + tb > LCPC_POS_INGEST_MAX_TREE_BYTES))
      break;
    n++, bytes += c.bytes, bytes2 += c.bytes2, rows += c.rows, tiles += nt, tree += tb;
  }
  g.job_hi = next = hi;
  return true;
}

// ---------------------------------------------------------------- ingest
struct IngestStep : RowGroup {
  // jobs[i].base = the image's offset in the staged arena; the bytes of that arena and of the encoded
  // buffer, the chaining values and digests of the group's jobs
  std::vector<PosIngestJob> jobs;
  size_t image_bytes = 0, enc_bytes = 0, cv_slots = 0, tree_digests = 0;
};

// A job goes the single-file path with enc above LCPC_POS_INGEST_MAX_ENC, an image above group_bytes or
// an encoded matrix above four times that, or more leaf chunks than the fold's stack holds.
class IngestPlanner {
 public:
  using Step = IngestStep;
  IngestPlanner(const size_t *n_bytes, const size_t *pre, const size_t *enc, size_t n_jobs, size_t group_bytes)
      : n_bytes_(n_bytes), pre_(pre), enc_(enc), n_jobs_(n_jobs), gb_(group_bytes) {}

  size_t rows(size_t j) const { return job_rows(n_bytes_[j], pre_[j]); }
  bool works(size_t) const { return true; }
  JobCost cost(size_t j) const {
    return {align_up(n_bytes_[j], 8), packed_bytes(rows(j), enc_[j]), rows(j), enc_[j]};
  }

  bool next(Step &st) {
    st = Step{};
    if (!cut_next(*this, n_jobs_, gb_, next_, st)) return false;
    if (st.single) return true;
    RowTables tab(st);
    size_t base = 0, eoff = 0, cv0 = 0, tree0 = 0;
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      const size_t enc = enc_[j], nr = rows(j);
      const uint32_t le = log2_pow2(enc);
      const size_t nc = tab.add((uint32_t)(j - st.job_lo), le, nr, enc);
      st.jobs.push_back(PosIngestJob{base, n_bytes_[j], eoff, cv0, tree0, (uint32_t)pre_[j], le, (uint32_t)nr,
                                     (uint32_t)rows_pad(nr), (uint32_t)nc, 0});
      base += align_up(n_bytes_[j], 8);
      eoff += packed_bytes(nr, enc);
      cv0 += nc * enc;
      tree0 += 2 * enc - 1;
    }
    st.image_bytes = base, st.enc_bytes = eoff, st.cv_slots = cv0, st.tree_digests = tree0;
    tab.finish();
    return true;
  }

 private:
  const size_t *n_bytes_, *pre_, *enc_;
  size_t n_jobs_, gb_, next_ = 0;
};

// ---------------------------------------------------------------- scrub
struct ScrubStep : RowGroup {
  // jobs[i].img = the packed image's offset in the staged arena (tree and root are set when the block
  // is laid out); col0[i] = jobs[i].col0; the bytes of the packed images, the chaining values, columns
  // and rows of the group's jobs
  std::vector<PosScrubJob> jobs;
  std::vector<size_t> col0;
  size_t image_bytes = 0, cv_slots = 0, n_cols = 0, n_rows = 0;
};

// A job goes to the single-file entries with enc above LCPC_POS_SCRUB_MAX_ENC, a packed image above
// group_bytes, or more leaf chunks than the fold's stack holds.
class ScrubPlanner {
 public:
  using Step = ScrubStep;
  ScrubPlanner(const size_t *rows, const size_t *pre, const size_t *enc, size_t n_jobs, size_t group_bytes)
      : rows_(rows), pre_(pre), enc_(enc), n_jobs_(n_jobs), gb_(group_bytes) {}

  size_t rows(size_t j) const { return rows_[j]; }
  bool works(size_t) const { return true; }
  JobCost cost(size_t j) const { return {packed_bytes(rows_[j], enc_[j]), 0, rows_[j], enc_[j]}; }

  bool next(Step &st) {
    st = Step{};
    if (!cut_next(*this, n_jobs_, gb_, next_, st)) return false;
    if (st.single) return true;
    RowTables tab(st);
    size_t img = 0, cv0 = 0, col0 = 0, row0 = 0;
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      const size_t enc = enc_[j], nr = rows_[j];
      const uint32_t le = log2_pow2(enc);
      const size_t nc = tab.add((uint32_t)(j - st.job_lo), le, nr, enc);
      st.jobs.push_back(PosScrubJob{img, 0, 0, cv0, col0, row0, (uint32_t)pre_[j], le, (uint32_t)nr,
                                    (uint32_t)rows_pad(nr), (uint32_t)nc, 0, 0, 0});
      st.col0.push_back(col0);
      img += packed_bytes(nr, enc);
      cv0 += nc * enc;
      col0 += enc;
      row0 += nr;
    }
    st.image_bytes = img, st.cv_slots = cv0, st.n_cols = col0, st.n_rows = row0;
    tab.finish();
    return true;
  }

 private:
  const size_t *rows_, *pre_, *enc_;
  size_t n_jobs_, gb_, next_ = 0;
};

// ---------------------------------------------------------------- repair
struct RepairStep : RowGroup {
  // jobs[i] is job job_lo + src[i] of the call (img = the packed image's offset in the staged arena; the
  // offsets of the maps, lists and leaves are set when the block is laid out) and col0[i] the first of
  // its enc columns among the group's; the bytes of the packed images and of the repaired columns, the
  // elements of the locator tables, the chaining values, repaired digests, columns and rows of the jobs
  std::vector<uint32_t> src;
  std::vector<size_t> col0;
  std::vector<PosRepairJob> jobs;
  size_t image_bytes = 0, rep_bytes = 0, tab_elems = 0, cv_slots = 0, n_dig = 0, n_cols = 0, n_rows = 0;
  size_t job_of(uint32_t i) const { return job_lo + src[i]; }
};

// A job goes to lcpc_pos_repair_columns with enc above LCPC_POS_REPAIR_MAX_ENC, an image above
// group_bytes, or more leaf chunks than the fold's stack holds.  A job with more listed columns than the
// code can restore is in no table: it does no device work and ends no group.
class RepairPlanner {
 public:
  using Step = RepairStep;
  RepairPlanner(const size_t *rows, const size_t *pre, const size_t *enc, const size_t *n_bad, size_t n_jobs,
                size_t group_bytes)
      : rows_(rows), pre_(pre), enc_(enc), n_bad_(n_bad), n_jobs_(n_jobs), gb_(group_bytes) {}

  size_t rows(size_t j) const { return rows_[j]; }
  // whether the code can restore the job's listed columns (else: no device work)
  bool works(size_t j) const { return n_bad_[j] <= enc_[j] - pre_[j]; }
  // the image on the device is the packed columns and the repaired ones: enc columns in all
  JobCost cost(size_t j) const { return {packed_bytes(rows_[j], enc_[j]), 0, rows_[j], enc_[j]}; }

  bool next(Step &st) {
    st = Step{};
    if (!cut_next(*this, n_jobs_, gb_, next_, st)) return false;
    if (st.single) return true;
    RowTables tab(st);
    size_t img = 0, rep = 0, tb = 0, cv0 = 0, dig0 = 0, col0 = 0, row0 = 0;
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      if (!works(j)) continue;
      const size_t enc = enc_[j], nr = rows_[j], nb = n_bad_[j];
      const uint32_t le = log2_pow2(enc);
      const size_t nc = tab.add((uint32_t)st.jobs.size(), le, nr, nb);
      PosRepairJob t{};
      t.img = img, t.lam0 = tb, t.dinv0 = tb + enc, t.rep = rep, t.cv0 = cv0, t.dig0 = dig0, t.row0 = row0;
      t.pre = (uint32_t)pre_[j], t.log_enc = le, t.n_rows = (uint32_t)nr, t.rows_pad = (uint32_t)rows_pad(nr);
      t.n_chunks = (uint32_t)nc, t.n_bad = (uint32_t)nb;
      st.jobs.push_back(t);
      st.src.push_back((uint32_t)(j - st.job_lo));
      st.col0.push_back(col0);
      img += packed_bytes(nr, enc - nb);
      rep += packed_bytes(nr, nb);
      tb += enc + nb;
      cv0 += nc * nb;
      dig0 += nb;
      col0 += enc;
      row0 += nr;
    }
    st.image_bytes = img, st.rep_bytes = rep, st.tab_elems = tb, st.cv_slots = cv0, st.n_dig = dig0;
    st.n_cols = col0, st.n_rows = row0;
    tab.finish();
    return true;
  }

 private:
  const size_t *rows_, *pre_, *enc_, *n_bad_;
  size_t n_jobs_, gb_, next_ = 0;
};

// ---------------------------------------------------------------- the tables in the block
// [jobs | tiles | wgs | waves] behind whatever the entry stages first: the offsets in the block of a
// group whose own data ends at `end`, and the bytes that go up (in_bytes)
struct TableOffsets {
  size_t o_jobs = 0, o_tiles = 0, o_wgs = 0, o_waves = 0, in_bytes = 0;
};

inline TableOffsets table_offsets(const RowGroup &g, size_t end, size_t n_jobs, size_t job_bytes) {
  TableOffsets o;
  o.o_jobs = align_up(end, 16);
  o.o_tiles = o.o_jobs + n_jobs * job_bytes;
  o.o_wgs = o.o_tiles + g.tiles.size() * sizeof(PosIngestTile);
  o.o_waves = o.o_wgs + g.wgs.size() * sizeof(PosIngestWg);
  o.in_bytes = align_up(o.o_waves + g.waves.size() * sizeof(PosIngestWave), 256);
  return o;
}

// the four tables into the block h; any of them may be empty (a tree-only group has a job and no more)
template <class Job>
void copy_tables(const RowGroup &g, const std::vector<Job> &jobs, const TableOffsets &o, uint8_t *h) {
  auto put = [&](size_t at, const auto &v) {
    if (!v.empty()) std::memcpy(h + at, v.data(), v.size() * sizeof(v[0]));
  };
  put(o.o_jobs, jobs);
  put(o.o_tiles, g.tiles);
  put(o.o_wgs, g.wgs);
  put(o.o_waves, g.waves);
}

// Packs the stored columns of a group's jobs into the block h: jobs[i]'s image src(i) (column c is
// src(i).row_capacity elements from byte c * row_capacity * 8 of src(i).porenc) goes to h + jobs[i].img,
// column c as packed column map(i, c), or not at all where map gives a negative number.  Per column
// only the written rows are copied -- the slack up to row_capacity never crosses the bus -- and the pad
// up to rows_pad is zeroed.  col0[i] is the first of jobs[i]'s columns among the group's n_cols.
template <class Job, class Src, class Map>
void pack_columns(const std::vector<Job> &jobs, const std::vector<size_t> &col0, size_t image_bytes, size_t n_cols,
                  uint8_t *h, Src src, Map map) {
  auto pack_col = [&](size_t i, size_t c) {
    const Job &t = jobs[i];
    const ptrdiff_t q = map(i, c);
    if (q < 0) return;
    const auto &job = src(i);
    const size_t col = (size_t)t.rows_pad * POS_WB, n = (size_t)t.n_rows * POS_WB;
    uint8_t *dst = h + t.img + (size_t)q * col;
    std::memcpy(dst, job.porenc + c * job.row_capacity * POS_WB, n);
    if (n != col) std::memset(dst + n, 0, col - n);
  };
  // little to copy: this thread; else the group's columns, whatever job they belong to, over the host
  // threads in one pass (column gc of the group is column gc - col0 of the last job with col0 <= gc)
  if (!image_bytes) return;
  if (image_bytes < ((size_t)4 << 20)) {
    for (size_t i = 0; i < jobs.size(); i++)
      for (size_t c = 0; jobs[i].n_rows && c < ((size_t)1 << jobs[i].log_enc); c++) pack_col(i, c);
  } else {
    parallel_for(n_cols, [&](size_t gc) {
      const size_t i = (size_t)(std::upper_bound(col0.begin(), col0.end(), gc) - col0.begin()) - 1;
      if (jobs[i].n_rows) pack_col(i, gc - col0[i]);
    });
  }
}

// ---------------------------------------------------------------- the work list
// What lcpc_pos_ingest_plan, lcpc_pos_scrub_plan and lcpc_pos_repair_plan give: the tiles of every
// group's row launch, workgroup by workgroup (launch = the group), and one record with launch ==
// LCPC_POS_GROUP_SINGLE for a job with rows that goes the single-file path.  A group none of whose
// jobs does device work is no launch.
template <class Planner>
void emit_plan(Planner &planner, lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches) {
  typename Planner::Step g;
  size_t n = 0, launches = 0;
  auto emit = [&](const lcpc_pos_ingest_tile &t) {
    if (n < cap) tiles[n] = t;
    n++;
  };
  while (planner.next(g)) {
    if (g.single) {
      const size_t j = g.job_lo, nr = planner.rows(j);
      if (nr) emit(lcpc_pos_ingest_tile{j, 0, nr, LCPC_POS_GROUP_SINGLE, 0});
      continue;
    }
    if (g.jobs.empty()) continue;
    for (size_t w = 0; w < g.wgs.size(); w++)
      for (uint32_t i = 0; i < g.wgs[w].n_tiles; i++) {
        const PosIngestTile &t = g.tiles[g.wgs[w].tile0 + i];
        emit(lcpc_pos_ingest_tile{g.job_of(t.job), t.row_lo, (uint64_t)t.row_lo + t.n_rows, (uint32_t)launches,
                                  (uint32_t)w});
      }
    launches++;
  }
  if (n_tiles) *n_tiles = n;
  if (n_launches) *n_launches = launches;
}

}  // namespace lcpc_host
