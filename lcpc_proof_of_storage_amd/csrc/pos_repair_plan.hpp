// pos_repair_plan.hpp -- what is the grouped repair's own of the host-only half of the
// grouped entries: how a group's page-locked block is laid out and how the columns that are not listed
// are packed into it.  The cut into staging groups and the group's tables are pos_rowgroup_plan.hpp's
// (RepairPlanner, RepairStep).  No device call, no allocation on a device: the CPU tests
// (lcpc_pos_repair_plan) and tools/hostsan/pos_rowgroup_san.cpp drive exactly this code;
// pos_repair_group_host.cpp adds the uploads and launches.
#pragma once
#include "pos_rowgroup_plan.hpp"

namespace lcpc_host {
namespace repair {

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
// waves] go up (T.in_bytes); [flags | digests | trees] (out_bytes, offsets within the device's output
// buffer) and, where a job wants them, [repaired columns] come back behind them.
struct Layout {
  TableOffsets T;
  size_t d_dig = 0, d_trees = 0, out_bytes = 0, total = 0;
  bool want_cols = false;
};

// Sets the offsets the planner left open in g.jobs.  tree_only: the step's one job went through
// lcpc_pos_repair_columns and only its tree is built here, from that call's digests.
inline Layout lay_out(RepairStep &g, const lcpc_pos_repair_job *all, bool tree_only) {
  Layout L;
  const size_t n_jobs = g.jobs.size();
  size_t o = align_up(g.image_bytes, 32), n_tree_dig = 0;
  for (size_t i = 0; i < n_jobs; i++) {
    const lcpc_pos_repair_job &job = all[g.job_of((uint32_t)i)];
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
  L.T = table_offsets(g, o, n_jobs, sizeof(PosRepairJob));
  L.d_dig = align_up(g.n_rows, 32);
  L.d_trees = L.d_dig + 32 * g.n_dig;
  L.out_bytes = align_up(L.d_trees + 32 * n_tree_dig + 1, 256);
  L.total = L.T.in_bytes + L.out_bytes + (L.want_cols ? g.rep_bytes : 0);
  return L;
}

// Fills the first T.in_bytes of the block h.  The maps come first: the packing reads them, and a listed
// column of an image is never addressed.
inline void pack(const RepairStep &g, const lcpc_pos_repair_job *all, const Layout &L, const uint8_t *single_digests,
                 uint8_t *h) {
  const size_t n_jobs = g.jobs.size();
  const bool tree_only = single_digests != nullptr;
  auto tables = [&](size_t i) {
    const PosRepairJob &t = g.jobs[i];
    const lcpc_pos_repair_job &job = all[g.job_of((uint32_t)i)];
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
  if (!tree_only)
    pack_columns(
        g.jobs, g.col0, g.image_bytes, g.n_cols, h,
        [&](size_t i) -> const lcpc_pos_repair_job & { return all[g.job_of((uint32_t)i)]; },
        [&](size_t i, size_t c) {
          const int32_t m = reinterpret_cast<const int32_t *>(h + g.jobs[i].cmap)[c];
          return (ptrdiff_t)(m >= 0 ? -1 : -1 - m);
        });
  copy_tables(g, g.jobs, L.T, h);
}

}  // namespace repair
}  // namespace lcpc_host
