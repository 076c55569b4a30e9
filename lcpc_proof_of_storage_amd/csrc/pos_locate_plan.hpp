// pos_locate_plan.hpp -- what is the grouped locate's own of the host-only half of the
// grouped entries.  The cut into staging groups and the group's tables are the grouped repair's
// (pos_rowgroup_plan.hpp: RepairPlanner, RepairStep, with the known columns as the listed ones), and so
// are the block's upload half and the packing (pos_repair_plan.hpp: a locate job is staged as the repair
// job with the same image and list, no leaves and no outputs).  What is added here: the per-job records
// of where a row's syndromes, position mask and column statuses go, their place behind the repair's
// tables, and the bytes that come back.  No device call, no allocation on a device:
// tools/hostsan/pos_locate_san.cpp drives exactly this code; pos_locate_group_host.cpp adds the uploads
// and launches.
#pragma once
#include "pos_repair_plan.hpp"

namespace lcpc_host {
namespace locate {

using lcpc::PosLocateJob;

// the repair job that stages what this locate job stages: same image, the known columns listed
inline lcpc_pos_repair_job as_repair(const lcpc_pos_locate_job &job) {
  lcpc_pos_repair_job r{};
  r.porenc = job.porenc, r.pre = job.pre, r.enc = job.enc, r.rows_written = job.rows_written;
  r.row_capacity = job.row_capacity, r.bad_cols = job.known_bad, r.n_bad = job.n_known;
  return r;
}

// The block of a group: the repair's upload half [packed images | maps, lists | jobs | tiles | wgs |
// waves] (R.T.in_bytes), then [locate records] go up (in_bytes); [row status | column status | row flags]
// (out_bytes, offsets within the device's output buffer) come back behind them.  The syndrome and mask
// arenas stay on the device: synd_elems 8-byte elements (at most the packed images': a row of enc - n_bad
// packed words has enc - pre - n_bad syndromes) and mask_words 64-bit words.
struct Layout {
  repair::Layout R;
  size_t o_ljobs = 0, in_bytes = 0, d_cols = 0, d_flags = 0, out_bytes = 0, total = 0;
  size_t synd_elems = 0, mask_words = 0, lds_bm = 0;
  bool any_listed = false;
};

inline Layout lay_out(RepairStep &g, const lcpc_pos_repair_job *shadow, std::vector<PosLocateJob> &ljobs) {
  Layout L;
  L.R = repair::lay_out(g, shadow, false);
  const size_t n_jobs = g.jobs.size();
  ljobs.assign(n_jobs, PosLocateJob{});
  size_t enc_max = 2;
  for (size_t i = 0; i < n_jobs; i++) {
    const PosRepairJob &t = g.jobs[i];
    const size_t enc = (size_t)1 << t.log_enc;
    ljobs[i].synd0 = L.synd_elems, ljobs[i].mask0 = L.mask_words, ljobs[i].col0 = g.col0[i];
    L.synd_elems += (size_t)t.n_rows * (enc - t.pre - t.n_bad);
    L.mask_words += (size_t)t.n_rows * std::max<size_t>(1, enc / 64);
    L.any_listed |= t.n_bad != 0;
    if (t.n_rows) enc_max = std::max(enc_max, enc);
  }
  L.lds_bm = lcpc::pos_locate_bm_lds(enc_max);
  L.o_ljobs = L.R.T.in_bytes;
  L.in_bytes = align_up(L.o_ljobs + n_jobs * sizeof(PosLocateJob), 256);
  L.d_cols = align_up(g.n_rows, 32);
  L.d_flags = align_up(L.d_cols + g.n_cols, 32);
  L.out_bytes = align_up(L.d_flags + g.n_rows + 1, 256);
  L.total = L.in_bytes + L.out_bytes;
  return L;
}

// Fills the first in_bytes of the block h (the known columns of an image are never addressed)
inline void pack(const RepairStep &g, const lcpc_pos_repair_job *shadow, const Layout &L,
                 const std::vector<PosLocateJob> &ljobs, uint8_t *h) {
  repair::pack(g, shadow, L.R, nullptr, h);
  if (!ljobs.empty()) std::memcpy(h + L.o_ljobs, ljobs.data(), ljobs.size() * sizeof(PosLocateJob));
}

// What the host makes of a job's returned bytes: the three counters of lcpc_pos_locate_porenc
struct Counters {
  size_t n_bad_cols = 0, n_dirty_rows = 0, n_unlocatable_rows = 0;
};

inline Counters count(const uint8_t *col_status, size_t enc, const uint8_t *rstat, size_t n_rows) {
  Counters c;
  for (size_t i = 0; i < enc; i++) c.n_bad_cols += col_status[i] != 0;
  for (size_t r = 0; r < n_rows; r++) c.n_dirty_rows += rstat[r] != 0, c.n_unlocatable_rows += rstat[r] == 2;
  return c;
}

}  // namespace locate
}  // namespace lcpc_host
