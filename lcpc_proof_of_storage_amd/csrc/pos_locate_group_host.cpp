// pos_locate_group_host.cpp -- grouped syndrome decode of stored files: a queue of (stored
// image, known-bad columns) jobs answered -- which columns hold a wrong element, how many rows are no
// codewords, how many of those name their wrong positions -- with a number of launches that does not
// grow with the number of files.
//
//   RepairPlanner  (pos_rowgroup_plan.hpp, host only) cuts the jobs, in order, into steps exactly as for
//                  the grouped repair with the known columns as the listed ones: a staging group of
//                  consecutive jobs (at most four launches) or one job for lcpc_pos_locate_porenc;
//   LocateRunner   stages a group -- the repair's upload half and the locate records
//                  (pos_locate_plan.hpp) in one page-locked block, one upload -- queues its launches and
//                  the read-back of row statuses, column statuses and row flags into the same block; two
//                  blocks alternate, and the host hands group k - 1 to the jobs while group k runs
//                  (pos_rowgroup_stage.hpp).
// A job one of whose read columns holds a word that is not < p (the row launch's flag) is answered by
// lcpc_pos_locate_porenc after the last group: that entry names such columns and takes them as erasures.
#include "pos_locate_plan.hpp"
#include "pos_rowgroup_stage.hpp"

namespace {

struct LocateRunner {
  Device *dev;
  hipStream_t s;
  const uint32_t *tw;
  lcpc_pos_locate_job *all;
  const lcpc_pos_repair_job *shadow;
  std::vector<uint8_t> &noncanon;  // per job of the call: a read column holds a word that is not < p
  DBuf arena, tabs, synd, masks, out;
  struct Pending {
    size_t job_lo = 0, o_rstat = 0, o_cols = 0, o_flags = 0;
    std::vector<uint32_t> src;
    std::vector<PosRepairJob> jobs;
    std::vector<locate::PosLocateJob> ljobs;
  };
  TwoSlotStager<Pending> stage;

  LocateRunner(Device *d, hipStream_t stream, const uint32_t *twiddles, lcpc_pos_locate_job *jobs,
               const lcpc_pos_repair_job *sh, std::vector<uint8_t> &nc)
      : dev(d), s(stream), tw(twiddles), all(jobs), shadow(sh), noncanon(nc),
        stage(d, stream, [this](Pending &p, const uint8_t *h) { scatter(p, h); }) {}

  void scatter(const Pending &p, const uint8_t *h) {
    prof::HostScope hs("pos_group_locate_scatter");
    auto one = [&](size_t i) {
      const PosRepairJob &g = p.jobs[i];
      const size_t j = p.job_lo + p.src[i];
      lcpc_pos_locate_job &job = all[j];
      const size_t enc = (size_t)1 << g.log_enc;
      const uint8_t *flags = h + p.o_flags + g.row0, *rstat = h + p.o_rstat + g.row0;
      const uint8_t *cols = h + p.o_cols + p.ljobs[i].col0;
      uint8_t any = 0;
      for (size_t r = 0; r < g.n_rows; r++) any |= flags[r];
      if (any & lcpc::POS_REPAIR_ROW_NONCANON) {  // (nothing of this job is written here)
        noncanon[j] = 1;
        return;
      }
      std::memcpy(job.col_status, cols, enc);
      if (job.row_status && g.n_rows) std::memcpy(job.row_status, rstat, g.n_rows);
      const locate::Counters c = locate::count(cols, enc, rstat, g.n_rows);
      job.n_bad_cols = c.n_bad_cols, job.n_dirty_rows = c.n_dirty_rows, job.n_unlocatable_rows = c.n_unlocatable_rows;
      job.status = LCPC_OK;
    };
    if (p.jobs.size() < 64) {
      for (size_t i = 0; i < p.jobs.size(); i++) one(i);
    } else {
      parallel_for(p.jobs.size(), one);
    }
  }

  lcpc_status run(RepairStep &g) {
    lcpc_status st;
    const size_t n_jobs = g.jobs.size();
    std::vector<locate::PosLocateJob> ljobs;
    const locate::Layout L = locate::lay_out(g, shadow, ljobs);
    const TableOffsets &T = L.R.T;
    uint8_t *h = nullptr;
    if ((st = stage.begin(L.total, &h))) return st;
    if ((st = ensure(arena, dev, L.in_bytes, (size_t)4 << 20)) || (st = ensure(tabs, dev, g.tab_elems * POS_WB + 16, (size_t)1 << 20)) ||
        (st = ensure(synd, dev, L.synd_elems * 8 + 16, (size_t)4 << 20)) ||
        (st = ensure(masks, dev, L.mask_words * 8 + 16, (size_t)1 << 20)) || (st = ensure(out, dev, L.out_bytes, (size_t)1 << 20)))
      return st;
    {
      prof::HostScope hs("pos_group_locate_gather");
      locate::pack(g, shadow, L, ljobs, h);
    }
    const uint8_t *d = arena.as<uint8_t>();
    uint8_t *dout = out.as<uint8_t>();
    st = h2d_blocks(dev, arena.as<uint8_t>(), h, L.in_bytes, L.in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_locate(d, reinterpret_cast<const PosRepairJob *>(d + T.o_jobs),
                               reinterpret_cast<const locate::PosLocateJob *>(d + L.o_ljobs), n_jobs,
                               reinterpret_cast<const PosIngestTile *>(d + T.o_tiles), g.tiles.size(),
                               reinterpret_cast<const PosIngestWg *>(d + T.o_wgs), g.wgs.size(), g.lds_bytes, L.lds_bm,
                               L.any_listed, tw, tabs.as<uint32_t>(), synd.as<uint64_t>(), masks.as<uint64_t>(),
                               dout + L.d_flags, dout, dout + L.d_cols, s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + L.in_bytes, out.p, L.out_bytes, hipMemcpyDeviceToHost, s));
    return stage.commit(Pending{g.job_lo, L.in_bytes, L.in_bytes + L.d_cols, L.in_bytes + L.d_flags, std::move(g.src),
                                std::move(g.jobs), std::move(ljobs)});
  }
};

// lcpc_pos_locate_porenc, whole, into the job's own fields; row_status has no per-file counterpart
lcpc_status locate_single(lcpc_pos_locate_job &job) {
  size_t n_bad = job.n_bad_cols, n_dirty = job.n_dirty_rows, n_unloc = job.n_unlocatable_rows;
  const lcpc_status st = lcpc_pos_locate_porenc(job.porenc, job.pre, job.enc, job.rows_written, job.row_capacity,
                                                job.known_bad, job.n_known, job.col_status, &n_bad, &n_dirty, &n_unloc);
  if (st != LCPC_OK && st != LCPC_ERR_UNRECOVERABLE) return st;
  job.status = st;
  if (st != LCPC_OK) return LCPC_OK;
  job.n_bad_cols = n_bad, job.n_dirty_rows = n_dirty, job.n_unlocatable_rows = n_unloc;
  if (job.row_status && job.rows_written) std::memset(job.row_status, LCPC_POS_LOCATE_ROW_NOT_EVALUATED, job.rows_written);
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_locate_files_grouped(lcpc_pos_locate_job *jobs, size_t n_jobs) {
  if (!jobs) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  std::vector<size_t> rows(n_jobs), pre(n_jobs), enc(n_jobs), n_known(n_jobs);
  std::vector<lcpc_pos_repair_job> shadow(n_jobs);
  std::vector<uint64_t> seen;
  for (size_t j = 0; j < n_jobs; j++) {
    const lcpc_pos_locate_job &job = jobs[j];
    const std::string at = "job " + std::to_string(j);
    if (!job.porenc && job.rows_written) return fail(LCPC_ERR_INVALID_ARG, at + " has no image");
    if (job.rows_written > job.row_capacity) return fail(LCPC_ERR_INVALID_ARG, at + ": rows_written > row_capacity");
    if (lcpc_status st = pos_dims_check(job.pre, job.enc)) return st;
    if (!job.col_status) return fail(LCPC_ERR_INVALID_ARG, at + " has no col_status");
    if (!job.known_bad && job.n_known) return fail(LCPC_ERR_INVALID_ARG, at + " has no column list");
    seen.assign(job.known_bad, job.known_bad + job.n_known);
    std::sort(seen.begin(), seen.end());
    if (!seen.empty() && seen.back() >= job.enc) return fail(LCPC_ERR_INVALID_ARG, at + ": column index out of range");
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return fail(LCPC_ERR_INVALID_ARG, at + ": duplicate column index");
    rows[j] = job.rows_written, pre[j] = job.pre, enc[j] = job.enc, n_known[j] = job.n_known;
    shadow[j] = locate::as_repair(job);
  }
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const uint32_t *tw = nullptr;
  if ((st = pos_group_twiddles(dev, lease.s, &tw))) return st;
  RepairPlanner planner(rows.data(), pre.data(), enc.data(), n_known.data(), n_jobs, pos_group_bytes());
  for (size_t j = 0; j < n_jobs; j++)
    if (!planner.works(j)) jobs[j].status = LCPC_ERR_UNRECOVERABLE;  // more erasures than the code's redundancy
  std::vector<uint8_t> noncanon(n_jobs, 0);
  {
    LocateRunner runner(dev, lease.s, tw, jobs, shadow.data(), noncanon);
    RepairStep g;
    while (planner.next(g)) {
      if (g.single) {
        if ((st = locate_single(jobs[g.job_lo]))) return st;
        continue;
      }
      if (g.jobs.empty()) continue;  // none of its jobs does device work
      if ((st = runner.run(g))) return st;
    }
    if ((st = runner.stage.finish())) return st;
  }
  for (size_t j = 0; j < n_jobs; j++)
    if (noncanon[j] && (st = locate_single(jobs[j]))) return st;
  return LCPC_OK;
}

}  // extern "C"
