// pos_repair_group_host.cpp -- grouped repair of stored files: a queue of (stored image,
// erasure set, leaves) jobs answered -- the listed columns recomputed from the others, their digests,
// the tree over the leaves with those digests in place, and a verdict per job -- with a number of
// launches that does not grow with the number of files.
//
//   RepairPlanner  (pos_rowgroup_plan.hpp, host only; the block's layout and the packing are
//                  pos_repair_plan.hpp) cuts the jobs, in order, into steps: a staging group of
//                  consecutive jobs (at most four launches) or one job for lcpc_pos_repair_columns;
//   RepairRunner   stages a group -- the written rows of the columns that are not listed packed, the
//                  leaves, the column maps, the lists and the tables in one page-locked block, one
//                  upload (h2d_blocks) -- queues its launches as the block lands and the read-back of
//                  flags, digests and trees (and of the repaired columns where a job wants them) into the
//                  same block; two blocks alternate, and the host hands group k - 1 to the jobs while
//                  group k runs (pos_rowgroup_stage.hpp);
//   lcpc_pos_repair_plan   the same steps as a work list, host only: what the CPU tests check.
#include "pos_repair_plan.hpp"
#include "pos_rowgroup_stage.hpp"

namespace {

using repair::wants_tree;

// One call's staging and launches.  run() returns with the group's upload, launches and read-back
// queued and the group before it handed to its jobs; the last group is handed over in finish().
struct RepairRunner {
  Device *dev;
  hipStream_t s;
  const uint32_t *tw;
  lcpc_pos_repair_job *all;
  DBuf arena, tabs, rep, cvs, out;
  struct Pending {
    bool tree_only = false, has_cols = false;
    size_t job_lo = 0, o_flags = 0, o_dig = 0, o_trees = 0, o_rep = 0;
    std::vector<uint32_t> src;
    std::vector<PosRepairJob> jobs;
  };
  TwoSlotStager<Pending> stage;

  RepairRunner(Device *d, hipStream_t stream, const uint32_t *twiddles, lcpc_pos_repair_job *jobs)
      : dev(d), s(stream), tw(twiddles), all(jobs),
        stage(d, stream, [this](Pending &p, const uint8_t *h) { scatter(p, h); }) {}

  void scatter(const Pending &p, const uint8_t *h) {
    prof::HostScope hs("pos_group_repair_scatter");
    auto one = [&](size_t i) {
      const PosRepairJob &g = p.jobs[i];
      lcpc_pos_repair_job &job = all[p.job_lo + p.src[i]];
      const size_t enc = (size_t)1 << g.log_enc;
      if (!p.tree_only) {
        uint8_t any = 0;
        for (size_t r = 0; r < g.n_rows; r++) any |= h[p.o_flags + g.row0 + r];
        job.status = any ? LCPC_ERR_UNRECOVERABLE : LCPC_OK;
        if (any) return;  // (the data outputs of a failed job are left as they were)
        if (job.digests_out && g.n_bad) std::memcpy(job.digests_out, h + p.o_dig + 32 * g.dig0, 32 * (size_t)g.n_bad);
        if (job.cols_out && p.has_cols)
          for (size_t c = 0; c < g.n_bad; c++)
            std::memcpy(job.cols_out + c * g.n_rows * POS_WB, h + p.o_rep + g.rep + c * g.rows_pad * POS_WB,
                        (size_t)g.n_rows * POS_WB);
      }
      if (g.has_tree) {
        const uint8_t *tree = h + p.o_trees + 32 * g.tree0;
        if (job.tree_out) std::memcpy(job.tree_out, tree, (2 * enc - 1) * 32);
        if (job.root_out) std::memcpy(job.root_out, tree + (2 * enc - 2) * 32, 32);
      }
    };
    if (p.jobs.size() < 64) {
      for (size_t i = 0; i < p.jobs.size(); i++) one(i);
    } else {
      parallel_for(p.jobs.size(), one);
    }
  }

  // single_digests: the step's one job went through lcpc_pos_repair_columns, which gave these digests of
  // its listed columns; only its tree is built here
  lcpc_status run(RepairStep &g, const uint8_t *single_digests = nullptr) {
    const bool tree_only = single_digests != nullptr;
    lcpc_status st;
    const size_t n_jobs = g.jobs.size();
    const repair::Layout L = repair::lay_out(g, all, tree_only);
    const TableOffsets &T = L.T;
    const size_t in_bytes = T.in_bytes, out_bytes = L.out_bytes;
    uint8_t *h = nullptr;
    if ((st = stage.begin(L.total, &h))) return st;
    if ((st = ensure(arena, dev, in_bytes, (size_t)4 << 20)) || (st = ensure(tabs, dev, g.tab_elems * POS_WB + 16, (size_t)1 << 20)) ||
        (st = ensure(rep, dev, g.rep_bytes + 16, (size_t)4 << 20)) || (st = ensure(cvs, dev, g.cv_slots * 32 + 32, (size_t)1 << 20)) ||
        (st = ensure(out, dev, out_bytes, (size_t)1 << 20)))
      return st;
    {
      prof::HostScope hs("pos_group_repair_gather");
      repair::pack(g, all, L, single_digests, h);
    }
    const uint8_t *d = arena.as<uint8_t>();
    uint8_t *dout = out.as<uint8_t>();
    st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_repair(d, reinterpret_cast<const PosRepairJob *>(d + T.o_jobs), n_jobs,
                               reinterpret_cast<const PosIngestTile *>(d + T.o_tiles),
                               reinterpret_cast<const PosIngestWg *>(d + T.o_wgs), g.wgs.size(), g.lds_bytes,
                               reinterpret_cast<const PosIngestWave *>(d + T.o_waves), g.waves.size(), g.max_chunks,
                               tree_only, tw, tabs.as<uint32_t>(), rep.as<uint8_t>(), cvs.as<uint32_t>(), dout,
                               dout + L.d_dig, dout + L.d_trees, s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + in_bytes, out.p, out_bytes, hipMemcpyDeviceToHost, s));
    if (L.want_cols) HIP_TRY(hipMemcpyAsync(h + in_bytes + out_bytes, rep.p, g.rep_bytes, hipMemcpyDeviceToHost, s));
    return stage.commit(Pending{tree_only, L.want_cols, g.job_lo, in_bytes, in_bytes + L.d_dig, in_bytes + L.d_trees,
                                in_bytes + out_bytes, std::move(g.src), std::move(g.jobs)});
  }
};

// lcpc_pos_repair_columns, whole; the tree (if wanted) goes through the group's last launch, alone
lcpc_status repair_single(lcpc_pos_repair_job &job, RepairRunner &runner, size_t j) {
  const bool tree = job.leaves && wants_tree(job);
  std::vector<uint8_t> own;
  uint8_t *digests = job.digests_out;
  if (tree && !digests && job.n_bad) {
    own.resize(job.n_bad * 32);
    digests = own.data();
  }
  const lcpc_status st = lcpc_pos_repair_columns(job.porenc, job.pre, job.enc, job.rows_written, job.row_capacity,
                                                 job.bad_cols, job.n_bad, job.cols_out, digests, nullptr);
  if (st != LCPC_OK && st != LCPC_ERR_UNRECOVERABLE) return st;
  job.status = st;
  if (st != LCPC_OK || !tree) return LCPC_OK;
  RepairStep g;
  g.job_lo = j, g.job_hi = j + 1;
  PosRepairJob t{};
  t.pre = (uint32_t)job.pre, t.log_enc = log2_pow2(job.enc), t.n_chunks = 1, t.n_bad = (uint32_t)job.n_bad;
  g.jobs.push_back(t);
  g.src.push_back(0);
  g.col0.push_back(0);
  g.lds_bytes = POS_INGEST_WG_ELEMS * POS_WB;
  const uint8_t none = 0;
  return runner.run(g, digests ? digests : &none);
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_repair_files_grouped(lcpc_pos_repair_job *jobs, size_t n_jobs) {
  if (!jobs) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  std::vector<size_t> rows(n_jobs), pre(n_jobs), enc(n_jobs), n_bad(n_jobs);
  std::vector<uint64_t> seen;
  for (size_t j = 0; j < n_jobs; j++) {
    const lcpc_pos_repair_job &job = jobs[j];
    const std::string at = "job " + std::to_string(j);
    if (!job.porenc && job.rows_written) return fail(LCPC_ERR_INVALID_ARG, at + " has no image");
    if (job.rows_written > job.row_capacity) return fail(LCPC_ERR_INVALID_ARG, at + ": rows_written > row_capacity");
    if (lcpc_status st = pos_dims_check(job.pre, job.enc)) return st;
    if (!job.bad_cols && job.n_bad) return fail(LCPC_ERR_INVALID_ARG, at + " has no column list");
    if (wants_tree(job) && !job.leaves) return fail(LCPC_ERR_INVALID_ARG, at + ": a tree or root needs the leaves");
    seen.assign(job.bad_cols, job.bad_cols + job.n_bad);
    std::sort(seen.begin(), seen.end());
    if (!seen.empty() && seen.back() >= job.enc) return fail(LCPC_ERR_INVALID_ARG, at + ": column index out of range");
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return fail(LCPC_ERR_INVALID_ARG, at + ": duplicate column index");
    rows[j] = job.rows_written, pre[j] = job.pre, enc[j] = job.enc, n_bad[j] = job.n_bad;
  }
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const uint32_t *tw = nullptr;
  if ((st = pos_group_twiddles(dev, lease.s, &tw))) return st;
  RepairPlanner planner(rows.data(), pre.data(), enc.data(), n_bad.data(), n_jobs, pos_group_bytes());
  for (size_t j = 0; j < n_jobs; j++) jobs[j].status = planner.works(j) ? LCPC_OK : LCPC_ERR_UNRECOVERABLE;
  RepairRunner runner(dev, lease.s, tw, jobs);
  RepairStep g;
  while (planner.next(g)) {
    if (g.single) {
      if ((st = repair_single(jobs[g.job_lo], runner, g.job_lo))) return st;
      continue;
    }
    if (g.jobs.empty()) continue;  // none of its jobs does device work
    if ((st = runner.run(g))) return st;
  }
  return runner.stage.finish();
}

lcpc_status lcpc_pos_repair_plan(const size_t *rows_written, const size_t *pre, const size_t *enc, const size_t *n_bad,
                                 size_t n_jobs, lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles,
                                 size_t *n_launches) {
  if (!rows_written || !pre || !enc || !n_bad || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  if (lcpc_status st = pos_dims_check(pre, enc, n_jobs)) return st;
  RepairPlanner planner(rows_written, pre, enc, n_bad, n_jobs, pos_group_bytes());
  emit_plan(planner, tiles, cap, n_tiles, n_launches);
  return LCPC_OK;
}

}  // extern "C"
