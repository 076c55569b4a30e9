// pos_repair_group_host.cpp -- grouped repair of stored files: a queue of (stored image,
// erasure set, leaves) jobs answered -- the listed columns recomputed from the others, their digests,
// the tree over the leaves with those digests in place, and a verdict per job -- with a number of
// launches that does not grow with the number of files.
//
//   repair::Planner  (pos_repair_plan.hpp, host only, with the block's layout and the packing) cuts the
//                  jobs, in order, into steps: a staging group of consecutive jobs (at most four launches)
//                  or one job for lcpc_pos_repair_columns;
//   RepairRunner   stages a group -- the written rows of the columns that are not listed packed, the
//                  leaves, the column maps, the lists and the tables in one page-locked block, one
//                  upload (h2d_blocks) -- queues its launches as the block lands and the read-back of
//                  flags, digests and trees (and of the repaired columns where a job wants them) into the
//                  same block; two blocks alternate, and the host hands group k - 1 to the jobs while
//                  group k runs;
//   lcpc_pos_repair_plan   the same steps as a work list, host only: what the CPU tests check.
#include "pos_internal.hpp"
#include "pos_repair_plan.hpp"

#include <map>
#include <mutex>

namespace {

using repair::align_up;
using repair::wants_tree;
using RepairStep = repair::Step;

// the twiddles of the grouped lengths (the encode's table), built once per device and kept
lcpc_status repair_twiddles(Device *dev, hipStream_t s, const uint32_t **out) {
  static std::mutex mu;
  static std::map<int, uint32_t *> tables;
  std::lock_guard<std::mutex> lk(mu);
  auto it = tables.find(dev->id);
  if (it == tables.end()) {
    uint32_t *tw = nullptr;
    HIP_TRY(device_malloc(&tw, ((size_t)1 << POS_INGEST_MAX_LOG_ENC) * POS_WB));
    hipError_t e = pos_ingest_twiddles(tw, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(tw);
      HIP_TRY(e);
    }
    it = tables.emplace(dev->id, tw).first;
  }
  *out = it->second;
  return LCPC_OK;
}

// One call's staging and launches.  run() returns with the group's upload, launches and read-back
// queued and the group before it handed to its jobs; the last group is handed over in finish().
struct RepairRunner {
  Device *dev;
  hipStream_t s;
  const uint32_t *tw;
  lcpc_pos_repair_job *all;
  DBuf arena, tabs, rep, cvs, out;
  Pinned stg[2];
  Events ev;
  struct Pending {
    bool live = false, tree_only = false, has_cols = false;
    size_t job_lo = 0, o_flags = 0, o_dig = 0, o_trees = 0, o_rep = 0;
    std::vector<uint32_t> src;
    std::vector<PosRepairJob> jobs;
  } pend[2];
  int k = 0;

  RepairRunner(Device *d, hipStream_t stream, const uint32_t *twiddles, lcpc_pos_repair_job *jobs)
      : dev(d), s(stream), tw(twiddles), all(jobs) {}
  // (an early return leaves copies queued on the blocks the members are about to give back)
  ~RepairRunner() { (void)hipStreamSynchronize(s); }

  lcpc_status drain(int slot) {
    Pending &p = pend[slot];
    if (!p.live) return LCPC_OK;
    p.live = false;
    HIP_TRY(hipEventSynchronize(ev.e[slot]));
    prof::HostScope hs("pos_group_repair_scatter");
    const uint8_t *h = stg[slot].b();
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
    return LCPC_OK;
  }

  // single_digests: the step's one job went through lcpc_pos_repair_columns, which gave these digests of
  // its listed columns; only its tree is built here
  lcpc_status run(RepairStep &g, const uint8_t *single_digests = nullptr) {
    const int slot = k & 1;
    const bool tree_only = single_digests != nullptr;
    lcpc_status st;
    HIP_TRY(ev.init());
    if ((st = drain(slot))) return st;  // (already drained by the run before this one, but for an error there)
    const size_t n_jobs = g.jobs.size();
    const repair::Layout L = repair::lay_out(g, all, tree_only);
    const size_t in_bytes = L.in_bytes, out_bytes = L.out_bytes;
    if (stg[slot].n < L.total && !stg[slot].get(dev, L.total)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    if (arena.n < in_bytes || !arena.p) HIP_TRY(arena.alloc(dev, align_up(in_bytes, (size_t)4 << 20)));
    if (tabs.n < g.tab_elems * POS_WB + 16 || !tabs.p) HIP_TRY(tabs.alloc(dev, align_up(g.tab_elems * POS_WB + 16, (size_t)1 << 20)));
    if (rep.n < g.rep_bytes + 16 || !rep.p) HIP_TRY(rep.alloc(dev, align_up(g.rep_bytes + 16, (size_t)4 << 20)));
    if (cvs.n < g.cv_slots * 32 + 32 || !cvs.p) HIP_TRY(cvs.alloc(dev, align_up(g.cv_slots * 32 + 32, (size_t)1 << 20)));
    if (out.n < out_bytes || !out.p) HIP_TRY(out.alloc(dev, align_up(out_bytes, (size_t)1 << 20)));
    uint8_t *h = stg[slot].b();
    {
      prof::HostScope hs("pos_group_repair_gather");
      repair::pack(g, all, L, single_digests, h);
    }
    const uint8_t *d = arena.as<uint8_t>();
    uint8_t *dout = out.as<uint8_t>();
    st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_repair(d, reinterpret_cast<const PosRepairJob *>(d + L.o_jobs), n_jobs,
                               reinterpret_cast<const PosIngestTile *>(d + L.o_tiles),
                               reinterpret_cast<const PosIngestWg *>(d + L.o_wgs), g.wgs.size(), g.lds_bytes,
                               reinterpret_cast<const PosIngestWave *>(d + L.o_waves), g.waves.size(), g.max_chunks,
                               tree_only, tw, tabs.as<uint32_t>(), rep.as<uint8_t>(), cvs.as<uint32_t>(), dout,
                               dout + L.d_dig, dout + L.d_trees, s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + in_bytes, out.p, out_bytes, hipMemcpyDeviceToHost, s));
    if (L.want_cols) HIP_TRY(hipMemcpyAsync(h + in_bytes + out_bytes, rep.p, g.rep_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev.e[slot], s));
    Pending &p = pend[slot];
    p.live = true;
    p.tree_only = tree_only;
    p.has_cols = L.want_cols;
    p.job_lo = g.job_lo;
    p.o_flags = in_bytes, p.o_dig = in_bytes + L.d_dig, p.o_trees = in_bytes + L.d_trees, p.o_rep = in_bytes + out_bytes;
    p.src = std::move(g.src);
    p.jobs = std::move(g.jobs);
    k++;
    return drain(slot ^ 1);  // the group before this one, while this one runs
  }

  lcpc_status finish() {
    lcpc_status st;
    if ((st = drain(k & 1))) return st;
    if ((st = drain((k & 1) ^ 1))) return st;
    HIP_TRY(hipStreamSynchronize(s));
    return LCPC_OK;
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
  t.pre = (uint32_t)job.pre, t.log_enc = repair::log2_pow2(job.enc), t.n_chunks = 1, t.n_bad = (uint32_t)job.n_bad;
  g.jobs.push_back(t);
  g.src.push_back(0);
  g.col0.push_back(0);
  g.lds_bytes = POS_INGEST_WG_ELEMS * POS_WB;
  const uint8_t none = 0;
  return runner.run(g, digests ? digests : &none);
}

lcpc_status repair_dims(const size_t *pre, const size_t *enc, size_t n_jobs) {
  for (size_t j = 0; j < n_jobs; j++)
    if (lcpc_status st = pos_dims_check(pre[j], enc[j])) return st;
  return LCPC_OK;
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
  if ((st = repair_twiddles(dev, lease.s, &tw))) return st;
  repair::Planner planner(rows.data(), pre.data(), enc.data(), n_bad.data(), n_jobs, pos_group_bytes());
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
  return runner.finish();
}

lcpc_status lcpc_pos_repair_plan(const size_t *rows_written, const size_t *pre, const size_t *enc, const size_t *n_bad,
                                 size_t n_jobs, lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles,
                                 size_t *n_launches) {
  if (!rows_written || !pre || !enc || !n_bad || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  if (lcpc_status st = repair_dims(pre, enc, n_jobs)) return st;
  repair::Planner planner(rows_written, pre, enc, n_bad, n_jobs, pos_group_bytes());
  RepairStep g;
  size_t n = 0, launches = 0;
  auto emit = [&](const lcpc_pos_ingest_tile &t) {
    if (n < cap) tiles[n] = t;
    n++;
  };
  while (planner.next(g)) {
    if (g.single) {
      const size_t j = g.job_lo;
      if (rows_written[j]) emit(lcpc_pos_ingest_tile{j, 0, rows_written[j], LCPC_POS_GROUP_SINGLE, 0});
      continue;
    }
    if (g.jobs.empty()) continue;
    for (size_t w = 0; w < g.wgs.size(); w++)
      for (uint32_t i = 0; i < g.wgs[w].n_tiles; i++) {
        const PosIngestTile &t = g.tiles[g.wgs[w].tile0 + i];
        emit(lcpc_pos_ingest_tile{g.job_lo + g.src[t.job], t.row_lo, (uint64_t)t.row_lo + t.n_rows, (uint32_t)launches,
                                  (uint32_t)w});
      }
    launches++;
  }
  if (n_tiles) *n_tiles = n;
  if (n_launches) *n_launches = launches;
  return LCPC_OK;
}

}  // extern "C"
