// pos_scrub_host.cpp -- grouped scrub of stored files: a queue of (stored image, stored
// tree, expected root) jobs answered -- column statuses and digests, dirty rows of the row code, the
// stored tree's consistency and its root -- with a number of launches that does not grow with the
// number of files.
//
//   ScrubPlanner   (pos_rowgroup_plan.hpp, host only, with the column packing) cuts the jobs, in order,
//                  into steps: a staging group of consecutive jobs (at most three launches) or one job
//                  for the single-file entries;
//   ScrubRunner    stages a group -- the written rows of every column packed, the stored digests, the
//                  expected roots and the tables in one page-locked block, one upload (h2d_blocks) --
//                  queues its launches as the block lands and one read-back of flags, statuses, dirty
//                  bytes and digests into the same block; two blocks alternate, and the host hands
//                  group k - 1 to the jobs while group k runs (pos_rowgroup_stage.hpp);
//   lcpc_pos_scrub_plan   the same steps as a work list, host only: what the CPU tests check.
#include "pos_rowgroup_stage.hpp"

namespace {

static_assert(LCPC_POS_SCRUB_NOT_EVALUATED == POS_SCRUB_NOT_EVALUATED);

// One call's staging and launches.  run() returns with the group's upload, launches and read-back
// queued and the group before it handed to its jobs; the last group is handed over in finish().
struct ScrubRunner {
  Device *dev;
  hipStream_t s;
  const uint32_t *tw;
  lcpc_pos_scrub_job *all;
  DBuf arena, cvs, cflags, out;
  struct Pending {
    bool has_dig = false;
    size_t job_lo = 0, o_flags = 0, o_status = 0, o_dirty = 0, o_dig = 0;
    std::vector<PosScrubJob> jobs;
  };
  TwoSlotStager<Pending> stage;

  ScrubRunner(Device *d, hipStream_t stream, const uint32_t *twiddles, lcpc_pos_scrub_job *jobs)
      : dev(d), s(stream), tw(twiddles), all(jobs),
        stage(d, stream, [this](Pending &p, const uint8_t *h) { scatter(p, h); }) {}

  void scatter(const Pending &p, const uint8_t *h) {
    prof::HostScope hs("pos_group_scrub_scatter");
    auto one = [&](size_t i) {
      const PosScrubJob &g = p.jobs[i];
      lcpc_pos_scrub_job &job = all[p.job_lo + i];
      job.tree_consistent = h[p.o_flags + 2 * i];
      job.root_ok = h[p.o_flags + 2 * i + 1];
      if (g.tree_only) return;
      const size_t enc = (size_t)1 << g.log_enc;
      const uint8_t *st = h + p.o_status + g.col0, *dr = h + p.o_dirty + g.row0;
      std::memcpy(job.col_status, st, enc);
      if (job.digests && p.has_dig) std::memcpy(job.digests, h + p.o_dig + 32 * g.col0, enc * 32);
      size_t n_bad = 0, n_noncanon = 0, n_dirty = 0;
      for (size_t c = 0; c < enc; c++) n_bad += st[c] != 0, n_noncanon += st[c] == 2;
      for (size_t r = 0; r < g.n_rows; r++) n_dirty += dr[r] != 0;
      job.n_bad = n_bad;
      // a word that is not < p voids the row check of its file: the per-file path treats it as an erasure
      job.n_dirty_rows = n_noncanon ? LCPC_POS_SCRUB_ROWS_UNCHECKED : n_dirty;
    };
    if (p.jobs.size() < 64) {
      for (size_t i = 0; i < p.jobs.size(); i++) one(i);
    } else {
      parallel_for(p.jobs.size(), one);
    }
  }

  // tree_only: the step's one job went through the single-file entries, only its stored tree is checked
  lcpc_status run(ScrubStep &g, bool tree_only = false) {
    lcpc_status st;
    const size_t n_jobs = g.jobs.size();
    bool want_dig = false;
    for (size_t j = g.job_lo; j < g.job_hi; j++) want_dig |= all[j].digests != nullptr;
    want_dig = want_dig && !tree_only;
    // the block: [packed images | stored digests and expected roots | jobs | tiles | wgs | waves] go up,
    // [flags | statuses | dirty bytes | digests] come back
    size_t o = align_up(g.image_bytes, 32);
    for (size_t i = 0; i < n_jobs; i++) {
      const lcpc_pos_scrub_job &job = all[g.job_lo + i];
      PosScrubJob &t = g.jobs[i];
      const size_t enc = (size_t)1 << t.log_enc;
      t.tree_kind = job.tree_digests == 0 ? 0 : job.tree_digests == enc ? 1 : 2;
      t.tree_only = tree_only;
      if (tree_only && t.tree_kind != 2) t.tree_kind = 0;
      if (t.tree_kind) {
        t.tree = o;
        o += job.tree_digests * 32;
      }
      t.has_root = t.tree_kind == 2 && job.expected_root != nullptr;
      if (t.has_root) {
        t.root = o;
        o += 32;
      }
    }
    const TableOffsets T = table_offsets(g, o, n_jobs, sizeof(PosScrubJob));
    const size_t in_bytes = T.in_bytes;
    // (offsets within the device's output buffer; the block holds it from in_bytes on)
    const size_t d_status = align_up(2 * n_jobs, 16), d_dirty = d_status + g.n_cols;
    const size_t d_dig = align_up(d_dirty + g.n_rows, 32), out_bytes = d_dig + 32 * g.n_cols;
    const size_t back_bytes = want_dig ? out_bytes : d_dig;
    const size_t total = in_bytes + out_bytes;
    uint8_t *h = nullptr;
    if ((st = stage.begin(total, &h))) return st;
    if ((st = ensure(arena, dev, in_bytes, (size_t)4 << 20)) || (st = ensure(cvs, dev, g.cv_slots * 32 + 32, (size_t)1 << 20)) ||
        (st = ensure(cflags, dev, g.cv_slots + 16, (size_t)1 << 16)) || (st = ensure(out, dev, out_bytes, (size_t)1 << 20)))
      return st;
    {
      prof::HostScope hs("pos_group_scrub_gather");
      // every column as it stands: packed column c is column c
      if (!tree_only)
        pack_columns(
            g.jobs, g.col0, g.image_bytes, g.n_cols, h,
            [&](size_t i) -> const lcpc_pos_scrub_job & { return all[g.job_lo + i]; },
            [](size_t, size_t c) { return (ptrdiff_t)c; });
      for (size_t i = 0; i < n_jobs; i++) {
        const PosScrubJob &t = g.jobs[i];
        const lcpc_pos_scrub_job &job = all[g.job_lo + i];
        if (t.tree_kind) std::memcpy(h + t.tree, job.tree, job.tree_digests * 32);
        if (t.has_root) std::memcpy(h + t.root, job.expected_root, 32);
      }
      copy_tables(g, g.jobs, T, h);
    }
    const uint8_t *d = arena.as<uint8_t>();
    uint8_t *dout = out.as<uint8_t>();
    st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_scrub(d, reinterpret_cast<const PosScrubJob *>(d + T.o_jobs), n_jobs,
                              reinterpret_cast<const PosIngestTile *>(d + T.o_tiles),
                              reinterpret_cast<const PosIngestWg *>(d + T.o_wgs), g.wgs.size(), g.lds_bytes,
                              reinterpret_cast<const PosIngestWave *>(d + T.o_waves), g.waves.size(), g.max_chunks, tw,
                              cvs.as<uint32_t>(), cflags.as<uint8_t>(), dout, dout + d_status, dout + d_dirty,
                              dout + d_dig, s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + in_bytes, out.p, back_bytes, hipMemcpyDeviceToHost, s));
    return stage.commit(Pending{want_dig, g.job_lo, in_bytes, in_bytes + d_status, in_bytes + d_dirty, in_bytes + d_dig,
                                std::move(g.jobs)});
  }
};

// the single-file entries, whole: the scrub entry for statuses and digests, the locator for the dirty
// rows; the stored tree (if whole) still goes through the group's third launch, alone
lcpc_status scrub_single(lcpc_pos_scrub_job &job, ScrubRunner &runner, size_t j) {
  lcpc_status st;
  const size_t enc = job.enc;
  std::vector<uint8_t> zero_leaves;
  const uint8_t *leaves = job.tree;
  if (!leaves) {
    zero_leaves.assign(enc * 32, 0);
    leaves = zero_leaves.data();
  }
  size_t n_bad = 0;
  if ((st = lcpc_pos_scrub_porenc(job.porenc, enc, job.rows_written, job.row_capacity, leaves, job.digests, job.col_status,
                                  &n_bad)))
    return st;
  size_t n_noncanon = 0;
  for (size_t c = 0; c < enc; c++) n_noncanon += job.col_status[c] == 2;
  if (!job.tree) {  // nothing to compare with: 0 or 2 only
    for (size_t c = 0; c < enc; c++)
      if (job.col_status[c] == 1) job.col_status[c] = 0;
    n_bad = n_noncanon;
  }
  job.n_bad = n_bad;
  if (n_noncanon) {
    job.n_dirty_rows = LCPC_POS_SCRUB_ROWS_UNCHECKED;
  } else {
    std::vector<uint8_t> located(enc);
    size_t n_dirty = 0;
    if ((st = lcpc_pos_locate_porenc(job.porenc, job.pre, enc, job.rows_written, job.row_capacity, nullptr, 0, located.data(),
                                     nullptr, &n_dirty, nullptr)))
      return st;
    job.n_dirty_rows = n_dirty;
  }
  job.tree_consistent = job.root_ok = LCPC_POS_SCRUB_NOT_EVALUATED;
  if (job.tree_digests != 2 * enc - 1) return LCPC_OK;
  ScrubStep g;
  g.job_lo = j, g.job_hi = j + 1;
  g.jobs.push_back(PosScrubJob{0, 0, 0, 0, 0, 0, (uint32_t)job.pre, log2_pow2(enc), 0, 0, 1, 0, 0, 1});
  g.lds_bytes = POS_INGEST_WG_ELEMS * POS_WB;
  return runner.run(g, true);
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_scrub_files_grouped(lcpc_pos_scrub_job *jobs, size_t n_jobs) {
  if (!jobs) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  std::vector<size_t> rows(n_jobs), pre(n_jobs), enc(n_jobs);
  for (size_t j = 0; j < n_jobs; j++) {
    const lcpc_pos_scrub_job &job = jobs[j];
    const std::string at = "job " + std::to_string(j);
    if (!job.col_status) return fail(LCPC_ERR_INVALID_ARG, at + " has no col_status");
    if (!job.porenc && job.rows_written) return fail(LCPC_ERR_INVALID_ARG, at + " has no image");
    if (job.rows_written > job.row_capacity) return fail(LCPC_ERR_INVALID_ARG, at + ": rows_written > row_capacity");
    if (lcpc_status st = pos_dims_check(job.pre, job.enc)) return st;
    if (job.tree_digests != 0 && job.tree_digests != job.enc && job.tree_digests != 2 * job.enc - 1)
      return fail(LCPC_ERR_INVALID_ARG, at + ": tree_digests must be 0, enc or 2 enc - 1");
    if ((job.tree == nullptr) != (job.tree_digests == 0))
      return fail(LCPC_ERR_INVALID_ARG, at + ": tree and tree_digests disagree");
    rows[j] = job.rows_written, pre[j] = job.pre, enc[j] = job.enc;
  }
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const uint32_t *tw = nullptr;
  if ((st = pos_group_twiddles(dev, lease.s, &tw))) return st;
  ScrubPlanner planner(rows.data(), pre.data(), enc.data(), n_jobs, pos_group_bytes());
  ScrubRunner runner(dev, lease.s, tw, jobs);
  ScrubStep g;
  while (planner.next(g)) {
    if (g.single) {
      if ((st = scrub_single(jobs[g.job_lo], runner, g.job_lo))) return st;
      continue;
    }
    if ((st = runner.run(g))) return st;
  }
  return runner.stage.finish();
}

lcpc_status lcpc_pos_scrub_plan(const size_t *rows_written, const size_t *pre, const size_t *enc, size_t n_jobs,
                                lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches) {
  if (!rows_written || !pre || !enc || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  if (lcpc_status st = pos_dims_check(pre, enc, n_jobs)) return st;
  ScrubPlanner planner(rows_written, pre, enc, n_jobs, pos_group_bytes());
  emit_plan(planner, tiles, cap, n_tiles, n_launches);
  return LCPC_OK;
}

}  // extern "C"
