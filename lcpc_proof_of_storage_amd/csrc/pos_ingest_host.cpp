// pos_ingest_host.cpp -- grouped ingest of small files: a queue of (raw image, pre, enc)
// jobs encoded, hashed and folded to Merkle trees with a number of launches that does not grow with
// the number of files.
//
//   IngestPlanner   (pos_rowgroup_plan.hpp, host only) cuts the jobs, in order, into steps: a staging
//                   group of consecutive jobs (at most three launches) or one job for the single-file
//                   path;
//   IngestRunner    stages a group -- images and tables in one page-locked block, one upload
//                   (h2d_blocks) -- queues its launches as the block lands and the read-back of trees,
//                   chaining values and encoded words into the same block; two blocks alternate, and
//                   the host scatters group k - 1 into the jobs' outputs while group k runs
//                   (pos_rowgroup_stage.hpp);
//   lcpc_pos_ingest_plan   the same steps as a work list, host only: what the CPU tests check.
#include "pos_rowgroup_stage.hpp"

namespace {

// One call's staging and launches.  run() returns with the group's upload, launches and read-back
// queued and the group before it scattered; the last group is scattered in finish().
struct IngestRunner {
  Device *dev;
  hipStream_t s;
  const uint32_t *tw;
  lcpc_pos_ingest_job *all;
  DBuf arena, encb, cvs, trees;
  struct Pending {
    size_t job_lo = 0, o_tree = 0, o_cv = 0, o_enc = 0;
    bool has_cv = false, has_enc = false;
    std::vector<PosIngestJob> jobs;
  };
  TwoSlotStager<Pending> stage;

  IngestRunner(Device *d, hipStream_t stream, const uint32_t *twiddles, lcpc_pos_ingest_job *jobs)
      : dev(d), s(stream), tw(twiddles), all(jobs),
        stage(d, stream, [this](Pending &p, const uint8_t *h) { scatter(p, h); }) {}

  void scatter(const Pending &p, const uint8_t *h) {
    prof::HostScope hs("pos_group_ingest_scatter");
    auto one = [&](size_t i, bool par) {
      const PosIngestJob &g = p.jobs[i];
      lcpc_pos_ingest_job &job = all[p.job_lo + i];
      const size_t enc = (size_t)1 << g.log_enc;
      const uint8_t *tree = h + p.o_tree + 32 * g.tree0;
      job.rows_written = g.n_rows;
      if (job.tree) std::memcpy(job.tree, tree, (2 * enc - 1) * 32);
      if (job.root) std::memcpy(job.root, tree + (2 * enc - 2) * 32, 32);
      if (job.cvs && p.has_cv) std::memcpy(job.cvs, h + p.o_cv + 32 * g.cv0, (size_t)g.n_chunks * enc * 32);
      if (job.porenc && p.has_enc && g.n_rows) {
        const uint8_t *src = h + p.o_enc + g.enc_off;
        const size_t stride = (size_t)g.rows_pad * POS_WB;
        if (par) {
          scatter_slices(job.porenc, job.row_capacity, 0, enc, 0, g.n_rows, stride, src);
        } else {
          for (size_t c = 0; c < enc; c++)
            std::memcpy(job.porenc + c * job.row_capacity * POS_WB, src + c * stride, (size_t)g.n_rows * POS_WB);
        }
      }
    };
    // few jobs: each job's columns over the host threads; many: the jobs over them
    if (p.jobs.size() < 16) {
      for (size_t i = 0; i < p.jobs.size(); i++) one(i, true);
    } else {
      parallel_for(p.jobs.size(), [&](size_t i) { one(i, false); });
    }
  }

  lcpc_status run(IngestStep &g) {
    lcpc_status st;
    const size_t n_jobs = g.jobs.size();
    bool want_cv = false, want_enc = false;
    for (size_t j = g.job_lo; j < g.job_hi; j++) want_cv |= all[j].cvs != nullptr, want_enc |= all[j].porenc != nullptr;
    want_enc = want_enc && g.enc_bytes;  // a group without a porenc copies no encoded word back
    // the block: [images | jobs | tiles | wgs | waves] go up, [trees | chaining values | encoded words] come back
    const TableOffsets T = table_offsets(g, g.image_bytes, n_jobs, sizeof(PosIngestJob));
    const size_t in_bytes = T.in_bytes;
    const size_t tree_bytes = g.tree_digests * 32, cv_bytes = g.cv_slots * 32;
    const size_t o_tree = in_bytes, o_cv = o_tree + tree_bytes, o_enc = align_up(o_cv + (want_cv ? cv_bytes : 0), 256);
    const size_t total = o_enc + (want_enc ? g.enc_bytes : 0);
    uint8_t *h = nullptr;
    if ((st = stage.begin(total, &h))) return st;
    if ((st = ensure(arena, dev, in_bytes, (size_t)4 << 20)) || (st = ensure(encb, dev, g.enc_bytes + 16, (size_t)4 << 20)) ||
        (st = ensure(cvs, dev, cv_bytes, (size_t)1 << 20)) || (st = ensure(trees, dev, tree_bytes, (size_t)1 << 20)))
      return st;
    {
      prof::HostScope hs("pos_group_ingest_gather");
      auto copy = [&](size_t i) {
        if (g.jobs[i].n_bytes) std::memcpy(h + g.jobs[i].base, all[g.job_lo + i].data, g.jobs[i].n_bytes);
      };
      if (g.image_bytes < ((size_t)4 << 20)) {
        for (size_t i = 0; i < n_jobs; i++) copy(i);
      } else {
        parallel_for(n_jobs, copy);
      }
      copy_tables(g, g.jobs, T, h);
    }
    const uint8_t *d = arena.as<uint8_t>();
    st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_ingest(d, reinterpret_cast<const PosIngestJob *>(d + T.o_jobs), n_jobs,
                               reinterpret_cast<const PosIngestTile *>(d + T.o_tiles),
                               reinterpret_cast<const PosIngestWg *>(d + T.o_wgs), g.wgs.size(), g.lds_bytes,
                               reinterpret_cast<const PosIngestWave *>(d + T.o_waves), g.waves.size(), g.max_chunks, tw,
                               encb.as<uint8_t>(), cvs.as<uint32_t>(), trees.as<uint8_t>(), s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + o_tree, trees.p, tree_bytes, hipMemcpyDeviceToHost, s));
    if (want_cv) HIP_TRY(hipMemcpyAsync(h + o_cv, cvs.p, cv_bytes, hipMemcpyDeviceToHost, s));
    if (want_enc) HIP_TRY(hipMemcpyAsync(h + o_enc, encb.p, g.enc_bytes, hipMemcpyDeviceToHost, s));
    return stage.commit(Pending{g.job_lo, o_tree, o_cv, o_enc, want_cv, want_enc, std::move(g.jobs)});
  }
};

// the single-file path, whole: lcpc_pos_encode_file's writer, its chaining values kept where asked
lcpc_status ingest_single(lcpc_pos_ingest_job &job) {
  lcpc_status st;
  lcpc_pos_writer *w = nullptr;
  if ((st = lcpc_pos_writer_new(job.pre, job.enc, job.porenc, job.row_capacity, 0, &w))) return st;
  std::unique_ptr<lcpc_pos_writer, void (*)(lcpc_pos_writer *)> guard(w, lcpc_pos_writer_free);
  if ((st = lcpc_pos_writer_push_bytes(w, job.data, job.n_bytes))) return st;
  std::vector<uint8_t> tmp;
  uint8_t *tree = job.tree;
  if (!tree) {
    tmp.resize((2 * job.enc - 1) * 32);
    tree = tmp.data();
  }
  size_t rows = 0;
  if ((st = lcpc_pos_writer_finalize(w, nullptr, tree, &rows, nullptr))) return st;
  job.rows_written = rows;
  if (job.root) std::memcpy(job.root, tree + (2 * job.enc - 2) * 32, 32);
  if (job.cvs && (st = lcpc_pos_writer_copy_cvs(w, job.cvs))) return st;
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_encode_files_grouped(lcpc_pos_ingest_job *jobs, size_t n_jobs) {
  if (!jobs) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  std::vector<size_t> n_bytes(n_jobs), pre(n_jobs), enc(n_jobs);
  for (size_t j = 0; j < n_jobs; j++) {
    const lcpc_pos_ingest_job &job = jobs[j];
    if (lcpc_status st = pos_dims_check(job.pre, job.enc)) return st;
    if (!job.data && job.n_bytes) return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + " has no image");
    if (!job.porenc && job.row_capacity)
      return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + ": row_capacity without a porenc");
    if (job.porenc && job.row_capacity < job_rows(job.n_bytes, job.pre))
      return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + ": row_capacity < rows to write");
    n_bytes[j] = job.n_bytes, pre[j] = job.pre, enc[j] = job.enc;
  }
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const uint32_t *tw = nullptr;
  if ((st = pos_group_twiddles(dev, lease.s, &tw))) return st;
  IngestPlanner planner(n_bytes.data(), pre.data(), enc.data(), n_jobs, pos_group_bytes());
  IngestRunner runner(dev, lease.s, tw, jobs);
  IngestStep g;
  while (planner.next(g)) {
    if (g.single) {
      if ((st = ingest_single(jobs[g.job_lo]))) return st;
      continue;
    }
    if ((st = runner.run(g))) return st;
  }
  return runner.stage.finish();
}

lcpc_status lcpc_pos_ingest_plan(const size_t *n_bytes, const size_t *pre, const size_t *enc, size_t n_jobs,
                                 lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches) {
  if (!n_bytes || !pre || !enc || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  if (lcpc_status st = pos_dims_check(pre, enc, n_jobs)) return st;
  IngestPlanner planner(n_bytes, pre, enc, n_jobs, pos_group_bytes());
  emit_plan(planner, tiles, cap, n_tiles, n_launches);
  return LCPC_OK;
}

}  // extern "C"
