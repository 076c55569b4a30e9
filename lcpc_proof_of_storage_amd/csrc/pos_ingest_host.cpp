// pos_ingest_host.cpp -- grouped ingest of small files: a queue of (raw image, pre, enc)
// jobs encoded, hashed and folded to Merkle trees with a number of launches that does not grow with
// the number of files.
//
//   IngestPlanner   cuts the jobs, in order, into steps: a staging group of consecutive jobs (at most
//                   three launches, its tables built here) or one job for the single-file path (enc
//                   above LCPC_POS_INGEST_MAX_ENC, an image or encoded matrix above the group's size, or
//                   more leaf chunks than the fold's stack holds);
//   IngestRunner    stages a group -- images and tables in one page-locked block, one upload
//                   (h2d_blocks) -- queues its launches as the block lands and the read-back of trees,
//                   chaining values and encoded words into the same block; two blocks alternate, and
//                   the host scatters group k - 1 into the jobs' outputs while group k runs;
//   lcpc_pos_ingest_plan   the same steps as a work list, host only: what the CPU tests check.
#include "pos_internal.hpp"

#include <map>
#include <mutex>

namespace {

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }
inline size_t job_rows(size_t n_bytes, size_t pre) { return ceil_div(ceil_div(n_bytes, POS_DB), pre); }
inline size_t rows_pad(size_t n_rows) { return align_up(n_rows, 2); }
inline size_t leaf_chunks(size_t n_rows) { return ceil_div(8 + 2 * n_rows, 256); }
inline size_t enc_bytes(size_t n_rows, size_t enc) { return rows_pad(n_rows) * enc * POS_WB; }
// tile slots of a workgroup of rows of enc points
inline size_t wg_slots(size_t enc) { return std::max<size_t>(1, POS_INGEST_WG_ELEMS / (POS_INGEST_TILE_ROWS * enc)); }

static_assert(((size_t)1 << POS_INGEST_MAX_LOG_ENC) == LCPC_POS_INGEST_MAX_ENC);
static_assert(POS_INGEST_TILE_ROWS == LCPC_POS_INGEST_TILE_ROWS);

struct IngestStep {
  bool single = false;
  size_t job_lo = 0, job_hi = 0;
  // a staging group: its tables (jobs[i].base = the image's offset in the staged arena), the bytes of
  // that arena and of the encoded buffer, the chaining values and digests of its jobs, the LDS of its
  // encode launch and the largest chunk count
  std::vector<PosIngestJob> jobs;
  std::vector<PosIngestTile> tiles;
  std::vector<PosIngestWg> wgs;
  std::vector<PosIngestWave> waves;
  size_t image_bytes = 0, enc_bytes = 0, cv_slots = 0, tree_digests = 0, lds_bytes = 0, max_chunks = 1;
};

class IngestPlanner {
 public:
  IngestPlanner(const size_t *n_bytes, const size_t *pre, const size_t *enc, size_t n_jobs)
      : n_bytes_(n_bytes), pre_(pre), enc_(enc), n_jobs_(n_jobs), gb_(pos_group_bytes()) {}

  bool next(IngestStep &st) {
    st = IngestStep{};
    if (next_ >= n_jobs_) return false;
    const size_t lo = next_;
    st.job_lo = lo;
    if (!grouped(lo)) {
      st.single = true;
      st.job_hi = next_ = lo + 1;
      return true;
    }
    size_t hi = lo, bytes = 0, eb = 0, rows = 0, tiles = 0, tree = 0;
    for (; hi < n_jobs_ && grouped(hi); hi++) {
      const size_t nb = align_up(n_bytes_[hi], 8), nr = job_rows(n_bytes_[hi], pre_[hi]);
      const size_t ne = enc_bytes(nr, enc_[hi]), nt = ceil_div(nr, POS_INGEST_TILE_ROWS), tb = (2 * enc_[hi] - 1) * 32;
      if (hi > lo && (bytes + nb > gb_ || eb + ne > 4 * gb_ || hi - lo >= LCPC_POS_INGEST_MAX_JOBS ||
                      rows + nr > LCPC_POS_INGEST_MAX_ROWS || tiles + nt > LCPC_POS_INGEST_MAX_TILES ||
                      tree + tb > LCPC_POS_INGEST_MAX_TREE_BYTES))
        break;
      bytes += nb, eb += ne, rows += nr, tiles += nt, tree += tb;
    }
    st.job_hi = next_ = hi;
    build(st);
    return true;
  }

 private:
  bool grouped(size_t j) const {
    const size_t nr = job_rows(n_bytes_[j], pre_[j]);
    return enc_[j] <= LCPC_POS_INGEST_MAX_ENC && align_up(n_bytes_[j], 8) <= gb_ && enc_bytes(nr, enc_[j]) <= 4 * gb_ &&
           leaf_chunks(nr) <= POS_INGEST_MAX_CHUNKS && nr <= LCPC_POS_INGEST_MAX_ROWS &&
           ceil_div(nr, POS_INGEST_TILE_ROWS) <= LCPC_POS_INGEST_MAX_TILES;
  }

  void build(IngestStep &st) const {
    // tiles by row length, the longest rows first (their workgroups run longest), jobs in order
    std::vector<PosIngestTile> by_len[POS_INGEST_MAX_LOG_ENC + 1];
    size_t base = 0, eoff = 0, cv0 = 0, tree0 = 0, max_enc = 2;
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      const size_t pre = pre_[j], enc = enc_[j], nr = job_rows(n_bytes_[j], pre), nc = leaf_chunks(nr);
      const uint32_t le = (uint32_t)log2_np2(enc), ji = (uint32_t)(j - st.job_lo);
      st.jobs.push_back(PosIngestJob{base, n_bytes_[j], eoff, cv0, tree0, (uint32_t)pre, le, (uint32_t)nr,
                                     (uint32_t)rows_pad(nr), (uint32_t)nc, 0});
      for (size_t r = 0; r < nr; r += POS_INGEST_TILE_ROWS)
        by_len[le].push_back(PosIngestTile{ji, (uint32_t)r, (uint32_t)std::min(POS_INGEST_TILE_ROWS, nr - r), 0});
      for (size_t c = 0; c < nc; c++)
        for (size_t k = 0; k < enc; k += 64) st.waves.push_back(PosIngestWave{ji, (uint32_t)k, (uint32_t)c, 0});
      if (nr) max_enc = std::max(max_enc, enc);
      st.max_chunks = std::max(st.max_chunks, nc);
      base += align_up(n_bytes_[j], 8);
      eoff += enc_bytes(nr, enc);
      cv0 += nc * enc;
      tree0 += 2 * enc - 1;
    }
    st.image_bytes = base;
    st.enc_bytes = eoff;
    st.cv_slots = cv0;
    st.tree_digests = tree0;
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

  const size_t *n_bytes_, *pre_, *enc_;
  size_t n_jobs_, gb_, next_ = 0;
};

// the twiddles of the grouped lengths, built once per device and kept
lcpc_status ingest_twiddles(Device *dev, hipStream_t s, const uint32_t **out) {
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
// queued and the group before it scattered; the last group is scattered in finish().
struct IngestRunner {
  Device *dev;
  hipStream_t s;
  const uint32_t *tw;
  lcpc_pos_ingest_job *all;
  DBuf arena, encb, cvs, trees;
  Pinned stg[2];
  Events ev;
  struct Pending {
    bool live = false;
    size_t job_lo = 0, o_tree = 0, o_cv = 0, o_enc = 0;
    bool has_cv = false, has_enc = false;
    std::vector<PosIngestJob> jobs;
  } pend[2];
  int k = 0;

  IngestRunner(Device *d, hipStream_t stream, const uint32_t *twiddles, lcpc_pos_ingest_job *jobs)
      : dev(d), s(stream), tw(twiddles), all(jobs) {}
  // (an early return leaves copies queued on the blocks the members are about to give back)
  ~IngestRunner() { (void)hipStreamSynchronize(s); }

  lcpc_status drain(int slot) {
    Pending &p = pend[slot];
    if (!p.live) return LCPC_OK;
    p.live = false;
    HIP_TRY(hipEventSynchronize(ev.e[slot]));
    prof::HostScope hs("pos_group_ingest_scatter");
    const uint8_t *h = stg[slot].b();
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
    return LCPC_OK;
  }

  lcpc_status run(IngestStep &g) {
    const int slot = k & 1;
    lcpc_status st;
    HIP_TRY(ev.init());
    if ((st = drain(slot))) return st;  // (already drained by the run before this one, but for an error there)
    const size_t n_jobs = g.jobs.size();
    bool want_cv = false, want_enc = false;
    for (size_t j = g.job_lo; j < g.job_hi; j++) want_cv |= all[j].cvs != nullptr, want_enc |= all[j].porenc != nullptr;
    want_enc = want_enc && g.enc_bytes;  // a group without a porenc copies no encoded word back
    // the block: [images | jobs | tiles | wgs | waves] go up, [trees | chaining values | encoded words] come back
    const size_t o_jobs = align_up(g.image_bytes, 16);
    const size_t o_tiles = o_jobs + n_jobs * sizeof(PosIngestJob);
    const size_t o_wgs = o_tiles + g.tiles.size() * sizeof(PosIngestTile);
    const size_t o_waves = o_wgs + g.wgs.size() * sizeof(PosIngestWg);
    const size_t in_bytes = align_up(o_waves + g.waves.size() * sizeof(PosIngestWave), 256);
    const size_t tree_bytes = g.tree_digests * 32, cv_bytes = g.cv_slots * 32;
    const size_t o_tree = in_bytes, o_cv = o_tree + tree_bytes, o_enc = align_up(o_cv + (want_cv ? cv_bytes : 0), 256);
    const size_t total = o_enc + (want_enc ? g.enc_bytes : 0);
    if (stg[slot].n < total && !stg[slot].get(dev, total)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    if (arena.n < in_bytes || !arena.p) HIP_TRY(arena.alloc(dev, align_up(in_bytes, (size_t)4 << 20)));
    if (encb.n < g.enc_bytes + 16 || !encb.p) HIP_TRY(encb.alloc(dev, align_up(g.enc_bytes + 16, (size_t)4 << 20)));
    if (cvs.n < cv_bytes || !cvs.p) HIP_TRY(cvs.alloc(dev, align_up(cv_bytes, (size_t)1 << 20)));
    if (trees.n < tree_bytes || !trees.p) HIP_TRY(trees.alloc(dev, align_up(tree_bytes, (size_t)1 << 20)));
    uint8_t *h = stg[slot].b();
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
      std::memcpy(h + o_jobs, g.jobs.data(), n_jobs * sizeof(PosIngestJob));
      if (!g.tiles.empty()) std::memcpy(h + o_tiles, g.tiles.data(), g.tiles.size() * sizeof(PosIngestTile));
      if (!g.wgs.empty()) std::memcpy(h + o_wgs, g.wgs.data(), g.wgs.size() * sizeof(PosIngestWg));
      std::memcpy(h + o_waves, g.waves.data(), g.waves.size() * sizeof(PosIngestWave));
    }
    const uint8_t *d = arena.as<uint8_t>();
    st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_ingest(d, reinterpret_cast<const PosIngestJob *>(d + o_jobs), n_jobs,
                               reinterpret_cast<const PosIngestTile *>(d + o_tiles),
                               reinterpret_cast<const PosIngestWg *>(d + o_wgs), g.wgs.size(), g.lds_bytes,
                               reinterpret_cast<const PosIngestWave *>(d + o_waves), g.waves.size(), g.max_chunks, tw,
                               encb.as<uint8_t>(), cvs.as<uint32_t>(), trees.as<uint8_t>(), s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + o_tree, trees.p, tree_bytes, hipMemcpyDeviceToHost, s));
    if (want_cv) HIP_TRY(hipMemcpyAsync(h + o_cv, cvs.p, cv_bytes, hipMemcpyDeviceToHost, s));
    if (want_enc) HIP_TRY(hipMemcpyAsync(h + o_enc, encb.p, g.enc_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev.e[slot], s));
    Pending &p = pend[slot];
    p.live = true;
    p.job_lo = g.job_lo;
    p.o_tree = o_tree, p.o_cv = o_cv, p.o_enc = o_enc;
    p.has_cv = want_cv, p.has_enc = want_enc;
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

lcpc_status ingest_dims(const size_t *pre, const size_t *enc, size_t n_jobs) {
  for (size_t j = 0; j < n_jobs; j++)
    if (lcpc_status st = pos_dims_check(pre[j], enc[j])) return st;
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
  if ((st = ingest_twiddles(dev, lease.s, &tw))) return st;
  IngestPlanner planner(n_bytes.data(), pre.data(), enc.data(), n_jobs);
  IngestRunner runner(dev, lease.s, tw, jobs);
  IngestStep g;
  while (planner.next(g)) {
    if (g.single) {
      if ((st = ingest_single(jobs[g.job_lo]))) return st;
      continue;
    }
    if ((st = runner.run(g))) return st;
  }
  return runner.finish();
}

lcpc_status lcpc_pos_ingest_plan(const size_t *n_bytes, const size_t *pre, const size_t *enc, size_t n_jobs,
                                 lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches) {
  if (!n_bytes || !pre || !enc || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  if (lcpc_status st = ingest_dims(pre, enc, n_jobs)) return st;
  IngestPlanner planner(n_bytes, pre, enc, n_jobs);
  IngestStep g;
  size_t n = 0, launches = 0;
  auto emit = [&](const lcpc_pos_ingest_tile &t) {
    if (n < cap) tiles[n] = t;
    n++;
  };
  while (planner.next(g)) {
    if (g.single) {
      const size_t j = g.job_lo, nr = job_rows(n_bytes[j], pre[j]);
      if (nr) emit(lcpc_pos_ingest_tile{j, 0, nr, LCPC_POS_GROUP_SINGLE, 0});
      continue;
    }
    for (size_t w = 0; w < g.wgs.size(); w++)
      for (uint32_t i = 0; i < g.wgs[w].n_tiles; i++) {
        const PosIngestTile &t = g.tiles[g.wgs[w].tile0 + i];
        emit(lcpc_pos_ingest_tile{g.job_lo + t.job, t.row_lo, (uint64_t)t.row_lo + t.n_rows, (uint32_t)launches,
                                  (uint32_t)w});
      }
    launches++;
  }
  if (n_tiles) *n_tiles = n;
  if (n_launches) *n_launches = launches;
  return LCPC_OK;
}

}  // extern "C"
