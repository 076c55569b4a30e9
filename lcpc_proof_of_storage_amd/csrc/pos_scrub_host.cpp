// pos_scrub_host.cpp -- grouped scrub of stored files: a queue of (stored image, stored
// tree, expected root) jobs answered -- column statuses and digests, dirty rows of the row code, the
// stored tree's consistency and its root -- with a number of launches that does not grow with the
// number of files.
//
//   ScrubPlanner   cuts the jobs, in order, into steps: a staging group of consecutive jobs (at most
//                  three launches, its tables built here) or one job for the single-file entries (enc
//                  above LCPC_POS_SCRUB_MAX_ENC, a packed image above the group's size, or more leaf
//                  chunks than the fold's stack holds);
//   ScrubRunner    stages a group -- the written rows of every column packed, the stored digests, the
//                  expected roots and the tables in one page-locked block, one upload (h2d_blocks) --
//                  queues its launches as the block lands and one read-back of flags, statuses, dirty
//                  bytes and digests into the same block; two blocks alternate, and the host hands
//                  group k - 1 to the jobs while group k runs;
//   lcpc_pos_scrub_plan   the same steps as a work list, host only: what the CPU tests check.
#include "pos_internal.hpp"

#include <map>
#include <mutex>

namespace {

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }
inline size_t rows_pad(size_t n_rows) { return align_up(n_rows, 2); }
inline size_t leaf_chunks(size_t n_rows) { return ceil_div(8 + 2 * n_rows, 256); }
// the written rows of every column, each column 16-byte aligned
inline size_t packed_bytes(size_t n_rows, size_t enc) { return rows_pad(n_rows) * enc * POS_WB; }
// tile slots of a workgroup of rows of enc points
inline size_t wg_slots(size_t enc) { return std::max<size_t>(1, POS_INGEST_WG_ELEMS / (POS_INGEST_TILE_ROWS * enc)); }

static_assert(LCPC_POS_SCRUB_MAX_ENC == LCPC_POS_INGEST_MAX_ENC);
static_assert(LCPC_POS_SCRUB_TILE_ROWS == POS_INGEST_TILE_ROWS);
static_assert(LCPC_POS_SCRUB_NOT_EVALUATED == POS_SCRUB_NOT_EVALUATED);

struct ScrubStep {
  bool single = false;
  size_t job_lo = 0, job_hi = 0;
  // a staging group: its tables (jobs[i].img = the packed image's offset in the staged arena; tree and
  // root are set when the block is laid out), the bytes of the packed images, the chaining values,
  // columns and rows of its jobs, the LDS of its row launch and the largest chunk count
  std::vector<PosScrubJob> jobs;
  std::vector<PosIngestTile> tiles;
  std::vector<PosIngestWg> wgs;
  std::vector<PosIngestWave> waves;
  size_t image_bytes = 0, cv_slots = 0, n_cols = 0, n_rows = 0, lds_bytes = 0, max_chunks = 1;
};

class ScrubPlanner {
 public:
  ScrubPlanner(const size_t *rows, const size_t *pre, const size_t *enc, size_t n_jobs)
      : rows_(rows), pre_(pre), enc_(enc), n_jobs_(n_jobs), gb_(pos_group_bytes()) {}

  bool next(ScrubStep &st) {
    st = ScrubStep{};
    if (next_ >= n_jobs_) return false;
    const size_t lo = next_;
    st.job_lo = lo;
    if (!grouped(lo)) {
      st.single = true;
      st.job_hi = next_ = lo + 1;
      return true;
    }
    size_t hi = lo, bytes = 0, rows = 0, tiles = 0, tree = 0;
    for (; hi < n_jobs_ && grouped(hi); hi++) {
      const size_t nr = rows_[hi], nb = packed_bytes(nr, enc_[hi]);
      const size_t nt = ceil_div(nr, POS_INGEST_TILE_ROWS), tb = (2 * enc_[hi] - 1) * 32;
      if (hi > lo && (bytes + nb > gb_ || hi - lo >= LCPC_POS_INGEST_MAX_JOBS || rows + nr > LCPC_POS_INGEST_MAX_ROWS ||
                      tiles + nt > LCPC_POS_INGEST_MAX_TILES || tree + tb > LCPC_POS_INGEST_MAX_TREE_BYTES))
        break;
      bytes += nb, rows += nr, tiles += nt, tree += tb;
    }
    st.job_hi = next_ = hi;
    build(st);
    return true;
  }

 private:
  bool grouped(size_t j) const {
    const size_t nr = rows_[j];
    return enc_[j] <= LCPC_POS_SCRUB_MAX_ENC && nr <= LCPC_POS_INGEST_MAX_ROWS && packed_bytes(nr, enc_[j]) <= gb_ &&
           leaf_chunks(nr) <= POS_INGEST_MAX_CHUNKS && ceil_div(nr, POS_INGEST_TILE_ROWS) <= LCPC_POS_INGEST_MAX_TILES;
  }

  void build(ScrubStep &st) const {
    // tiles by row length, the longest rows first (their workgroups run longest), jobs in order
    std::vector<PosIngestTile> by_len[POS_INGEST_MAX_LOG_ENC + 1];
    size_t img = 0, cv0 = 0, col0 = 0, row0 = 0, max_enc = 2;
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      const size_t pre = pre_[j], enc = enc_[j], nr = rows_[j], nc = leaf_chunks(nr);
      const uint32_t le = (uint32_t)log2_np2(enc), ji = (uint32_t)(j - st.job_lo);
      st.jobs.push_back(PosScrubJob{img, 0, 0, cv0, col0, row0, (uint32_t)pre, le, (uint32_t)nr, (uint32_t)rows_pad(nr),
                                    (uint32_t)nc, 0, 0, 0});
      for (size_t r = 0; r < nr; r += POS_INGEST_TILE_ROWS)
        by_len[le].push_back(PosIngestTile{ji, (uint32_t)r, (uint32_t)std::min(POS_INGEST_TILE_ROWS, nr - r), 0});
      for (size_t c = 0; c < nc; c++)
        for (size_t k = 0; k < enc; k += 64) st.waves.push_back(PosIngestWave{ji, (uint32_t)k, (uint32_t)c, 0});
      if (nr) max_enc = std::max(max_enc, enc);
      st.max_chunks = std::max(st.max_chunks, nc);
      img += packed_bytes(nr, enc);
      cv0 += nc * enc;
      col0 += enc;
      row0 += nr;
    }
    st.image_bytes = img;
    st.cv_slots = cv0;
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

  const size_t *rows_, *pre_, *enc_;
  size_t n_jobs_, gb_, next_ = 0;
};

// the twiddles of the grouped lengths (the encode's table), built once per device and kept
lcpc_status scrub_twiddles(Device *dev, hipStream_t s, const uint32_t **out) {
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
struct ScrubRunner {
  Device *dev;
  hipStream_t s;
  const uint32_t *tw;
  lcpc_pos_scrub_job *all;
  DBuf arena, cvs, cflags, out;
  Pinned stg[2];
  Events ev;
  struct Pending {
    bool live = false, has_dig = false;
    size_t job_lo = 0, o_flags = 0, o_status = 0, o_dirty = 0, o_dig = 0;
    std::vector<PosScrubJob> jobs;
  } pend[2];
  int k = 0;

  ScrubRunner(Device *d, hipStream_t stream, const uint32_t *twiddles, lcpc_pos_scrub_job *jobs)
      : dev(d), s(stream), tw(twiddles), all(jobs) {}
  // (an early return leaves copies queued on the blocks the members are about to give back)
  ~ScrubRunner() { (void)hipStreamSynchronize(s); }

  lcpc_status drain(int slot) {
    Pending &p = pend[slot];
    if (!p.live) return LCPC_OK;
    p.live = false;
    HIP_TRY(hipEventSynchronize(ev.e[slot]));
    prof::HostScope hs("pos_group_scrub_scatter");
    const uint8_t *h = stg[slot].b();
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
    return LCPC_OK;
  }

  // tree_only: the step's one job went through the single-file entries, only its stored tree is checked
  lcpc_status run(ScrubStep &g, bool tree_only = false) {
    const int slot = k & 1;
    lcpc_status st;
    HIP_TRY(ev.init());
    if ((st = drain(slot))) return st;  // (already drained by the run before this one, but for an error there)
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
    const size_t o_jobs = align_up(o, 16);
    const size_t o_tiles = o_jobs + n_jobs * sizeof(PosScrubJob);
    const size_t o_wgs = o_tiles + g.tiles.size() * sizeof(PosIngestTile);
    const size_t o_waves = o_wgs + g.wgs.size() * sizeof(PosIngestWg);
    const size_t in_bytes = align_up(o_waves + g.waves.size() * sizeof(PosIngestWave), 256);
    // (offsets within the device's output buffer; the block holds it from in_bytes on)
    const size_t d_status = align_up(2 * n_jobs, 16), d_dirty = d_status + g.n_cols;
    const size_t d_dig = align_up(d_dirty + g.n_rows, 32), out_bytes = d_dig + 32 * g.n_cols;
    const size_t back_bytes = want_dig ? out_bytes : d_dig;
    const size_t total = in_bytes + out_bytes;
    if (stg[slot].n < total && !stg[slot].get(dev, total)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    if (arena.n < in_bytes || !arena.p) HIP_TRY(arena.alloc(dev, align_up(in_bytes, (size_t)4 << 20)));
    if (cvs.n < g.cv_slots * 32 + 32 || !cvs.p) HIP_TRY(cvs.alloc(dev, align_up(g.cv_slots * 32 + 32, (size_t)1 << 20)));
    if (cflags.n < g.cv_slots + 16 || !cflags.p) HIP_TRY(cflags.alloc(dev, align_up(g.cv_slots + 16, (size_t)1 << 16)));
    if (out.n < out_bytes || !out.p) HIP_TRY(out.alloc(dev, align_up(out_bytes, (size_t)1 << 20)));
    uint8_t *h = stg[slot].b();
    {
      prof::HostScope hs("pos_group_scrub_gather");
      // per column only the written rows: the slack up to row_capacity never crosses the bus
      auto pack_col = [&](size_t i, size_t c) {
        const PosScrubJob &t = g.jobs[i];
        const lcpc_pos_scrub_job &job = all[g.job_lo + i];
        const size_t col = (size_t)t.rows_pad * POS_WB, n = (size_t)t.n_rows * POS_WB;
        uint8_t *dst = h + t.img + c * col;
        std::memcpy(dst, job.porenc + c * job.row_capacity * POS_WB, n);
        if (n != col) std::memset(dst + n, 0, col - n);
      };
      // little to copy: this thread; else the group's columns, whatever job they belong to, over the
      // host threads in one pass (column gc of the group is column gc - col0 of the last job with col0 <= gc)
      const bool images = !tree_only && g.image_bytes;
      if (images && g.image_bytes < ((size_t)4 << 20)) {
        for (size_t i = 0; i < n_jobs; i++)
          for (size_t c = 0; g.jobs[i].n_rows && c < ((size_t)1 << g.jobs[i].log_enc); c++) pack_col(i, c);
      } else if (images) {
        parallel_for(g.n_cols, [&](size_t gc) {
          const auto it = std::upper_bound(g.jobs.begin(), g.jobs.end(), gc,
                                           [](size_t v, const PosScrubJob &t) { return v < t.col0; });
          const size_t i = (size_t)(it - g.jobs.begin()) - 1;
          if (g.jobs[i].n_rows) pack_col(i, gc - g.jobs[i].col0);
        });
      }
      for (size_t i = 0; i < n_jobs; i++) {
        const PosScrubJob &t = g.jobs[i];
        const lcpc_pos_scrub_job &job = all[g.job_lo + i];
        if (t.tree_kind) std::memcpy(h + t.tree, job.tree, job.tree_digests * 32);
        if (t.has_root) std::memcpy(h + t.root, job.expected_root, 32);
      }
      std::memcpy(h + o_jobs, g.jobs.data(), n_jobs * sizeof(PosScrubJob));
      if (!g.tiles.empty()) std::memcpy(h + o_tiles, g.tiles.data(), g.tiles.size() * sizeof(PosIngestTile));
      if (!g.wgs.empty()) std::memcpy(h + o_wgs, g.wgs.data(), g.wgs.size() * sizeof(PosIngestWg));
      if (!g.waves.empty()) std::memcpy(h + o_waves, g.waves.data(), g.waves.size() * sizeof(PosIngestWave));
    }
    const uint8_t *d = arena.as<uint8_t>();
    uint8_t *dout = out.as<uint8_t>();
    st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_scrub(d, reinterpret_cast<const PosScrubJob *>(d + o_jobs), n_jobs,
                              reinterpret_cast<const PosIngestTile *>(d + o_tiles),
                              reinterpret_cast<const PosIngestWg *>(d + o_wgs), g.wgs.size(), g.lds_bytes,
                              reinterpret_cast<const PosIngestWave *>(d + o_waves), g.waves.size(), g.max_chunks, tw,
                              cvs.as<uint32_t>(), cflags.as<uint8_t>(), dout, dout + d_status, dout + d_dirty,
                              dout + d_dig, s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + in_bytes, out.p, back_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev.e[slot], s));
    Pending &p = pend[slot];
    p.live = true;
    p.has_dig = want_dig;
    p.job_lo = g.job_lo;
    p.o_flags = in_bytes, p.o_status = in_bytes + d_status, p.o_dirty = in_bytes + d_dirty, p.o_dig = in_bytes + d_dig;
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
  g.jobs.push_back(PosScrubJob{0, 0, 0, 0, 0, 0, (uint32_t)job.pre, (uint32_t)log2_np2(enc), 0, 0, 1, 0, 0, 1});
  g.lds_bytes = POS_INGEST_WG_ELEMS * POS_WB;
  return runner.run(g, true);
}

lcpc_status scrub_dims(const size_t *pre, const size_t *enc, size_t n_jobs) {
  for (size_t j = 0; j < n_jobs; j++)
    if (lcpc_status st = pos_dims_check(pre[j], enc[j])) return st;
  return LCPC_OK;
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
  if ((st = scrub_twiddles(dev, lease.s, &tw))) return st;
  ScrubPlanner planner(rows.data(), pre.data(), enc.data(), n_jobs);
  ScrubRunner runner(dev, lease.s, tw, jobs);
  ScrubStep g;
  while (planner.next(g)) {
    if (g.single) {
      if ((st = scrub_single(jobs[g.job_lo], runner, g.job_lo))) return st;
      continue;
    }
    if ((st = runner.run(g))) return st;
  }
  return runner.finish();
}

lcpc_status lcpc_pos_scrub_plan(const size_t *rows_written, const size_t *pre, const size_t *enc, size_t n_jobs,
                                lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches) {
  if (!rows_written || !pre || !enc || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  if (lcpc_status st = scrub_dims(pre, enc, n_jobs)) return st;
  ScrubPlanner planner(rows_written, pre, enc, n_jobs);
  ScrubStep g;
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
