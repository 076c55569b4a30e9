// pos_group_host.cpp -- grouped audits of stored files: u^T M for a queue of jobs over
// different files with a number of launches that does not grow with the number of files.
//
//   GroupPlanner   cuts the jobs, in order, into steps: a staging group of consecutive jobs (one
//                  grouped launch, its tables built here) or one job for the single-file path (pre
//                  no power of two >= 8, or an image above the staging group's size);
//   GroupRunner    stages a group -- images, left vectors and tables in one page-locked block, one
//                  upload (h2d_blocks) -- and queues its launch as the block lands; two blocks
//                  alternate, so the host gathers group k + 1 while group k uploads and runs;
//   lcpc_pos_group_plan   the same steps as a work list, host only: what the CPU tests check.
//
// The split rule is left_mul_split's for the launch as a whole: with R runs (threads without a row
// split) over all jobs of the launch, every job may split its rows ceil(2^18 / R) ways, and keeps
// at least 8 rows per thread where it has them.
#include "pos_internal.hpp"

namespace {

constexpr size_t GROUP_WANT_THREADS = (size_t)1 << 18;  // left_mul_split's
// what bounds a launch's tables and result block besides the image bytes
constexpr size_t GROUP_MAX_JOBS = (size_t)1 << 16, GROUP_MAX_OUT_WORDS = (size_t)1 << 20,
                 GROUP_MAX_ROWS = (size_t)1 << 20, GROUP_MAX_TILES = (size_t)1 << 17;

size_t group_bytes() { return pos_group_bytes(); }

struct GroupStep {
  bool single = false;
  size_t job_lo = 0, job_hi = 0;
  // a grouped launch: its tables (jobs[i].base = the image's offset in a staged arena), the image
  // bytes of that arena, the left words and output words of its jobs (consecutive in the call's
  // lefts / out), the words of res (outputs, then partials)
  std::vector<PosGroupJob> jobs;
  std::vector<PosGroupTile> tiles;
  std::vector<PosGroupWave> waves;
  std::vector<PosGroupFold> folds;
  size_t image_bytes = 0, left_words = 0, out_words = 0, res_words = 0;
};

class GroupPlanner {
 public:
  GroupPlanner(const size_t *n_bytes, const size_t *pre, size_t n_jobs)
      : n_bytes_(n_bytes), pre_(pre), n_jobs_(n_jobs), gb_(group_bytes()) {}

  bool next(GroupStep &st) {
    st = GroupStep{};
    if (next_ >= n_jobs_) return false;
    const size_t lo = next_;
    st.job_lo = lo;
    if (!grouped(lo)) {
      st.single = true;
      st.job_hi = next_ = lo + 1;
      return true;
    }
    size_t hi = lo, bytes = 0, rows = 0, out_w = 0, tiles_ub = 0, runs = 0;
    for (; hi < n_jobs_ && grouped(hi); hi++) {
      const size_t nb = align_up(n_bytes_[hi], 8), nr = job_rows(n_bytes_[hi], pre_[hi]), n_runs = pre_[hi] / 8;
      const size_t tub = ceil_div(nr, 8) * ceil_div(n_runs, 64);
      if (hi > lo && (bytes + nb > gb_ || hi - lo >= GROUP_MAX_JOBS || out_w + pre_[hi] > GROUP_MAX_OUT_WORDS ||
                      rows + nr > GROUP_MAX_ROWS || tiles_ub + tub > GROUP_MAX_TILES))
        break;
      bytes += nb, rows += nr, out_w += pre_[hi], tiles_ub += tub, runs += n_runs;
    }
    st.job_hi = next_ = hi;
    build(st, runs, out_w);
    return true;
  }

 private:
  bool grouped(size_t j) const { return pos_left_mul_bytes_ok(pre_[j]) && n_bytes_[j] <= gb_; }

  struct Piece {
    uint32_t job, row_lo, n_rows, run_lo, log_w;
    uint64_t dst;
  };

  void build(GroupStep &st, size_t runs, size_t out_words) const {
    const size_t ways = ceil_div(GROUP_WANT_THREADS, runs);
    std::vector<Piece> pieces;
    size_t base = 0, left_off = 0, out_off = 0, part_off = out_words;
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      const size_t pre = pre_[j], nr = job_rows(n_bytes_[j], pre), n_runs = pre / 8;
      const size_t rows_per = std::min(nr, std::max<size_t>(ceil_div(nr, ways), 8)), n_split = ceil_div(nr, rows_per);
      const size_t w = std::min<size_t>(n_runs, 64);
      const uint32_t log_w = (uint32_t)log2_np2(w);
      st.jobs.push_back(PosGroupJob{base, n_bytes_[j], left_off, pre});
      for (size_t y = 0; y < n_split; y++) {
        const size_t r0 = y * rows_per, r1 = std::min(nr, r0 + rows_per);
        const uint64_t dst = n_split == 1 ? out_off : part_off + y * pre;
        for (size_t g = 0; g < n_runs; g += w)
          pieces.push_back(Piece{(uint32_t)(j - st.job_lo), (uint32_t)r0, (uint32_t)(r1 - r0), (uint32_t)g, log_w, dst});
      }
      if (n_split > 1) {
        for (size_t c = 0; c < pre; c += 64)
          st.folds.push_back(PosGroupFold{out_off, part_off, (uint32_t)n_split, (uint32_t)pre, (uint32_t)c,
                                          (uint32_t)std::min<size_t>(64, pre - c)});
        part_off += n_split * pre;
      }
      base += align_up(n_bytes_[j], 8);
      left_off += nr;
      out_off += pre;
    }
    st.image_bytes = base;
    st.left_words = left_off;
    st.out_words = out_words;
    st.res_words = part_off;
    // waves of one width and one row count, the deepest first (they run longest)
    std::stable_sort(pieces.begin(), pieces.end(), [](const Piece &a, const Piece &b) {
      return a.log_w != b.log_w ? a.log_w > b.log_w : a.n_rows > b.n_rows;
    });
    st.tiles.reserve(pieces.size());
    for (const Piece &p : pieces) {
      const uint32_t per_wave = 64u >> p.log_w;
      if (st.waves.empty() || st.waves.back().log_w != p.log_w || st.waves.back().n_rows != p.n_rows ||
          st.waves.back().n_tiles == per_wave)
        st.waves.push_back(PosGroupWave{(uint32_t)st.tiles.size(), 0, p.log_w, p.n_rows});
      st.waves.back().n_tiles++;
      st.tiles.push_back(PosGroupTile{p.job, p.row_lo, p.run_lo, 0, p.dst});
    }
  }

  const size_t *n_bytes_, *pre_;
  size_t n_jobs_, gb_, next_ = 0;
};

// the arguments both entries share; *n_left and *n_out: the totals the jobs ask for
lcpc_status group_args(const void *images, const size_t *n_bytes, const size_t *pre, size_t n_jobs,
                       const uint64_t *lefts, size_t n_left_total, uint64_t *out, size_t n_out_total) {
  if (!images || !n_bytes || !pre || !lefts || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  size_t n_left = 0, n_out = 0;
  for (size_t j = 0; j < n_jobs; j++) {
    if (!n_bytes[j] || !pre[j]) return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + " is empty");
    n_left += job_rows(n_bytes[j], pre[j]);
    n_out += pre[j];
  }
  if (n_left != n_left_total) return fail(LCPC_ERR_INVALID_ARG, "n_left_total != the jobs' row counts");
  if (n_out != n_out_total) return fail(LCPC_ERR_INVALID_ARG, "n_out_total != the jobs' pre");
  return LCPC_OK;
}

// One call's staging and launches.  run() returns with the group's upload, launch and read-back
// queued; its words reach the caller's out when its page-locked block is next reused, or in finish().
struct GroupRunner {
  Device *dev;
  hipStream_t s;
  const uint8_t *d_images;  // the caller's device arena, or nullptr: host images, staged
  DBuf arena, res;
  Pinned stg[2];
  Events ev;
  struct Pending {
    uint64_t *dst = nullptr;
    size_t off = 0, words = 0;
  } pend[2];
  int k = 0;

  GroupRunner(Device *d, hipStream_t stream, const uint8_t *images) : dev(d), s(stream), d_images(images) {}
  // (an early return leaves copies queued on the blocks the members are about to give back)
  ~GroupRunner() { (void)hipStreamSynchronize(s); }

  void drain(int slot) {
    if (pend[slot].dst) std::memcpy(pend[slot].dst, stg[slot].b() + pend[slot].off, pend[slot].words * 8);
    pend[slot].dst = nullptr;
  }

  // bytes / offsets: those of the step's first job on
  lcpc_status run(GroupStep &g, const uint8_t *const *bytes, const size_t *offsets, const uint64_t *lefts,
                  uint64_t *out) {
    const int slot = k & 1;
    HIP_TRY(ev.init());
    HIP_TRY(ev.reuse(k));
    drain(slot);
    const size_t n_jobs = g.jobs.size();
    // the block: [images | lefts | jobs | tiles | waves | folds] go up, [outputs] come back
    const size_t o_left = d_images ? 0 : align_up(g.image_bytes, 16);
    const size_t o_jobs = align_up(o_left + g.left_words * 8, 16);
    const size_t o_tiles = o_jobs + n_jobs * sizeof(PosGroupJob);
    const size_t o_waves = align_up(o_tiles + g.tiles.size() * sizeof(PosGroupTile), 16);
    const size_t o_folds = o_waves + g.waves.size() * sizeof(PosGroupWave);
    const size_t in_bytes = align_up(o_folds + g.folds.size() * sizeof(PosGroupFold), 256);
    const size_t total = in_bytes + g.out_words * 8;
    if (stg[slot].n < total && !stg[slot].get(dev, total)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    if (lcpc_status st = ensure(arena, dev, in_bytes, (size_t)4 << 20)) return st;
    if (lcpc_status st = ensure(res, dev, g.res_words * 8, (size_t)1 << 20)) return st;
    uint8_t *h = stg[slot].b();
    {
      prof::HostScope hs("pos_group_gather");
      if (d_images) {
        for (size_t i = 0; i < n_jobs; i++) g.jobs[i].base = offsets[i];
      } else if (g.image_bytes < ((size_t)4 << 20)) {
        for (size_t i = 0; i < n_jobs; i++) std::memcpy(h + g.jobs[i].base, bytes[i], g.jobs[i].n_bytes);
      } else {
        parallel_for(n_jobs, [&](size_t i) { std::memcpy(h + g.jobs[i].base, bytes[i], g.jobs[i].n_bytes); });
      }
      std::memcpy(h + o_left, lefts, g.left_words * 8);
      std::memcpy(h + o_jobs, g.jobs.data(), n_jobs * sizeof(PosGroupJob));
      std::memcpy(h + o_tiles, g.tiles.data(), g.tiles.size() * sizeof(PosGroupTile));
      std::memcpy(h + o_waves, g.waves.data(), g.waves.size() * sizeof(PosGroupWave));
      if (!g.folds.empty()) std::memcpy(h + o_folds, g.folds.data(), g.folds.size() * sizeof(PosGroupFold));
    }
    const uint8_t *d = arena.as<uint8_t>();
    lcpc_status st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_left_mul(d_images ? d_images : d, reinterpret_cast<const PosGroupJob *>(d + o_jobs),
                                 reinterpret_cast<const PosGroupTile *>(d + o_tiles),
                                 reinterpret_cast<const PosGroupWave *>(d + o_waves), g.waves.size(),
                                 reinterpret_cast<const PosGroupFold *>(d + o_folds), g.folds.size(),
                                 reinterpret_cast<const uint32_t *>(d + o_left), res.as<uint32_t>(), s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + in_bytes, res.p, g.out_words * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev.e[slot], s));
    pend[slot] = Pending{out, in_bytes, g.out_words};
    k++;
    return LCPC_OK;
  }

  lcpc_status finish() {
    HIP_TRY(hipStreamSynchronize(s));
    drain(0);
    drain(1);
    return LCPC_OK;
  }
};

// the steps of one call; images: host pointers (bytes) or a device arena with offsets
lcpc_status run_grouped(const uint8_t *const *bytes, const uint8_t *d_arena, const size_t *offsets,
                        const size_t *n_bytes, const size_t *pre, size_t n_jobs, const uint64_t *lefts,
                        uint64_t *out) {
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  GroupPlanner planner(n_bytes, pre, n_jobs);
  GroupRunner runner(dev, lease.s, d_arena);
  GroupStep g;
  size_t left_off = 0, out_off = 0;
  while (planner.next(g)) {
    const size_t j = g.job_lo;
    if (g.single) {
      // the single-file path, whole: its own staging, kernels and read-back into out
      const size_t nr = job_rows(n_bytes[j], pre[j]);
      st = d_arena ? lcpc_pos_left_multiply_bytes_device(d_arena + offsets[j], n_bytes[j], pre[j], lefts + left_off, nr,
                                                         out + out_off)
                   : lcpc_pos_left_multiply_bytes(bytes[j], n_bytes[j], pre[j], lefts + left_off, nr, out + out_off);
      if (st) return st;
      left_off += nr;
      out_off += pre[j];
      continue;
    }
    if ((st = runner.run(g, d_arena ? nullptr : bytes + j, d_arena ? offsets + j : nullptr, lefts + left_off,
                         out + out_off)))
      return st;
    left_off += g.left_words;
    out_off += g.out_words;
  }
  return runner.finish();
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_left_multiply_bytes_grouped(const uint8_t *const *bytes, const size_t *n_bytes, const size_t *pre,
                                                 size_t n_jobs, const uint64_t *lefts, size_t n_left_total,
                                                 uint64_t *out, size_t n_out_total) {
  lcpc_status st = group_args(bytes, n_bytes, pre, n_jobs, lefts, n_left_total, out, n_out_total);
  if (st) return st;
  for (size_t j = 0; j < n_jobs; j++)
    if (!bytes[j]) return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + " has no image");
  return run_grouped(bytes, nullptr, nullptr, n_bytes, pre, n_jobs, lefts, out);
}

lcpc_status lcpc_pos_left_multiply_bytes_grouped_device(const void *d_arena, const size_t *offsets,
                                                        const size_t *n_bytes, const size_t *pre, size_t n_jobs,
                                                        const uint64_t *lefts, size_t n_left_total, uint64_t *out,
                                                        size_t n_out_total) {
  if (!offsets) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  lcpc_status st = group_args(d_arena, n_bytes, pre, n_jobs, lefts, n_left_total, out, n_out_total);
  if (st) return st;
  if ((uintptr_t)d_arena & 7) return fail(LCPC_ERR_INVALID_ARG, "device arena must be 8-byte aligned");
  for (size_t j = 0; j < n_jobs; j++)
    if (offsets[j] & 7) return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + ": offset is no multiple of 8");
  return run_grouped(nullptr, static_cast<const uint8_t *>(d_arena), offsets, n_bytes, pre, n_jobs, lefts, out);
}

lcpc_status lcpc_pos_group_plan(const size_t *n_bytes, const size_t *pre, size_t n_jobs, lcpc_pos_group_tile *tiles,
                                size_t cap, size_t *n_tiles, size_t *n_launches) {
  if (!n_bytes || !pre || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  for (size_t j = 0; j < n_jobs; j++)
    if (!n_bytes[j] || !pre[j]) return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + " is empty");
  GroupPlanner planner(n_bytes, pre, n_jobs);
  GroupStep g;
  size_t n = 0, launches = 0;
  auto emit = [&](const lcpc_pos_group_tile &t) {
    if (n < cap) tiles[n] = t;
    n++;
  };
  while (planner.next(g)) {
    if (g.single) {
      const size_t j = g.job_lo;
      emit(lcpc_pos_group_tile{j, 0, job_rows(n_bytes[j], pre[j]), 0, ceil_div(pre[j], 8), LCPC_POS_GROUP_SINGLE, 0});
      continue;
    }
    for (size_t w = 0; w < g.waves.size(); w++) {
      const PosGroupWave &wv = g.waves[w];
      for (uint32_t i = 0; i < wv.n_tiles; i++) {
        const PosGroupTile &t = g.tiles[wv.tile0 + i];
        emit(lcpc_pos_group_tile{g.job_lo + t.job, t.row_lo, (uint64_t)t.row_lo + wv.n_rows, t.run_lo,
                                 (uint64_t)t.run_lo + ((uint64_t)1 << wv.log_w), (uint32_t)launches, (uint32_t)w});
      }
    }
    launches++;
  }
  if (n_tiles) *n_tiles = n;
  if (n_launches) *n_launches = launches;
  return LCPC_OK;
}

lcpc_status lcpc_field_to_montgomery(lcpc_field f, const uint64_t *in, uint64_t *out, size_t n) {
  if (!valid_field(f) || ((!in || !out) && n)) return fail(LCPC_ERR_INVALID_ARG, "field or null argument");
  if (f != LCPC_FT63) return fail(LCPC_ERR_UNSUPPORTED, "lcpc_field_to_montgomery: Ft63 only");
  const uint64_t p = field_info(POS_FID).p[0];
  for (size_t i = 0; i < n; i++) out[i] = (uint64_t)((((unsigned __int128)in[i]) << 64) % p);
  return LCPC_OK;
}

}  // extern "C"
