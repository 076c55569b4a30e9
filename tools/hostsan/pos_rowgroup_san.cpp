// pos_rowgroup_san.cpp -- the host-only half of the grouped ingest, scrub and repair of stored files
// (csrc/pos_rowgroup_plan.hpp, csrc/pos_repair_plan.hpp) under ASan + UBSan.
//
//   the plans    the fleets of tests/golden/gen_pos_group_plans.py rebuilt here (the same cross products
//                and placements, this program's own draws) cut by the ingest, scrub and repair planners
//                at the default group size, 65536 and 4096 bytes: every step checked against the limits,
//                every (job, row) in exactly one record, and every group's tables copied through the
//                ladder of offsets into a buffer of exactly in_bytes;
//   the blocks   random fleets with images: every scrub and repair group packed into a buffer of exactly
//                its size and compared with the images.  The rows past rows_written of every column, and
//                the listed columns of a repair job whole, are poisoned: a read of either ends the run;
//   the empties  a tree-only group (one job, no tile, workgroup or wave) and a group with no table at all.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <random>

#include "pos_repair_plan.hpp"

using namespace lcpc_host;
using namespace lcpc_host::repair;

static int bad = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      bad++;                            \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fputc('\n', stderr);         \
    }                                   \
  } while (0)

// ---------------------------------------------------------------- the plans
struct Sizes {
  std::vector<size_t> n_bytes, rows, pre, enc, n_bad;
  void add(std::mt19937_64 &rng, size_t e, size_t p, size_t r, size_t b) {
    enc.push_back(e), pre.push_back(p), rows.push_back(r), n_bad.push_back(b);
    n_bytes.push_back(r ? POS_DB * p * (r - 1) + 1 + rng() % (POS_DB * p) : 0);   // the last row full or ragged
  }
  size_t size() const { return enc.size(); }
};

static const size_t ENCS[] = {2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048};
static const size_t ROWS[] = {0, 1, 7, 8, 9, 124, 125, 1023, 1024, 1025};

static std::vector<size_t> pres_of(size_t e) {
  std::vector<size_t> p{1, e - 1};
  if (e >= 4) p.push_back(3);
  if (e >= 8) p.push_back(3 * e / 4 - 1);
  std::sort(p.begin(), p.end());
  p.erase(std::unique(p.begin(), p.end()), p.end());
  return p;
}

static std::vector<Sizes> plan_fleets(std::mt19937_64 &rng) {
  std::vector<Sizes> out;
  struct J { size_t e, p, r, b; };
  std::vector<J> cross;
  for (size_t e : ENCS)
    for (size_t p : pres_of(e))
      for (size_t r : ROWS) {
        const size_t kinds[] = {0, 1, e - p, e - p + 1};
        cross.push_back({e, p, r, kinds[rng() % 4]});
      }
  Sizes a, b, c, d, x, y;
  for (const J &j : cross) a.add(rng, j.e, j.p, j.r, j.b);
  std::shuffle(cross.begin(), cross.end(), rng);
  for (const J &j : cross) b.add(rng, j.e, j.p, j.r, j.b);
  static const size_t short_rows[] = {0, 1, 2, 7, 8, 9, 17, 124, 125};
  for (int i = 0; i < 3000; i++) {
    const size_t e = ENCS[rng() % 11];
    const std::vector<size_t> ps = pres_of(e);
    const size_t p = ps[rng() % ps.size()], kinds[] = {0, 1, e - p, e - p + 1};
    c.add(rng, e, p, short_rows[rng() % 9], kinds[rng() % 4]);
  }
  for (size_t i = 0; i < LCPC_POS_INGEST_MAX_JOBS + 100; i++) d.add(rng, 2, 1, 1, 0);
  // jobs that do no work (X) at the start, in the middle and at the end of a group, and between groups
  const J w{16, 8, 8, 1}, X{16, 8, 8, 9}, big{16, 8, 32, 8};
  for (const J &j : {X, w, w, w, w, w, X, w, w, X, w, w, w, w, X, X, X, big, X, big, w, w, w, X, X}) x.add(rng, j.e, j.p, j.r, j.b);
  for (size_t e : {2, 16, 1024, 2048})
    for (size_t p : {(size_t)1, e - 1})
      for (size_t r : {0, 9}) y.add(rng, e, p, r, e - p + 1);
  for (Sizes *s : {&a, &b, &c, &d, &x, &y}) out.push_back(std::move(*s));
  return out;
}

// the ladder and the copy: a buffer of exactly in_bytes, the four tables read back from their offsets
template <class Step>
static void check_tables(const Step &g, size_t end) {
  const TableOffsets T = table_offsets(g, end, g.jobs.size(), sizeof(g.jobs[0]));
  CHECK(T.o_jobs % 16 == 0 && T.o_jobs >= end && T.in_bytes % 256 == 0, "ladder");
  CHECK(T.o_tiles % 16 == 0 && T.o_wgs % 16 == 0 && T.o_waves % 16 == 0, "ladder alignment");
  CHECK(T.o_waves + g.waves.size() * sizeof(PosIngestWave) <= T.in_bytes, "ladder end");
  std::vector<uint8_t> h(T.in_bytes, 0xA5);
  copy_tables(g, g.jobs, T, h.data());
  auto same = [&](size_t at, const auto &v) { return v.empty() || !std::memcmp(h.data() + at, v.data(), v.size() * sizeof(v[0])); };
  CHECK(same(T.o_jobs, g.jobs) && same(T.o_tiles, g.tiles) && same(T.o_wgs, g.wgs) && same(T.o_waves, g.waves), "tables");
}

// wave_cols(t): the columns of job table entry t that get chunk waves
template <class Planner, class WaveCols>
static void check_plan(const char *what, const Planner &fresh, size_t n, size_t group_bytes, WaveCols wave_cols) {
  Planner planner = fresh;
  std::vector<std::vector<uint8_t>> seen(n);   // [job][row] -> records
  for (size_t j = 0; j < n; j++) seen[j].assign(planner.rows(j), 0);
  typename Planner::Step g;
  size_t next = 0, launches = 0;
  while (planner.next(g)) {
    CHECK(g.job_lo == next && g.job_hi > g.job_lo && g.job_hi <= n, "%s: steps are consecutive", what);
    next = g.job_hi;
    if (g.single) {
      const size_t j = g.job_lo;
      CHECK(g.job_hi == j + 1 && planner.works(j) && !fits_group(planner.cost(j), group_bytes), "%s: job %zu routed without cause", what, j);
      CHECK(g.jobs.empty() && g.tiles.empty() && g.wgs.empty() && g.waves.empty(), "%s: a routed job with tables", what);
      for (uint8_t &x : seen[j]) x++;
      continue;
    }
    size_t bytes = 0, bytes2 = 0, rows = 0, tiles = 0, tree = 0, working = 0;
    for (size_t j = g.job_lo; j < g.job_hi; j++) {
      if (!planner.works(j)) continue;
      const JobCost c = planner.cost(j);
      CHECK(fits_group(c, group_bytes), "%s: job %zu fits no group", what, j);
      working++, bytes += c.bytes, bytes2 += c.bytes2, rows += c.rows, tiles += ceil_div(c.rows, POS_INGEST_TILE_ROWS);
      tree += (2 * c.enc - 1) * 32;
    }
    CHECK(g.jobs.size() == working, "%s: %zu table entries for %zu jobs", what, g.jobs.size(), working);
    CHECK(working <= 1 || (bytes <= group_bytes && bytes2 <= 4 * group_bytes), "%s: a group of %zu + %zu bytes", what, bytes, bytes2);
    CHECK(working <= LCPC_POS_INGEST_MAX_JOBS && rows <= LCPC_POS_INGEST_MAX_ROWS && tiles <= LCPC_POS_INGEST_MAX_TILES &&
              (working <= 1 || tree <= LCPC_POS_INGEST_MAX_TREE_BYTES), "%s: a group past the tables' limits", what);
    CHECK(g.tiles.size() == tiles, "%s: %zu tiles, not %zu", what, g.tiles.size(), tiles);
    size_t in_wgs = 0, max_chunks = 1;
    for (size_t w = 0; w < g.wgs.size(); w++) {
      const PosIngestWg &wg = g.wgs[w];
      CHECK(wg.n_tiles >= 1 && wg.n_tiles <= wg_slots((size_t)1 << wg.log_enc) && wg.tile0 == in_wgs, "%s: workgroup", what);
      CHECK(w == 0 || g.wgs[w - 1].log_enc >= wg.log_enc, "%s: the longest rows first", what);
      CHECK(((size_t)wg.n_tiles << (3 + wg.log_enc)) * POS_WB <= g.lds_bytes && g.lds_bytes <= 65536, "%s: LDS", what);
      in_wgs += wg.n_tiles;
      if (wg.tile0 + wg.n_tiles > g.tiles.size()) continue;
      for (uint32_t i = 0; i < wg.n_tiles; i++) {
        const PosIngestTile &t = g.tiles[wg.tile0 + i];
        const bool ok = t.job < g.jobs.size() && g.jobs[t.job].log_enc == wg.log_enc && t.n_rows >= 1 && t.n_rows <= 8 &&
                        t.row_lo + t.n_rows <= g.jobs[t.job].n_rows;
        CHECK(ok, "%s: tile", what);
        if (!ok) continue;
        for (uint32_t r = 0; r < t.n_rows; r++) seen[g.job_of(t.job)][t.row_lo + r]++;
      }
    }
    CHECK(in_wgs == g.tiles.size(), "%s: tiles outside the workgroups", what);
    size_t want_waves = 0;
    for (const auto &t : g.jobs) {
      want_waves += (size_t)t.n_chunks * ceil_div(wave_cols(t), 64);
      max_chunks = std::max<size_t>(max_chunks, t.n_chunks);
      CHECK(t.n_chunks == leaf_chunks(t.n_rows) && t.rows_pad == rows_pad(t.n_rows), "%s: job entry", what);
    }
    CHECK(g.waves.size() == want_waves && g.max_chunks == max_chunks, "%s: waves", what);
    for (const PosIngestWave &w : g.waves)
      CHECK(w.job < g.jobs.size() && w.col_lo < wave_cols(g.jobs[w.job]) && w.chunk < g.jobs[w.job].n_chunks, "%s: wave", what);
    check_tables(g, bytes);
    if (!g.jobs.empty()) launches++;
  }
  CHECK(next == n, "%s: jobs covered", what);
  size_t want = 0;
  for (size_t j = 0; j < n; j++) {
    if (planner.works(j)) want += planner.rows(j);
    for (uint8_t x : seen[j]) CHECK(x == (planner.works(j) ? 1 : 0), "%s: a row of job %zu in %d records", what, j, x);
  }
  // the work list, through a short and an exact buffer
  size_t n_tiles = 0, n_launches = 0;
  lcpc_pos_ingest_tile two[2];
  Planner short_list = fresh, whole_list = fresh;
  emit_plan(short_list, two, 2, &n_tiles, &n_launches);
  CHECK(n_launches == launches, "%s: %zu launches, not %zu", what, n_launches, launches);
  std::vector<lcpc_pos_ingest_tile> all(n_tiles);
  size_t again = 0;
  emit_plan(whole_list, all.data(), all.size(), &again, nullptr);
  size_t listed = 0;
  for (const lcpc_pos_ingest_tile &t : all) listed += t.row_hi - t.row_lo;
  CHECK(again == n_tiles && listed == want, "%s: the work list holds %zu rows, not %zu", what, listed, want);
}

static void check_plans(std::mt19937_64 &rng) {
  const std::vector<Sizes> fleets = plan_fleets(rng);
  for (size_t gb : {(size_t)LCPC_POS_GROUP_STAGE_BYTES, (size_t)65536, (size_t)4096})
    for (const Sizes &f : fleets) {
      const size_t n = f.size();
      check_plan("ingest", IngestPlanner(f.n_bytes.data(), f.pre.data(), f.enc.data(), n, gb), n, gb,
                 [](const PosIngestJob &t) { return (size_t)1 << t.log_enc; });
      check_plan("scrub", ScrubPlanner(f.rows.data(), f.pre.data(), f.enc.data(), n, gb), n, gb,
                 [](const PosScrubJob &t) { return (size_t)1 << t.log_enc; });
      check_plan("repair", RepairPlanner(f.rows.data(), f.pre.data(), f.enc.data(), f.n_bad.data(), n, gb), n, gb,
                 [](const PosRepairJob &t) { return (size_t)t.n_bad; });
    }
}

// ---------------------------------------------------------------- the blocks
struct Fleet {
  std::vector<size_t> rows, pre, enc, n_bad, cap;
  std::vector<std::vector<uint64_t>> lists;
  std::vector<std::vector<uint8_t>> images, leaves;
  std::vector<lcpc_pos_repair_job> jobs;
  std::vector<lcpc_pos_scrub_job> scrub_jobs;
  uint8_t sink[32];

  // listed: the listed columns are poisoned whole (repair); else every column has its written rows
  Fleet(std::mt19937_64 &rng, size_t n, bool big, bool listed_poison) {
    static const size_t encs[] = {2, 4, 16, 32, 256, 1024, 2048}, rws[] = {0, 1, 7, 8, 9, 129};
    for (size_t j = 0; j < n; j++) {
      const size_t e = encs[rng() % (big ? 7 : 5)], p = 1 + rng() % (e - 1), r = rws[rng() % 6];
      const size_t room = e - p, pick[] = {0, 1, room, room + 1, rng() % (room + 1)};
      const size_t nb = std::min(e, pick[rng() % 5]);
      rows.push_back(r), pre.push_back(p), enc.push_back(e), n_bad.push_back(nb), cap.push_back(2 * r + 3);
      std::vector<uint64_t> cols(e);
      for (size_t c = 0; c < e; c++) cols[c] = c;
      std::shuffle(cols.begin(), cols.end(), rng);
      cols.resize(nb);
      lists.push_back(cols);
      std::vector<uint8_t> img(e * cap[j] * POS_WB);
      for (auto &b : img) b = (uint8_t)rng();
      images.push_back(std::move(img));
      leaves.emplace_back(rng() % 2 ? e * 32 : 0, (uint8_t)j);
    }
    for (size_t j = 0; j < n; j++) {
      std::vector<uint8_t> listed(enc[j], 0);
      if (listed_poison)
        for (uint64_t c : lists[j]) listed[c] = 1;
      for (size_t c = 0; c < enc[j]; c++) {
        uint8_t *col = images[j].data() + c * cap[j] * POS_WB;
        if (listed[c])
          ASAN_POISON_MEMORY_REGION(col, cap[j] * POS_WB);
        else
          ASAN_POISON_MEMORY_REGION(col + rows[j] * POS_WB, (cap[j] - rows[j]) * POS_WB);
      }
      lcpc_pos_repair_job job{};
      job.porenc = images[j].data(), job.pre = pre[j], job.enc = enc[j], job.rows_written = rows[j];
      job.row_capacity = cap[j], job.bad_cols = lists[j].data(), job.n_bad = n_bad[j];
      job.leaves = leaves[j].empty() ? nullptr : leaves[j].data();
      job.tree_out = job.leaves && rng() % 2 ? sink : nullptr;   // (never written here)
      job.cols_out = rng() % 2 ? sink : nullptr;
      jobs.push_back(job);
      lcpc_pos_scrub_job sj{};
      sj.porenc = images[j].data(), sj.pre = pre[j], sj.enc = enc[j], sj.rows_written = rows[j], sj.row_capacity = cap[j];
      scrub_jobs.push_back(sj);
    }
  }
  ~Fleet() {
    for (auto &img : images) ASAN_UNPOISON_MEMORY_REGION(img.data(), img.size());
  }
};

static void check_repair_block(const Fleet &f, RepairStep &g, const uint8_t *single_digests) {
  const Layout L = lay_out(g, f.jobs.data(), single_digests != nullptr);
  std::vector<uint8_t> h(L.T.in_bytes, 0xA5);   // exactly the bytes that go up
  pack(g, f.jobs.data(), L, single_digests, h.data());
  CHECK(L.total >= L.T.in_bytes + L.out_bytes && L.T.o_jobs % 16 == 0 && L.T.in_bytes % 256 == 0, "layout");
  CHECK(!std::memcmp(h.data() + L.T.o_jobs, g.jobs.data(), g.jobs.size() * sizeof(PosRepairJob)), "job table");
  size_t end = 0;
  for (size_t i = 0; i < g.jobs.size(); i++) {
    const PosRepairJob &t = g.jobs[i];
    const size_t j = g.job_of((uint32_t)i), enc = f.enc[j];
    CHECK(((size_t)1 << t.log_enc) == enc && t.n_bad == f.n_bad[j] && t.pre == f.pre[j], "job %zu: dims", j);
    CHECK(t.img % 16 == 0 && t.cmap % 4 == 0 && t.bad % 4 == 0 && t.leaves % 32 == 0 && t.dig_in % 32 == 0, "job %zu: alignment", j);
    end = std::max({end, (size_t)t.cmap + 4 * enc, (size_t)t.bad + 4 * t.n_bad});
    const int32_t *cmap = reinterpret_cast<const int32_t *>(h.data() + t.cmap);
    const uint32_t *list = reinterpret_cast<const uint32_t *>(h.data() + t.bad);
    std::vector<int> hit_k(t.n_bad, 0), hit_q(enc - t.n_bad, 0);
    for (size_t c = 0; c < enc; c++) {
      const int32_t m = cmap[c];
      if (m >= 0) {
        CHECK((size_t)m < t.n_bad && list[m] == c && f.lists[j][m] == c, "job %zu: column %zu maps to list entry %d", j, c, m);
        if ((size_t)m < t.n_bad) hit_k[m]++;
        continue;
      }
      const size_t q = (size_t)(-1 - m);
      CHECK(q < enc - t.n_bad, "job %zu: column %zu maps to packed column %zu", j, c, q);
      if (q >= enc - t.n_bad) continue;
      hit_q[q]++;
      if (single_digests || !t.n_rows) continue;
      const uint8_t *got = h.data() + t.img + q * t.rows_pad * POS_WB;
      CHECK(!std::memcmp(got, f.images[j].data() + c * f.cap[j] * POS_WB, t.n_rows * POS_WB), "job %zu column %zu: bytes", j, c);
      for (size_t b = t.n_rows * POS_WB; b < t.rows_pad * POS_WB; b++) CHECK(got[b] == 0, "job %zu column %zu: pad", j, c);
    }
    for (int x : hit_k) CHECK(x == 1, "job %zu: a list entry without its column", j);
    for (int x : hit_q) CHECK(x == 1, "job %zu: a packed column used %d times", j, x);
    if (t.has_tree) CHECK(!std::memcmp(h.data() + t.leaves, f.leaves[j].data(), enc * 32), "job %zu: leaves", j);
    if (single_digests && t.n_bad) CHECK(!std::memcmp(h.data() + t.dig_in, single_digests, t.n_bad * 32), "job %zu: digests", j);
  }
  CHECK(end <= L.T.o_jobs, "tables overlap");
}

static void check_repair_fleet(std::mt19937_64 &rng, size_t n, size_t group_bytes, bool big) {
  Fleet f(rng, n, big, true);
  RepairPlanner planner(f.rows.data(), f.pre.data(), f.enc.data(), f.n_bad.data(), n, group_bytes);
  RepairStep g;
  while (planner.next(g)) {
    if (g.single) {
      // what the routed job's tree launch stages
      const size_t j = g.job_lo;
      if (f.jobs[j].leaves && wants_tree(f.jobs[j])) {
        RepairStep one;
        one.job_lo = j, one.job_hi = j + 1;
        PosRepairJob t{};
        t.pre = (uint32_t)f.pre[j], t.log_enc = log2_pow2(f.enc[j]), t.n_chunks = 1, t.n_bad = (uint32_t)f.n_bad[j];
        one.jobs.push_back(t);
        one.src.push_back(0);
        one.col0.push_back(0);
        std::vector<uint8_t> dig(std::max<size_t>(1, f.n_bad[j] * 32), 0x5C);
        check_repair_block(f, one, dig.data());
      }
      continue;
    }
    if (!g.jobs.empty()) check_repair_block(f, g, nullptr);
  }
}

// a scrub group's images: every column, its written rows, the pad zeroed, into exactly image_bytes
static void check_scrub_fleet(std::mt19937_64 &rng, size_t n, size_t group_bytes, bool big) {
  Fleet f(rng, n, big, false);
  ScrubPlanner planner(f.rows.data(), f.pre.data(), f.enc.data(), n, group_bytes);
  ScrubStep g;
  while (planner.next(g)) {
    if (g.single) continue;
    std::vector<uint8_t> h(g.image_bytes, 0xA5);
    pack_columns(
        g.jobs, g.col0, g.image_bytes, g.n_cols, h.data(),
        [&](size_t i) -> const lcpc_pos_scrub_job & { return f.scrub_jobs[g.job_of((uint32_t)i)]; },
        [](size_t, size_t c) { return (ptrdiff_t)c; });
    for (size_t i = 0; i < g.jobs.size(); i++) {
      const PosScrubJob &t = g.jobs[i];
      const size_t j = g.job_of((uint32_t)i);
      CHECK(t.col0 == g.col0[i] && t.img % 16 == 0, "scrub job %zu: entry", j);
      for (size_t c = 0; t.n_rows && c < f.enc[j]; c++) {
        const uint8_t *got = h.data() + t.img + c * t.rows_pad * POS_WB;
        CHECK(!std::memcmp(got, f.images[j].data() + c * f.cap[j] * POS_WB, t.n_rows * POS_WB), "scrub job %zu column %zu: bytes", j, c);
        for (size_t b = t.n_rows * POS_WB; b < t.rows_pad * POS_WB; b++) CHECK(got[b] == 0, "scrub job %zu column %zu: pad", j, c);
      }
    }
  }
}

// ---------------------------------------------------------------- the empties
static void check_empties() {
  // what scrub_single stages for a routed job's stored tree: one job, no other table
  ScrubStep one;
  one.job_lo = 5, one.job_hi = 6;
  one.jobs.push_back(PosScrubJob{0, 0, 0, 0, 0, 0, 3, 11, 0, 0, 1, 0, 0, 1});
  check_tables(one, 4095 * 32 + 32);
  // nothing at all: no table is touched, no byte is written
  RowGroup none;
  const std::vector<PosIngestJob> no_jobs;
  const TableOffsets T = table_offsets(none, 0, 0, sizeof(PosIngestJob));
  CHECK(T.o_jobs == 0 && T.o_waves == 0 && T.in_bytes == 0, "empty ladder");
  copy_tables(none, no_jobs, T, nullptr);
  const std::vector<PosScrubJob> no_scrub;
  const std::vector<size_t> no_col0;
  pack_columns(
      no_scrub, no_col0, 0, 0, nullptr, [&](size_t) -> const lcpc_pos_scrub_job & { std::abort(); },
      [](size_t, size_t c) { return (ptrdiff_t)c; });
}

int main() {
  std::mt19937_64 rng(20241021);
  check_plans(rng);
  for (size_t n : {1, 2, 3, 17, 257})
    for (int it = 0; it < 6; it++) check_repair_fleet(rng, n, (size_t)32 << 20, it & 1);
  for (size_t n : {1, 3, 64, 300}) check_repair_fleet(rng, n, (size_t)1 << 20, true);   // the lowered seam: more groups, more routed jobs
  check_repair_fleet(rng, 2000, (size_t)1 << 16, false);                               // above the threshold of the threaded packing
  check_repair_fleet(rng, 700, (size_t)32 << 20, false);
  for (size_t n : {1, 3, 64, 300}) check_scrub_fleet(rng, n, (size_t)1 << 20, true);
  check_scrub_fleet(rng, 2000, (size_t)1 << 16, false);
  check_scrub_fleet(rng, 700, (size_t)32 << 20, false);                                // the threaded packing
  check_empties();
  std::printf("pos_rowgroup bad %d\n", bad);
  return bad != 0;
}
