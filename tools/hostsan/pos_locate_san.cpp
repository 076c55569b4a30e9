// pos_locate_san.cpp -- the host-only half of the grouped locate of stored files
// (csrc/pos_locate_plan.hpp over csrc/pos_repair_plan.hpp and csrc/pos_rowgroup_plan.hpp) under ASan +
// UBSan: random fleets with images cut by the repair planner with the known columns as the listed ones,
// every group laid out and packed into a buffer of exactly the bytes that go up, and compared with the
// images.  The rows past rows_written of every column, and the known columns whole, are poisoned: a read
// of either ends the run.  The locate records are checked against the arenas' sizes (a row's syndromes
// and mask words overlap no other row's and end inside the arena; the syndrome arena is no larger than the
// packed images), the returned bytes against their offsets, and the counters against a count by hand.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <random>

#include "pos_locate_plan.hpp"

using namespace lcpc_host;

static int bad = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      bad++;                            \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fputc('\n', stderr);         \
    }                                   \
  } while (0)

struct Fleet {
  std::vector<size_t> rows, pre, enc, n_known, cap;
  std::vector<std::vector<uint64_t>> lists;
  std::vector<std::vector<uint8_t>> images;
  std::vector<lcpc_pos_locate_job> jobs;
  std::vector<lcpc_pos_repair_job> shadow;
  uint8_t sink[2048];

  Fleet(std::mt19937_64 &rng, size_t n, bool big) {
    static const size_t encs[] = {2, 4, 16, 32, 256, 1024, 2048}, rws[] = {0, 1, 7, 8, 9, 129};
    for (size_t j = 0; j < n; j++) {
      const size_t e = encs[rng() % (big ? 7 : 5)], p = 1 + rng() % (e - 1), r = rws[rng() % 6];
      const size_t room = e - p, pick[] = {0, 1, room, room + 1, rng() % (room + 1)};
      const size_t nk = std::min(e, pick[rng() % 5]);
      rows.push_back(r), pre.push_back(p), enc.push_back(e), n_known.push_back(nk), cap.push_back(2 * r + 3);
      std::vector<uint64_t> cols(e);
      for (size_t c = 0; c < e; c++) cols[c] = c;
      std::shuffle(cols.begin(), cols.end(), rng);
      cols.resize(nk);
      lists.push_back(cols);
      std::vector<uint8_t> img(e * cap[j] * POS_WB);
      for (auto &b : img) b = (uint8_t)rng();
      images.push_back(std::move(img));
    }
    for (size_t j = 0; j < n; j++) {
      std::vector<uint8_t> listed(enc[j], 0);
      for (uint64_t c : lists[j]) listed[c] = 1;
      for (size_t c = 0; c < enc[j]; c++) {
        uint8_t *col = images[j].data() + c * cap[j] * POS_WB;
        if (listed[c])
          ASAN_POISON_MEMORY_REGION(col, cap[j] * POS_WB);
        else
          ASAN_POISON_MEMORY_REGION(col + rows[j] * POS_WB, (cap[j] - rows[j]) * POS_WB);
      }
      lcpc_pos_locate_job job{};
      job.porenc = images[j].data(), job.pre = pre[j], job.enc = enc[j], job.rows_written = rows[j];
      job.row_capacity = cap[j], job.known_bad = lists[j].data(), job.n_known = n_known[j];
      job.col_status = sink, job.row_status = rng() % 2 ? sink : nullptr;   // (never written here)
      jobs.push_back(job);
      shadow.push_back(locate::as_repair(job));
    }
  }
  ~Fleet() {
    for (auto &img : images) ASAN_UNPOISON_MEMORY_REGION(img.data(), img.size());
  }
};

static void check_block(const Fleet &f, RepairStep &g) {
  std::vector<locate::PosLocateJob> lj;
  const locate::Layout L = locate::lay_out(g, f.shadow.data(), lj);
  std::vector<uint8_t> h(L.in_bytes, 0xA5);   // exactly the bytes that go up
  locate::pack(g, f.shadow.data(), L, lj, h.data());
  CHECK(L.o_ljobs == L.R.T.in_bytes && L.o_ljobs % 16 == 0 && L.in_bytes % 256 == 0, "layout");
  CHECK(L.o_ljobs + lj.size() * sizeof(locate::PosLocateJob) <= L.in_bytes && lj.size() == g.jobs.size(), "records end");
  CHECK(!std::memcmp(h.data() + L.o_ljobs, lj.data(), lj.size() * sizeof(locate::PosLocateJob)), "records");
  CHECK(!std::memcmp(h.data() + L.R.T.o_jobs, g.jobs.data(), g.jobs.size() * sizeof(PosRepairJob)), "job table");
  CHECK(L.d_cols >= g.n_rows && L.d_flags >= L.d_cols + g.n_cols && L.out_bytes > L.d_flags + g.n_rows, "returned bytes");
  CHECK(L.total == L.in_bytes + L.out_bytes, "total");
  CHECK(L.synd_elems * 8 <= g.image_bytes, "the syndrome arena is larger than the packed images");
  size_t synd = 0, mask = 0, col = 0, enc_max = 2;
  bool listed = false;
  for (size_t i = 0; i < g.jobs.size(); i++) {
    const PosRepairJob &t = g.jobs[i];
    const size_t j = g.job_of((uint32_t)i), enc = f.enc[j];
    CHECK(((size_t)1 << t.log_enc) == enc && t.n_bad == f.n_known[j] && t.pre == f.pre[j] && t.n_rows == f.rows[j], "job %zu: dims", j);
    CHECK(!t.has_tree && !t.tree_only, "job %zu: a tree", j);
    CHECK(lj[i].synd0 == synd && lj[i].mask0 == mask && lj[i].col0 == col, "job %zu: record", j);
    synd += f.rows[j] * (enc - f.pre[j] - f.n_known[j]);
    mask += f.rows[j] * std::max<size_t>(1, enc / 64);
    col += enc;
    listed |= f.n_known[j] != 0;
    if (f.rows[j]) enc_max = std::max(enc_max, enc);
    const int32_t *cmap = reinterpret_cast<const int32_t *>(h.data() + t.cmap);
    size_t packed = 0;
    for (size_t c = 0; c < enc; c++) {
      const int32_t m = cmap[c];
      if (m >= 0) {
        CHECK((size_t)m < t.n_bad && f.lists[j][m] == c, "job %zu: column %zu maps to list entry %d", j, c, m);
        continue;
      }
      const size_t q = (size_t)(-1 - m);
      CHECK(q == packed, "job %zu: column %zu is packed column %zu", j, c, q);
      packed++;
      if (!t.n_rows || q >= enc - t.n_bad) continue;
      const uint8_t *got = h.data() + t.img + q * t.rows_pad * POS_WB;
      CHECK(!std::memcmp(got, f.images[j].data() + c * f.cap[j] * POS_WB, t.n_rows * POS_WB), "job %zu column %zu: bytes", j, c);
      for (size_t b = t.n_rows * POS_WB; b < t.rows_pad * POS_WB; b++) CHECK(got[b] == 0, "job %zu column %zu: pad", j, c);
    }
    CHECK(packed == enc - t.n_bad, "job %zu: packed columns", j);
  }
  CHECK(synd == L.synd_elems && mask == L.mask_words && col == g.n_cols, "arena sizes");
  CHECK(listed == L.any_listed && L.lds_bm == lcpc::pos_locate_bm_lds(enc_max) && L.lds_bm <= 20 * 1024, "launch parameters");
}

static void check_fleet(std::mt19937_64 &rng, size_t n, size_t group_bytes, bool big) {
  Fleet f(rng, n, big);
  RepairPlanner planner(f.rows.data(), f.pre.data(), f.enc.data(), f.n_known.data(), n, group_bytes);
  RepairStep g;
  size_t next = 0;
  while (planner.next(g)) {
    CHECK(g.job_lo == next, "steps are consecutive");
    next = g.job_hi;
    if (g.single || g.jobs.empty()) continue;
    check_block(f, g);
  }
  CHECK(next == n, "every job is in a step");
}

static void check_counters(std::mt19937_64 &rng) {
  for (int it = 0; it < 200; it++) {
    const size_t enc = (size_t)1 << (1 + rng() % 10), rows = rng() % 40;
    std::vector<uint8_t> cs(enc), rs(rows);   // exactly their sizes
    size_t nb = 0, nd = 0, nu = 0;
    for (auto &c : cs) c = (uint8_t)(rng() % 4), nb += c != 0;
    for (auto &r : rs) r = (uint8_t)(rng() % 3), nd += r != 0, nu += r == 2;
    const locate::Counters c = locate::count(cs.data(), enc, rs.data(), rows);
    CHECK(c.n_bad_cols == nb && c.n_dirty_rows == nd && c.n_unlocatable_rows == nu, "counters");
  }
}

int main() {
  std::mt19937_64 rng(20261021);
  for (size_t n : {1, 2, 3, 17, 257})
    for (int it = 0; it < 6; it++) check_fleet(rng, n, (size_t)32 << 20, it & 1);
  for (size_t n : {1, 3, 64, 300}) check_fleet(rng, n, (size_t)1 << 20, true);   // the lowered seam: more groups, more routed jobs
  check_fleet(rng, 2000, (size_t)1 << 16, false);
  check_fleet(rng, 700, (size_t)32 << 20, false);                               // the threaded packing
  check_counters(rng);
  std::printf("pos_locate bad %d\n", bad);
  return bad != 0;
}
