// pos_repair_san.cpp -- the host-only half of the grouped repair (csrc/pos_repair_plan.hpp) under ASan +
// UBSan: random fleets cut into staging groups, every group's block laid out and packed into a buffer of
// exactly its size, and the packed bytes compared with the images.  The listed columns of every image,
// and the rows past rows_written of the others, are poisoned: a read of either ends the run.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <map>
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

struct Fleet {
  std::vector<size_t> rows, pre, enc, n_bad, cap;
  std::vector<std::vector<uint64_t>> lists;
  std::vector<std::vector<uint8_t>> images, leaves;
  std::vector<lcpc_pos_repair_job> jobs;
  uint8_t sink[32];

  Fleet(std::mt19937_64 &rng, size_t n, bool big) {
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
    }
  }
  ~Fleet() {
    for (auto &img : images) ASAN_UNPOISON_MEMORY_REGION(img.data(), img.size());
  }
};

static void check_block(const Fleet &f, Step &g, const uint8_t *single_digests) {
  const Layout L = lay_out(g, f.jobs.data(), single_digests != nullptr);
  std::vector<uint8_t> h(L.in_bytes, 0xA5);   // exactly the bytes that go up
  pack(g, f.jobs.data(), L, single_digests, h.data());
  CHECK(L.total >= L.in_bytes + L.out_bytes && L.o_jobs % 16 == 0 && L.in_bytes % 256 == 0, "layout");
  CHECK(!std::memcmp(h.data() + L.o_jobs, g.jobs.data(), g.jobs.size() * sizeof(PosRepairJob)), "job table");
  size_t end = 0;
  for (size_t i = 0; i < g.jobs.size(); i++) {
    const PosRepairJob &t = g.jobs[i];
    const size_t j = g.job_lo + g.src[i], enc = f.enc[j];
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
  CHECK(end <= L.o_jobs, "tables overlap");
}

static void check_fleet(std::mt19937_64 &rng, size_t n, size_t group_bytes, bool big) {
  Fleet f(rng, n, big);
  Planner planner(f.rows.data(), f.pre.data(), f.enc.data(), f.n_bad.data(), n, group_bytes);
  std::map<std::pair<size_t, size_t>, int> seen;   // (job, row) -> records
  Step g;
  size_t next = 0;
  while (planner.next(g)) {
    CHECK(g.job_lo == next && g.job_hi > g.job_lo && g.job_hi <= n, "steps are consecutive");
    next = g.job_hi;
    if (g.single) {
      const size_t j = g.job_lo;
      CHECK(planner.works(j) && (f.enc[j] > LCPC_POS_REPAIR_MAX_ENC || packed_bytes(f.rows[j], f.enc[j]) > group_bytes),
            "job %zu routed without cause", j);
      for (size_t r = 0; r < f.rows[j]; r++) seen[{j, r}]++;
      // what the routed job's tree launch stages
      if (f.jobs[j].leaves && wants_tree(f.jobs[j])) {
        Step one;
        one.job_lo = j, one.job_hi = j + 1;
        PosRepairJob t{};
        t.pre = (uint32_t)f.pre[j], t.log_enc = log2_pow2(f.enc[j]), t.n_chunks = 1, t.n_bad = (uint32_t)f.n_bad[j];
        one.jobs.push_back(t);
        one.src.push_back(0);
        one.col0.push_back(0);
        std::vector<uint8_t> dig(std::max<size_t>(1, f.n_bad[j] * 32), 0x5C);
        check_block(f, one, dig.data());
      }
      continue;
    }
    size_t bytes = 0;
    for (size_t i = 0; i < g.jobs.size(); i++) bytes += packed_bytes(g.jobs[i].n_rows, (size_t)1 << g.jobs[i].log_enc);
    CHECK(g.jobs.size() <= 1 || bytes <= group_bytes, "a group of %zu bytes", bytes);
    for (const PosIngestWg &w : g.wgs) {
      CHECK(w.n_tiles >= 1 && w.n_tiles <= wg_slots((size_t)1 << w.log_enc) && w.tile0 + w.n_tiles <= g.tiles.size(), "workgroup");
      CHECK(((size_t)w.n_tiles << (3 + w.log_enc)) * POS_WB <= g.lds_bytes && g.lds_bytes <= 65536, "LDS");
      for (uint32_t i = 0; i < w.n_tiles; i++) {
        const PosIngestTile &t = g.tiles[w.tile0 + i];
        CHECK(t.job < g.jobs.size() && g.jobs[t.job].log_enc == w.log_enc && t.n_rows >= 1 && t.n_rows <= 8 &&
                  t.row_lo + t.n_rows <= g.jobs[t.job].n_rows, "tile");
        for (uint32_t r = 0; r < t.n_rows; r++) seen[{g.job_lo + g.src[t.job], t.row_lo + r}]++;
      }
    }
    for (const PosIngestWave &w : g.waves)
      CHECK(w.job < g.jobs.size() && w.col_lo < g.jobs[w.job].n_bad && w.chunk < g.jobs[w.job].n_chunks, "wave");
    if (!g.jobs.empty()) check_block(f, g, nullptr);
  }
  CHECK(next == n, "jobs covered");
  size_t want = 0;
  for (size_t j = 0; j < n; j++)
    if (planner.works(j)) want += f.rows[j];
  CHECK(seen.size() == want, "%zu (job, row) pairs covered, not %zu", seen.size(), want);
  for (const auto &kv : seen) CHECK(kv.second == 1 && planner.works(kv.first.first), "a row in %d records", kv.second);
}

int main() {
  std::mt19937_64 rng(20241021);
  for (size_t n : {1, 2, 3, 17, 257})
    for (int it = 0; it < 6; it++) check_fleet(rng, n, (size_t)32 << 20, it & 1);
  for (size_t n : {1, 3, 64, 300}) check_fleet(rng, n, (size_t)1 << 20, true);   // the lowered seam: more groups, more routed jobs
  check_fleet(rng, 2000, (size_t)1 << 16, false);                               // above the threshold of the threaded packing
  check_fleet(rng, 700, (size_t)32 << 20, false);
  std::printf("pos_repair bad %d\n", bad);
  return bad != 0;
}
