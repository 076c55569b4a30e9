// pos_verify_group_host.cpp -- the client's check of a queue of stored-file audit responses (DESIGN
// §5h): many (result vector, opened columns with paths) verified together, with a number of launches
// that does not grow with the number of responses.
//
//   result vectors   one decode (ifft_oi) per distinct enc and one encode per distinct (pre, enc) over
//                    all jobs' rows, through the batched row entries the single check calls with one
//                    row; the side vectors and <dec[:pre], right> on the host (Montgomery words of
//                    reduced values: the same words as the device's);
//   VerifyPlanner    cuts the jobs, in order, into steps: a staging group of consecutive jobs (two
//                    launches, its wave tables built here) or one job for the single sequence (its
//                    columns above the group's size or count);
//   VerifyRunner     stages a group -- columns at a 16-byte aligned stride, paths, roots, indices, the
//                    re-encoded result at those indices, left vectors and tables in one page-locked
//                    block, one upload (h2d_blocks) -- and queues its two launches as the block lands;
//                    two blocks alternate, so the host gathers group k + 1 while group k runs;
//   lcpc_pos_verify_group_plan   the same steps as a work list, host only: what the CPU tests check.
#include "pos_internal.hpp"

namespace {

constexpr size_t VG_MAX_JOBS = (size_t)1 << 16, VG_MAX_COLS = (size_t)1 << 16, VG_MAX_WAVES = (size_t)1 << 20;

// a staged column: 2 n_rows words rounded up to a 16-byte unit; its leaf message: 8 zero words first
inline size_t col_words(size_t n_rows) { return align_up(2 * n_rows, 4); }

// ---- Ft63 Montgomery words on the host (R = 2^64; every operand but b is reduced)
struct Mont63 {
  uint64_t p, ninv, one;
  Mont63() {
    p = field_info(POS_FID).p[0];
    uint64_t inv = p;  // p^-1 mod 2^64 by Newton's iteration (p odd: 3 bits to start with)
    for (int i = 0; i < 6; i++) inv *= 2 - p * inv;
    ninv = 0 - inv;
    one = (uint64_t)((((unsigned __int128)1) << 64) % p);
  }
  // a b R^-1 mod p in [0, p) for a < p and any 64-bit b
  uint64_t mul(uint64_t a, uint64_t b) const {
    const unsigned __int128 t = (unsigned __int128)a * b;
    const uint64_t m = (uint64_t)t * ninv;
    const uint64_t r = (uint64_t)((t + (unsigned __int128)m * p) >> 64);
    return r >= p ? r - p : r;
  }
  uint64_t add(uint64_t a, uint64_t b) const {
    const uint64_t r = a + b;  // a, b < p < 2^63
    return r >= p ? r - p : r;
  }
  uint64_t pow(uint64_t a, uint64_t e) const {
    uint64_t r = one;
    for (; e; e >>= 1, a = mul(a, a))
      if (e & 1) r = mul(r, a);
    return r;
  }
  // dst[i] = base^i, i < n
  void powers(uint64_t base, size_t n, uint64_t *dst) const {
    uint64_t v = one;
    for (size_t i = 0; i < n; i++, v = mul(v, base)) dst[i] = v;
  }
};

struct VerifyStep {
  bool single = false;
  size_t job_lo = 0, job_hi = 0;
  // a grouped step: its waves and, per job, where its columns, chunk slots and left words start
  std::vector<PosVerifyWave> waves, fwaves;
  std::vector<size_t> col0, cv0, left0;
  size_t n_cols = 0, n_slots = 0, left_words = 0, col_bytes = 0, max_chunks = 0;
};

class VerifyPlanner {
 public:
  VerifyPlanner(const size_t *file_len, const size_t *pre, const size_t *n_cols, size_t n_jobs)
      : len_(file_len), pre_(pre), nc_(n_cols), n_jobs_(n_jobs), gb_(pos_group_bytes()) {}

  bool next(VerifyStep &st) {
    st = VerifyStep{};
    if (next_ >= n_jobs_) return false;
    const size_t lo = next_;
    st.job_lo = lo;
    if (!grouped(lo)) {
      st.single = true;
      st.job_hi = next_ = lo + 1;
      return true;
    }
    size_t hi = lo, bytes = 0, cols = 0, waves = 0;
    for (; hi < n_jobs_ && grouped(hi); hi++) {
      const size_t cb = job_bytes(hi), w = job_waves(hi);
      if (hi > lo && (bytes + cb > gb_ || hi - lo >= VG_MAX_JOBS || cols + nc_[hi] > VG_MAX_COLS ||
                      waves + w > VG_MAX_WAVES))
        break;
      bytes += cb, cols += nc_[hi], waves += w;
    }
    st.job_hi = next_ = hi;
    build(st);
    return true;
  }

 private:
  size_t rows(size_t j) const { return job_rows(len_[j], pre_[j]); }
  size_t job_bytes(size_t j) const { return nc_[j] * col_words(rows(j)) * 4; }
  size_t job_waves(size_t j) const { return ceil_div(nc_[j], 64) * leaf_chunks(rows(j)); }
  bool grouped(size_t j) const {
    if (!nc_[j]) return true;  // nothing to stage
    // (the products cannot overflow: a column count above the bound is refused first)
    return nc_[j] <= VG_MAX_COLS && rows(j) <= gb_ / 8 && job_bytes(j) <= gb_ &&
           leaf_chunks(rows(j)) <= POS_VERIFY_MAX_CHUNKS && job_waves(j) <= VG_MAX_WAVES;
  }

  void build(VerifyStep &st) const {
    for (size_t j = st.job_lo; j < st.job_hi; j++) {
      const size_t nc = nc_[j], nr = nc ? rows(j) : 0, chunks = nc ? leaf_chunks(nr) : 0;
      st.col0.push_back(st.n_cols);
      st.cv0.push_back(st.n_slots);
      st.left0.push_back(st.left_words);
      for (size_t c = 0; c < nc; c += 64) {
        st.fwaves.push_back(PosVerifyWave{(uint32_t)(j - st.job_lo), (uint32_t)c, 0, 0});
        for (size_t k = 0; k < chunks; k++)
          st.waves.push_back(PosVerifyWave{(uint32_t)(j - st.job_lo), (uint32_t)c, (uint32_t)k, 0});
      }
      st.n_cols += nc;
      st.n_slots += nc * chunks;
      st.left_words += nr;
      st.col_bytes += nc * col_words(nr) * 4;
      st.max_chunks = std::max(st.max_chunks, chunks);
    }
  }

  const size_t *len_, *pre_, *nc_;
  size_t n_jobs_, gb_, next_ = 0;
};

// One call's staging and launches.  run() returns with the group's upload, launches and read-back
// queued; its verdicts are reduced from the column bits when its page-locked block is next reused,
// or in finish().
struct VerifyRunner {
  Device *dev;
  hipStream_t s;
  const lcpc_pos_audit_job *jobs;  // the call's
  const uint64_t *enc_rows;        // the re-encoded result vectors, job j's at row_off[j]
  const size_t *row_off;
  uint8_t *verdict;
  const Mont63 &mf;
  DBuf arena, cvs, partials, bits;
  Pinned stg[2];
  Events ev;
  struct Pending {
    bool live = false;
    size_t off = 0, job_lo = 0, job_hi = 0;
  } pend[2];
  int k = 0;

  VerifyRunner(Device *d, hipStream_t stream, const lcpc_pos_audit_job *j, const uint64_t *er, const size_t *ro,
               uint8_t *v, const Mont63 &m)
      : dev(d), s(stream), jobs(j), enc_rows(er), row_off(ro), verdict(v), mf(m) {}
  // (an early return leaves copies queued on the blocks the members are about to give back)
  ~VerifyRunner() { (void)hipStreamSynchronize(s); }

  // paths first, then values
  void drain(int slot) {
    if (!pend[slot].live) return;
    const uint32_t *b = reinterpret_cast<const uint32_t *>(stg[slot].b() + pend[slot].off);
    for (size_t j = pend[slot].job_lo; j < pend[slot].job_hi; j++) {
      uint32_t all = 3;
      for (size_t c = 0; c < jobs[j].n_cols; c++) all &= b[c];
      b += jobs[j].n_cols;
      verdict[j] = !(all & 1) ? 1 : !(all & 2) ? 2 : 0;
    }
    pend[slot].live = false;
  }

  lcpc_status run(const VerifyStep &g) {
    if (g.waves.empty()) return LCPC_OK;  // no job of the group opened a column: they all pass
    const int slot = k & 1;
    HIP_TRY(ev.init());
    HIP_TRY(ev.reuse(k));
    drain(slot);
    const size_t n_jobs = g.job_hi - g.job_lo;
    const lcpc_pos_audit_job *jb = jobs + g.job_lo;
    // the block: [columns | paths | roots | idx | want | lefts | jobs | waves | fwaves] go up, [bits] come back
    std::vector<PosVerifyJob> tab(n_jobs);
    size_t o = 0;
    for (size_t i = 0; i < n_jobs; i++) {
      const size_t nc = jb[i].n_cols, nr = nc ? job_rows(jb[i].file_len, jb[i].pre) : 0;
      tab[i] = PosVerifyJob{o, 0, g.left0[i], g.col0[i], g.cv0[i], (uint32_t)nr, (uint32_t)nc,
                            (uint32_t)(nc ? leaf_chunks(nr) : 0), (uint32_t)log2_np2(jb[i].enc), (uint32_t)col_words(nr), 0};
      o += nc * col_words(nr) * 4;
    }
    for (size_t i = 0; i < n_jobs; i++) {
      tab[i].paths = o;
      o += (size_t)tab[i].n_cols * tab[i].path_len * 32;
    }
    const size_t o_roots = o;
    const size_t o_idx = o_roots + n_jobs * 32;
    const size_t o_want = o_idx + g.n_cols * 8;
    const size_t o_left = o_want + g.n_cols * 8;
    const size_t o_jobs = align_up(o_left + g.left_words * 8, 16);
    const size_t o_waves = o_jobs + n_jobs * sizeof(PosVerifyJob);
    const size_t o_fwaves = o_waves + g.waves.size() * sizeof(PosVerifyWave);
    const size_t in_bytes = align_up(o_fwaves + g.fwaves.size() * sizeof(PosVerifyWave), 256);
    const size_t total = in_bytes + g.n_cols * 4;
    if (stg[slot].n < total && !stg[slot].get(dev, total)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    lcpc_status est;
    if ((est = ensure(arena, dev, in_bytes, (size_t)4 << 20)) || (est = ensure(cvs, dev, g.n_slots * 32, (size_t)1 << 20)) ||
        (est = ensure(partials, dev, g.n_slots * 8, (size_t)1 << 20)) || (est = ensure(bits, dev, g.n_cols * 4, (size_t)1 << 16)))
      return est;
    uint8_t *h = stg[slot].b();
    {
      prof::HostScope hs("pos_group_verify_gather");
      auto gather = [&](size_t i) {
        const PosVerifyJob &t = tab[i];
        const lcpc_pos_audit_job &a = jb[i];
        std::memcpy(h + o_roots + 32 * i, a.root, 32);
        if (!t.n_cols) return;
        const size_t row_b = (size_t)t.n_rows * 8, stride = (size_t)t.col_words * 4;
        if (row_b == stride) {
          std::memcpy(h + t.cols, a.cols, t.n_cols * row_b);
        } else {  // an odd row count: 8 zero bytes end every column's stride
          for (size_t c = 0; c < t.n_cols; c++) {
            std::memcpy(h + t.cols + c * stride, a.cols + c * t.n_rows, row_b);
            std::memset(h + t.cols + c * stride + row_b, 0, stride - row_b);
          }
        }
        std::memcpy(h + t.paths, a.paths, (size_t)t.n_cols * t.path_len * 32);
        std::memcpy(h + o_idx + 8 * t.col0, a.idx, (size_t)t.n_cols * 8);
        uint64_t *want = reinterpret_cast<uint64_t *>(h + o_want) + t.col0;
        const uint64_t *row = enc_rows + row_off[g.job_lo + i];
        for (size_t c = 0; c < t.n_cols; c++) want[c] = row[a.idx[c]];
        // left = [1, x^pre, x^(2 pre), ...]
        mf.powers(mf.pow(a.point % mf.p, a.pre), t.n_rows, reinterpret_cast<uint64_t *>(h + o_left) + t.left);
      };
      if (g.col_bytes < ((size_t)4 << 20)) {
        for (size_t i = 0; i < n_jobs; i++) gather(i);
      } else {
        parallel_for(n_jobs, gather);
      }
      std::memcpy(h + o_jobs, tab.data(), n_jobs * sizeof(PosVerifyJob));
      std::memcpy(h + o_waves, g.waves.data(), g.waves.size() * sizeof(PosVerifyWave));
      std::memcpy(h + o_fwaves, g.fwaves.data(), g.fwaves.size() * sizeof(PosVerifyWave));
    }
    const uint8_t *d = arena.as<uint8_t>();
    lcpc_status st = h2d_blocks(dev, arena.as<uint8_t>(), h, in_bytes, in_bytes, s, [&](size_t, size_t) -> lcpc_status {
      HIP_TRY(pos_group_verify(d, reinterpret_cast<const PosVerifyJob *>(d + o_jobs),
                               reinterpret_cast<const PosVerifyWave *>(d + o_waves), g.waves.size(),
                               reinterpret_cast<const PosVerifyWave *>(d + o_fwaves), g.fwaves.size(), g.max_chunks,
                               reinterpret_cast<const uint32_t *>(d + o_left), d + o_roots,
                               reinterpret_cast<const uint64_t *>(d + o_idx), reinterpret_cast<const uint32_t *>(d + o_want),
                               cvs.as<uint32_t>(), partials.as<uint32_t>(), bits.as<uint32_t>(), s));
      return LCPC_OK;
    });
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + in_bytes, bits.p, g.n_cols * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev.e[slot], s));
    pend[slot] = Pending{true, in_bytes, g.job_lo, g.job_hi};
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

// the single sequence for one job: leaves, paths, column values (the result is already re-encoded)
lcpc_status verify_single(const lcpc_pos_audit_job &a, const uint64_t *enc_row, const Mont63 &mf, uint8_t *verdict) {
  const size_t n = a.n_cols, nr = job_rows(a.file_len, a.pre), pl = log2_np2(a.enc);
  std::vector<uint8_t> leaves(32 * n), ok(n);
  lcpc_status st;
  if ((st = lcpc_hash_field_columns((lcpc_field)POS_FID, a.cols, nr, n, leaves.data()))) return st;
  if ((st = lcpc_verify_leaf_paths(leaves.data(), a.paths, n, pl, a.idx, a.root, ok.data()))) return st;
  if (!std::all_of(ok.begin(), ok.end(), [](uint8_t v) { return v != 0; })) {
    *verdict = 1;
    return LCPC_OK;
  }
  std::vector<uint64_t> left(nr);
  mf.powers(mf.pow(a.point % mf.p, a.pre), nr, left.data());
  if ((st = lcpc_verify_column_values((lcpc_field)POS_FID, a.cols, n, nr, left.data(), enc_row, a.enc, a.idx, ok.data())))
    return st;
  *verdict = std::all_of(ok.begin(), ok.end(), [](uint8_t v) { return v != 0; }) ? 0 : 2;
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_verify_evaluations_grouped(const lcpc_pos_audit_job *jobs, size_t n_jobs, uint8_t *verdict,
                                                uint64_t *values) {
  if (!jobs || !verdict || !values) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  for (size_t j = 0; j < n_jobs; j++) {
    const lcpc_pos_audit_job &a = jobs[j];
    const std::string who = "job " + std::to_string(j);
    if (!a.root || !a.result || (a.n_cols && (!a.idx || !a.cols || !a.paths)))
      return fail(LCPC_ERR_INVALID_ARG, who + ": null argument");
    if (!a.file_len || !a.pre || !a.enc) return fail(LCPC_ERR_INVALID_ARG, who + " is empty");
    if ((a.enc & (a.enc - 1)) || a.enc <= a.pre)
      return fail(LCPC_ERR_INVALID_ARG, who + ": enc must be a power of two > pre");
    for (size_t c = 0; c < a.n_cols; c++)
      if (a.idx[c] >= a.enc || (c && a.idx[c] <= a.idx[c - 1]))
        return fail(LCPC_ERR_INVALID_ARG, who + ": column indices must be strictly increasing and below enc");
  }
  for (size_t j = 0; j < n_jobs; j++)
    if (lcpc_status st = check_fft_len(POS_FID, jobs[j].enc)) return st;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  prof::HostScope whole("pos_group_verify_call");  // the call's wall time, beside its device regions
  const Mont63 mf;
  std::memset(verdict, 0, n_jobs);

  // ---- the result vectors: rows ordered by (enc, pre), so a distinct enc and a distinct (pre, enc)
  // are each one run of rows
  std::vector<size_t> order(n_jobs), row_off(n_jobs);
  for (size_t j = 0; j < n_jobs; j++) order[j] = j;
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    return jobs[x].enc != jobs[y].enc ? jobs[x].enc < jobs[y].enc : jobs[x].pre < jobs[y].pre;
  });
  size_t words = 0;
  for (size_t j : order) row_off[j] = words, words += jobs[j].enc;
  std::vector<uint64_t> rows(words);
  for (size_t j = 0; j < n_jobs; j++) std::memcpy(rows.data() + row_off[j], jobs[j].result, jobs[j].enc * 8);
  for (size_t i = 0; i < n_jobs;) {  // decode: one call per distinct enc
    size_t e = i;
    while (e < n_jobs && jobs[order[e]].enc == jobs[order[i]].enc) e++;
    if ((st = lcpc_ifft_oi_rows((lcpc_field)POS_FID, rows.data() + row_off[order[i]], e - i, jobs[order[i]].enc))) return st;
    i = e;
  }
  // <dec[:pre], right>, right = [1, x, x^2, ...]; then dec[pre:] = 0 for the encode
  parallel_for(n_jobs, [&](size_t j) {
    const lcpc_pos_audit_job &a = jobs[j];
    uint64_t *dec = rows.data() + row_off[j];
    const uint64_t x = a.point % mf.p;
    uint64_t v = 0, r = mf.one;
    for (size_t i = 0; i < a.pre; i++, r = mf.mul(r, x)) v = mf.add(v, mf.mul(r, dec[i]));
    values[j] = v;
    std::memset(dec + a.pre, 0, (a.enc - a.pre) * 8);
  });
  for (size_t i = 0; i < n_jobs;) {  // encode: one call per distinct (pre, enc)
    const lcpc_pos_audit_job &a = jobs[order[i]];
    size_t e = i;
    while (e < n_jobs && jobs[order[e]].enc == a.enc && jobs[order[e]].pre == a.pre) e++;
    lcpc_encoding *ep = nullptr;
    if ((st = make_rs_encoding(POS_FID, a.pre, a.enc, 0, 0, &ep))) return st;
    std::unique_ptr<lcpc_encoding> enc(ep);
    if ((st = lcpc_encode_rows(ep, rows.data() + row_off[order[i]], e - i, a.enc))) return st;
    i = e;
  }

  // ---- the columns: staging groups, two launches each
  std::vector<size_t> lens(n_jobs), pres(n_jobs), ncs(n_jobs);
  for (size_t j = 0; j < n_jobs; j++) lens[j] = jobs[j].file_len, pres[j] = jobs[j].pre, ncs[j] = jobs[j].n_cols;
  VerifyPlanner planner(lens.data(), pres.data(), ncs.data(), n_jobs);
  VerifyRunner runner(dev, lease.s, jobs, rows.data(), row_off.data(), verdict, mf);
  VerifyStep g;
  while (planner.next(g)) {
    if (g.single) {
      if ((st = verify_single(jobs[g.job_lo], rows.data() + row_off[g.job_lo], mf, verdict + g.job_lo))) return st;
      continue;
    }
    if ((st = runner.run(g))) return st;
  }
  return runner.finish();
}

lcpc_status lcpc_pos_verify_group_plan(const size_t *file_len, const size_t *pre, const size_t *n_cols, size_t n_jobs,
                                       lcpc_pos_verify_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches) {
  if (!file_len || !pre || !n_cols || (!tiles && cap)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_jobs) return fail(LCPC_ERR_INVALID_ARG, "no jobs");
  for (size_t j = 0; j < n_jobs; j++)
    if (!file_len[j] || !pre[j]) return fail(LCPC_ERR_INVALID_ARG, "job " + std::to_string(j) + " is empty");
  VerifyPlanner planner(file_len, pre, n_cols, n_jobs);
  VerifyStep g;
  size_t n = 0, launches = 0;
  auto emit = [&](const lcpc_pos_verify_tile &t) {
    if (n < cap) tiles[n] = t;
    n++;
  };
  while (planner.next(g)) {
    if (g.single) {
      const size_t j = g.job_lo, chunks = leaf_chunks(job_rows(file_len[j], pre[j]));
      for (size_t k = 0; k < chunks; k++) emit(lcpc_pos_verify_tile{j, 0, n_cols[j], k, LCPC_POS_GROUP_SINGLE, 0});
      continue;
    }
    if (g.waves.empty()) continue;
    for (size_t w = 0; w < g.waves.size(); w++) {
      const PosVerifyWave &wv = g.waves[w];
      const size_t j = g.job_lo + wv.job;
      emit(lcpc_pos_verify_tile{j, wv.col_lo, std::min<size_t>(n_cols[j], (size_t)wv.col_lo + 64), wv.chunk,
                                (uint32_t)launches, (uint32_t)w});
    }
    launches++;
  }
  if (n_tiles) *n_tiles = n;
  if (n_launches) *n_launches = launches;
  return LCPC_OK;
}

}  // extern "C"
