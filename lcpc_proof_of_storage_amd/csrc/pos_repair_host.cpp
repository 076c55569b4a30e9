// pos_repair_host.cpp -- Reed-Solomon erasure decoding, scrub and repair of stored files, and error
// location by syndromes (kernels: erasure.hip, rs_locate.hip).
#include "pos_internal.hpp"

// No counterpart in the reference (its decode_row is a plain ifft_oi and verify_all_files_agree can
// only say "trees differ"): the redundancy of the rate <= 1/2 code is used to locate damaged columns
// of a stored file against its Merkle leaves and to recompute them.  Kernels: erasure.hip.
namespace {

// a * b R^-1 mod p on 32-bit words (CIOS), host side: only lcpc_rs_domain_points needs it
template <class F>
void host_mont_mul(const uint32_t *a, const uint32_t *b, uint32_t *out) {
  constexpr int N = F::N;
  uint32_t t[N + 2] = {0};
  for (int i = 0; i < N; i++) {
    uint64_t c = 0;
    for (int j = 0; j < N; j++) {
      const uint64_t x = (uint64_t)a[j] * b[i] + t[j] + c;
      t[j] = (uint32_t)x;
      c = x >> 32;
    }
    uint64_t x = (uint64_t)t[N] + c;
    t[N] = (uint32_t)x;
    t[N + 1] = (uint32_t)(x >> 32);
    const uint32_t m = t[0] * F::NP;
    x = (uint64_t)m * F::P[0] + t[0];
    c = x >> 32;
    for (int j = 1; j < N; j++) {
      x = (uint64_t)m * F::P[j] + t[j] + c;
      t[j - 1] = (uint32_t)x;
      c = x >> 32;
    }
    x = (uint64_t)t[N] + c;
    t[N - 1] = (uint32_t)x;
    t[N] = t[N + 1] + (uint32_t)(x >> 32);
  }
  bool ge = t[N] != 0;
  if (!ge) {
    ge = true;  // t == p also subtracts
    for (int i = N - 1; i >= 0; i--)
      if (t[i] != F::P[i]) {
        ge = t[i] > F::P[i];
        break;
      }
  }
  if (ge) {
    uint64_t br = 0;
    for (int i = 0; i < N; i++) {
      const uint64_t d = (uint64_t)t[i] - F::P[i] - br;
      t[i] = (uint32_t)d;
      br = (d >> 32) & 1;
    }
  }
  for (int i = 0; i < N; i++) out[i] = t[i];
}

inline size_t bitrev_host(size_t i, int log_n) {
  size_t r = 0;
  for (int b = 0; b < log_n; b++) r |= ((i >> b) & 1) << (log_n - 1 - b);
  return r;
}

// the erasure set as the kernels take it; the argument rules of lcpc_rs_erasure_decode_rows
lcpc_status erasure_check(size_t len, size_t n_per_row, const uint64_t *erased, size_t n_erased,
                          std::vector<uint32_t> &e32) {
  if (n_per_row < 1 || n_per_row >= len) return fail(LCPC_ERR_INVALID_ARG, "n_per_row outside [1, len)");
  if (!erased && n_erased) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (len > ((size_t)1 << 24)) return fail(LCPC_ERR_UNSUPPORTED, "length beyond the NTT range");
  std::vector<bool> seen(len, false);
  e32.resize(n_erased);
  for (size_t i = 0; i < n_erased; i++) {
    if (erased[i] >= len) return fail(LCPC_ERR_INVALID_ARG, "erased index out of range");
    if (seen[erased[i]]) return fail(LCPC_ERR_INVALID_ARG, "duplicate erased index");
    seen[erased[i]] = true;
    e32[i] = (uint32_t)erased[i];
  }
  if (n_erased > len - n_per_row)
    return fail(LCPC_ERR_UNRECOVERABLE, "more erasures than the code's redundancy (len - n_per_row)");
  return LCPC_OK;
}

// Per-call device state of an erasure decode: both plans, the locator's tables, the check flag.
struct ErasureCtx {
  int fid = 0, log_n = 0;
  size_t n = 0, n_erased = 0, deg_bound = 0;
  hipStream_t s = nullptr;
  NttPlan fwd, inv;
  DBuf erased, slot, lambda, dinv, dscale, flag;
  ~ErasureCtx() {
    if (s) (void)hipStreamSynchronize(s);
    ntt_plan_free(fwd);
    ntt_plan_free(inv);
  }
};

lcpc_status erasure_ctx_init(ErasureCtx &c, Device *dev, hipStream_t s, int fid, size_t len, size_t n_per_row,
                             const std::vector<uint32_t> &e32) {
  c.fid = fid;
  c.log_n = (int)log2_np2(len);
  c.n = len;
  c.n_erased = e32.size();
  c.deg_bound = n_per_row + e32.size();
  c.s = s;
  const int wb = field_bytes(fid);
  for (bool inverse : {false, true}) {
    const hipError_t he = ntt_plan_init(inverse ? c.inv : c.fwd, fid, c.log_n, inverse, s);
    if (he == hipErrorInvalidValue) return fail(LCPC_ERR_UNSUPPORTED, "length beyond the NTT range");
    HIP_TRY(he);
  }
  HIP_TRY(c.erased.alloc(dev, e32.size() * 4));
  HIP_TRY(c.slot.alloc(dev, len * 4));
  HIP_TRY(c.lambda.alloc(dev, len * wb));
  HIP_TRY(c.dinv.alloc(dev, e32.size() * wb));
  HIP_TRY(c.dscale.alloc(dev, len * wb));
  HIP_TRY(c.flag.alloc(dev, 8));
  HIP_TRY(hipMemsetAsync(c.flag.p, 0, 8, s));
  if (!e32.empty()) HIP_TRY(hipMemcpyAsync(c.erased.p, e32.data(), e32.size() * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(erasure_locator(fid, c.fwd.d_tw, c.log_n, c.erased.as<uint32_t>(), c.n_erased, c.slot.as<int32_t>(),
                          c.lambda.as<uint32_t>(), c.dinv.as<uint32_t>(), s));
  uint32_t inv[8] = {0};
  inv_pow2_canon(fid, c.log_n, inv);
  HIP_TRY(erasure_dscale(fid, c.log_n, inv, c.dscale.as<uint32_t>(), s));
  // (e32 is pageable host memory: the copy above has left it once the stream drains)
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

// g: B masked rows in the inverse plan's input order (clobbered).  On return h holds P'(x_c) in
// codeword order (not computed when nothing is erased) and the flag has the degree check's verdict.
lcpc_status erasure_core(ErasureCtx &c, uint32_t *g, uint32_t *h, size_t B) {
  HIP_TRY(ntt_rows(c.inv, g, c.n, c.n, h, c.n, B, c.s));
  HIP_TRY(erasure_deriv(c.fid, h, g, c.log_n, B, c.dscale.as<uint32_t>(), c.deg_bound, c.flag.as<uint32_t>(), c.s));
  if (c.n_erased) HIP_TRY(ntt_rows(c.fwd, g, c.n, c.n, h, c.n, B, c.s));
  return LCPC_OK;
}

// The values of the erased positions e32 of every row (filled[r][j], Montgomery), rows untouched;
// LCPC_ERR_UNRECOVERABLE if a row fails the degree check.
lcpc_status erasure_decode_values(Device *dev, hipStream_t s, int f, const uint64_t *rows, size_t n_rows, size_t len,
                                  size_t n_per_row, const std::vector<uint32_t> &e32, std::vector<uint64_t> &filled) {
  lcpc_status st;
  const size_t n_erased = e32.size();
  const size_t wb = (size_t)field_bytes(f), nl = wb / 8;
  ErasureCtx c;
  if ((st = erasure_ctx_init(c, dev, s, f, len, n_per_row, e32))) return st;
  // 16 MiB of row elements per batch (2^21 Ft63 elements still fill the device): 64 rows at the
  // stored files' 2^15-point shape
  const size_t bmax = std::max<size_t>(1, std::min(n_rows, ((size_t)16 << 20) / (len * wb)));
  DBuf a, g, h, vals;
  HIP_TRY(a.alloc(dev, bmax * len * wb));
  HIP_TRY(g.alloc(dev, bmax * len * wb));
  HIP_TRY(h.alloc(dev, bmax * len * wb));
  HIP_TRY(vals.alloc(dev, bmax * n_erased * wb));
  filled.assign(n_rows * n_erased * nl, 0);
  for (size_t r0 = 0; r0 < n_rows; r0 += bmax) {
    const size_t B = std::min(bmax, n_rows - r0);
    HIP_TRY(hipMemcpyAsync(a.p, rows + r0 * len * nl, B * len * wb, hipMemcpyHostToDevice, s));
    HIP_TRY(erasure_masked_rows(f, a.as<uint32_t>(), g.as<uint32_t>(), c.log_n, B, c.slot.as<int32_t>(),
                                c.lambda.as<uint32_t>(), s));
    if ((st = erasure_core(c, g.as<uint32_t>(), h.as<uint32_t>(), B))) return st;
    if (n_erased) {
      HIP_TRY(erasure_fill(f, h.as<uint32_t>(), c.log_n, B, c.erased.as<uint32_t>(), n_erased, c.dinv.as<uint32_t>(),
                           vals.as<uint32_t>(), nullptr, nullptr, false, s));
      HIP_TRY(hipMemcpyAsync(filled.data() + r0 * n_erased * nl, vals.p, B * n_erased * wb, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
  }
  uint32_t flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, c.flag.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag)
    return fail(LCPC_ERR_UNRECOVERABLE, "a row is not a codeword on its surviving positions (degree check failed)");
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_rs_domain_points(lcpc_field f, size_t len, uint64_t *out) {
  if (!valid_field(f) || !out) return fail(LCPC_ERR_INVALID_ARG, "arguments");
  lcpc_status st = check_fft_len(f, len);
  if (st) return st;
  const int log_n = (int)log2_np2(len);
  dispatch_field(f, [&]<class F>() {
    constexpr int N = F::N;
    // the forward transform's root (ntt_plan_init): ROOT_OF_UNITY^(2^(S - log_n)), or its inverse
    uint32_t w[N], x[N];
    for (int i = 0; i < N; i++) w[i] = LCPC_FFT_OMEGA_INVERSE ? F::ROOT_INV[i] : F::ROOT[i];
    for (int k = 0; k < F::S - log_n; k++) host_mont_mul<F>(w, w, w);
    for (int i = 0; i < N; i++) x[i] = F::ONE[i];
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    for (size_t e = 0; e < len; e++) {  // x = w^e is the point of position bitrev(e) (or e)
      const size_t c = LCPC_FFT_OUTPUT_BITREV ? bitrev_host(e, log_n) : e;
      std::memcpy(o + c * N, x, sizeof(x));
      host_mont_mul<F>(x, w, x);
    }
    return 0;
  });
  return LCPC_OK;
}

lcpc_status lcpc_rs_erasure_decode_rows(lcpc_field f, uint64_t *rows, size_t n_rows, size_t len, size_t n_per_row,
                                        const uint64_t *erased, size_t n_erased) {
  if (!valid_field(f) || (!rows && n_rows)) return fail(LCPC_ERR_INVALID_ARG, "arguments");
  if (!field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field has no gfx950 kernels");
  lcpc_status st = check_fft_len(f, len);
  if (st) return st;
  std::vector<uint32_t> e32;
  if ((st = erasure_check(len, n_per_row, erased, n_erased, e32))) return st;
  if (n_rows == 0) return LCPC_OK;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const size_t wb = (size_t)field_bytes(f), nl = wb / 8;
  // the recovered values of every row stay here until the degree check has passed for all rows
  std::vector<uint64_t> filled;
  if ((st = erasure_decode_values(dev, lease.s, f, rows, n_rows, len, n_per_row, e32, filled))) return st;
  // only the erased positions are written: every other limb keeps its bits
  for (size_t r = 0; r < n_rows; r++)
    for (size_t j = 0; j < n_erased; j++)
      std::memcpy(rows + (r * len + e32[j]) * nl, filled.data() + (r * n_erased + j) * nl, wb);
  return LCPC_OK;
}

lcpc_status lcpc_pos_scrub_porenc(const uint8_t *porenc, size_t enc, size_t rows_written, size_t row_capacity,
                                  const uint8_t *leaves, uint8_t *digests, uint8_t *status, size_t *n_bad) {
  if (enc < 2 || (enc & (enc - 1))) return fail(LCPC_ERR_INVALID_ARG, "encoded width must be a power of 2 (>= 2)");
  if (!leaves || !status || (!porenc && rows_written)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (rows_written > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "rows_written > row_capacity");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const int fid = POS_FID;
  const size_t cpb = column_block_cols(enc, rows_written * POS_WB, pos_stage_bytes());
  DBuf hashes, dleaves, scratch[2], dbad, dstatus;
  HIP_TRY(hashes.alloc(dev, enc * 32));
  HIP_TRY(dleaves.alloc(dev, enc * 32));
  HIP_TRY(dbad.alloc(dev, enc * 4));
  HIP_TRY(dstatus.alloc(dev, enc));
  for (auto &x : scratch) HIP_TRY(x.alloc(dev, leaf_hash_scratch_bytes(fid, rows_written, cpb)));
  HIP_TRY(hipMemsetAsync(dbad.p, 0, enc * 4, s));
  HIP_TRY(hipMemcpyAsync(dleaves.p, leaves, enc * 32, hipMemcpyHostToDevice, s));
  const ImageSrc img{porenc, -1, row_capacity};
  st = for_column_blocks(
      dev, s, img, enc, cpb, 0, rows_written, rows_written, [&](uint32_t *d_cols, size_t c0, size_t nc, int slot) -> lcpc_status {
        // a non-canonical element is a finding of its column, not an error of the call
        if (rows_written) HIP_TRY(scrub_col_canon(fid, d_cols, rows_written, nc, dbad.as<uint32_t>() + c0, s));
        // the leaves hash canonical bytes: the slice is hashed as it is, without a conversion round trip
        HIP_TRY(leaf_hashes_cols(fid, d_cols, rows_written, nc, hashes.as<uint8_t>() + c0 * 32, scratch[slot].p, s, true));
        return LCPC_OK;
      });
  if (st) return st;
  HIP_TRY(scrub_status(hashes.as<uint8_t>(), dleaves.as<uint8_t>(), dbad.as<uint32_t>(), enc, dstatus.as<uint8_t>(), s));
  HIP_TRY(hipMemcpyAsync(status, dstatus.p, enc, hipMemcpyDeviceToHost, s));
  if (digests) HIP_TRY(hipMemcpyAsync(digests, hashes.p, enc * 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (n_bad) {
    size_t n = 0;
    for (size_t c = 0; c < enc; c++) n += status[c] != 0;
    *n_bad = n;
  }
  return LCPC_OK;
}

lcpc_status lcpc_pos_repair_columns(const uint8_t *porenc, size_t pre, size_t enc, size_t rows_written,
                                    size_t row_capacity, const uint64_t *bad_cols, size_t n_bad, uint8_t *cols_out,
                                    uint8_t *digests_out, uint8_t *data_out) {
  lcpc_status st = pos_dims_check(pre, enc);
  if (st) return st;
  if (rows_written > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "rows_written > row_capacity");
  if (!porenc && rows_written) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  std::vector<uint32_t> e32;
  if ((st = erasure_check(enc, pre, bad_cols, n_bad, e32))) return st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const int fid = POS_FID;
  const size_t rows = rows_written;
  ErasureCtx c;
  if ((st = erasure_ctx_init(c, dev, s, fid, enc, pre, e32))) return st;
  std::vector<uint8_t> is_bad(enc, 0);
  for (uint32_t j : e32) is_bad[j] = 1;
  // batches of whole BLAKE3 chunks of the column messages, as the writer's
  const size_t n_chunks = leaf_n_chunks(fid, rows);
  const ChunkBatches batches = repair_batches(rows, n_chunks, enc, pos_stage_bytes());
  const size_t bmax = batches.max_rows();
  const bool want_vals = n_bad && (cols_out || digests_out);
  DBuf src, a, g, h, vals, cm, dcv, dbytes, dbad;
  HIP_TRY(src.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(g.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(h.alloc(dev, bmax * enc * POS_WB));
  if (data_out) {
    HIP_TRY(a.alloc(dev, bmax * enc * POS_WB));
    HIP_TRY(dbytes.alloc(dev, bmax * pre * POS_DB + 64));
  }
  HIP_TRY(vals.alloc(dev, bmax * n_bad * POS_WB));
  HIP_TRY(cm.alloc(dev, bmax * n_bad * POS_WB));
  HIP_TRY(dcv.alloc(dev, n_chunks * n_bad * 32));
  HIP_TRY(dbad.alloc(dev, 8));
  HIP_TRY(hipMemsetAsync(dbad.p, 0, 8, s));
  Pinned stg[2], ocols, odata;
  for (auto &x : stg)
    if (!x.get(dev, bmax * enc * POS_WB)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  if (cols_out && n_bad && !ocols.get(dev, bmax * n_bad * POS_WB)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  if (data_out && !odata.get(dev, bmax * pre * POS_DB)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  // the damaged columns are never read, neither here nor by the kernels
  const ImageSrc img{porenc, -1, row_capacity, is_bad.data()};
  auto stage = [&](int slot, const ChunkBatches::Batch &b) {
    gather_slices(img, 0, enc, b.r0, b.B, b.B * POS_WB, stg[slot].b());
  };
  stage(0, batches.at(0));
  int k = 0;
  for (size_t c_lo = 0, c_hi = 0; c_lo < n_chunks; c_lo = c_hi, k++) {
    const auto [r0, B, next] = batches.at(c_lo);
    c_hi = next;
    const int slot = k & 1;
    if (B) {
      HIP_TRY(hipMemcpyAsync(src.p, stg[slot].p, enc * B * POS_WB, hipMemcpyHostToDevice, s));
      HIP_TRY(erasure_masked_cols(fid, src.as<uint32_t>(), B, c.log_n, g.as<uint32_t>(),
                                  data_out ? a.as<uint32_t>() : nullptr, c.slot.as<int32_t>(),
                                  c.lambda.as<uint32_t>(), dbad.as<uint32_t>(), s));
      if ((st = erasure_core(c, g.as<uint32_t>(), h.as<uint32_t>(), B))) return st;
      if (n_bad && (want_vals || data_out))
        HIP_TRY(erasure_fill(fid, h.as<uint32_t>(), c.log_n, B, c.erased.as<uint32_t>(), n_bad, c.dinv.as<uint32_t>(),
                             vals.as<uint32_t>(), cols_out ? cm.as<uint32_t>() : nullptr,
                             data_out ? a.as<uint32_t>() : nullptr, true, s));
      if (cols_out && n_bad)
        HIP_TRY(hipMemcpyAsync(ocols.p, cm.p, n_bad * B * POS_WB, hipMemcpyDeviceToHost, s));
      if (data_out) {
        // decode of the completed rows, as lcpc_pos_decode_porenc (g is free by now)
        uint32_t *x = nullptr, *y = nullptr;
        if ((st = ifft_oi_device(c.inv, fid, c.log_n, a.as<uint32_t>(), g.as<uint32_t>(), B, s, &x, &y))) return st;
        if ((st = decode_rows_to_bytes(x, y, pre, enc, B, dbytes.as<uint8_t>(), s))) return st;
        HIP_TRY(hipMemcpyAsync(odata.p, dbytes.p, B * pre * POS_DB, hipMemcpyDeviceToHost, s));
      }
    }
    // column-digest chunks of the repaired columns' rows (the writer's chunk machinery)
    if (digests_out && n_bad)
      HIP_TRY(leaf_chunk_cvs(fid, vals.as<uint32_t>(), r0, rows, n_bad, n_bad, c_lo, c_hi,
                             dcv.as<uint32_t>() + c_lo * n_bad * 8, s, true));
    // the next batch's rows gather on the host while this one runs
    if (c_hi < n_chunks) stage((k + 1) & 1, batches.at(c_hi));
    HIP_TRY(hipStreamSynchronize(s));
    // (the repaired columns are an image of n_bad columns, `rows` rows each)
    if (cols_out && n_bad) scatter_slices(cols_out, rows, 0, n_bad, r0, B, B * POS_WB, ocols.b());
    if (B && data_out) par_memcpy(data_out + r0 * pre * POS_DB, odata.b(), B * pre * POS_DB);
  }
  uint32_t flags[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&flags[0], c.flag.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&flags[1], dbad.p, 4, hipMemcpyDeviceToHost, s));
  if (digests_out && n_bad) {
    DBuf leaves;
    HIP_TRY(leaves.alloc(dev, n_bad * 32));
    HIP_TRY(leaves_from_cvs(dcv.as<uint32_t>(), n_bad, (int)n_chunks, leaves.as<uint8_t>(), s));
    HIP_TRY(hipMemcpyAsync(digests_out, leaves.p, n_bad * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (flags[1])
    return fail(LCPC_ERR_UNRECOVERABLE, "a column not listed as damaged holds a non-canonical element");
  if (flags[0])
    return fail(LCPC_ERR_UNRECOVERABLE, "a row is not a codeword on the columns not listed as damaged (degree check failed)");
  return LCPC_OK;
}

}  // extern "C"

// ================================================================= R-S error location by syndromes
// No counterpart in the reference.  The erasure decoder above needs to be told where the damage is;
// here the rows say it themselves: the coefficients its degree check tests for zero are power sums
// of the wrong positions, Berlekamp-Massey finds their shortest recurrence and one forward
// transform of its connection polynomial has its zeros at the wrong positions.  Kernels: rs_locate.hip.
namespace {

// Per-call device state of the locator, for batches of at most bmax rows.
struct LocateCtx {
  size_t bmax = 0, n_synd = 0;
  DBuf flag, dirty, bm_len, n_zero, on_erased, dstatus, mask, status, nerr, col_any, coef;
  std::vector<uint8_t> hflag;
  std::vector<uint32_t> hdirty;  // the batch's rows with a non-zero syndrome, ascending
};

lcpc_status locate_ctx_init(LocateCtx &lc, const ErasureCtx &c, Device *dev, size_t bmax) {
  lc.bmax = bmax;
  lc.n_synd = c.n - c.deg_bound;
  const size_t wb = (size_t)field_bytes(c.fid);
  HIP_TRY(lc.flag.alloc(dev, bmax));
  HIP_TRY(lc.dirty.alloc(dev, bmax * 4));
  HIP_TRY(lc.bm_len.alloc(dev, bmax * 4));
  HIP_TRY(lc.n_zero.alloc(dev, bmax * 4));
  HIP_TRY(lc.on_erased.alloc(dev, bmax * 4));
  HIP_TRY(lc.dstatus.alloc(dev, bmax));
  HIP_TRY(lc.status.alloc(dev, bmax));
  HIP_TRY(lc.nerr.alloc(dev, bmax * 4));
  HIP_TRY(lc.col_any.alloc(dev, c.n));
  HIP_TRY(hipMemsetAsync(lc.col_any.p, 0, c.n, c.s));
  if (lc.n_synd) {
    HIP_TRY(lc.mask.alloc(dev, bmax * c.n));
    HIP_TRY(lc.coef.alloc(dev, bmax * c.n * wb));
  }
  lc.hflag.assign(bmax, 0);
  return LCPC_OK;
}

// g: B masked rows in the inverse plan's input order; h: B rows of room.  Queues the inverse
// transform, the syndrome scan and the copy of the row flags to lc.hflag; the caller drains the
// stream before locate_dirty.
lcpc_status locate_scan(ErasureCtx &c, LocateCtx &lc, uint32_t *g, uint32_t *h, size_t B) {
  HIP_TRY(hipMemsetAsync(lc.status.p, 0, B, c.s));
  HIP_TRY(hipMemsetAsync(lc.nerr.p, 0, B * 4, c.s));
  if (!lc.n_synd) return LCPC_OK;
  HIP_TRY(hipMemsetAsync(lc.flag.p, 0, B, c.s));
  HIP_TRY(ntt_rows(c.inv, g, c.n, c.n, h, c.n, B, c.s));
  HIP_TRY(rs_locate_scan(c.fid, h, c.log_n, B, c.deg_bound, lc.flag.as<uint8_t>(), c.s));
  HIP_TRY(hipMemcpyAsync(lc.hflag.data(), lc.flag.p, B, hipMemcpyDeviceToHost, c.s));
  return LCPC_OK;
}

// After locate_scan and a drained stream: the flagged rows go through gather, Berlekamp-Massey, the
// root transform and the zero scan (g and h are clobbered).  On return the stream is drained,
// lc.hdirty lists the flagged rows, lc.status / lc.nerr hold the batch's verdicts, lc.mask[d] the
// located positions of row lc.hdirty[d], and lc.col_any has accumulated them.
lcpc_status locate_dirty(ErasureCtx &c, LocateCtx &lc, uint32_t *g, uint32_t *h, size_t B) {
  lc.hdirty.clear();
  if (!lc.n_synd) return LCPC_OK;
  for (size_t r = 0; r < B; r++)
    if (lc.hflag[r]) lc.hdirty.push_back((uint32_t)r);
  const size_t nd = lc.hdirty.size();
  if (!nd) return LCPC_OK;  // codewords: nothing more to pay
  HIP_TRY(hipMemcpyAsync(lc.dirty.p, lc.hdirty.data(), nd * 4, hipMemcpyHostToDevice, c.s));
  HIP_TRY(rs_locate_gather(c.fid, h, c.log_n, lc.dirty.as<uint32_t>(), nd, c.deg_bound, lc.n_synd, g, c.s));
  HIP_TRY(rs_locate_bm(c.fid, g, nd, lc.n_synd, c.log_n, lc.coef.as<uint32_t>(), lc.bm_len.as<uint32_t>(), c.s));
  {
    prof::Scope ps("rs_locate_root_ntt", c.s);
    HIP_TRY(ntt_rows(c.fwd, lc.coef.as<uint32_t>(), c.n, c.n, h, c.n, nd, c.s));
  }
  HIP_TRY(rs_locate_zeros(c.fid, h, c.log_n, nd, c.slot.as<int32_t>(), lc.mask.as<uint8_t>(),
                          lc.n_zero.as<uint32_t>(), lc.on_erased.as<uint32_t>(), c.s));
  HIP_TRY(rs_locate_finish(lc.dirty.as<uint32_t>(), nd, c.log_n, lc.bm_len.as<uint32_t>(), lc.n_zero.as<uint32_t>(),
                           lc.on_erased.as<uint32_t>(), lc.dstatus.as<uint8_t>(), lc.mask.as<uint8_t>(),
                           lc.status.as<uint8_t>(), lc.nerr.as<uint32_t>(), lc.col_any.as<uint8_t>(), c.s));
  HIP_TRY(hipStreamSynchronize(c.s));
  return LCPC_OK;
}

// lcpc_rs_locate_errors_rows after its argument checks; every output may be null
lcpc_status locate_rows(Device *dev, hipStream_t s, int f, const uint64_t *rows, size_t n_rows, size_t len,
                        size_t n_per_row, const std::vector<uint32_t> &e32, uint8_t *row_status,
                        uint32_t *row_n_errors, uint8_t *err_mask, uint8_t *col_any) {
  lcpc_status st;
  const size_t wb = (size_t)field_bytes(f), nl = wb / 8;
  ErasureCtx c;
  if ((st = erasure_ctx_init(c, dev, s, f, len, n_per_row, e32))) return st;
  const size_t bmax = std::max<size_t>(1, std::min(n_rows, ((size_t)16 << 20) / (len * wb)));
  LocateCtx lc;
  if ((st = locate_ctx_init(lc, c, dev, bmax))) return st;
  DBuf a, g, h;
  HIP_TRY(a.alloc(dev, bmax * len * wb));
  HIP_TRY(g.alloc(dev, bmax * len * wb));
  HIP_TRY(h.alloc(dev, bmax * len * wb));
  std::vector<uint8_t> hmask;
  for (size_t r0 = 0; r0 < n_rows; r0 += bmax) {
    const size_t B = std::min(bmax, n_rows - r0);
    HIP_TRY(hipMemcpyAsync(a.p, rows + r0 * len * nl, B * len * wb, hipMemcpyHostToDevice, s));
    HIP_TRY(erasure_masked_rows(f, a.as<uint32_t>(), g.as<uint32_t>(), c.log_n, B, c.slot.as<int32_t>(),
                                c.lambda.as<uint32_t>(), s));
    if ((st = locate_scan(c, lc, g.as<uint32_t>(), h.as<uint32_t>(), B))) return st;
    HIP_TRY(hipStreamSynchronize(s));
    if ((st = locate_dirty(c, lc, g.as<uint32_t>(), h.as<uint32_t>(), B))) return st;
    const size_t nd = lc.hdirty.size();
    if (row_status) HIP_TRY(hipMemcpyAsync(row_status + r0, lc.status.p, B, hipMemcpyDeviceToHost, s));
    if (row_n_errors) HIP_TRY(hipMemcpyAsync(row_n_errors + r0, lc.nerr.p, B * 4, hipMemcpyDeviceToHost, s));
    if (err_mask) {
      std::memset(err_mask + r0 * len, 0, B * len);
      if (nd) {
        hmask.resize(nd * len);
        HIP_TRY(hipMemcpyAsync(hmask.data(), lc.mask.p, nd * len, hipMemcpyDeviceToHost, s));
      }
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (err_mask)
      for (size_t d = 0; d < nd; d++) std::memcpy(err_mask + (r0 + lc.hdirty[d]) * len, hmask.data() + d * len, len);
  }
  if (col_any) HIP_TRY(hipMemcpyAsync(col_any, lc.col_any.p, len, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

lcpc_status locate_args(lcpc_field f, const void *rows, size_t n_rows, size_t len, size_t n_per_row,
                        const uint64_t *erased, size_t n_erased, std::vector<uint32_t> &e32) {
  if (!valid_field(f) || (!rows && n_rows)) return fail(LCPC_ERR_INVALID_ARG, "arguments");
  if (!field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field has no gfx950 kernels");
  lcpc_status st = check_fft_len(f, len);
  if (st) return st;
  return erasure_check(len, n_per_row, erased, n_erased, e32);
}

// One pass of lcpc_pos_locate_porenc over the image with the columns e32 never read.  col_any[c] = 1
// where a row located a wrong element; *noncanon = 1 if a column that was read holds an element
// that is not < p (the verdicts are then void: such elements were taken as zero).
lcpc_status pos_locate_pass(Device *dev, hipStream_t s, const uint8_t *porenc, size_t pre, size_t enc, size_t rows,
                            size_t row_capacity, const std::vector<uint32_t> &e32, uint8_t *col_any, size_t *n_dirty,
                            size_t *n_unlocatable, uint32_t *noncanon) {
  lcpc_status st;
  const int fid = POS_FID;
  ErasureCtx c;
  if ((st = erasure_ctx_init(c, dev, s, fid, enc, pre, e32))) return st;
  std::vector<uint8_t> is_bad(enc, 0);
  for (uint32_t j : e32) is_bad[j] = 1;
  // batches of whole BLAKE3 chunks of the column messages, as lcpc_pos_repair_columns
  const size_t n_chunks = leaf_n_chunks(fid, rows);
  const ChunkBatches batches = repair_batches(rows, n_chunks, enc, pos_stage_bytes());
  const size_t bmax = batches.max_rows();
  LocateCtx lc;
  if ((st = locate_ctx_init(lc, c, dev, bmax))) return st;
  DBuf src, g, h, dbad;
  HIP_TRY(src.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(g.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(h.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(dbad.alloc(dev, 8));
  HIP_TRY(hipMemsetAsync(dbad.p, 0, 8, s));
  Pinned stg[2];
  for (auto &x : stg)
    if (!x.get(dev, bmax * enc * POS_WB)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  // the known columns are never read, neither here nor by the kernels
  const ImageSrc img{porenc, -1, row_capacity, is_bad.data()};
  auto stage = [&](int slot, const ChunkBatches::Batch &b) {
    gather_slices(img, 0, enc, b.r0, b.B, b.B * POS_WB, stg[slot].b());
  };
  std::vector<uint8_t> hstatus(bmax);
  size_t nd_total = 0, nu_total = 0;
  stage(0, batches.at(0));
  int k = 0;
  for (size_t c_lo = 0, c_hi = 0; c_lo < n_chunks; c_lo = c_hi, k++) {
    const auto [r0, B, next] = batches.at(c_lo);
    c_hi = next;
    const int slot = k & 1;
    if (B) {
      HIP_TRY(hipMemcpyAsync(src.p, stg[slot].p, enc * B * POS_WB, hipMemcpyHostToDevice, s));
      HIP_TRY(erasure_masked_cols(fid, src.as<uint32_t>(), B, c.log_n, g.as<uint32_t>(), nullptr,
                                  c.slot.as<int32_t>(), c.lambda.as<uint32_t>(), dbad.as<uint32_t>(), s));
      if ((st = locate_scan(c, lc, g.as<uint32_t>(), h.as<uint32_t>(), B))) return st;
    }
    // the next batch's rows gather on the host while this one runs
    if (c_hi < n_chunks) stage((k + 1) & 1, batches.at(c_hi));
    HIP_TRY(hipStreamSynchronize(s));
    if (!B) continue;
    if ((st = locate_dirty(c, lc, g.as<uint32_t>(), h.as<uint32_t>(), B))) return st;
    if (!lc.hdirty.empty()) {
      HIP_TRY(hipMemcpyAsync(hstatus.data(), lc.status.p, B, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      nd_total += lc.hdirty.size();
      for (uint32_t r : lc.hdirty) nu_total += hstatus[r] == 2;
    }
  }
  HIP_TRY(hipMemcpyAsync(noncanon, dbad.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(col_any, lc.col_any.p, enc, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_dirty = nd_total;
  *n_unlocatable = nu_total;
  return LCPC_OK;
}

// col_bad[c] = 1 for the columns not in `skip` that hold an element that is not < p
lcpc_status pos_noncanonical_columns(Device *dev, hipStream_t s, const uint8_t *porenc, size_t enc, size_t rows,
                                     size_t row_capacity, const std::vector<uint8_t> &skip,
                                     std::vector<uint32_t> &col_bad) {
  col_bad.assign(enc, 0);
  if (!rows) return LCPC_OK;
  DBuf dbad;
  HIP_TRY(dbad.alloc(dev, enc * 4));
  HIP_TRY(hipMemsetAsync(dbad.p, 0, enc * 4, s));
  const ImageSrc img{porenc, -1, row_capacity, skip.data(), true};  // never read: zeros are canonical
  const size_t cpb = column_block_cols(enc, rows * POS_WB, pos_stage_bytes());
  lcpc_status st = for_column_blocks(dev, s, img, enc, cpb, 0, rows, rows,
                                     [&](uint32_t *d_cols, size_t c0, size_t nc, int) -> lcpc_status {
                                       HIP_TRY(scrub_col_canon(POS_FID, d_cols, rows, nc, dbad.as<uint32_t>() + c0, s));
                                       return LCPC_OK;
                                     });
  if (st) return st;
  HIP_TRY(hipMemcpyAsync(col_bad.data(), dbad.p, enc * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

}  // namespace

extern "C" {

size_t lcpc_rs_locate_max_errors(lcpc_field f) { return valid_field(f) ? rs_locate_cap(f) : 0; }

lcpc_status lcpc_rs_locate_errors_rows(lcpc_field f, const uint64_t *rows, size_t n_rows, size_t len, size_t n_per_row,
                                       const uint64_t *erased, size_t n_erased, uint8_t *row_status,
                                       uint32_t *row_n_errors, uint8_t *err_mask, uint8_t *col_any) {
  std::vector<uint32_t> e32;
  lcpc_status st = locate_args(f, rows, n_rows, len, n_per_row, erased, n_erased, e32);
  if (st) return st;
  if (!row_status && n_rows) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (n_rows == 0) {
    if (col_any) std::memset(col_any, 0, len);
    return LCPC_OK;
  }
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  return locate_rows(dev, lease.s, f, rows, n_rows, len, n_per_row, e32, row_status, row_n_errors, err_mask, col_any);
}

lcpc_status lcpc_rs_decode_rows(lcpc_field f, uint64_t *rows, size_t n_rows, size_t len, size_t n_per_row,
                                const uint64_t *erased, size_t n_erased, uint8_t *row_status) {
  std::vector<uint32_t> e32;
  lcpc_status st = locate_args(f, rows, n_rows, len, n_per_row, erased, n_erased, e32);
  if (st) return st;
  if (n_rows == 0) return LCPC_OK;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const size_t wb = (size_t)field_bytes(f), nl = wb / 8;
  std::vector<uint8_t> status(n_rows), mask(n_rows * len);
  if ((st = locate_rows(dev, s, f, rows, n_rows, len, n_per_row, e32, status.data(), nullptr, mask.data(), nullptr)))
    return st;
  if (row_status) std::memcpy(row_status, status.data(), n_rows);
  for (size_t r = 0; r < n_rows; r++)
    if (status[r] == 2)
      return fail(LCPC_ERR_UNRECOVERABLE, "a row has more wrong positions than can be located (row " +
                                              std::to_string(r) + ")");
  // Erasure decoding with the known and the located positions as the erasure set: the same codeword,
  // which any n_per_row positions fix.  Consecutive rows share a set while its size fits the code's
  // redundancy; a row alone always fits (n_erased + its errors <= n_erased + (len - n_per_row - n_erased) / 2).
  struct Write {
    size_t r, pos;
    size_t val;  // index of the value's first limb in `vals`
  };
  std::vector<Write> writes;
  std::vector<uint64_t> vals, filled;
  const size_t room = len - n_per_row;
  std::vector<uint8_t> in_union(len);
  size_t lo = 0;
  while (lo < n_rows) {
    std::fill(in_union.begin(), in_union.end(), 0);
    for (uint32_t j : e32) in_union[j] = 1;
    size_t count = n_erased, hi = lo;
    std::vector<uint32_t> set = e32;
    for (; hi < n_rows; hi++) {
      const uint8_t *m = mask.data() + hi * len;
      size_t extra = 0;
      for (size_t p = 0; p < len; p++) extra += m[p] && !in_union[p];
      if (hi > lo && count + extra > room) break;
      for (size_t p = 0; p < len; p++)
        if (m[p] && !in_union[p]) {
          in_union[p] = 1;
          set.push_back((uint32_t)p);
        }
      count += extra;
    }
    if ((st = erasure_decode_values(dev, s, f, rows + lo * len * nl, hi - lo, len, n_per_row, set, filled))) return st;
    for (size_t r = lo; r < hi; r++)
      for (size_t j = 0; j < set.size(); j++)
        if (j < n_erased || mask[r * len + set[j]]) {
          writes.push_back({r, set[j], vals.size()});
          const uint64_t *v = filled.data() + ((r - lo) * set.size() + j) * nl;
          vals.insert(vals.end(), v, v + nl);
        }
    lo = hi;
  }
  // nothing was written so far: only the located and the erased positions are, every other limb keeps its bits
  for (const Write &w : writes) std::memcpy(rows + (w.r * len + w.pos) * nl, vals.data() + w.val, wb);
  return LCPC_OK;
}

lcpc_status lcpc_pos_locate_porenc(const uint8_t *porenc, size_t pre, size_t enc, size_t rows_written,
                                   size_t row_capacity, const uint64_t *known_bad, size_t n_known, uint8_t *col_status,
                                   size_t *n_bad_cols, size_t *n_dirty_rows, size_t *n_unlocatable_rows) {
  lcpc_status st = pos_dims_check(pre, enc);
  if (st) return st;
  if (rows_written > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "rows_written > row_capacity");
  if (!col_status || (!porenc && rows_written)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  std::vector<uint32_t> e32;
  if ((st = erasure_check(enc, pre, known_bad, n_known, e32))) return st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  std::vector<uint8_t> col_any(enc, 0), is_known(enc, 0), is_noncanon(enc, 0);
  for (uint32_t j : e32) is_known[j] = 1;
  size_t n_dirty = 0, n_unloc = 0;
  if (rows_written) {
    // optimistic: the masked load's flag says whether any column it read is non-canonical; only then
    // the image is scanned to name those columns, which join the erasure set for a second pass
    uint32_t noncanon = 0;
    if ((st = pos_locate_pass(dev, s, porenc, pre, enc, rows_written, row_capacity, e32, col_any.data(), &n_dirty,
                              &n_unloc, &noncanon)))
      return st;
    if (noncanon) {
      std::vector<uint32_t> col_bad;
      if ((st = pos_noncanonical_columns(dev, s, porenc, enc, rows_written, row_capacity, is_known, col_bad)))
        return st;
      for (size_t c = 0; c < enc; c++)
        if (col_bad[c] && !is_known[c]) {
          is_noncanon[c] = 1;
          e32.push_back((uint32_t)c);
        }
      if (e32.size() > enc - pre)
        return fail(LCPC_ERR_UNRECOVERABLE, "more known and non-canonical columns than the code's redundancy (enc - pre)");
      if ((st = pos_locate_pass(dev, s, porenc, pre, enc, rows_written, row_capacity, e32, col_any.data(), &n_dirty,
                                &n_unloc, &noncanon)))
        return st;
    }
  }
  size_t n_bad = 0;
  for (size_t c = 0; c < enc; c++) {
    col_status[c] = is_known[c] ? 3 : is_noncanon[c] ? 2 : col_any[c] ? 1 : 0;
    n_bad += col_status[c] != 0;
  }
  if (n_bad_cols) *n_bad_cols = n_bad;
  if (n_dirty_rows) *n_dirty_rows = n_dirty;
  if (n_unlocatable_rows) *n_unlocatable_rows = n_unloc;
  return LCPC_OK;
}

}  // extern "C"
