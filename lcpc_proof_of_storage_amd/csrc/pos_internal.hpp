// pos_internal.hpp -- what the proof-of-storage host units share (lcpc_host.cpp, pos_files_host.cpp,
// pos_repair_host.cpp, pos_group_host.cpp, pos_verify_group_host.cpp, pos_ingest_host.cpp, pos_scrub_host.cpp, pos_repair_group_host.cpp): constants, page-locked staging, argument checks and the device-side steps
// that more than one entry point runs.  The image's host side is pos_image.hpp; the arithmetic of an
// image's rows and chunks and the planning of the grouped ingest, scrub and repair are
// pos_rowgroup_plan.hpp (host only), their two-slot staging pos_rowgroup_stage.hpp.  Stateless, inline.
#pragma once
#include "host_internal.hpp"
#include "pos_image.hpp"
#include "pos_rowgroup_plan.hpp"

namespace lcpc_host {

// an R-S (Ligero) encoding of the current device; defined in lcpc_host.cpp
__attribute__((visibility("hidden"))) lcpc_status make_rs_encoding(int fid, size_t n_per_row, size_t n_cols, size_t nco, size_t ndt, lcpc_encoding **out);

constexpr int POS_FID = LCPC_FT63;  // WriteableFt63: Ft63's modulus (writable_ft63.rs:8-12)

// Encoded bytes per pipelined batch or column block: 256 MiB.  LCPC_POS_STAGE_BYTES (a test seam,
// read at every call) can only lower it; zero or an unparsable value is ignored.
inline size_t pos_stage_bytes() {
  constexpr size_t budget = (size_t)256 << 20;
  if (const char *env = std::getenv("LCPC_POS_STAGE_BYTES")) {
    const unsigned long long v = std::strtoull(env, nullptr, 10);
    if (v) return std::min<size_t>(budget, (size_t)v);
  }
  return budget;
}

// Bytes per staging group of the grouped stored-file entries (pos_group_host.cpp: image bytes;
// pos_verify_group_host.cpp: column bytes).  LCPC_POS_GROUP_BYTES (a test seam, read at every call)
// can only lower it; zero or an unparsable value is ignored.
inline size_t pos_group_bytes() {
  if (const char *env = std::getenv("LCPC_POS_GROUP_BYTES")) {
    const unsigned long long v = std::strtoull(env, nullptr, 10);
    if (v) return std::min<size_t>(LCPC_POS_GROUP_STAGE_BYTES, (size_t)v);
  }
  return LCPC_POS_GROUP_STAGE_BYTES;
}

// a page-locked block from the device's pool, returned at scope exit
struct Pinned {
  Device *d = nullptr;
  void *p = nullptr;
  size_t n = 0;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  ~Pinned() { reset(); }
  void reset() {
    if (d && p) d->pinned_put(p);
    p = nullptr;
    n = 0;
  }
  bool get(Device *dev, size_t bytes) {
    reset();
    d = dev;
    p = dev->pinned_get(bytes);
    n = p ? bytes : 0;
    return p != nullptr;
  }
  uint8_t *b() const { return (uint8_t *)p; }
};

// the events of two staging slots, destroyed at scope exit
struct Events {
  hipEvent_t e[2] = {nullptr, nullptr};
  ~Events() {
    for (auto &x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipError_t init() {
    for (auto &x : e)
      if (!x) {
        hipError_t r = hipEventCreateWithFlags(&x, hipEventDisableTiming);
        if (r != hipSuccess) return r;
      }
    return hipSuccess;
  }
  // before step k refills slot k & 1: what step k - 2 recorded on it has completed
  hipError_t reuse(int k) const { return k >= 2 ? hipEventSynchronize(e[k & 1]) : hipSuccess; }
};

// a device buffer that only grows, in steps of `granule`: at least `bytes` of it after this
inline lcpc_status ensure(DBuf &b, Device *dev, size_t bytes, size_t granule) {
  if (b.n < bytes || !b.p) HIP_TRY(b.alloc(dev, align_up(bytes, granule)));
  return LCPC_OK;
}

inline lcpc_status pos_dims_check(size_t pre, size_t enc) {
  // EncodedFileWriter::convert_unencoded_file / new (encoded_file_writer.rs:53-67, 146-163)
  if (pre < 1) return fail(LCPC_ERR_INVALID_ARG, "Number of pre-encoded columns must be greater than 0");
  if (enc < 2 || (enc & (enc - 1)))
    return fail(LCPC_ERR_INVALID_ARG, "Number of encoded columns must be a power of 2 (>= 2)");
  if (enc <= pre)
    return fail(LCPC_ERR_INVALID_ARG, "Number of encoded columns must be greater than the number of columns");
  if ((int)log2_np2(enc) > field_info(POS_FID).s) return fail(LCPC_FFT_TOO_BIG, "FFTError::TooBig");
  return LCPC_OK;
}
// the same for every job of a queue, the first failure returned
inline lcpc_status pos_dims_check(const size_t *pre, const size_t *enc, size_t n_jobs) {
  for (size_t j = 0; j < n_jobs; j++)
    if (lcpc_status st = pos_dims_check(pre[j], enc[j])) return st;
  return LCPC_OK;
}

// n^-1 mod p for n = 2^log_n | p - 1, canonical: p - (p - 1) / n
inline void inv_pow2_canon(int fid, int log_n, uint32_t *words) {
  const FieldInfo fi = field_info(fid);
  uint64_t q[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
  for (int i = 0; i < fi.limbs; i++) q[i] = fi.p[i];
  q[0] -= 1;  // p odd: no borrow
  for (int k = 0; k < log_n; k++) {  // q >>= 1 (multi-limb)
    for (int i = 0; i < fi.limbs; i++) {
      q[i] >>= 1;
      if (i + 1 < fi.limbs) q[i] |= q[i + 1] << 63;
    }
  }
  uint64_t br = 0;
  for (int i = 0; i < fi.limbs; i++) {
    const uint64_t a = fi.p[i], b = q[i];
    const uint64_t d = a - b - br;
    br = (a < b) || (a - b < br);
    r[i] = d;
  }
  for (int i = 0; i < fi.limbs; i++) {
    words[2 * i] = (uint32_t)r[i];
    words[2 * i + 1] = (uint32_t)(r[i] >> 32);
  }
}

inline lcpc_status check_fft_len(int fid, size_t len) {
  if (len == 0 || (len & (len - 1))) return fail(LCPC_FFT_NOT_POWER_OF_TWO, "FFTError::NotPowerOfTwo");
  if ((int)log2_np2(len) > field_info(fid).s) return fail(LCPC_FFT_TOO_BIG, "FFTError::TooBig");
  return LCPC_OK;
}

// The device flag "an element read from the image is not < p" (raw_bytes_to_field_vec:
// from_repr(..).unwrap(), data_field.rs:72-81); verdict() once the read-back's stream has drained.
struct BadFlag {
  DBuf d;
  uint32_t host = 0;
  lcpc_status init(Device *dev, hipStream_t s) {
    HIP_TRY(d.alloc(dev, 4));
    HIP_TRY(hipMemsetAsync(d.p, 0, 4, s));
    return LCPC_OK;
  }
  uint32_t *p() const { return d.as<uint32_t>(); }
  lcpc_status read_back(hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(&host, d.p, 4, hipMemcpyDeviceToHost, s));
    return LCPC_OK;
  }
  lcpc_status verdict() const {
    if (host) return fail(LCPC_ERR_INVALID_ARG, "encoded file holds a non-canonical element (from_repr fails)");
    return LCPC_OK;
  }
};

// An inverse NTT plan for one call: freed at scope exit, once the stream that used it has drained.
struct InversePlan {
  NttPlan plan;
  hipStream_t s = nullptr;
  ~InversePlan() {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    ntt_plan_free(plan);
  }
  lcpc_status init(int fid, int log_n, hipStream_t stream) {
    const hipError_t he = ntt_plan_init(plan, fid, log_n, true, stream);
    if (he != hipSuccess) {
      ntt_plan_free(plan);
      if (he == hipErrorInvalidValue) return fail(LCPC_ERR_UNSUPPORTED, "length beyond the NTT range");
      HIP_TRY(he);
    }
    s = stream;
    return LCPC_OK;
  }
};

// fffft::ifft_oi (decode_row, lcpc_online.rs:568-574) on B rows of 2^log_n elements in x: the
// evaluations reordered to natural order (bit-reversed ones: include/lcpc_fft_convention.h), DIF
// with the inverse root, bit-reversed back and scaled by 2^-log_n.  x and y (as large) are both
// clobbered; *res is the one that holds the coefficients, *spare the other.
inline lcpc_status ifft_oi_device(const NttPlan &inverse, int fid, int log_n, uint32_t *x, uint32_t *y, size_t B,
                                  hipStream_t s, uint32_t **res, uint32_t **spare) {
  const size_t len = (size_t)1 << log_n;
  uint32_t inv[8] = {0};
  inv_pow2_canon(fid, log_n, inv);
  if (LCPC_FFT_OUTPUT_BITREV) {
    HIP_TRY(bitrev_scale(fid, x, y, log_n, B, nullptr, s));
    std::swap(x, y);
  }
  HIP_TRY(ntt_rows(inverse, x, len, len, y, len, B, s));
  HIP_TRY(bitrev_scale(fid, y, x, log_n, B, inv, s));
  *res = x;
  *spare = y;
  return LCPC_OK;
}

// decoded_row.drain(pre..) then field_vec_to_byte_vec: the first pre coefficients of B decoded rows
// of enc elements (res), 7 data bytes each, into d_bytes; spare (B * pre elements of room) is clobbered.
inline lcpc_status decode_rows_to_bytes(const uint32_t *res, uint32_t *spare, size_t pre, size_t enc, size_t B,
                                        uint8_t *d_bytes, hipStream_t s) {
  HIP_TRY(hipMemcpy2DAsync(spare, pre * POS_WB, res, enc * POS_WB, pre * POS_WB, B, hipMemcpyDeviceToDevice, s));
  HIP_TRY(pos_unpack7(reinterpret_cast<const uint64_t *>(spare), B * pre, d_bytes, B * pre * POS_DB, s));
  return LCPC_OK;
}

// B rows of pre elements from n_bytes host data bytes (7 per element, the last row may be short:
// zero-padded), Ligero-encoded to enc canonical elements per row in comm -- the file's repr words
// and the leaves' input without conversion -- and, with dout, transposed to the image's [enc][B].
inline lcpc_status pack_encode_batch(const lcpc_encoding *e, const uint8_t *bytes, size_t n_bytes, size_t B,
                                     DBuf &dbytes, DBuf &coeffs, DBuf &comm, DBuf *dout, hipStream_t s) {
  const size_t pre = e->n_per_row, enc = e->n_cols;
  const size_t ne = (n_bytes + POS_DB - 1) / POS_DB;
  HIP_TRY(hipMemcpyAsync(dbytes.p, bytes, n_bytes, hipMemcpyHostToDevice, s));
  if (B * pre > ne) HIP_TRY(hipMemsetAsync(coeffs.as<uint8_t>() + ne * POS_WB, 0, (B * pre - ne) * POS_WB, s));
  HIP_TRY(pos_pack7(dbytes.as<uint8_t>(), n_bytes, coeffs.as<uint64_t>(), s));
  HIP_TRY(ntt_rows(e->plan, coeffs.as<uint32_t>(), pre, pre, comm.as<uint32_t>(), enc, B, s, nullptr, 0, true));
  if (dout) HIP_TRY(transpose_elems(e->fid, comm.as<uint32_t>(), B, enc, enc, enc, dout->as<uint32_t>(), B, s));
  return LCPC_OK;
}

// Rows [r0, r0 + R) of every column of the image, a block of cpb (column_block_cols) columns at a
// time: fn(d_cols, c0, nc, slot) gets the columns [c0, c0 + nc) in device memory, col_elems (>= R)
// elements apart, and queues its kernels on s.  Two page-locked and two device blocks alternate
// (slot): the host gather of a block overlaps the upload and kernels of the one before.  With no
// rows fn is still called, once.  On return the staging is free; the kernels may still be queued.
// (The host phases keep the names they had when only the chunk cache had them.)
template <class Fn>
lcpc_status for_column_blocks(Device *dev, hipStream_t s, const ImageSrc &img, size_t enc, size_t cpb, size_t r0,
                              size_t R, size_t col_elems, Fn fn) {
  const size_t col_bytes = col_elems * POS_WB;
  DBuf dcols[2];
  Pinned stg[2];
  Events ev;
  HIP_TRY(ev.init());
  for (int i = 0; i < 2; i++) {
    HIP_TRY(dcols[i].alloc(dev, cpb * col_bytes));
    if (col_bytes && !stg[i].get(dev, cpb * col_bytes)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  }
  const int rc = for_blocks(enc, cpb, [&](size_t c0, size_t nc, int k) -> int {
    const int slot = k & 1;
    if (col_bytes) {
      HIP_TRY(ev.reuse(k));
      const bool whole = [&] {
        prof::HostScope hs("cache_image_read");
        return gather_slices(img, c0, nc, r0, R, col_bytes, stg[slot].b());
      }();
      if (!whole) {
        (void)hipStreamSynchronize(s);  // the other slot's upload may still be reading its staging
        return fail(LCPC_ERR_INVALID_ARG, "encoded file shorter than row_capacity * encoded_size elements");
      }
      prof::Scope ps("cache_h2d", s);
      HIP_TRY(hipMemcpyAsync(dcols[slot].p, stg[slot].p, nc * col_bytes, hipMemcpyHostToDevice, s));
      HIP_TRY(hipEventRecord(ev.e[slot], s));
    }
    return fn(dcols[slot].as<uint32_t>(), c0, nc, slot);
  });
  if (rc) return (lcpc_status)rc;
  // the page-locked blocks go back to the pool: the last uploads (if any) must have left them
  for (hipEvent_t e : ev.e) HIP_TRY(hipEventSynchronize(e));
  return LCPC_OK;
}

}  // namespace lcpc_host

// The column chunk-CV cache of a stored file (pos_files_host.cpp keeps it up to date;
// pos_read_host.cpp reads it): [chunk][column] chaining values in device memory.
struct lcpc_pos_chunk_cache {
  lcpc_host::Device *dev = nullptr;
  size_t enc = 0, rows = 0, n_chunks = 0, cap_chunks = 0;
  lcpc_host::DBuf cvs;  // cap_chunks x enc x 32 B, the first n_chunks chunk rows valid
};
