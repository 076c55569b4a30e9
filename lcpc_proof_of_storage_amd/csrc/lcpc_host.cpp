// lcpc_host.cpp -- host orchestration and C ABI of liblcpc_mi.so (see include/lcpc_mi.h).
//
// The reference's lcpc-2d commit / prove / verify (lcpc-2d/src/lib.rs:651-1123) restated for
// one MI355X: every field operation and every hash runs in the gfx950 kernels (ntt*.hip,
// blake3.hip, collapse.hip); this file only sequences them, moves the proof-sized vectors
// across PCIe, and runs the inherently serial Fiat-Shamir steps (transcript.cpp).
// There is no CPU fallback: with no usable HIP device every compute entry point fails with
// LCPC_ERR_NO_DEVICE.
#include "pos_internal.hpp"

using namespace lcpc;
using namespace lcpc_host;

// ---------------------------------------------------------------- internal helpers
lcpc_status lcpc_host::make_rs_encoding(int fid, size_t n_per_row, size_t n_cols, size_t nco, size_t ndt,
                                        lcpc_encoding **out) {
  if (!out) return fail(LCPC_ERR_INVALID_ARG, "null out");
  if (!valid_field(fid)) return fail(LCPC_ERR_INVALID_ARG, "unknown field");
  if (!field_gpu_supported(fid)) return fail(LCPC_ERR_UNSUPPORTED, "field has no gfx950 kernels");
  // LigeroEncodingRho::_dims_ok (lib.rs:114-118) is asserted by new_from_dims
  if (!(n_per_row < n_cols) || !n_cols || (n_cols & (n_cols - 1)))
    return fail(LCPC_ERR_INVALID_ARG, "dims_ok failed: need n_per_row < n_cols, n_cols = 2^k");
  const int log_n = (int)log2_np2(n_cols);
  const FieldInfo fi = field_info(fid);
  if (log_n > fi.s) return fail(LCPC_FFT_TOO_BIG, "FFTError::TooBig: log2(n_cols) > S");
  lcpc_status st;
  Device *dev = get_device(g_device, &st);
  if (!dev) return st;
  auto e = std::make_unique<lcpc_encoding>();
  e->fid = fid;
  e->n_per_row = n_per_row;
  e->n_cols = n_cols;
  e->n_col_opens = nco;
  e->n_degree_tests = ndt;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipError_t he = ntt_plan_init(e->plan, fid, log_n, false, lease.s);
  if (he == hipErrorInvalidValue) return fail(LCPC_ERR_UNSUPPORTED, "n_cols beyond the supported NTT range");
  HIP_TRY(he);
  HIP_TRY(hipStreamSynchronize(lease.s));
  e->dev = dev;
  *out = e.release();
  return LCPC_OK;
}

namespace {
// SdigEncodingS::_new_from_np1 / new_from_dims (lcpc-brakedown-pc/src/lib.rs:69-137) with the
// n_per_row already chosen; want_cols = 0 accepts the generated codeword length.
lcpc_status make_sdig_encoding(int fid, int code, size_t n_per_row, size_t want_cols, uint64_t seed,
                               lcpc_encoding **out) {
  if (!out) return fail(LCPC_ERR_INVALID_ARG, "null out");
  if (!valid_field(fid)) return fail(LCPC_ERR_INVALID_ARG, "unknown field");
  if (!field_gpu_supported(fid)) return fail(LCPC_ERR_UNSUPPORTED, "field has no gfx950 kernels");
  const SdigSpec *sp = sdig_spec(code);
  if (!sp) return fail(LCPC_ERR_INVALID_ARG, "SDIG code id must be 1..6");
  if (!(n_per_row > sp->blen))  // matgen::get_dims asserts n > baselen
    return fail(LCPC_ERR_INVALID_ARG, "SDIG: n_per_row must exceed the code's base length");
  if (n_per_row > 0xffffffffu) return fail(LCPC_ERR_INVALID_ARG, "SDIG: n_per_row too large");
  lcpc_status st;
  Device *dev = get_device(g_device, &st);
  if (!dev) return st;
  const FieldInfo fi = field_info(fid);
  std::vector<CsrHost> pre, post;
  if (!sdig_generate(fi.limbs, fi.num_bits, fi.p, code, n_per_row, seed, pre, post))
    return fail(LCPC_ERR_INVALID_ARG, "SDIG: matrix generation failed");
  const size_t nc = sdig_codeword_length(pre, post);
  if (want_cols && want_cols != nc)  // new_from_dims asserts n_cols == codeword_length
    return fail(LCPC_ERR_INVALID_ARG, "SDIG: n_cols does not match the code's codeword length");
  auto e = std::make_unique<lcpc_encoding>();
  e->fid = fid;
  e->kind = KIND_SDIG;
  e->code = code;
  e->seed = seed;
  e->n_per_row = n_per_row;
  e->n_cols = nc;
  e->n_col_opens = sdig_n_col_opens(code);
  e->n_degree_tests = lcpc_n_degree_tests(128, nc, fi.num_bits - 1);
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  HIP_TRY(sdig_plan_upload(e->sdig, fid, pre, post, lease.s));
  e->dev = dev;
  *out = e.release();
  return LCPC_OK;
}

// upload block: about 8 MiB, whole rows of `row_bytes` (at least one)
inline size_t upload_block(size_t row_bytes) {
  const size_t target = (size_t)8 << 20;
  return std::max<size_t>(1, target / std::max<size_t>(row_bytes, 1)) * row_bytes;
}

// src_bytes != 0: d_src is a device proof-of-storage file image of src_bytes bytes, 7 per
// WriteableFt63 element (len = ceil(src_bytes / 7)), packed as DataField::from_byte_vec does
// (fields/data_field.rs:38-46) -- at the PoS default dims straight into the one-pass encode
// eval_left / eval_out (n_rows / n_cols elements, host): also u^T Enc(M) over the new codeword
// (lcpc_online.rs:454-484, as lcpc_pos_eval_encoded), fused into the leaf hashing's pass over
// the codeword where the leaf kernel can carry it (leaf_eval_fusable), else one more pass after it
lcpc_status commit_device(const lcpc_encoding *e, const void *d_src, bool src_is_host, size_t len,
                          lcpc_commit **out, size_t src_bytes = 0, const uint64_t *eval_left = nullptr,
                          uint64_t *eval_out = nullptr) {
  prof::HostScope hs_total("host_commit_total");
  if (!e || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (src_bytes || eval_left || eval_out) {
    lcpc_status st = require_blake3(e, "a proof-of-storage commitment");
    if (st) return st;
  }
  const size_t np = e->n_per_row, nc = e->n_cols;
  const size_t n_rows = (len + np - 1) / np;  // LcEncoding::get_dims
  // commit's assertions (lcpc-2d/src/lib.rs:659-661) -> invalid argument
  if (len == 0 || n_rows * np < len || (n_rows - 1) * np >= len)
    return fail(LCPC_ERR_INVALID_ARG, "commit: coefficient count incompatible with dims");
  if (encoding_dims_ok(e, np, nc) != LCPC_OK) return fail(LCPC_ERR_INVALID_ARG, "commit: dims_ok");
  const size_t np2 = next_pow2(nc);
  if (np2 == 0) return fail(LCPC_PROVER_TOO_BIG, "n_cols too large");
  Device *dev = e->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const int fid = e->fid, wb = field_bytes(fid);
  DBuf packed;  // bytes off the fused path: the element image (at function scope: no block-exit drain)
  DBuf image;   // a host file image's device copy
  const uint8_t *src_b = nullptr;
  bool host_image = false;  // src_b fills block by block from the host (encoded as blocks land)
  if (src_bytes) {
    if (fid != LCPC_FT63) return fail(LCPC_ERR_INVALID_ARG, "file image: WriteableFt63 only");
    const bool fuse = e->kind != KIND_SDIG && ntt_row1_bytes(e->plan) && ntt_rows_pos_bytes_ok(e->plan, np);
    if (src_is_host) {
      const size_t padded = (src_bytes + 15) / 16 * 16 + 16;
      HIP_TRY(image.alloc(dev, padded));
      // (only the padding past the file: the upload writes the rest on its own stream)
      HIP_TRY(hipMemsetAsync(image.as<uint8_t>() + src_bytes, 0, padded - src_bytes, s));
      if (fuse) {
        src_b = image.as<uint8_t>();
        host_image = true;
      } else {
        lcpc_status st = h2d_blocks(dev, image.as<uint8_t>(), (const uint8_t *)d_src, src_bytes, (size_t)8 << 20, s,
                                    [](size_t, size_t) { return LCPC_OK; });
        if (st) return st;
        d_src = image.p;
      }
      src_is_host = false;
    } else if (fuse && !((uintptr_t)d_src & 15)) {
      src_b = (const uint8_t *)d_src;
    }
    if (!src_b) {
      HIP_TRY(packed.alloc(dev, len * 8));
      HIP_TRY(pos_pack7((const uint8_t *)d_src, src_bytes, packed.as<uint64_t>(), s));
      d_src = packed.p;
    }
  }
  auto c = std::make_unique<lcpc_commit>();
  c->fid = fid;
  c->digest = e->digest;
  c->dev = dev;
  c->n_rows = n_rows;
  c->n_cols = nc;
  c->n_per_row = np;
  c->n_hashes = 2 * np2 - 1;
  // coeffs, zero padded to n_rows * n_per_row (:665, :669-674); comm row r = encode(coeffs
  // row r || zeros) (:677-682)
  HIP_TRY(c->coeffs.alloc(dev, n_rows * np * wb));
  HIP_TRY(c->comm.alloc(dev, n_rows * nc * wb));
  uint8_t *cf = c->coeffs.as<uint8_t>();
  uint8_t *cm = c->comm.as<uint8_t>();
  DBuf tmp;  // (SDIG scratch; at function scope, so that no block exit drains the stream)
  DBuf scratch;  // the leaf hashing's chunk chaining values
  const bool eval = eval_left && eval_out;
  int fused_chunks = 0;  // > 0: the encode's second pass left the leaf chunks' chaining values in scratch
  if (e->kind == KIND_SDIG) {
    // element-major codeword [n_cols][n_rows]: the message part is the coefficient matrix
    // transposed, the SDIG levels fill the rest, and each leaf is a contiguous column.  The
    // codeword is held canonical: the transpose writes canonical values, and every level is a
    // sum of Montgomery products by Montgomery constants (SpMM values, Reed-Solomon points), so
    // canonical inputs give canonical outputs -- the leaves then hash it without a per-element
    // conversion, as the Ligero codeword (opened columns convert back, as there)
    c->col_major = true;
    c->canon = true;
    if (src_is_host) {
      lcpc_status st = h2d_blocks(dev, cf, (const uint8_t *)d_src, len * wb, (size_t)8 << 20, s,
                                  [](size_t, size_t) { return LCPC_OK; });
      if (st) return st;
      if (n_rows * np > len) HIP_TRY(hipMemsetAsync(cf + len * wb, 0, (n_rows * np - len) * wb, s));
      HIP_TRY(transpose_elems(fid, (const uint32_t *)cf, n_rows, np, np, np, (uint32_t *)cm, n_rows, s,
                              TR_FROM_MONT));
    } else {
      // one pass over the caller's coefficients writes both the transposed message part and
      // the commitment's zero-padded row-major copy (no separate device-to-device copy)
      HIP_TRY(transpose_elems(fid, (const uint32_t *)d_src, n_rows, np, np, np, (uint32_t *)cm, n_rows, s,
                              TR_FROM_MONT, nullptr, len, (uint32_t *)cf, np));
    }
    HIP_TRY(tmp.alloc(dev, e->sdig.tmp_elems * n_rows * wb));
    HIP_TRY(sdig_encode_cm(e->sdig, (uint32_t *)cm, n_rows, tmp.as<uint32_t>(), s));
  } else if (src_is_host) {
    // the caller's rows land in the commitment's coefficient matrix block by block, each block's
    // rows encoded as soon as they are there (the copy of the next block overlaps)
    c->canon = true;
    const size_t row_b = np * wb, total = len * wb;
    lcpc_status st = h2d_blocks(dev, cf, (const uint8_t *)d_src, total, upload_block(row_b), s,
                                [&](size_t off, size_t n) -> lcpc_status {
      const bool last = off + n == total;
      const size_t r0 = off / row_b, r1 = last ? n_rows : (off + n) / row_b;
      if (last && n_rows * np > len) HIP_TRY(hipMemsetAsync(cf + total, 0, (n_rows * np - len) * wb, s));
      if (r1 > r0)
        HIP_TRY(ntt_rows(e->plan, (const uint32_t *)(cf + r0 * row_b), np, np, (uint32_t *)(cm + r0 * nc * wb), nc,
                         r1 - r0, s, nullptr, 0, true));
      return LCPC_OK;
    });
    if (st) return st;
  } else if (host_image) {
    // a host file image: uploaded block by block (whole rows of 7 n_per_row bytes), each block's
    // rows unpacked and encoded by the one-pass kernel as soon as they are there
    c->canon = true;
    const size_t row_b = 7 * np;
    lcpc_status st = h2d_blocks(dev, image.as<uint8_t>(), (const uint8_t *)d_src, src_bytes, upload_block(row_b), s,
                                [&](size_t off, size_t n) -> lcpc_status {
      const bool last = off + n == src_bytes;
      const size_t r0 = off / row_b, r1 = last ? n_rows : (off + n) / row_b;
      if (r1 > r0)
        HIP_TRY(ntt_rows_pos_bytes(e->plan, src_b + r0 * row_b, src_bytes - r0 * row_b,
                                   (uint32_t *)(cm + r0 * nc * wb), nc, r1 - r0, s, (uint32_t *)(cf + r0 * np * wb), np));
      return LCPC_OK;
    });
    if (st) return st;
  } else if (src_b) {
    // the file image, unpacked inside the encode, which also writes the coefficient matrix
    c->canon = true;
    HIP_TRY(ntt_rows_pos_bytes(e->plan, src_b, src_bytes, (uint32_t *)cm, nc, n_rows, s, (uint32_t *)cf, np));
  } else {
    // full rows are encoded straight from the caller's buffer; the first NTT pass writes the
    // commitment's own coefficient copy as it reads them (no separate D2D copy)
    c->canon = true;
    const size_t full = len / np, tail = len - full * np;
    if (!tail && !eval && c->digest == DIGEST_BLAKE3 && ntt_rows_leaf_ok(e->plan, nc, true)) {
      // whole rows, BLAKE3 leaves, no u^T Enc(M): pass B hashes the columns as it stores them, and
      // no leaf pass reads the codeword back (ntt_rows_leaf_cvs)
      fused_chunks = (int)leaf_n_chunks(fid, n_rows);
      HIP_TRY(scratch.alloc(dev, (size_t)fused_chunks * nc * 32));
      HIP_TRY(ntt_rows_leaf_cvs(e->plan, (const uint32_t *)d_src, np, np, (uint32_t *)cm, nc, n_rows, s, (uint32_t *)cf,
                                np, scratch.as<uint32_t>()));
    } else {
      HIP_TRY(ntt_rows(e->plan, (const uint32_t *)d_src, np, np, (uint32_t *)cm, nc, full, s,
                       (uint32_t *)cf, np, true));
    }
    if (tail) {
      uint8_t *last = cf + full * np * wb;
      HIP_TRY(hipMemcpyAsync(last, (const uint8_t *)d_src + full * np * wb, tail * wb,
                             hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemsetAsync(last + tail * wb, 0, (np - tail) * wb, s));
      HIP_TRY(ntt_rows(e->plan, (const uint32_t *)last, np, np, (uint32_t *)(cm + full * nc * wb),
                       nc, 1, s, nullptr, 0, true));
    }
  }
  // Merkle tree (:685-697, merkleize :720-734); leaves past n_cols stay zero digests
  HIP_TRY(c->hashes.alloc(dev, c->n_hashes * 32));
  if (np2 > nc) HIP_TRY(hipMemsetAsync(c->hashes.as<uint8_t>() + nc * 32, 0, (np2 - nc) * 32, s));
  DBuf dleft, partials, dsum;
  if (!fused_chunks) HIP_TRY(scratch.alloc(dev, leaf_hash_scratch_bytes(fid, n_rows, nc)));
  const bool fused = eval && !c->col_major && c->canon && leaf_eval_fusable(fid);
  if (eval) {
    if (c->col_major) return fail(LCPC_ERR_UNSUPPORTED, "u^T Enc(M): row-major (Ligero) commitments only");
    lcpc_status st = upload(dev, dleft, eval_left, n_rows * wb);
    if (st) return st;
    HIP_TRY(dsum.alloc(dev, nc * wb));
  }
  if (fused_chunks) {
    HIP_TRY(leaves_from_cvs(scratch.as<uint32_t>(), nc, fused_chunks, c->hashes.as<uint8_t>(), s));
  } else if (c->digest != DIGEST_BLAKE3) {
    // D = SHA-256 / SHA3-256 / Keccak-256 (digest.hip); (eval is BLAKE3-only: refused above)
    if (c->col_major)
      HIP_TRY(leaf_hashes_cols_d(c->digest, fid, c->comm.as<uint32_t>(), n_rows, nc, c->hashes.as<uint8_t>(), nullptr, s,
                                 c->canon));
    else
      HIP_TRY(leaf_hashes_d(c->digest, fid, c->comm.as<uint32_t>(), n_rows, nc, nc, c->hashes.as<uint8_t>(), nullptr, s,
                            c->canon));
  } else if (c->col_major) {
    HIP_TRY(leaf_hashes_cols(fid, c->comm.as<uint32_t>(), n_rows, nc, c->hashes.as<uint8_t>(), scratch.p, s,
                             c->canon));
  } else if (fused) {
    // the leaf pass also sums each (chunk, column)'s share of u^T Enc(M); the shares fold below
    const size_t n_chunks = leaf_n_chunks(fid, n_rows);
    HIP_TRY(partials.alloc(dev, n_chunks * nc * wb));
    HIP_TRY(leaf_hashes_eval(fid, c->comm.as<uint32_t>(), n_rows, nc, nc, c->hashes.as<uint8_t>(), scratch.p,
                             dleft.as<uint32_t>(), partials.as<uint32_t>(), s));
    HIP_TRY(collapse_fold_rows(fid, partials.as<uint32_t>(), n_chunks, nc, dsum.as<uint32_t>(), s));
  } else {
    HIP_TRY(leaf_hashes(fid, c->comm.as<uint32_t>(), n_rows, nc, nc, c->hashes.as<uint8_t>(), scratch.p, s,
                        c->canon));
    if (eval) {
      DBuf cs;
      HIP_TRY(cs.alloc(dev, collapse_scratch_bytes(fid, n_rows, nc, 1)));
      HIP_TRY(collapse_rows(fid, c->comm.as<uint32_t>(), n_rows, nc, dleft.as<uint32_t>(), 1, dsum.as<uint32_t>(),
                            cs.p, s));
    }
  }
  HIP_TRY(merkle_tree_d(c->digest, c->hashes.as<uint8_t>(), np2, s));
  if (eval) {
    // over a canonical matrix the Montgomery products come out as canonical values
    if (c->canon) HIP_TRY(convert(fid, dsum.as<uint32_t>(), dsum.as<uint32_t>(), nc, true, s));
    HIP_TRY(d2h_staged(eval_out, dsum.p, nc * wb, s));
  }
  uint8_t *h_root = (uint8_t *)t_pin[PIN_OUTER].get(32);
  if (!h_root) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  HIP_TRY(d2h(h_root, c->hashes.as<uint8_t>() + (c->n_hashes - 1) * 32, 32, s));
  HIP_TRY(hipStreamSynchronize(s));
  // this commit's work is complete: its scratch needs no fence
  tmp.settle();
  scratch.settle();
  packed.settle();
  image.settle();
  std::memcpy(c->root, h_root, 32);
  c->coeffs.settle();
  c->comm.settle();
  c->hashes.settle();
  *out = c.release();
  return LCPC_OK;
}
}  // namespace

// ================================================================= C ABI
extern "C" {

int lcpc_abi_version(void) { return LCPC_ABI_VERSION; }
const char *lcpc_last_error(void) { return g_err.c_str(); }

lcpc_status lcpc_set_device(int device) {
  if (device < 0) return fail(LCPC_ERR_INVALID_ARG, "negative device");
  g_device = device;
  lcpc_status st;
  return get_device(device, &st) ? LCPC_OK : st;
}

int lcpc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

lcpc_status lcpc_field_random(lcpc_field f, uint64_t seed, uint64_t *out, size_t n) {
  // F::random(&mut ChaCha20Rng::seed_from_u64(seed)) x n (ff_derive; rand_core 0.6)
  if (!valid_field(f) || (!out && n)) return fail(LCPC_ERR_INVALID_ARG, "field / out");
  ChaCha20Rng rng = ChaCha20Rng::seed_from_u64(seed);
  const FieldInfo fi = field_info(f);
  field_random(rng, fi.limbs, fi.num_bits, fi.p, out, n);
  return LCPC_OK;
}

int lcpc_field_limbs(lcpc_field f) { return valid_field(f) ? field_info(f).limbs : 0; }
int lcpc_field_num_bits(lcpc_field f) { return valid_field(f) ? field_info(f).num_bits : 0; }

size_t lcpc_log2(size_t v) { return log2_np2(v); }

size_t lcpc_n_degree_tests(size_t lambda, size_t len, size_t flog2) {
  const size_t den = flog2 - log2_np2(len);
  return (lambda + den - 1) / den;
}

size_t lcpc_ligero_n_col_opens(size_t rho_num, size_t rho_den) {
  const double rho = (double)rho_num / (double)rho_den;
  const double den = std::log2((1.0 + rho) / 2.0);
  return (size_t)std::ceil(-128.0 / den);
}

lcpc_status lcpc_ligero_get_dims(lcpc_field f, size_t rn, size_t rd, size_t len, size_t *nr,
                                 size_t *npr, size_t *nc) {
  // LigeroEncodingRho::_get_dims (lcpc-ligero-pc/src/lib.rs:70-112)
  if (!valid_field(f) || !(rn < rd) || len == 0 || !nr || !npr || !nc)
    return fail(LCPC_ERR_INVALID_ARG, "get_dims arguments");
  const FieldInfo fi = field_info(f);
  const size_t flog2 = fi.num_bits - 1;
  const double rho = (double)rn / (double)rd;
  const size_t nco = lcpc_ligero_n_col_opens(rn, rd);
  const double lncf = (double)(nco * len);
  const double ndt = (double)lcpc_n_degree_tests(128, (size_t)std::ceil(std::sqrt(lncf) / rho), flog2);
  const size_t nc1 = next_pow2((size_t)std::ceil(std::sqrt(lncf / ndt) / rho));
  if (fi.s < 63 && nc1 > ((size_t)1 << fi.s)) return fail(LCPC_PROVER_TOO_BIG, "n_cols > 2^S");
  const size_t np1 = nc1 * rn / rd;
  if (np1 == 0) return fail(LCPC_ERR_INVALID_ARG, "degenerate dims");
  const size_t nr1 = (len + np1 - 1) / np1;
  const size_t nd1 = lcpc_n_degree_tests(128, nc1, flog2);
  const size_t nc2 = nc1 / 2, np2 = np1 / 2;
  if (np2 == 0)  // the reference divides by np2 = 0 here and panics
    return fail(LCPC_ERR_INVALID_ARG, "get_dims: len too small (n_per_row / 2 == 0)");
  const size_t nr2 = (len + np2 - 1) / np2;
  const size_t nd2 = lcpc_n_degree_tests(128, nc2, flog2);
  const size_t sz1 = nco * nr1 + (1 + nd1) * np1;
  const size_t sz2 = nco * nr2 + (1 + nd2) * np2;
  if (sz1 < sz2) {
    *nr = nr1; *npr = np1; *nc = nc1;
  } else {
    *nr = nr2; *npr = np2; *nc = nc2;
  }
  return LCPC_OK;
}

lcpc_status lcpc_ligero_new_from_dims(lcpc_field f, size_t rn, size_t rd, size_t n_per_row,
                                      size_t n_cols, lcpc_encoding **out) {
  if (!valid_field(f) || !(rn < rd)) return fail(LCPC_ERR_INVALID_ARG, "rate");
  const size_t nco = lcpc_ligero_n_col_opens(rn, rd);
  const size_t ndt = lcpc_n_degree_tests(128, n_cols, field_info(f).num_bits - 1);
  return make_rs_encoding(f, n_per_row, n_cols, nco, ndt, out);
}

lcpc_status lcpc_ligero_new(lcpc_field f, size_t rn, size_t rd, size_t len, lcpc_encoding **out) {
  size_t nr, np, nc;
  lcpc_status st = lcpc_ligero_get_dims(f, rn, rd, len, &nr, &np, &nc);
  if (st != LCPC_OK) return st;
  return lcpc_ligero_new_from_dims(f, rn, rd, np, nc, out);
}

lcpc_status lcpc_ligero_new_ml(lcpc_field f, size_t rn, size_t rd, size_t n_vars,
                               lcpc_encoding **out) {
  // LigeroEncodingRho::new_ml (lib.rs:130-136)
  if (n_vars >= 63) return fail(LCPC_ERR_INVALID_ARG, "n_vars");
  const size_t n_mon = (size_t)1 << n_vars;
  size_t nr, np, nc;
  lcpc_status st = lcpc_ligero_get_dims(f, rn, rd, n_mon, &nr, &np, &nc);
  if (st != LCPC_OK) return st;
  if ((nr & (nr - 1)) || (np & (np - 1)) || nr * np != n_mon)
    return fail(LCPC_ERR_INVALID_ARG, "new_ml: dims are not powers of two");
  return lcpc_ligero_new_from_dims(f, rn, rd, np, nc, out);
}

lcpc_status lcpc_rs_encoding_new(lcpc_field f, size_t n_per_row, size_t n_cols, size_t nco,
                                 size_t ndt, lcpc_encoding **out) {
  return make_rs_encoding(f, n_per_row, n_cols, nco, ndt, out);
}

size_t lcpc_sdig_n_col_opens(int code) { return sdig_n_col_opens(code); }

lcpc_status lcpc_sdig_get_n_per_row(lcpc_field f, int code, size_t len, size_t *n_per_row) {
  if (!valid_field(f) || !sdig_spec(code) || !n_per_row || len == 0)
    return fail(LCPC_ERR_INVALID_ARG, "sdig_get_n_per_row arguments");
  *n_per_row = sdig_new_np(code, field_info(f).num_bits, len);
  return LCPC_OK;
}

lcpc_status lcpc_sdig_new(lcpc_field f, int code, size_t len, uint64_t seed, lcpc_encoding **out) {
  // SdigEncodingS::new (lcpc-brakedown-pc/src/lib.rs:103-110)
  if (!valid_field(f) || !sdig_spec(code) || len == 0)
    return fail(LCPC_ERR_INVALID_ARG, "sdig_new arguments");
  return make_sdig_encoding(f, code, sdig_new_np(code, field_info(f).num_bits, len), 0, seed, out);
}

lcpc_status lcpc_sdig_new_ml(lcpc_field f, int code, size_t n_vars, uint64_t seed,
                             lcpc_encoding **out) {
  // SdigEncodingS::new_ml (lib.rs:114-123)
  if (!valid_field(f) || !sdig_spec(code) || n_vars >= 63)
    return fail(LCPC_ERR_INVALID_ARG, "sdig_new_ml arguments");
  return make_sdig_encoding(f, code, sdig_new_ml_np(code, field_info(f).num_bits, n_vars), 0, seed, out);
}

lcpc_status lcpc_sdig_new_from_dims(lcpc_field f, int code, size_t n_per_row, size_t n_cols,
                                    uint64_t seed, lcpc_encoding **out) {
  // SdigEncodingS::new_from_dims (lib.rs:126-137)
  if (n_cols == 0) return fail(LCPC_ERR_INVALID_ARG, "n_cols");
  return make_sdig_encoding(f, code, n_per_row, n_cols, seed, out);
}

int lcpc_encoding_kind(const lcpc_encoding *e) { return e->kind; }

size_t lcpc_encoding_matrix_nnz(const lcpc_encoding *e) {
  size_t nnz = 0;
  for (const auto &m : e->sdig.pre) nnz += m.nnz;
  for (const auto &m : e->sdig.post) nnz += m.nnz;
  return nnz;
}

void lcpc_encoding_free(lcpc_encoding *e) { delete e; }
lcpc_field lcpc_encoding_field(const lcpc_encoding *e) { return (lcpc_field)e->fid; }

void lcpc_encoding_get_dims(const lcpc_encoding *e, size_t len, size_t *nr, size_t *np, size_t *nc) {
  *nr = (len + e->n_per_row - 1) / e->n_per_row;
  *np = e->n_per_row;
  *nc = e->n_cols;
}
int lcpc_encoding_dims_ok(const lcpc_encoding *e, size_t np, size_t nc) {
  return encoding_dims_ok(e, np, nc) == LCPC_OK;
}
size_t lcpc_encoding_n_col_opens(const lcpc_encoding *e) { return e->n_col_opens; }
size_t lcpc_encoding_n_degree_tests(const lcpc_encoding *e) { return e->n_degree_tests; }
size_t lcpc_encoding_n_per_row(const lcpc_encoding *e) { return e->n_per_row; }
size_t lcpc_encoding_n_cols(const lcpc_encoding *e) { return e->n_cols; }
lcpc_status lcpc_encoding_set_row_kernel(lcpc_encoding *e, int kernel) {
  if (!e || kernel < LCPC_ROW_KERNEL_AUTO || kernel > LCPC_ROW_KERNEL_ONEPASS)
    return fail(LCPC_ERR_INVALID_ARG, "row kernel");
  e->plan.row_kernel = kernel;
  return LCPC_OK;
}

int lcpc_encoding_leaf_fuse(const lcpc_encoding *e) {
  return e && e->kind != KIND_SDIG && ntt_rows_leaf_ok(e->plan, e->n_cols, true) ? 1 : 0;
}

const char *lcpc_digest_name(lcpc_digest d) { return digest_name((int)d); }
lcpc_status lcpc_encoding_set_digest(lcpc_encoding *e, lcpc_digest d) {
  if (!e || !digest_valid((int)d)) return fail(LCPC_ERR_INVALID_ARG, "digest");
  e->digest = (int)d;
  return LCPC_OK;
}
lcpc_digest lcpc_encoding_digest(const lcpc_encoding *e) { return (lcpc_digest)(e ? e->digest : 0); }

lcpc_status lcpc_reserve(const lcpc_encoding *e, size_t len, size_t count) {
  if (!e || !len) return fail(LCPC_ERR_INVALID_ARG, "reserve arguments");
  Device *dev = e->dev;
  HIP_TRY(hipSetDevice(dev->id));
  const size_t wb = (size_t)field_bytes(e->fid), np = e->n_per_row, nc = e->n_cols, nco = e->n_col_opens;
  const size_t nr = (len + np - 1) / np, np2 = next_pow2(nc), pl = log2_np2(nc);
  // the blocks commit_device and lcpc_prove ask of the pool, by size
  std::vector<size_t> sizes = {nr * np * wb, nr * nc * wb, (2 * np2 - 1) * 32,
                               leaf_hash_scratch_bytes(e->fid, nr, nc), 2 * nr * wb, 2 * np * wb,
                               collapse_scratch_bytes(e->fid, nr, np, 2), np * wb, nco * 8, nco * nr * wb,
                               nco * pl * 32};
  if (e->kind == KIND_SDIG) sizes.push_back(e->sdig.tmp_elems * nr * wb);
  std::vector<void *> blocks;
  lcpc_status st = LCPC_OK;
  for (size_t k = 0; k < count && !st; k++)
    for (size_t b : sizes) {
      void *p = nullptr;
      if (dev->alloc(&p, b) != hipSuccess) {
        st = fail(LCPC_ERR_OUT_OF_MEMORY, "reserve: device pool");
        break;
      }
      blocks.push_back(p);
    }
  for (void *p : blocks) dev->release(p);
  std::vector<hipStream_t> lo, hi;
  for (size_t k = 0; k < count; k++) {
    lo.push_back(dev->acquire_stream(POOL_BULK));
    hi.push_back(dev->acquire_stream(POOL_PROVER));
  }
  for (hipStream_t s : lo)
    if (s) dev->release_stream(s, POOL_BULK);
  for (hipStream_t s : hi)
    if (s) dev->release_stream(s, POOL_PROVER);
  // the page-locked blocks of `count` proofs (p_random, p_eval, columns, paths)
  const size_t ndt = e->n_degree_tests;
  std::vector<void *> pins;
  for (size_t k = 0; k < count; k++)
    for (size_t b : {ndt * np * wb, np * wb, nco * nr * wb, nco * pl * 32})
      if (b >= PinnedHeap::MIN)
        if (void *p = g_pinned_heap.get(b)) pins.push_back(p);
  for (void *p : pins) g_pinned_heap.put(p);
  return st;
}

lcpc_status lcpc_prepare_thread(const lcpc_encoding *e, size_t n_rows) {
  if (!e) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  // the sizes lcpc_prove asks of each thread-local slot
  const size_t wb = (size_t)field_bytes(e->fid), np = e->n_per_row, nco = e->n_col_opens;
  const size_t ndt = e->n_degree_tests, pl = log2_np2(e->n_cols);
  (void)ndt;
  (void)pl;
  // (p_random, p_eval and the columns land in the proof's own page-locked vectors)
  const size_t want[PIN_N] = {2 * np * wb, 1, 1, 1, nco * 8, n_rows * wb, n_rows * wb, 1, 1};
  for (int i = 0; i < PIN_N; i++)
    if (!t_pin[i].get(std::max<size_t>(1, want[i]))) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  t_eval_repr.reserve(np * wb);
  return LCPC_OK;
}

static lcpc_status encode_rows_chunk(const lcpc_encoding *e, uint64_t *rows, size_t n_rows, size_t stride) {
  Device *dev = e->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(e->fid);
  DBuf d;
  HIP_TRY(d.alloc(dev, n_rows * e->n_cols * wb));
  HIP_TRY(hipMemcpy2DAsync(d.p, e->n_cols * wb, rows, stride * wb, e->n_cols * wb, n_rows,
                           hipMemcpyHostToDevice, lease.s));
  lcpc_status st = encode_rows_any(e, d.as<uint32_t>(), e->n_cols, e->n_cols, d.as<uint32_t>(),
                                   e->n_cols, n_rows, lease.s);
  if (st) return st;
  HIP_TRY(hipMemcpy2DAsync(rows, stride * wb, d.p, e->n_cols * wb, e->n_cols * wb, n_rows,
                           hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_encode_rows(const lcpc_encoding *e, uint64_t *rows, size_t n_rows, size_t stride) {
  if (!e || (!rows && n_rows)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (stride < e->n_cols) return fail(LCPC_ERR_INVALID_ARG, "row stride < n_cols");
  if (n_rows == 0) return LCPC_OK;
  // The rows are the caller's pageable memory, so one stream's H2D -> encode -> D2H runs
  // serially.  Chunks of ~16 MiB on up to 8 host threads (each with its own leased stream)
  // overlap one chunk's copies with another's kernels, as concurrent per-row callers do
  // (tools/encode_rows_bench.py at the cfg3 row size: 62 GB/s of H2D + D2H for 16 callers
  // against 52 GB/s for the whole batch on one stream).
  const size_t row_bytes = e->n_cols * (size_t)field_bytes(e->fid);
  const size_t chunk = std::max<size_t>(1, ((size_t)16 << 20) / row_bytes);
  const size_t n_chunks = (n_rows + chunk - 1) / chunk;
  if (n_chunks < 2) return encode_rows_chunk(e, rows, n_rows, stride);
  const size_t T = std::min<size_t>(8, n_chunks);
  std::atomic<size_t> next{0};
  std::mutex mu;
  lcpc_status first = LCPC_OK;
  std::string msg;
  auto work = [&] {
    for (size_t k; (k = next.fetch_add(1)) < n_chunks;) {
      const size_t r0 = k * chunk, nr = std::min(chunk, n_rows - r0);
      const lcpc_status st = encode_rows_chunk(e, rows + r0 * stride * (size_t)field_info(e->fid).limbs, nr, stride);
      if (st) {
        std::lock_guard<std::mutex> lk(mu);
        if (!first) first = st, msg = g_err;
        next.store(n_chunks);
      }
    }
  };
  std::vector<std::thread> th;
  for (size_t i = 1; i < T; i++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  return first ? fail(first, msg) : LCPC_OK;
}

lcpc_status lcpc_encode(const lcpc_encoding *e, uint64_t *inp, size_t len) {
  // fffft::fft_io_pc: the slice length must equal the precomputation length
  if (!e || !inp) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (e->kind == KIND_SDIG && len != e->n_cols)  // encode.rs:42 asserts the codeword length
    return fail(LCPC_ERR_INVALID_ARG, "SDIG encode: slice length != codeword length");
  if (len != e->n_cols) {
    if (len == 0 || (len & (len - 1))) return fail(LCPC_FFT_NOT_POWER_OF_TWO, "FFTError::NotPowerOfTwo");
    if ((int)log2_np2(len) > field_info(e->fid).s) return fail(LCPC_FFT_TOO_BIG, "FFTError::TooBig");
    return fail(LCPC_FFT_WRONG_SIZE_PRECOMP, "FFTError::WrongSizePrecomp");
  }
  return lcpc_encode_rows(e, inp, 1, len);
}

lcpc_status lcpc_encode_rows_device(const lcpc_encoding *e, const void *d_src, size_t src_stride,
                                    size_t n_valid, void *d_dst, size_t dst_stride, size_t n_rows,
                                    void *stream) {
  if (!e || !d_dst || (!d_src && n_valid)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (n_valid > e->n_cols || dst_stride < e->n_cols)
    return fail(LCPC_ERR_INVALID_ARG, "encode_rows_device: bad lengths");
  Device *dev = e->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : lease.s;
  StreamAs on_s(s);  // (SDIG's scratch codeword: taken and fenced on the stream that uses it)
  lcpc_status st = encode_rows_any(e, (const uint32_t *)d_src, src_stride, n_valid,
                                   (uint32_t *)d_dst, dst_stride, n_rows, s);
  if (st) return st;
  if (!stream) HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

// ---------------------------------------------------------------- commit
lcpc_status lcpc_commit_new(const lcpc_encoding *e, const uint64_t *coeffs, size_t len,
                            lcpc_commit **out) {
  if (!coeffs) return fail(LCPC_ERR_INVALID_ARG, "null coeffs");
  return commit_device(e, coeffs, true, len, out);
}

lcpc_status lcpc_commit_new_device(const lcpc_encoding *e, const void *d_coeffs, size_t len,
                                   lcpc_commit **out) {
  if (!d_coeffs) return fail(LCPC_ERR_INVALID_ARG, "null coeffs");
  return commit_device(e, d_coeffs, false, len, out);
}

lcpc_status lcpc_pos_commit_bytes_device(const lcpc_encoding *e, const void *d_bytes, size_t n_bytes,
                                         lcpc_commit **out) {
  if (!d_bytes || !n_bytes) return fail(LCPC_ERR_INVALID_ARG, "null or empty file image");
  if ((uintptr_t)d_bytes & 7) return fail(LCPC_ERR_INVALID_ARG, "device file image must be 8-byte aligned");
  return commit_device(e, d_bytes, false, (n_bytes + 6) / 7, out, n_bytes);  // 7 data bytes per element
}

lcpc_status lcpc_pos_commit_eval_bytes_device(const lcpc_encoding *e, const void *d_bytes, size_t n_bytes,
                                              const uint64_t *left, size_t n_rows, uint64_t *eval_out,
                                              lcpc_commit **out) {
  if (!e || !d_bytes || !n_bytes || !left || !eval_out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if ((uintptr_t)d_bytes & 7) return fail(LCPC_ERR_INVALID_ARG, "device file image must be 8-byte aligned");
  const size_t len = (n_bytes + 6) / 7;
  if (!e->n_per_row || n_rows != (len + e->n_per_row - 1) / e->n_per_row)
    return fail(LCPC_ERR_INVALID_ARG, "left vector length != the commitment's n_rows");
  return commit_device(e, d_bytes, false, len, out, n_bytes, left, eval_out);
}

lcpc_status lcpc_pos_commit_bytes(const lcpc_encoding *e, const uint8_t *bytes, size_t n_bytes, lcpc_commit **out) {
  if (!bytes || !n_bytes) return fail(LCPC_ERR_INVALID_ARG, "null or empty file image");
  return commit_device(e, bytes, true, (n_bytes + 6) / 7, out, n_bytes);
}

int lcpc_last_upload_pinned(void) { return t_last_upload.pinned ? 1 : 0; }

void lcpc_commit_free(lcpc_commit *c) {
  if (!c) return;
  Device *dev = c->dev;
  Lease lease(dev);
  (void)hipSetDevice(dev->id);
  (void)hipStreamSynchronize(lease.s);
  delete c;
}

lcpc_status lcpc_commit_get_root(const lcpc_commit *c, uint8_t root[32]) {
  std::memcpy(root, c->root, 32);
  return LCPC_OK;
}
size_t lcpc_commit_n_rows(const lcpc_commit *c) { return c->n_rows; }
size_t lcpc_commit_n_cols(const lcpc_commit *c) { return c->n_cols; }
size_t lcpc_commit_n_per_row(const lcpc_commit *c) { return c->n_per_row; }
size_t lcpc_commit_n_hashes(const lcpc_commit *c) { return c->n_hashes; }
lcpc_digest lcpc_commit_digest(const lcpc_commit *c) { return (lcpc_digest)(c ? c->digest : 0); }
const void *lcpc_commit_device_comm(const lcpc_commit *c) { return c->comm.p; }
const void *lcpc_commit_device_coeffs(const lcpc_commit *c) { return c->coeffs.p; }

static lcpc_status copy_out(const lcpc_commit *c, void *dst, const void *src, size_t bytes) {
  Lease lease(c->dev);
  HIP_TRY(hipSetDevice(c->dev->id));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}
lcpc_status lcpc_commit_copy_comm(const lcpc_commit *c, uint64_t *out) {
  const size_t bytes = c->n_rows * c->n_cols * field_bytes(c->fid);
  if (c->canon && !c->col_major) {  // canonical on the device -> the reference's Montgomery words
    Lease lease(c->dev);
    HIP_TRY(hipSetDevice(c->dev->id));
    DBuf mm;
    HIP_TRY(mm.alloc(c->dev, bytes));
    HIP_TRY(convert(c->fid, c->comm.as<uint32_t>(), mm.as<uint32_t>(), c->n_rows * c->n_cols, true, lease.s));
    HIP_TRY(hipMemcpyAsync(out, mm.p, bytes, hipMemcpyDeviceToHost, lease.s));
    HIP_TRY(hipStreamSynchronize(lease.s));
    return LCPC_OK;
  }
  if (!c->col_major) return copy_out(c, out, c->comm.p, bytes);
  // element-major on the device -> the reference's row-major Vec<F>
  Lease lease(c->dev);
  HIP_TRY(hipSetDevice(c->dev->id));
  DBuf rm;
  HIP_TRY(rm.alloc(c->dev, bytes));
  HIP_TRY(transpose_elems(c->fid, c->comm.as<uint32_t>(), c->n_cols, c->n_rows, c->n_rows, c->n_rows,
                          rm.as<uint32_t>(), c->n_cols, lease.s));
  if (c->canon) HIP_TRY(convert(c->fid, rm.as<uint32_t>(), rm.as<uint32_t>(), c->n_rows * c->n_cols, true, lease.s));
  HIP_TRY(hipMemcpyAsync(out, rm.p, bytes, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}
int lcpc_commit_col_major(const lcpc_commit *c) { return c->col_major ? 1 : 0; }
int lcpc_commit_comm_canonical(const lcpc_commit *c) { return c->canon ? 1 : 0; }
lcpc_status lcpc_commit_copy_coeffs(const lcpc_commit *c, uint64_t *out) {
  return copy_out(c, out, c->coeffs.p, c->n_rows * c->n_per_row * field_bytes(c->fid));
}
lcpc_status lcpc_commit_copy_hashes(const lcpc_commit *c, uint8_t *out) {
  return copy_out(c, out, c->hashes.p, c->n_hashes * 32);
}

lcpc_status lcpc_commit_from_parts(lcpc_field f, size_t n_rows, size_t n_cols, size_t n_per_row,
                                   const uint64_t *comm, const uint64_t *coeffs, const uint8_t *hashes,
                                   size_t n_hashes, lcpc_commit **out) {
  return lcpc_commit_from_parts_d(LCPC_DIGEST_BLAKE3, f, n_rows, n_cols, n_per_row, comm, coeffs, hashes, n_hashes, out);
}

lcpc_status lcpc_commit_from_parts_d(lcpc_digest d, lcpc_field f, size_t n_rows, size_t n_cols, size_t n_per_row,
                                     const uint64_t *comm, const uint64_t *coeffs, const uint8_t *hashes,
                                     size_t n_hashes, lcpc_commit **out) {
  // LcCommit's Deserialize (WrappedLcCommit::unwrap, lcpc-2d/src/lib.rs:193-229): the fields as
  // given (row-major Montgomery comm and coeffs, the hashes in commit order, root last), loaded
  // into HBM so that prove / open_column run on them.  The reference takes any lengths and fails
  // later (check_comm, or a panic in open_column); here the lengths must be the ones commit
  // produces, else LCPC_ERR_INVALID_ARG.
  if (!out || (!comm && n_rows * n_cols) || (!coeffs && n_rows * n_per_row) || !hashes)
    return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!digest_valid((int)d)) return fail(LCPC_ERR_INVALID_ARG, "digest");
  if (!valid_field(f) || !field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field");
  if (!n_rows || !n_cols || n_per_row > n_cols || n_hashes != 2 * next_pow2(n_cols) - 1)
    return fail(LCPC_ERR_INVALID_ARG, "commitment parts of inconsistent sizes");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  auto c = std::make_unique<lcpc_commit>();
  c->fid = f;
  c->digest = (int)d;
  c->dev = dev;
  c->n_rows = n_rows;
  c->n_cols = n_cols;
  c->n_per_row = n_per_row;
  c->n_hashes = n_hashes;
  const size_t wb = field_bytes(f);
  if ((st = upload(dev, c->comm, comm, n_rows * n_cols * wb))) return st;
  if ((st = upload(dev, c->coeffs, coeffs, n_rows * n_per_row * wb))) return st;
  if ((st = upload(dev, c->hashes, hashes, n_hashes * 32))) return st;
  std::memcpy(c->root, hashes + (n_hashes - 1) * 32, 32);
  HIP_TRY(hipStreamSynchronize(lease.s));
  for (auto *b : {&c->comm, &c->coeffs, &c->hashes}) b->settle();
  *out = c.release();
  return LCPC_OK;
}

lcpc_status lcpc_check_comm(const lcpc_commit *c, const lcpc_encoding *e) {
  // check_comm (lcpc-2d/src/lib.rs:703-718); buffer sizes hold by construction
  if (!c || !e) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  // D is a type parameter of LcCommit in the reference: a mismatch cannot be written there
  if (c->digest != e->digest)
    return fail(LCPC_ERR_INVALID_ARG, std::string("the commitment's digest is ") + digest_name(c->digest) +
                                          ", the encoding's " + digest_name(e->digest));
  const bool hashlen = c->n_hashes != 2 * next_pow2(c->n_cols) - 1;
  if (hashlen || encoding_dims_ok(e, c->n_per_row, c->n_cols) != LCPC_OK || c->fid != e->fid)
    return fail(LCPC_PROVER_COMMIT, "ProverError::Commit");
  return LCPC_OK;
}

lcpc_status lcpc_open_column(const lcpc_commit *c, size_t column, uint64_t *col_out,
                             uint8_t *path_out) {
  // open_column (lcpc-2d/src/lib.rs:818-855)
  if (!c) return fail(LCPC_ERR_INVALID_ARG, "null commit");
  if (column >= c->n_cols) return fail(LCPC_PROVER_COLUMN_NUMBER, "ProverError::ColumnNumber");
  Device *dev = c->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const uint64_t idx = column;
  const size_t path_len = log2_np2(c->n_cols);
  DBuf didx, dcol, dpath;
  lcpc_status st = upload(dev, didx, &idx, 8);
  if (st) return st;
  const int wb = field_bytes(c->fid);
  HIP_TRY(dcol.alloc(dev, c->n_rows * wb));
  HIP_TRY(dpath.alloc(dev, path_len * 32));
  HIP_TRY(gather_columns(c->fid, c->comm.as<uint32_t>(), c->n_rows, c->n_cols, didx.as<uint64_t>(), 1,
                         dcol.as<uint32_t>(), lease.s, c->col_major, c->canon));
  HIP_TRY(gather_paths(c->hashes.as<uint8_t>(), c->n_hashes, didx.as<uint64_t>(), 1, path_len,
                       dpath.as<uint8_t>(), lease.s));
  if (col_out) HIP_TRY(hipMemcpyAsync(col_out, dcol.p, c->n_rows * wb, hipMemcpyDeviceToHost, lease.s));
  if (path_out && path_len)
    HIP_TRY(hipMemcpyAsync(path_out, dpath.p, path_len * 32, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

// ---------------------------------------------------------------- transcript
lcpc_transcript *lcpc_transcript_new(const uint8_t *label, size_t n) {
  return new lcpc_transcript(label, n);
}
lcpc_transcript *lcpc_transcript_from_ops(const lcpc_transcript_ops *ops) {
  if (!ops || !ops->append_message || !ops->challenge_bytes) {
    fail(LCPC_ERR_INVALID_ARG, "transcript ops need append_message and challenge_bytes");
    return nullptr;
  }
  return new lcpc_transcript(*ops);
}
int lcpc_transcript_status(const lcpc_transcript *t) { return t ? t->cb_status : 0; }
lcpc_transcript *lcpc_transcript_clone(const lcpc_transcript *t) {
  if (!t) return nullptr;
  if (t->external) {  // the caller's state lives on its side of the boundary
    fail(LCPC_ERR_UNSUPPORTED, "a caller-owned (ops) transcript cannot be cloned here; clone it on the caller's side");
    return nullptr;
  }
  return new lcpc_transcript(*t);
}
void lcpc_transcript_free(lcpc_transcript *t) { delete t; }
void lcpc_transcript_append_message(lcpc_transcript *t, const uint8_t *l, size_t ln,
                                    const uint8_t *m, size_t mn) {
  t->append_message(l, ln, m, mn);
}
void lcpc_transcript_append_messages(lcpc_transcript *t, const uint8_t *l, size_t ln, const uint8_t *msgs,
                                     size_t msg_len, size_t n_msgs) {
  t->append_messages(l, ln, msgs, msg_len, n_msgs);
}
void lcpc_transcript_challenge_bytes(lcpc_transcript *t, const uint8_t *l, size_t ln, uint8_t *d,
                                     size_t n) {
  t->challenge_bytes(l, ln, d, n);
}

// ---------------------------------------------------------------- prove
lcpc_status lcpc_prove(const lcpc_commit *c, const uint64_t *outer, size_t outer_len,
                       const lcpc_encoding *e, lcpc_transcript *tr, lcpc_proof **out) {
  // prove (lcpc-2d/src/lib.rs:1034-1123)
  prof::HostScope hs_total("host_prove_total");
  if (!c || !e || !tr || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  lcpc_status st = lcpc_check_comm(c, e);
  if (st) return st;
  if (outer_len != c->n_rows || (!outer && outer_len))
    return fail(LCPC_PROVER_OUTER_TENSOR, "ProverError::OuterTensor");
  Device *dev = c->dev;
  Lease lease(dev, POOL_PROVER);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const int fid = c->fid, wb = field_bytes(fid), limbs = wb / 8;
  const size_t nr = c->n_rows, np = c->n_per_row, ndt = e->n_degree_tests, nco = e->n_col_opens;
  auto p = std::make_unique<lcpc_proof>();
  p->fid = fid;
  p->n_cols = c->n_cols;
  p->n_per_row = np;
  p->n_rows = nr;
  p->ndt = ndt;
  p->nco = nco;
  p->path_len = log2_np2(c->n_cols);

  // the proof's own vectors are page-locked (pinned_vector): results land there by DMA
  p->p_random.resize(ndt * np * limbs);
  p->p_eval.resize(np * limbs);
  uint8_t *h_prand = (uint8_t *)p->p_random.data();
  uint8_t *h_peval = (uint8_t *)p->p_eval.data();
  uint8_t *h_tens = (uint8_t *)t_pin[PIN_TENSOR].get(nr * wb);
  uint8_t *h_outer = (uint8_t *)t_pin[PIN_OUTER].get(nr * wb);
  if (!h_tens || !h_outer) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  std::memcpy(h_outer, outer, nr * wb);

  // tensors on device: [t_i | outer] -- the evaluation tensor rides along with the first
  // degree test so the coefficient matrix is read once for both (results are independent).
  DBuf dtens, dres, scratch;
  HIP_TRY(dtens.alloc(dev, 2 * nr * wb));
  HIP_TRY(dres.alloc(dev, 2 * np * wb));
  HIP_TRY(scratch.alloc(dev, collapse_scratch_bytes(fid, nr, np, 2)));
  HIP_TRY(h2d(dtens.as<uint8_t>() + nr * wb, h_outer, nr * wb, s));
  std::vector<uint64_t> tensor;
  const uint8_t *repr = nullptr;
  bool eval_done = false;
  // the evaluation's repr bytes, converted in the first round's GPU round trip (its absorb comes
  // after the last degree test's): one round trip fewer on the proof's serial path
  std::vector<uint8_t> &eval_repr = t_eval_repr;
  bool eval_repr_ready = false;
  for (size_t i = 0; i < ndt; i++) {
    {
      prof::HostScope hs("host_prove_round_issue");
      challenge_tensor(*tr, fid, nr, tensor);
      if ((st = transcript_status(tr))) return st;
      std::memcpy(h_tens, tensor.data(), nr * wb);
      HIP_TRY(h2d(dtens.p, h_tens, nr * wb, s));
      const int nt = eval_done ? 1 : 2;
      HIP_TRY(collapse_rows(fid, c->coeffs.as<uint32_t>(), nr, np, dtens.as<uint32_t>(), nt,
                            dres.as<uint32_t>(), scratch.p, s));
      HIP_TRY(d2h(h_prand + i * np * wb, dres.p, np * wb, s));
      if (!eval_done) {
        HIP_TRY(d2h(h_peval, dres.as<uint8_t>() + np * wb, np * wb, s));
        eval_done = true;
      }
    }
    const bool with_eval = i == 0;  // round 0 also holds the evaluation (dres[np, 2 np))
    {
      prof::HostScope hs("host_prove_gpu_wait");
      st = to_repr_host(dev, fid, dres.as<uint32_t>(), with_eval ? 2 * np : np, &repr);  // syncs the stream
    }
    if (st) return st;
    if (with_eval) {
      eval_repr.assign(repr + np * wb, repr + 2 * np * wb);
      eval_repr_ready = true;
    }
    {
      prof::HostScope hs("host_prove_transcript");
      tr->append_messages(LABEL_PR, 6, repr, wb, np);
    }
    if ((st = transcript_status(tr))) return st;
  }
  const uint32_t *d_eval = dres.as<uint32_t>() + np * limbs * 2;  // second collapse output
  if (!eval_done) {
    HIP_TRY(collapse_rows(fid, c->coeffs.as<uint32_t>(), nr, np, dtens.as<uint32_t>() + nr * limbs * 2, 1,
                          dres.as<uint32_t>(), scratch.p, s));
    HIP_TRY(d2h(h_peval, dres.p, np * wb, s));
    d_eval = dres.as<uint32_t>();
  }
  if (eval_repr_ready) {
    repr = eval_repr.data();
  } else {
    prof::HostScope hs("host_prove_gpu_wait");
    st = to_repr_host(dev, fid, d_eval, np, &repr);
  }
  if (st) return st;
  {
    prof::HostScope hs("host_prove_transcript");
    tr->append_messages(LABEL_PE, 6, repr, wb, np);
  }

  // columns (:1101-1115)
  challenge_columns(*tr, c->n_cols, nco, p->col_idx);
  if ((st = transcript_status(tr))) return st;
  p->cols.resize(nco * nr * limbs);
  p->paths.resize(nco * p->path_len * 32);
  uint8_t *h_cols = (uint8_t *)p->cols.data();
  uint8_t *h_paths = p->paths.data();
  uint8_t *h_idx = (uint8_t *)t_pin[PIN_PATHS].get(std::max<size_t>(1, nco * 8));
  if (!h_idx) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  std::memcpy(h_idx, p->col_idx.data(), nco * 8);
  DBuf didx, dcols, dpaths;
  HIP_TRY(didx.alloc(dev, nco * 8));
  if (nco) HIP_TRY(h2d(didx.p, h_idx, nco * 8, s));
  HIP_TRY(dcols.alloc(dev, nco * nr * wb));
  HIP_TRY(dpaths.alloc(dev, nco * p->path_len * 32));
  HIP_TRY(gather_columns(fid, c->comm.as<uint32_t>(), nr, c->n_cols, didx.as<uint64_t>(), nco,
                         dcols.as<uint32_t>(), s, c->col_major, c->canon));
  HIP_TRY(gather_paths(c->hashes.as<uint8_t>(), c->n_hashes, didx.as<uint64_t>(), nco, p->path_len,
                       dpaths.as<uint8_t>(), s));
  if (nco) {
    HIP_TRY(d2h(h_cols, dcols.p, nco * nr * wb, s));
    if (p->path_len)
      HIP_TRY(d2h(h_paths, dpaths.p, nco * p->path_len * 32, s));
  }
  {
    prof::HostScope hs("host_prove_cols_wait");
    HIP_TRY(hipStreamSynchronize(s));
  }
  *out = p.release();
  return LCPC_OK;
}

void lcpc_proof_free(lcpc_proof *p) { delete p; }
size_t lcpc_proof_n_cols(const lcpc_proof *p) { return p->n_cols; }
size_t lcpc_proof_n_per_row(const lcpc_proof *p) { return p->n_per_row; }
size_t lcpc_proof_n_rows(const lcpc_proof *p) { return p->n_rows; }
size_t lcpc_proof_n_degree_tests(const lcpc_proof *p) { return p->ndt; }
size_t lcpc_proof_n_col_opens(const lcpc_proof *p) { return p->nco; }
size_t lcpc_proof_path_len(const lcpc_proof *p) { return p->path_len; }
lcpc_field lcpc_proof_field(const lcpc_proof *p) { return (lcpc_field)p->fid; }

lcpc_status lcpc_proof_copy_p_eval(const lcpc_proof *p, uint64_t *out) {
  std::memcpy(out, p->p_eval.data(), p->p_eval.size() * 8);
  return LCPC_OK;
}
lcpc_status lcpc_proof_copy_p_random(const lcpc_proof *p, size_t i, uint64_t *out) {
  if (i >= p->ndt) return fail(LCPC_ERR_INVALID_ARG, "degree test index");
  const size_t n = p->n_per_row * (field_bytes(p->fid) / 8);
  std::memcpy(out, p->p_random.data() + i * n, n * 8);
  return LCPC_OK;
}
lcpc_status lcpc_proof_copy_column(const lcpc_proof *p, size_t k, uint64_t *col, uint8_t *path) {
  if (k >= p->nco) return fail(LCPC_ERR_INVALID_ARG, "column index");
  const size_t n = p->n_rows * (field_bytes(p->fid) / 8);
  if (col) std::memcpy(col, p->cols.data() + k * n, n * 8);
  if (path && p->path_len) std::memcpy(path, p->paths.data() + k * p->path_len * 32, p->path_len * 32);
  return LCPC_OK;
}

lcpc_status lcpc_proof_from_parts(lcpc_field f, size_t n_cols, size_t n_per_row, size_t n_rows,
                                  size_t ndt, size_t nco, size_t path_len, const uint64_t *p_eval,
                                  const uint64_t *p_random, const uint64_t *cols,
                                  const uint8_t *paths, lcpc_proof **out) {
  if (!valid_field(f) || !out) return fail(LCPC_ERR_INVALID_ARG, "field / out");
  auto p = std::make_unique<lcpc_proof>();
  const size_t limbs = field_info(f).limbs;
  p->fid = f;
  p->n_cols = n_cols;
  p->n_per_row = n_per_row;
  p->n_rows = n_rows;
  p->ndt = ndt;
  p->nco = nco;
  p->path_len = path_len;
  p->p_eval.assign(p_eval, p_eval + n_per_row * limbs);
  if (ndt) p->p_random.assign(p_random, p_random + ndt * n_per_row * limbs);
  if (nco) p->cols.assign(cols, cols + nco * n_rows * limbs);
  if (nco && path_len) p->paths.assign(paths, paths + nco * path_len * 32);
  *out = p.release();
  return LCPC_OK;
}

// ---------------------------------------------------------------- verify
lcpc_status lcpc_verify(const uint8_t root[32], const uint64_t *outer, size_t outer_len,
                        const uint64_t *inner, size_t inner_len, const lcpc_proof *p,
                        const lcpc_encoding *e, lcpc_transcript *tr, uint64_t *eval_out) {
  // verify (lcpc-2d/src/lib.rs:862-982)
  if (!root || !p || !e || !tr) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  const size_t nco = e->n_col_opens;
  if (nco != p->nco || nco == 0) return fail(LCPC_VERIFIER_NUM_COL_OPENS, "VerifierError::NumColOpens");
  const size_t nr = p->n_rows, nc = p->n_cols, np = p->n_per_row;
  if (inner_len != np) return fail(LCPC_VERIFIER_INNER_TENSOR, "VerifierError::InnerTensor");
  if (outer_len != nr) return fail(LCPC_VERIFIER_OUTER_TENSOR, "VerifierError::OuterTensor");
  if (encoding_dims_ok(e, np, nc) != LCPC_OK || p->fid != e->fid)
    return fail(LCPC_VERIFIER_ENCODING_DIMS, "VerifierError::EncodingDims");
  const size_t ndt = e->n_degree_tests;
  if (p->ndt != ndt) return fail(LCPC_VERIFIER_ENCODING_DIMS, "proof has a different number of degree tests");
  const int fid = e->fid, wb = field_bytes(fid), limbs = wb / 8;
  Device *dev = e->dev;
  Lease lease(dev, POOL_HIGH);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;

  // device copies: tensors [ndt | outer] (n_rows each), encodings [ndt + 1][n_cols]
  DBuf dtens, denc, dvec, didx, dcols, dpaths, dleaves, dflags, dpflags, scratch, dinner, dout, droot;
  HIP_TRY(dtens.alloc(dev, (ndt + 1) * nr * wb));
  HIP_TRY(denc.alloc(dev, (ndt + 1) * nc * wb));
  HIP_TRY(hipMemcpyAsync(dtens.as<uint8_t>() + ndt * nr * wb, outer, nr * wb, hipMemcpyHostToDevice, s));
  std::vector<uint64_t> tensor;
  const uint8_t *repr = nullptr;
  lcpc_status st;
  for (size_t i = 0; i < ndt; i++) {
    challenge_tensor(*tr, fid, nr, tensor);
    HIP_TRY(hipMemcpyAsync(dtens.as<uint8_t>() + i * nr * wb, tensor.data(), nr * wb,
                           hipMemcpyHostToDevice, s));
    st = upload(dev, dvec, p->p_random.data() + i * np * limbs, np * wb);
    if (st) return st;
    st = encode_rows_any(e, dvec.as<uint32_t>(), np, np, denc.as<uint32_t>() + i * nc * limbs * 2, nc, 1, s);
    if (st) return st;
    st = to_repr_host(dev, fid, dvec.as<uint32_t>(), np, &repr);
    if (st) return st;
    tr->append_messages(LABEL_PR, 6, repr, wb, np);
    if ((st = transcript_status(tr))) return st;
  }
  st = upload(dev, dvec, p->p_eval.data(), np * wb);
  if (st) return st;
  st = to_repr_host(dev, fid, dvec.as<uint32_t>(), np, &repr);
  if (st) return st;
  tr->append_messages(LABEL_PE, 6, repr, wb, np);
  std::vector<uint64_t> idx;
  challenge_columns(*tr, nc, nco, idx);
  if ((st = transcript_status(tr))) return st;
  st = encode_rows_any(e, dvec.as<uint32_t>(), np, np, denc.as<uint32_t>() + ndt * nc * limbs * 2, nc, 1, s);
  if (st) return st;

  // per-column checks (:953-974)
  st = upload(dev, didx, idx.data(), nco * 8);
  if (st) return st;
  st = upload(dev, dcols, p->cols.data(), nco * nr * wb);
  if (st) return st;
  st = upload(dev, dpaths, p->paths.data(), nco * p->path_len * 32);
  if (st) return st;
  st = upload(dev, droot, root, 32);
  if (st) return st;
  HIP_TRY(dflags.alloc(dev, nco * (ndt + 1) * 4));
  HIP_TRY(dpflags.alloc(dev, nco * 4));
  HIP_TRY(dleaves.alloc(dev, nco * 32));
  HIP_TRY(scratch.alloc(dev, leaf_hash_scratch_bytes(fid, nr, nco)));
  HIP_TRY(column_checks(fid, dcols.as<uint32_t>(), nco, nr, dtens.as<uint32_t>(), (int)(ndt + 1),
                        denc.as<uint32_t>(), nc, didx.as<uint64_t>(), dflags.as<uint32_t>(), s));
  // the verifier's encoding says which digest the root belongs to
  HIP_TRY(leaf_hashes_cols_d(e->digest, fid, dcols.as<uint32_t>(), nr, nco, dleaves.as<uint8_t>(), scratch.p, s));
  HIP_TRY(path_checks_d(e->digest, dleaves.as<uint8_t>(), dpaths.as<uint8_t>(), nco, p->path_len,
                        didx.as<uint64_t>(), droot.as<uint8_t>(), dpflags.as<uint32_t>(), s));
  std::vector<uint32_t> flags(nco * (ndt + 1)), pflags(nco);
  HIP_TRY(hipMemcpyAsync(flags.data(), dflags.p, flags.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(pflags.data(), dpflags.p, pflags.size() * 4, hipMemcpyDeviceToHost, s));
  // final inner product (:977-981)
  st = upload(dev, dinner, inner, np * wb);
  if (st) return st;
  HIP_TRY(dout.alloc(dev, wb));
  HIP_TRY(dot(fid, dinner.as<uint32_t>(), dvec.as<uint32_t>(), np, dout.as<uint32_t>(), nullptr, s));
  std::vector<uint64_t> ev(limbs);
  HIP_TRY(hipMemcpyAsync(ev.data(), dout.p, wb, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t k = 0; k < nco; k++) {
    bool rnd = true;
    for (size_t i = 0; i < ndt; i++) rnd &= flags[k * (ndt + 1) + i] != 0;
    const bool ev_ok = flags[k * (ndt + 1) + ndt] != 0;
    if (!rnd) return fail(LCPC_VERIFIER_COLUMN_DEGREE, "VerifierError::ColumnDegree");
    if (!ev_ok) return fail(LCPC_VERIFIER_COLUMN_EVAL, "VerifierError::ColumnEval");
    if (!pflags[k]) return fail(LCPC_VERIFIER_COLUMN_PATH, "VerifierError::ColumnPath");
  }
  if (eval_out) std::memcpy(eval_out, ev.data(), wb);
  return LCPC_OK;
}

// prove / verify over a caller-owned transcript for the length of one call (the reference's
// `&mut Transcript` argument, lcpc-2d/src/lib.rs:319-326, 547-556)
lcpc_status lcpc_prove_ops(const lcpc_commit *c, const uint64_t *outer, size_t outer_len, const lcpc_encoding *e,
                           const lcpc_transcript_ops *ops, lcpc_proof **out) {
  if (!ops || !ops->append_message || !ops->challenge_bytes)
    return fail(LCPC_ERR_INVALID_ARG, "transcript ops need append_message and challenge_bytes");
  lcpc_transcript tr(*ops);
  return lcpc_prove(c, outer, outer_len, e, &tr, out);
}
lcpc_status lcpc_verify_ops(const uint8_t root[32], const uint64_t *outer, size_t outer_len, const uint64_t *inner,
                            size_t inner_len, const lcpc_proof *p, const lcpc_encoding *e,
                            const lcpc_transcript_ops *ops, uint64_t *eval_out) {
  if (!ops || !ops->append_message || !ops->challenge_bytes)
    return fail(LCPC_ERR_INVALID_ARG, "transcript ops need append_message and challenge_bytes");
  lcpc_transcript tr(*ops);
  return lcpc_verify(root, outer, outer_len, inner, inner_len, p, e, &tr, eval_out);
}

// ---------------------------------------------------------------- free functions

lcpc_status lcpc_collapse_columns(lcpc_field f, const uint64_t *coeffs, const uint64_t *tensor,
                                  uint64_t *poly, size_t n_rows, size_t n_per_row) {
  if (!valid_field(f)) return fail(LCPC_ERR_INVALID_ARG, "field");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(f);
  DBuf dc, dt, dp, scratch;
  if ((st = upload(dev, dc, coeffs, n_rows * n_per_row * wb))) return st;
  if ((st = upload(dev, dt, tensor, n_rows * wb))) return st;
  HIP_TRY(dp.alloc(dev, n_per_row * wb));
  HIP_TRY(scratch.alloc(dev, collapse_scratch_bytes(f, n_rows, n_per_row, 1)));
  HIP_TRY(collapse_rows(f, dc.as<uint32_t>(), n_rows, n_per_row, dt.as<uint32_t>(), 1, dp.as<uint32_t>(),
                        scratch.p, lease.s));
  HIP_TRY(hipMemcpyAsync(poly, dp.p, n_per_row * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_merkle_tree(const uint8_t *ins, size_t n_ins, uint8_t *outs) {
  return lcpc_merkle_tree_d(LCPC_DIGEST_BLAKE3, ins, n_ins, outs);
}

lcpc_status lcpc_merkle_tree_d(lcpc_digest d, const uint8_t *ins, size_t n_ins, uint8_t *outs) {
  if (!digest_valid((int)d)) return fail(LCPC_ERR_INVALID_ARG, "digest");
  if (!n_ins || (n_ins & (n_ins - 1))) return fail(LCPC_ERR_INVALID_ARG, "ins.len() must be 2^k");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf t;
  HIP_TRY(t.alloc(dev, (2 * n_ins - 1) * 32));
  HIP_TRY(hipMemcpyAsync(t.p, ins, n_ins * 32, hipMemcpyHostToDevice, lease.s));
  HIP_TRY(merkle_tree_d((int)d, t.as<uint8_t>(), n_ins, lease.s));
  if (n_ins > 1)
    HIP_TRY(hipMemcpyAsync(outs, t.as<uint8_t>() + n_ins * 32, (n_ins - 1) * 32, hipMemcpyDeviceToHost,
                           lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_hash_columns(lcpc_field f, const uint64_t *comm, size_t n_rows, size_t n_cols,
                              uint8_t *out) {
  return lcpc_hash_columns_d(LCPC_DIGEST_BLAKE3, f, comm, n_rows, n_cols, out);
}

lcpc_status lcpc_hash_columns_d(lcpc_digest d, lcpc_field f, const uint64_t *comm, size_t n_rows, size_t n_cols,
                                uint8_t *out) {
  if (!digest_valid((int)d)) return fail(LCPC_ERR_INVALID_ARG, "digest");
  if (!valid_field(f) || !field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(f);
  DBuf dm, dl, scratch;
  if ((st = upload(dev, dm, comm, n_rows * n_cols * wb))) return st;
  HIP_TRY(dl.alloc(dev, n_cols * 32));
  HIP_TRY(scratch.alloc(dev, leaf_hash_scratch_bytes(f, n_rows, n_cols)));
  HIP_TRY(leaf_hashes_d((int)d, f, dm.as<uint32_t>(), n_rows, n_cols, n_cols, dl.as<uint8_t>(), scratch.p, lease.s));
  HIP_TRY(hipMemcpyAsync(out, dl.p, n_cols * 32, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

int lcpc_verify_column_path(lcpc_field f, const uint64_t *col, size_t n_rows, const uint8_t *path,
                            size_t path_len, size_t col_num, const uint8_t root[32]) {
  return lcpc_verify_column_path_d(LCPC_DIGEST_BLAKE3, f, col, n_rows, path, path_len, col_num, root);
}

int lcpc_verify_column_path_d(lcpc_digest d, lcpc_field f, const uint64_t *col, size_t n_rows, const uint8_t *path,
                              size_t path_len, size_t col_num, const uint8_t root[32]) {
  if (!digest_valid((int)d)) return 0;
  if (!valid_field(f) || !field_gpu_supported(f)) return 0;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return 0;
  Lease lease(dev);
  if (hipSetDevice(dev->id) != hipSuccess) return 0;
  const int wb = field_bytes(f);
  DBuf dc, dp, di, dr, dl, dfl, scratch;
  const uint64_t idx = col_num;
  if (upload(dev, dc, col, n_rows * wb) || upload(dev, dp, path, path_len * 32) ||
      upload(dev, di, &idx, 8) || upload(dev, dr, root, 32))
    return 0;
  if (dl.alloc(dev, 32) || dfl.alloc(dev, 4) || scratch.alloc(dev, leaf_hash_scratch_bytes(f, n_rows, 1)))
    return 0;
  if (leaf_hashes_cols_d((int)d, f, dc.as<uint32_t>(), n_rows, 1, dl.as<uint8_t>(), scratch.p, lease.s) ||
      path_checks_d((int)d, dl.as<uint8_t>(), dp.as<uint8_t>(), 1, path_len, di.as<uint64_t>(), dr.as<uint8_t>(),
                  dfl.as<uint32_t>(), lease.s))
    return 0;
  uint32_t flag = 0;
  if (hipMemcpyAsync(&flag, dfl.p, 4, hipMemcpyDeviceToHost, lease.s) ||
      hipStreamSynchronize(lease.s))
    return 0;
  return flag != 0;
}

lcpc_status lcpc_hash_field_columns(lcpc_field f, const uint64_t *cols, size_t n_rows, size_t n_cols,
                                    uint8_t *out) {
  // hash_field_vec_to_digest / hash_column_to_digest (lcpc_online.rs:431-452) for n_cols
  // columns given one after another ([n_cols][n_rows])
  if (!valid_field(f) || !field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field");
  if ((!cols && n_rows * n_cols) || (!out && n_cols)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_cols) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(f);
  DBuf dm, dl, scratch;
  if ((st = upload(dev, dm, cols, n_rows * n_cols * wb))) return st;
  HIP_TRY(dl.alloc(dev, n_cols * 32));
  HIP_TRY(scratch.alloc(dev, leaf_hash_scratch_bytes(f, n_rows, n_cols)));
  HIP_TRY(leaf_hashes_cols(f, dm.as<uint32_t>(), n_rows, n_cols, dl.as<uint8_t>(), scratch.p, lease.s));
  HIP_TRY(hipMemcpyAsync(out, dl.p, n_cols * 32, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_verify_leaf_paths(const uint8_t *leaves, const uint8_t *paths, size_t n,
                                   size_t path_len, const uint64_t *idx, const uint8_t root[32],
                                   uint8_t *ok) {
  // client_online_verify_column_paths_without_full_columns (lcpc_online.rs:280-318): ok[k] = 1
  // iff the path of leaf digest k at column idx[k] hashes up to root
  if ((!leaves || !paths || !idx || !ok) && n) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!root) return fail(LCPC_ERR_INVALID_ARG, "null root");
  if (!n) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf dl, dp, di, dr, dfl;
  // exactly the caller's n * path_len digests (none when path_len is 0: an empty upload still
  // allocates a block, and k_path_checks then reads no path word)
  if ((st = upload(dev, dl, leaves, n * 32)) || (st = upload(dev, dp, paths, n * path_len * 32)) ||
      (st = upload(dev, di, idx, n * 8)) || (st = upload(dev, dr, root, 32)))
    return st;
  HIP_TRY(dfl.alloc(dev, n * 4));
  HIP_TRY(path_checks(dl.as<uint8_t>(), dp.as<uint8_t>(), n, path_len, di.as<uint64_t>(), dr.as<uint8_t>(),
                      dfl.as<uint32_t>(), lease.s));
  std::vector<uint32_t> fl(n);
  HIP_TRY(hipMemcpyAsync(fl.data(), dfl.p, n * 4, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  for (size_t k = 0; k < n; k++) ok[k] = fl[k] ? 1 : 0;
  return LCPC_OK;
}

lcpc_status lcpc_verify_column_values(lcpc_field f, const uint64_t *cols, size_t n, size_t n_rows,
                                      const uint64_t *tensor, const uint64_t *values, size_t n_values,
                                      const uint64_t *idx, uint8_t *ok) {
  // verify_column_value (lcpc-2d/src/lib.rs:1014-1030) for n columns at once, also
  // verify_proper_partial_polynomial_evaluation's check (lcpc_online.rs:487-516): ok[k] = 1 iff
  // sum_r tensor[r] cols[k][r] == values[idx[k]]
  if (!valid_field(f) || !field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field");
  if ((!cols || !idx || !ok) && n) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if ((!tensor && n_rows) || (!values && n_values)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  for (size_t k = 0; k < n; k++)
    if (idx[k] >= n_values) return fail(LCPC_ERR_INVALID_ARG, "value index out of range");
  if (!n) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(f);
  DBuf dc, dt, dv, di, dfl;
  if ((st = upload(dev, dc, cols, n * n_rows * wb)) || (st = upload(dev, dt, tensor, n_rows * wb)) ||
      (st = upload(dev, dv, values, n_values * wb)) || (st = upload(dev, di, idx, n * 8)))
    return st;
  HIP_TRY(dfl.alloc(dev, n * 4));
  HIP_TRY(column_checks(f, dc.as<uint32_t>(), n, n_rows, dt.as<uint32_t>(), 1, dv.as<uint32_t>(), n_values,
                        di.as<uint64_t>(), dfl.as<uint32_t>(), lease.s));
  std::vector<uint32_t> fl(n);
  HIP_TRY(hipMemcpyAsync(fl.data(), dfl.p, n * 4, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  for (size_t k = 0; k < n; k++) ok[k] = fl[k] ? 1 : 0;
  return LCPC_OK;
}

int lcpc_verify_column_value(lcpc_field f, const uint64_t *col, const uint64_t *tensor,
                             size_t n_rows, const uint64_t *poly_eval) {
  if (!valid_field(f)) return 0;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return 0;
  Lease lease(dev);
  if (hipSetDevice(dev->id) != hipSuccess) return 0;
  const int wb = field_bytes(f);
  DBuf dc, dt, de, di, dfl;
  const uint64_t zero = 0;
  if (upload(dev, dc, col, n_rows * wb) || upload(dev, dt, tensor, n_rows * wb) ||
      upload(dev, de, poly_eval, wb) || upload(dev, di, &zero, 8) || dfl.alloc(dev, 4))
    return 0;
  if (column_checks(f, dc.as<uint32_t>(), 1, n_rows, dt.as<uint32_t>(), 1, de.as<uint32_t>(), 1,
                    di.as<uint64_t>(), dfl.as<uint32_t>(), lease.s))
    return 0;
  uint32_t flag = 0;
  if (hipMemcpyAsync(&flag, dfl.p, 4, hipMemcpyDeviceToHost, lease.s) ||
      hipStreamSynchronize(lease.s))
    return 0;
  return flag != 0;
}

}  // extern "C"

// ================================================================= proof-of-storage producers
namespace {

// Encode `len` host elements with e into a temporary row-major codeword (Leaves /
// ColumnsWithoutPath requests, lcpc_online.rs:144-224): no commitment, no Merkle tree.
lcpc_status encode_matrix(const lcpc_encoding *e, const uint64_t *elems, size_t len, DBuf &comm,
                          size_t *n_rows_out, hipStream_t s) {
  const size_t np = e->n_per_row, nc = e->n_cols;
  const size_t n_rows = (len + np - 1) / np;
  const int wb = field_bytes(e->fid);
  DBuf coeffs;
  HIP_TRY(coeffs.alloc(e->dev, n_rows * np * wb));
  HIP_TRY(hipMemcpyAsync(coeffs.p, elems, len * wb, hipMemcpyHostToDevice, s));
  if (n_rows * np > len)
    HIP_TRY(hipMemsetAsync(coeffs.as<uint8_t>() + len * wb, 0, (n_rows * np - len) * wb, s));
  HIP_TRY(comm.alloc(e->dev, n_rows * nc * wb));
  lcpc_status st = encode_rows_any(e, coeffs.as<uint32_t>(), np, np, comm.as<uint32_t>(), nc, n_rows, s);
  if (st) return st;
  *n_rows_out = n_rows;
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_bytes_to_field_device(const void *d_bytes, size_t n_bytes, void *d_out,
                                           void *stream) {
  if ((!d_bytes || !d_out) && n_bytes) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)d_bytes & 7) || ((uintptr_t)d_out & 7))
    return fail(LCPC_ERR_INVALID_ARG, "device buffers must be 8-byte aligned");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : lease.s;
  HIP_TRY(pos_pack7((const uint8_t *)d_bytes, n_bytes, (uint64_t *)d_out, s));
  if (!stream) HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

lcpc_status lcpc_pos_bytes_to_field(const uint8_t *bytes, size_t n_bytes, uint64_t *out,
                                    size_t *n_out) {
  if ((!bytes || !out) && n_bytes) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  const size_t n = (n_bytes + 6) / 7;
  if (n_out) *n_out = n;
  if (!n) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf db, de;
  if ((st = upload(dev, db, bytes, n_bytes))) return st;
  HIP_TRY(de.alloc(dev, n * 8));
  HIP_TRY(pos_pack7(db.as<uint8_t>(), n_bytes, de.as<uint64_t>(), lease.s));
  HIP_TRY(hipMemcpyAsync(out, de.p, n * 8, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_pos_field_to_bytes(const uint64_t *elems, size_t n, uint8_t *out,
                                    size_t expected_len) {
  if ((!elems && n) || (!out && expected_len)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (expected_len > 7 * n) return fail(LCPC_ERR_INVALID_ARG, "expected_len > 7 * n");
  if (!expected_len) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf de, db;
  if ((st = upload(dev, de, elems, n * 8))) return st;
  HIP_TRY(db.alloc(dev, expected_len));
  HIP_TRY(pos_unpack7(de.as<uint64_t>(), n, db.as<uint8_t>(), expected_len, lease.s));
  HIP_TRY(hipMemcpyAsync(out, db.p, expected_len, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

void lcpc_pos_default_dims(size_t field_len, size_t *n_per_row, size_t *n_cols, size_t *soundness) {
  // get_aspect_ratio_default_from_field_len (networking/server.rs:1139-1158): f32 sqrt
  const size_t w = (size_t)std::ceil(std::sqrt((float)field_len));
  const size_t np = (w & (w - 1)) == 0 ? w : next_pow2(w);  // fields::is_power_of_two
  const size_t nc = next_pow2(np + 1);
  // get_soundness_from_matrix_dims (:1160-1170)
  const double den = std::log2((1.0 + (double)np / (double)nc) / 2.0);
  const size_t th = (size_t)std::ceil(-128.0 / den);
  if (n_per_row) *n_per_row = np;
  if (n_cols) *n_cols = nc;
  if (soundness) *soundness = th < nc ? th : nc;
}

lcpc_status lcpc_pos_column_indices(uint64_t seed, size_t amount, size_t max_index, uint64_t *out,
                                    size_t *n_out) {
  // get_column_indicies_from_random_seed (networking/client.rs:443-456): ChaCha8Rng +
  // IteratorRandom::choose_multiple (rand 0.8 reservoir; gen_index = gen_range(0..ub as u32))
  if (!out && amount) return fail(LCPC_ERR_INVALID_ARG, "null out");
  ChaCha20Rng rng = ChaCha20Rng::seed_from_u64(seed, 8);
  size_t filled = 0;
  for (size_t i = 0; i < max_index && filled < amount; i++) out[filled++] = i;
  if (filled == amount) {
    for (size_t i = 0; amount + i < max_index; i++) {
      const size_t ub = i + 1 + amount;
      size_t k;
      if (ub <= 0xffffffffu) {
        const uint32_t range = (uint32_t)ub;
        const uint32_t zone = (range << __builtin_clz(range)) - 1;
        for (;;) {
          const uint64_t m = (uint64_t)rng.next_u32() * range;
          if ((uint32_t)m <= zone) {
            k = (size_t)(m >> 32);
            break;
          }
        }
      } else {
        const uint64_t zone = ((uint64_t)ub << __builtin_clzll((uint64_t)ub)) - 1;
        for (;;) {
          const unsigned __int128 m = (unsigned __int128)rng.next_u64() * ub;
          if ((uint64_t)m <= zone) {
            k = (size_t)(m >> 64);
            break;
          }
        }
      }
      if (k < amount) out[k] = amount + i;
    }
  }
  if (n_out) *n_out = filled;
  return LCPC_OK;
}

lcpc_status lcpc_pos_side_vectors(lcpc_field f, const uint64_t *x, size_t n_rows, size_t n_cols,
                                  uint64_t *left, uint64_t *right) {
  // form_side_vectors_for_polynomial_evaluation_from_point (lcpc_online.rs:603-627):
  // right = [1, x, ..., x^(n_cols-1)], left = [1, x^n_cols, x^(2 n_cols), ...]
  if (!valid_field(f) || !x || (!left && n_rows) || (!right && n_cols))
    return fail(LCPC_ERR_INVALID_ARG, "side vector arguments");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(f);
  DBuf dx, dl, dr;
  if ((st = upload(dev, dx, x, wb))) return st;
  HIP_TRY(dl.alloc(dev, n_rows * wb));
  HIP_TRY(dr.alloc(dev, n_cols * wb));
  HIP_TRY(powers(f, dx.as<uint32_t>(), 1, n_cols, dr.as<uint32_t>(), lease.s));
  HIP_TRY(powers(f, dx.as<uint32_t>(), (uint64_t)n_cols, n_rows, dl.as<uint32_t>(), lease.s));
  if (n_cols) HIP_TRY(hipMemcpyAsync(right, dr.p, n_cols * wb, hipMemcpyDeviceToHost, lease.s));
  if (n_rows) HIP_TRY(hipMemcpyAsync(left, dl.p, n_rows * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_pos_eval_encoded(const lcpc_commit *c, const uint64_t *left, size_t n_rows,
                                  uint64_t *out) {
  // verifiable_polynomial_evaluation (lcpc_online.rs:454-484): out[j] = sum_r left[r] comm[r][j]
  if (!c || !left || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (n_rows != c->n_rows) return fail(LCPC_ERR_INVALID_ARG, "left vector length != n_rows");
  if (c->col_major) return fail(LCPC_ERR_UNSUPPORTED, "row-major (Ligero) commitments only");
  Device *dev = c->dev;
  Lease lease(dev, POOL_HIGH);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(c->fid);
  DBuf dt, dout, scratch;
  lcpc_status st;
  if ((st = upload(dev, dt, left, n_rows * wb))) return st;
  HIP_TRY(dout.alloc(dev, c->n_cols * wb));
  HIP_TRY(scratch.alloc(dev, collapse_scratch_bytes(c->fid, n_rows, c->n_cols, 1)));
  HIP_TRY(collapse_rows(c->fid, c->comm.as<uint32_t>(), n_rows, c->n_cols, dt.as<uint32_t>(), 1,
                        dout.as<uint32_t>(), scratch.p, lease.s));
  // over a canonical matrix the Montgomery products come out as canonical values
  if (c->canon) HIP_TRY(convert(c->fid, dout.as<uint32_t>(), dout.as<uint32_t>(), c->n_cols, true, lease.s));
  HIP_TRY(d2h_staged(out, dout.p, c->n_cols * wb, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_ifft_oi_rows(lcpc_field f, uint64_t *rows, size_t n_rows, size_t len) {
  // fffft::ifft_oi on each row (decode_row, lcpc_online.rs:568-574): bit-reversed evaluations
  // in, natural-order coefficients out
  if (!valid_field(f) || (!rows && n_rows)) return fail(LCPC_ERR_INVALID_ARG, "arguments");
  if (!field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field has no gfx950 kernels");
  lcpc_status st = check_fft_len(f, len);
  if (st) return st;
  if (n_rows == 0) return LCPC_OK;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int log_n = (int)log2_np2(len);
  const int wb = field_bytes(f);
  InversePlan inverse;
  if ((st = inverse.init(f, log_n, lease.s))) return st;
  DBuf a, b;
  if ((st = upload(dev, a, rows, n_rows * len * wb))) return st;
  HIP_TRY(b.alloc(dev, n_rows * len * wb));
  uint32_t *x = nullptr, *y = nullptr;
  if ((st = ifft_oi_device(inverse.plan, f, log_n, a.as<uint32_t>(), b.as<uint32_t>(), n_rows, lease.s, &x, &y))) return st;
  HIP_TRY(hipMemcpyAsync(rows, x, n_rows * len * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_open_columns(const lcpc_commit *c, const uint64_t *idx, size_t n, uint64_t *cols_out,
                              uint8_t *paths_out) {
  // open_column (lcpc-2d/src/lib.rs:818-855) for n columns at once (PoS server_retreive_columns,
  // lcpc_online.rs:241-247)
  if (!c || (!idx && n)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  for (size_t k = 0; k < n; k++)
    if (idx[k] >= c->n_cols) return fail(LCPC_PROVER_COLUMN_NUMBER, "ProverError::ColumnNumber");
  if (!n) return LCPC_OK;
  Device *dev = c->dev;
  Lease lease(dev, POOL_HIGH);
  HIP_TRY(hipSetDevice(dev->id));
  const size_t path_len = log2_np2(c->n_cols);
  const int wb = field_bytes(c->fid);
  DBuf didx, dcol, dpath;
  lcpc_status st;
  if ((st = upload(dev, didx, idx, n * 8))) return st;
  HIP_TRY(dcol.alloc(dev, n * c->n_rows * wb));
  HIP_TRY(dpath.alloc(dev, n * path_len * 32 + 32));
  HIP_TRY(gather_columns(c->fid, c->comm.as<uint32_t>(), c->n_rows, c->n_cols, didx.as<uint64_t>(), n,
                         dcol.as<uint32_t>(), lease.s, c->col_major, c->canon));
  HIP_TRY(gather_paths(c->hashes.as<uint8_t>(), c->n_hashes, didx.as<uint64_t>(), n, path_len,
                       dpath.as<uint8_t>(), lease.s));
  if (cols_out) HIP_TRY(d2h_staged(cols_out, dcol.p, n * c->n_rows * wb, lease.s));
  if (paths_out && path_len)
    HIP_TRY(d2h_staged(paths_out, dpath.p, n * path_len * 32, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_pos_columns(const lcpc_encoding *e, const uint64_t *elems, size_t len,
                             const uint64_t *idx, size_t n, uint64_t *cols_out, uint8_t *leaves_out) {
  // CommitRequestType::ColumnsWithoutPath / Leaves (lcpc_online.rs:144-224): encode the file,
  // then return the requested columns and / or their BLAKE3 leaf digests -- no Merkle tree
  if (!e || !elems || len == 0 || (!idx && n)) return fail(LCPC_ERR_INVALID_ARG, "arguments");
  if (lcpc_status bst = require_blake3(e, "lcpc_pos_columns")) return bst;
  for (size_t k = 0; k < n; k++)
    if (idx[k] >= e->n_cols) return fail(LCPC_PROVER_COLUMN_NUMBER, "ProverError::ColumnNumber");
  Device *dev = e->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf comm, didx, dcol, dleaves, scratch;
  size_t n_rows = 0;
  lcpc_status st = encode_matrix(e, elems, len, comm, &n_rows, lease.s);
  if (st) return st;
  if (!n) return LCPC_OK;
  const int wb = field_bytes(e->fid);
  if ((st = upload(dev, didx, idx, n * 8))) return st;
  HIP_TRY(dcol.alloc(dev, n * n_rows * wb));
  HIP_TRY(gather_columns(e->fid, comm.as<uint32_t>(), n_rows, e->n_cols, didx.as<uint64_t>(), n,
                         dcol.as<uint32_t>(), lease.s));
  if (leaves_out) {
    HIP_TRY(dleaves.alloc(dev, n * 32));
    HIP_TRY(scratch.alloc(dev, leaf_hash_scratch_bytes(e->fid, n_rows, n)));
    HIP_TRY(leaf_hashes_cols(e->fid, dcol.as<uint32_t>(), n_rows, n, dleaves.as<uint8_t>(), scratch.p,
                             lease.s));
    HIP_TRY(hipMemcpyAsync(leaves_out, dleaves.p, n * 32, hipMemcpyDeviceToHost, lease.s));
  }
  if (cols_out) HIP_TRY(hipMemcpyAsync(cols_out, dcol.p, n * n_rows * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

}  // extern "C"

// ================================================================= update audits (pos_eval.hip)
namespace {

// sum_{i<n} c_i x^(i + d) from a device source (elements of field f, or with n_bytes a file image)
lcpc_status eval_poly_dev(Device *dev, hipStream_t s, int f, const void *d_src, size_t n, size_t n_bytes,
                          const uint64_t *x, uint64_t d, uint64_t *out) {
  const int wb = field_bytes(f);
  DBuf dx, dout, scratch;
  lcpc_status st;
  if ((st = upload(dev, dx, x, wb))) return st;
  HIP_TRY(dout.alloc(dev, wb));
  HIP_TRY(scratch.alloc(dev, poly_eval_scratch_bytes(f, n)));
  HIP_TRY(poly_eval(f, d_src, n, n_bytes, dx.as<uint32_t>(), d, dout.as<uint32_t>(), scratch.p, s));
  HIP_TRY(hipMemcpyAsync(out, dout.p, wb, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

lcpc_status eval_poly_args(lcpc_field f, const void *coeffs, size_t n, const uint64_t *x, uint64_t *out) {
  if (!valid_field(f) || !x || !out || (!coeffs && n)) return fail(LCPC_ERR_INVALID_ARG, "polynomial evaluation arguments");
  if (!field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field has no gfx950 kernels");
  return LCPC_OK;
}

// u^T M over a device file image: rows of pre elements, left (host) of n_left = the row count
lcpc_status left_multiply_dev(Device *dev, hipStream_t s, const uint8_t *d_bytes, size_t n_bytes, size_t pre,
                              const uint64_t *left, size_t n_left, uint64_t *out) {
  const size_t len = (n_bytes + 6) / 7, n_rows = (len + pre - 1) / pre;
  if (n_left != n_rows) return fail(LCPC_ERR_INVALID_ARG, "left vector length != the file's row count");
  DBuf dl, dout, scratch, m;
  lcpc_status st;
  if ((st = upload(dev, dl, left, n_rows * 8))) return st;
  HIP_TRY(dout.alloc(dev, pre * 8));
  if (pos_left_mul_bytes_ok(pre)) {
    HIP_TRY(scratch.alloc(dev, pos_left_mul_bytes_scratch_bytes(pre, n_rows)));
    HIP_TRY(pos_left_mul_bytes(d_bytes, n_bytes, pre, n_rows, dl.as<uint32_t>(), dout.as<uint32_t>(), scratch.p, s));
  } else {
    // other widths: the element image (zero padded to whole rows), then the commitment's collapse
    HIP_TRY(m.alloc(dev, n_rows * pre * 8));
    if (n_rows * pre > len) HIP_TRY(hipMemsetAsync(m.as<uint64_t>() + len, 0, (n_rows * pre - len) * 8, s));
    HIP_TRY(pos_pack7(d_bytes, n_bytes, m.as<uint64_t>(), s));
    HIP_TRY(scratch.alloc(dev, collapse_scratch_bytes(LCPC_FT63, n_rows, pre, 1)));
    HIP_TRY(collapse_rows(LCPC_FT63, m.as<uint32_t>(), n_rows, pre, dl.as<uint32_t>(), 1, dout.as<uint32_t>(), scratch.p,
                          s));
  }
  HIP_TRY(hipMemcpyAsync(out, dout.p, pre * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

// ---- many vectors, one pass over the image (batched audits of a stored file)
static_assert(LCPC_BATCH_MAX_TENSORS == POS_LEFT_MANY_MAX_VECS, "header bound = kernel bound");

lcpc_status left_multiply_many_args(const void *bytes, size_t n_bytes, size_t pre, const uint64_t *lefts, size_t n_vecs,
                                    size_t n_left, uint64_t *out) {
  if (!bytes || !n_bytes || !pre || !lefts || !out) return fail(LCPC_ERR_INVALID_ARG, "null or empty argument");
  if (n_vecs == 0 || n_vecs > LCPC_BATCH_MAX_TENSORS)
    return fail(LCPC_ERR_INVALID_ARG, "n_vecs must be in [1, LCPC_BATCH_MAX_TENSORS]");
  const size_t len = (n_bytes + 6) / 7, n_rows = (len + pre - 1) / pre;
  if (n_left != n_rows) return fail(LCPC_ERR_INVALID_ARG, "left vector length != the file's row count");
  return LCPC_OK;
}

// the state of one many-vector product: the vectors and the kernel's tables on the device, then
// piece(...) for every run of whole rows of the image, in order, then finish()
struct LeftMany {
  Device *dev;
  hipStream_t s;
  size_t n_bytes, pre, n_vecs, n_rows, piece_rows;
  int kernel;
  DBuf dl, prep, partials, dout;
  size_t splits_done = 0;

  // piece_rows: the rows per piece of a staged image (even), 0 = the whole image in one piece
  lcpc_status begin(const uint64_t *lefts, size_t rows_per_piece) {
    n_rows = ((n_bytes + 6) / 7 + pre - 1) / pre;
    piece_rows = rows_per_piece ? rows_per_piece : n_rows;
    kernel = pos_left_mul_many_kernel(pre, n_vecs);
    lcpc_status st;
    if ((st = upload(dev, dl, lefts, n_vecs * n_rows * 8))) return st;
    HIP_TRY(dout.alloc(dev, n_vecs * pre * 8));
    if (kernel == POS_LEFT_MANY_PACK) return LCPC_OK;
    const size_t full = n_rows / piece_rows, rest = n_rows % piece_rows;
    const size_t splits = full * pos_left_mul_many_splits(kernel, pre, piece_rows, n_vecs) +
                          (rest ? pos_left_mul_many_splits(kernel, pre, rest, n_vecs) : 0);
    HIP_TRY(partials.alloc(dev, splits * n_vecs * pre * 8));
    HIP_TRY(prep.alloc(dev, std::max<size_t>(pos_left_mul_many_prep_bytes(kernel, n_rows, n_vecs), 8)));
    HIP_TRY(pos_left_mul_many_prepare(kernel, dl.as<uint32_t>(), n_rows, n_vecs, prep.p, s));
    return LCPC_OK;
  }
  // rows [row0, row0 + rows) of the image at d_piece (bytes: to the image's end at most)
  lcpc_status piece(const uint8_t *d_piece, size_t bytes, size_t row0, size_t rows) {
    HIP_TRY(pos_left_mul_many_partials(kernel, d_piece, bytes, pre, rows, row0, dl.as<uint32_t>(), n_rows, n_vecs,
                                       prep.p, partials.as<uint32_t>() + 2 * splits_done * n_vecs * pre, s));
    splits_done += pos_left_mul_many_splits(kernel, pre, rows, n_vecs);
    return LCPC_OK;
  }
  // other widths: the element image (zero padded to whole rows), then the commitment's many-tensor collapse
  lcpc_status pack_first(const uint8_t *d_bytes) {
    const size_t len = (n_bytes + 6) / 7;
    DBuf m, scratch;
    HIP_TRY(m.alloc(dev, n_rows * pre * 8));
    if (n_rows * pre > len) HIP_TRY(hipMemsetAsync(m.as<uint64_t>() + len, 0, (n_rows * pre - len) * 8, s));
    HIP_TRY(pos_pack7(d_bytes, n_bytes, m.as<uint64_t>(), s));
    HIP_TRY(scratch.alloc(dev, collapse_many_scratch_bytes(LCPC_FT63, n_rows, pre, n_vecs)));
    HIP_TRY(collapse_rows_many(LCPC_FT63, m.as<uint32_t>(), n_rows, pre, dl.as<uint32_t>(), n_vecs, dout.as<uint32_t>(),
                               scratch.p, s));
    return LCPC_OK;
  }
  lcpc_status finish(uint64_t *out) {
    if (kernel != POS_LEFT_MANY_PACK)
      HIP_TRY(pos_left_mul_many_fold(kernel, partials.as<uint32_t>(), splits_done, pre, n_rows, n_vecs, prep.p,
                                     dout.as<uint32_t>(), s));
    HIP_TRY(hipMemcpyAsync(out, dout.p, n_vecs * pre * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return LCPC_OK;
  }
};

}  // namespace

extern "C" {

lcpc_status lcpc_eval_poly(lcpc_field f, const uint64_t *coeffs, size_t n, const uint64_t *x, uint64_t degree_offset,
                           uint64_t *out) {
  lcpc_status st = eval_poly_args(f, coeffs, n, x, out);
  if (st) return st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf dc;
  if ((st = upload(dev, dc, coeffs, n * field_bytes(f)))) return st;
  return eval_poly_dev(dev, lease.s, f, dc.p, n, 0, x, degree_offset, out);
}

lcpc_status lcpc_eval_poly_device(lcpc_field f, const void *d_coeffs, size_t n, const uint64_t *x,
                                  uint64_t degree_offset, uint64_t *out) {
  lcpc_status st = eval_poly_args(f, d_coeffs, n, x, out);
  if (st) return st;
  if ((uintptr_t)d_coeffs & 7) return fail(LCPC_ERR_INVALID_ARG, "device coefficients must be 8-byte aligned");
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  return eval_poly_dev(dev, lease.s, f, d_coeffs, n, 0, x, degree_offset, out);
}

lcpc_status lcpc_pos_eval_poly_bytes_device(const void *d_bytes, size_t n_bytes, const uint64_t *x,
                                            uint64_t degree_offset, uint64_t *out) {
  lcpc_status st = eval_poly_args(LCPC_FT63, d_bytes, n_bytes, x, out);
  if (st) return st;
  if ((uintptr_t)d_bytes & 7) return fail(LCPC_ERR_INVALID_ARG, "device file image must be 8-byte aligned");
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  return eval_poly_dev(dev, lease.s, LCPC_FT63, d_bytes, (n_bytes + 6) / 7, n_bytes, x, degree_offset, out);
}

lcpc_status lcpc_pos_eval_poly_bytes(const uint8_t *bytes, size_t n_bytes, const uint64_t *x, uint64_t degree_offset,
                                     uint64_t *out) {
  lcpc_status st = eval_poly_args(LCPC_FT63, bytes, n_bytes, x, out);
  if (st) return st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  // The image goes up in staging blocks of whole tiles; block b's polynomial is evaluated as soon
  // as it has landed, elevated by the index of its first element, and the values are summed at the
  // end: x^degree_offset multiplies the sum (start + degree_offset could pass 2^64).
  constexpr size_t BLOCK = LCPC_POS_EVAL_STAGE_BYTES;
  static_assert(BLOCK % (7 * (size_t)POS_EVAL_TILE) == 0 && BLOCK % 16 == 0, "staging blocks of whole tiles");
  const size_t nb = (n_bytes + BLOCK - 1) / BLOCK;
  DBuf image, dx, vals, dout, scratch;
  if ((st = upload(dev, dx, x, 8))) return st;
  HIP_TRY(dout.alloc(dev, 8));
  HIP_TRY(vals.alloc(dev, std::max<size_t>(nb, 1) * 8));
  HIP_TRY(image.alloc(dev, n_bytes));
  const size_t sb = (poly_eval_scratch_bytes(LCPC_FT63, BLOCK / 7) + 255) & ~(size_t)255;
  HIP_TRY(scratch.alloc(dev, std::max<size_t>(nb, 1) * sb));
  st = h2d_blocks(dev, image.as<uint8_t>(), bytes, n_bytes, BLOCK, s, [&](size_t off, size_t n) -> lcpc_status {
    const size_t b = off / BLOCK;
    HIP_TRY(poly_eval(LCPC_FT63, image.as<uint8_t>() + off, (n + 6) / 7, n, dx.as<uint32_t>(), (uint64_t)(off / 7),
                      vals.as<uint32_t>() + 2 * b, scratch.as<uint8_t>() + b * sb, s));
    return LCPC_OK;
  });
  if (st) return st;
  HIP_TRY(poly_eval_sum_scale(LCPC_FT63, vals.as<uint32_t>(), nb, dx.as<uint32_t>(), degree_offset, dout.as<uint32_t>(), s));
  HIP_TRY(hipMemcpyAsync(out, dout.p, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

lcpc_status lcpc_pos_left_multiply_bytes_device(const void *d_bytes, size_t n_bytes, size_t pre, const uint64_t *left,
                                                size_t n_left, uint64_t *out) {
  if (!d_bytes || !n_bytes || !pre || !left || !out) return fail(LCPC_ERR_INVALID_ARG, "null or empty argument");
  if ((uintptr_t)d_bytes & 7) return fail(LCPC_ERR_INVALID_ARG, "device file image must be 8-byte aligned");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  return left_multiply_dev(dev, lease.s, (const uint8_t *)d_bytes, n_bytes, pre, left, n_left, out);
}

lcpc_status lcpc_pos_left_multiply_bytes(const uint8_t *bytes, size_t n_bytes, size_t pre, const uint64_t *left,
                                         size_t n_left, uint64_t *out) {
  if (!bytes || !n_bytes || !pre || !left || !out) return fail(LCPC_ERR_INVALID_ARG, "null or empty argument");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf image;
  HIP_TRY(image.alloc(dev, n_bytes));
  st = h2d_blocks(dev, image.as<uint8_t>(), bytes, n_bytes, (size_t)8 << 20, lease.s,
                  [](size_t, size_t) { return LCPC_OK; });
  if (st) return st;
  return left_multiply_dev(dev, lease.s, image.as<uint8_t>(), n_bytes, pre, left, n_left, out);
}

int lcpc_pos_left_multiply_many_kernel(size_t pre, size_t n_vecs) { return pos_left_mul_many_kernel(pre, n_vecs); }

lcpc_status lcpc_pos_left_multiply_bytes_many_device(const void *d_bytes, size_t n_bytes, size_t pre,
                                                     const uint64_t *lefts, size_t n_vecs, size_t n_left,
                                                     uint64_t *out) {
  lcpc_status st = left_multiply_many_args(d_bytes, n_bytes, pre, lefts, n_vecs, n_left, out);
  if (st) return st;
  if ((uintptr_t)d_bytes & 7) return fail(LCPC_ERR_INVALID_ARG, "device file image must be 8-byte aligned");
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  LeftMany lm{dev, lease.s, n_bytes, pre, n_vecs};
  if ((st = lm.begin(lefts, 0))) return st;
  if (lm.kernel == POS_LEFT_MANY_PACK)
    st = lm.pack_first((const uint8_t *)d_bytes);
  else
    st = lm.piece((const uint8_t *)d_bytes, n_bytes, 0, lm.n_rows);
  return st ? st : lm.finish(out);
}

lcpc_status lcpc_pos_left_multiply_bytes_many(const uint8_t *bytes, size_t n_bytes, size_t pre, const uint64_t *lefts,
                                              size_t n_vecs, size_t n_left, uint64_t *out) {
  lcpc_status st = left_multiply_many_args(bytes, n_bytes, pre, lefts, n_vecs, n_left, out);
  if (st) return st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  // The image goes up in staging blocks of whole rows (an even number of them, near 8 MiB); block
  // b's rows are contracted as soon as they have landed, one set of partials per block, and the
  // partials are folded at the end: field sums are exact, so the blocks do not show in the result.
  const size_t row_b = 7 * pre;
  const size_t block_rows = std::max<size_t>(2, (((size_t)8 << 20) / row_b) & ~(size_t)1);
  LeftMany lm{dev, lease.s, n_bytes, pre, n_vecs};
  DBuf image;
  HIP_TRY(image.alloc(dev, n_bytes));
  if ((st = lm.begin(lefts, block_rows))) return st;
  const bool pack = lm.kernel == POS_LEFT_MANY_PACK;
  st = h2d_blocks(dev, image.as<uint8_t>(), bytes, n_bytes, block_rows * row_b, lease.s,
                  [&](size_t off, size_t n) -> lcpc_status {
    if (pack) return LCPC_OK;
    const size_t r0 = off / row_b;
    return lm.piece(image.as<uint8_t>() + off, n, r0, std::min(block_rows, lm.n_rows - r0));
  });
  if (st) return st;
  if (pack && (st = lm.pack_first(image.as<uint8_t>()))) return st;
  return lm.finish(out);
}

lcpc_status lcpc_selftest_recombine63(const int32_t *y, uint64_t *out, size_t n) {
  if (!y || !out) return fail(LCPC_ERR_INVALID_ARG, "null accumulators or output");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  if (!n) return LCPC_OK;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf dy, dout;
  if ((st = upload(dev, dy, y, n * 8 * sizeof(int32_t)))) return st;
  HIP_TRY(dout.alloc(dev, n * 8));
  HIP_TRY(pos_recombine63(dy.as<int>(), dout.as<uint32_t>(), n, lease.s));
  HIP_TRY(hipMemcpyAsync(out, dout.p, n * 8, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_pos_update_rows(size_t old_len, size_t offset, size_t len, size_t pre, size_t *row_lo, size_t *row_hi,
                                 size_t *old_lo, size_t *old_hi) {
  if (!len || offset > old_len || !pre || !row_lo || !row_hi || !old_lo || !old_hi)
    return fail(LCPC_ERR_INVALID_ARG, "update: len == 0, offset > old_len, pre == 0 or a null result");
  if (pre > SIZE_MAX / 7 || len > SIZE_MAX - offset || offset + len > SIZE_MAX - 7 * pre)
    return fail(LCPC_ERR_INVALID_ARG, "update: range overflows");
  const size_t row_b = 7 * pre;
  *row_lo = offset / row_b;
  *row_hi = (offset + len - 1) / row_b + 1;
  *old_lo = std::min(*row_lo * row_b, old_len);
  *old_hi = std::min(*row_hi * row_b, old_len);
  return LCPC_OK;
}

lcpc_status lcpc_pos_update_evaluation(const lcpc_encoding *e_old, const void *d_old, size_t n_old,
                                       const lcpc_encoding *e_new, const void *d_new, size_t n_new, const uint64_t *x,
                                       const uint64_t *idx_old, size_t n_idx_old, const uint64_t *idx_new,
                                       size_t n_idx_new, uint64_t *result_old, uint64_t *cols_old, uint8_t *paths_old,
                                       uint8_t root_old[32], uint64_t *result_new, uint64_t *cols_new,
                                       uint8_t *paths_new, uint8_t root_new[32], uint64_t *expected_eval) {
  if (!e_old || !e_new || !d_old || !d_new || !n_old || !n_new || !x || !result_old || !result_new || !root_old ||
      !root_new)
    return fail(LCPC_ERR_INVALID_ARG, "null or empty argument");
  lcpc_status st;
  if ((st = require_blake3(e_old, "an update audit")) || (st = require_blake3(e_new, "an update audit"))) return st;
  if (e_old->fid != LCPC_FT63 || e_new->fid != LCPC_FT63)
    return fail(LCPC_ERR_INVALID_ARG, "update audit: WriteableFt63 encodings only");
  struct Side {
    const lcpc_encoding *e;
    const void *d;
    size_t n;
    const uint64_t *idx;
    size_t n_idx;
    uint64_t *result, *cols;
    uint8_t *paths, *root;
  } sides[2] = {{e_old, d_old, n_old, idx_old, n_idx_old, result_old, cols_old, paths_old, root_old},
                {e_new, d_new, n_new, idx_new, n_idx_new, result_new, cols_new, paths_new, root_new}};
  for (const Side &sd : sides) {
    // left = [1, x^pre, x^(2 pre), ...] over this commitment's rows: the value is the file polynomial's
    const size_t pre = sd.e->n_per_row;
    if (!pre) return fail(LCPC_ERR_INVALID_ARG, "encoding without dims");
    const size_t n_rows = ((sd.n + 6) / 7 + pre - 1) / pre;
    std::vector<uint64_t> left(n_rows);
    {
      Device *dev = sd.e->dev;
      Lease lease(dev, POOL_HIGH);
      HIP_TRY(hipSetDevice(dev->id));
      DBuf dx, dl;
      if ((st = upload(dev, dx, x, 8))) return st;
      HIP_TRY(dl.alloc(dev, n_rows * 8));
      HIP_TRY(powers(LCPC_FT63, dx.as<uint32_t>(), (uint64_t)pre, n_rows, dl.as<uint32_t>(), lease.s));
      HIP_TRY(hipMemcpyAsync(left.data(), dl.p, n_rows * 8, hipMemcpyDeviceToHost, lease.s));
      HIP_TRY(hipStreamSynchronize(lease.s));
    }
    lcpc_commit *c = nullptr;
    if ((st = lcpc_pos_commit_eval_bytes_device(sd.e, sd.d, sd.n, left.data(), n_rows, sd.result, &c))) return st;
    st = lcpc_open_columns(c, sd.idx, sd.n_idx, sd.cols, sd.paths);
    std::memcpy(sd.root, c->root, 32);
    lcpc_commit_free(c);
    if (st) return st;
  }
  if (expected_eval) return lcpc_pos_eval_poly_bytes_device(d_new, n_new, x, 0, expected_eval);
  return LCPC_OK;
}

}  // extern "C"

