// pos.hpp -- launchers of the proof-of-storage producer kernels (pos.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace lcpc {

// DataField::from_byte_vec (WriteableFt63): ceil(n_bytes / 7) raw u64 limbs
hipError_t pos_pack7(const uint8_t *bytes, size_t n_bytes, uint64_t *out, hipStream_t s);
// field_vec_to_byte_vec truncated to n_bytes
hipError_t pos_unpack7(const uint64_t *elems, size_t n_elems, uint8_t *out, size_t n_bytes,
                       hipStream_t s);
// out[r][bitrev(i)] = in[r][i] (* scale, given as canonical words, if non-null); rows of 2^log_n
hipError_t bitrev_scale(int fid, const uint32_t *in, uint32_t *out, int log_n, size_t n_rows,
                        const uint32_t *scale_canon_words, hipStream_t s);
// dst[i] = base^(i * step_exp)
hipError_t powers(int fid, const uint32_t *base, uint64_t step_exp, size_t n, uint32_t *dst,
                  hipStream_t s);

// ---- pos_eval.hip
// coefficients per block of the polynomial evaluation (every power of it is a reduction level)
constexpr int POS_EVAL_TILE = 2048;
// out[0] = sum_{i<n} c_i x^(i + d) (n = 0: zero).  n_bytes == 0: src = n elements of field fid;
// else src = a WriteableFt63 file image of n_bytes bytes (fid 0, n = ceil(n_bytes / 7), 8-byte
// aligned).  x, out: device, one Montgomery element each.
size_t poly_eval_scratch_bytes(int fid, size_t n);
hipError_t poly_eval(int fid, const void *src, size_t n, size_t n_bytes, const uint32_t *x, uint64_t d,
                     uint32_t *out, void *scratch, hipStream_t s);
// out[0] = (vals[0] + ... + vals[nb - 1]) * x^d
hipError_t poly_eval_sum_scale(int fid, const uint32_t *vals, size_t nb, const uint32_t *x, uint64_t d,
                               uint32_t *out, hipStream_t s);
// out[c] = sum_r left[r] * M[r][c], c < pre, M the image's rows of pre elements (7 bytes each, the
// last row zero padded); pre a power of two >= 8 (pos_left_mul_bytes_ok), bytes 8-byte aligned
bool pos_left_mul_bytes_ok(size_t pre);
size_t pos_left_mul_bytes_scratch_bytes(size_t pre, size_t n_rows);
hipError_t pos_left_mul_bytes(const uint8_t *bytes, size_t n_bytes, size_t pre, size_t n_rows, const uint32_t *left,
                              uint32_t *out, void *scratch, hipStream_t s);

// ---- many vectors in one pass (batched audits of a stored file)
// out[t pre + c] = sum_r lefts[t n_rows + r] * M[r][c], 1 <= n_vecs <= POS_LEFT_MANY_MAX_VECS, bit
// for bit n_vecs calls of pos_left_mul_bytes.  The kernel is a function of (pre, n_vecs) and
// LCPC_NO_MFMA: POS_LEFT_MANY_PACK (pre no power of two >= 8: the caller packs the image and runs
// collapse_rows_many), _VALU (k_left_mul_bytes_many) or _MFMA (pos_eval_mfma.hpp).
// A caller runs prepare once (the matrix-core kernel's digit table and correction, in prep), then
// partials for every piece of whole rows of the image as it becomes available (row_base even, the
// piece's partials after those of the pieces before it: pos_left_mul_many_splits sets each), then fold.
constexpr int POS_LEFT_MANY_PACK = 0, POS_LEFT_MANY_VALU = 1, POS_LEFT_MANY_MFMA = 2;
constexpr size_t POS_LEFT_MANY_MAX_VECS = 4096;  // == LCPC_BATCH_MAX_TENSORS
// (the adoption measurement of DESIGN §5f: at the 1 GiB default dims the matrix cores win from 16 vectors on)
constexpr size_t POS_LEFT_MANY_MFMA_MIN_VECS = 16;
int pos_left_mul_many_kernel(size_t pre, size_t n_vecs);
size_t pos_left_mul_many_splits(int kernel, size_t pre, size_t n_rows, size_t n_vecs);
size_t pos_left_mul_many_prep_bytes(int kernel, size_t n_rows, size_t n_vecs);
hipError_t pos_left_mul_many_prepare(int kernel, const uint32_t *lefts, size_t n_rows, size_t n_vecs, void *prep,
                                     hipStream_t s);
hipError_t pos_left_mul_many_partials(int kernel, const uint8_t *bytes, size_t n_bytes, size_t pre, size_t n_rows,
                                      size_t row_base, const uint32_t *lefts, size_t n_rows_total, size_t n_vecs,
                                      const void *prep, uint32_t *partials, hipStream_t s);
hipError_t pos_left_mul_many_fold(int kernel, const uint32_t *partials, size_t n_split, size_t pre, size_t n_rows_total,
                                  size_t n_vecs, const void *prep, uint32_t *out, hipStream_t s);
// out[i] = recombine_redc63 of the 8 accumulators y[8 i ..] (selftest)
hipError_t pos_recombine63(const int *y, uint32_t *out, size_t n, hipStream_t s);

// ---- pos_group.hip: u^T M of many files in one launch (grouped audits)
// The host builds the tables of a launch (pos_group_host.cpp); all offsets are in elements of the
// named buffer unless they say bytes.
//   job    an image of n_bytes bytes at byte offset base of the launch's arena (a multiple of 8), rows
//          of pre elements (a power of two >= 8), its left vector at element left_off of the lefts
//   tile   rows [row_lo, row_lo + the wave's n_rows) x 56-byte runs [run_lo, run_lo + 2^log_w) of one
//          job, one lane per run; the row vector it accumulates into starts at element dst of res (the
//          job's output when the job has one row split, else one of its partials)
//   wave   n_tiles tiles from tile0 on, all 2^log_w lanes wide (2^log_w = min(pre / 8, 64)) and n_rows
//          rows deep, so the row loop is uniform over the wave: lane l works on tile l >> log_w
//   fold   columns [col0, col0 + n_cols) (at most 64, one lane each) of a job split in rows:
//          res[out + c] = sum_{y < n_split} res[part + y pre + c]
struct PosGroupJob {
  uint64_t base, n_bytes, left_off, pre;
};
struct PosGroupTile {
  uint32_t job, row_lo, run_lo, pad;
  uint64_t dst;
};
struct PosGroupWave {
  uint32_t tile0, n_tiles, log_w, n_rows;
};
struct PosGroupFold {
  uint64_t out, part;
  uint32_t n_split, pre, col0, n_cols;
};
// one launch over n_waves waves (4 per workgroup), then with n_folds != 0 one fold launch (a wave per
// fold); n_waves / 4 and n_folds / 4 stay below 2^24 workgroups as in pos_left_mul_bytes
hipError_t pos_group_left_mul(const uint8_t *arena, const PosGroupJob *jobs, const PosGroupTile *tiles,
                              const PosGroupWave *waves, size_t n_waves, const PosGroupFold *folds, size_t n_folds,
                              const uint32_t *lefts, uint32_t *res, hipStream_t s);

// ---- pos_verify_group.hip: many stored-file audit responses checked in one pass
// The host builds the tables of a launch (pos_verify_group_host.cpp).
//   job    n_cols opened columns of n_rows Montgomery elements, staged at byte offset cols of the
//          launch's arena (a multiple of 16), column k at cols + k * col_words * 4 (col_words = 2 n_rows
//          rounded up to 4 words, the pad zero); their Merkle paths (n_cols x path_len x 32 B) at byte
//          offset paths; the left vector at element left of the lefts; the job's columns are
//          [col0, col0 + n_cols) of the launch's per-column arrays (idx, want, bits) and the chaining
//          value and partial sum of (chunk, column k) are slot cv0 + chunk * n_cols + k of cvs / partials
//   wave   columns [col_lo, min(col_lo + 64, n_cols)) of one job, a lane each, and one 1-KiB chunk of
//          their leaf messages (k_group_leaf_dot); the finish launch has one wave per 64 columns of a job
struct PosVerifyJob {
  uint64_t cols, paths, left, col0, cv0;
  uint32_t n_rows, n_cols, n_chunks, path_len, col_words, pad;
};
struct PosVerifyWave {
  uint32_t job, col_lo, chunk, pad;
};
constexpr size_t POS_VERIFY_MAX_CHUNKS = (size_t)1 << 16;  // chunks of one column's leaf (the fold's stack)
// The two launches of a staging group: k_group_leaf_dot over n_waves waves (4 per workgroup) leaves
// every (chunk, column)'s chaining value and its share of sum_r left[r] col[r]; k_group_leaf_finish
// over n_fwaves waves folds each column's leaf, walks its path to its job's root (roots: 32 B per
// job) and compares its sum with want: bits[col] = (path leads to the root) | (sum == want) << 1.
// max_chunks: the largest n_chunks of the launch's jobs (<= POS_VERIFY_MAX_CHUNKS).
hipError_t pos_group_verify(const uint8_t *arena, const PosVerifyJob *jobs, const PosVerifyWave *waves, size_t n_waves,
                            const PosVerifyWave *fwaves, size_t n_fwaves, size_t max_chunks, const uint32_t *lefts,
                            const uint8_t *roots, const uint64_t *idx, const uint32_t *want, uint32_t *cvs,
                            uint32_t *partials, uint32_t *bits, hipStream_t s);

// ---- pos_ingest.hip: many small files encoded, hashed and folded to trees in one pass
// The host builds the tables of a staging group (pos_ingest_host.cpp).
//   job    an image of n_bytes bytes at byte offset base of the group's arena (a multiple of 8), rows of
//          pre elements encoded to 2^log_enc; its encoded block [enc][rows_pad] of canonical 8-byte
//          words at byte offset enc_off of the encoded buffer (a multiple of 16; rows_pad = n_rows
//          rounded up to even, so every column starts 16-byte aligned and the pad word is never
//          written); the chaining value of (chunk, column c) is slot cv0 + chunk * enc + c of cvs and
//          the job's 2 enc - 1 digests start at digest tree0 of trees
//   tile   rows [row_lo, row_lo + n_rows) of one job, n_rows <= POS_INGEST_TILE_ROWS
//   wg     n_tiles tiles from tile0 on, all of rows of 2^log_enc points: a workgroup of k_group_encode,
//          each tile in a slot of POS_INGEST_TILE_ROWS x enc elements of its LDS
//   wave   columns [col_lo, min(col_lo + 64, enc)) of one job, a lane each, and one 1-KiB chunk of
//          their leaf messages (k_group_ingest_chunks)
struct PosIngestJob {
  uint64_t base, n_bytes, enc_off, cv0, tree0;
  uint32_t pre, log_enc, n_rows, rows_pad, n_chunks, pad;
};
struct PosIngestTile {
  uint32_t job, row_lo, n_rows, pad;
};
struct PosIngestWg {
  uint32_t tile0, n_tiles, log_enc, pad;
};
struct PosIngestWave {
  uint32_t job, col_lo, chunk, pad;
};
constexpr int POS_INGEST_MAX_LOG_ENC = 10;  // == log2(LCPC_POS_INGEST_MAX_ENC): a tile of 8 rows is 64 KiB of LDS
constexpr size_t POS_INGEST_TILE_ROWS = 8;  // a column segment of a full tile is one 64-byte store
// elements of a workgroup's LDS: tiles of short rows share a workgroup until it holds this many
// (8 per thread), a tile of longer rows has one to itself
constexpr size_t POS_INGEST_WG_ELEMS = 2048;
constexpr size_t POS_INGEST_MAX_CHUNKS = (size_t)1 << 16;  // chunks of one column's leaf (the fold's stack)
// the twiddles of the grouped lengths: tw[e] = w^e, w of order 2^POS_INGEST_MAX_LOG_ENC (the forward
// root of include/lcpc_fft_convention.h), 2^POS_INGEST_MAX_LOG_ENC Montgomery elements
hipError_t pos_ingest_twiddles(uint32_t *tw, hipStream_t s);
// The launches of a staging group, at most three: k_group_encode over n_wgs workgroups with lds_bytes
// of LDS each (none when no job has a row), k_group_ingest_chunks over n_waves waves (4 per
// workgroup), k_group_ingest_trees with a workgroup per job.  max_chunks: the largest n_chunks of the
// group's jobs (<= POS_INGEST_MAX_CHUNKS).  n_wgs, n_waves / 4 and n_jobs stay below 2^24.
hipError_t pos_group_ingest(const uint8_t *arena, const PosIngestJob *jobs, size_t n_jobs, const PosIngestTile *tiles,
                            const PosIngestWg *wgs, size_t n_wgs, size_t lds_bytes, const PosIngestWave *waves,
                            size_t n_waves, size_t max_chunks, const uint32_t *tw, uint8_t *enc, uint32_t *cvs,
                            uint8_t *trees, hipStream_t s);

// ---- pos_scrub.hip: many stored files checked against their leaves, trees and the row code in one pass
// (DESIGN §5j).  The host builds the tables of a staging group (pos_scrub_host.cpp); tiles, workgroups
// and waves are the ingest's records.
//   job    the first n_rows rows of a stored image, packed [enc][rows_pad] canonical 8-byte words at byte
//          offset img of the group's arena (a multiple of 16; rows_pad = n_rows rounded up to even, the
//          pad word zero); its stored digests (tree_kind 1: the enc leaves, 2: all 2 enc - 1) at byte
//          offset tree and, with has_root, the root to expect at byte offset root (multiples of 16); the
//          chaining value and the canonicity flag of (chunk, column c) are slot cv0 + chunk * enc + c of
//          cvs / cflags; its columns are [col0, col0 + enc) of the group's status and digests and its
//          rows [row0, row0 + n_rows) of the group's dirty bytes.  tree_only: a job routed to the
//          single-file entries, whose stored tree alone is checked here (no rows, no columns).
struct PosScrubJob {
  uint64_t img, tree, root, cv0, col0, row0;
  uint32_t pre, log_enc, n_rows, rows_pad, n_chunks, tree_kind, has_root, tree_only;
};
constexpr uint8_t POS_SCRUB_NOT_EVALUATED = 0xff;  // == LCPC_POS_SCRUB_NOT_EVALUATED
// The launches of a staging group, at most three: k_group_scrub_rows over n_wgs workgroups with
// lds_bytes of LDS each (none when no job has a row): dirty[row] = the row is no codeword;
// k_group_scrub_chunks over n_waves waves (4 per workgroup; none for tree-only jobs);
// k_group_scrub_leaves with a workgroup per job: status and digests per column, and per job
// flags[2 j] = the stored parents hash from their stored children, flags[2 j + 1] = the stored root is the
// expected one (POS_SCRUB_NOT_EVALUATED where there is nothing to compare).  tw: pos_ingest_twiddles.
// max_chunks as pos_group_ingest; n_wgs, n_waves / 4 and n_jobs stay below 2^24.
hipError_t pos_group_scrub(const uint8_t *arena, const PosScrubJob *jobs, size_t n_jobs, const PosIngestTile *tiles,
                           const PosIngestWg *wgs, size_t n_wgs, size_t lds_bytes, const PosIngestWave *waves,
                           size_t n_waves, size_t max_chunks, const uint32_t *tw, uint32_t *cvs, uint8_t *cflags,
                           uint8_t *flags, uint8_t *status, uint8_t *dirty, uint8_t *digests, hipStream_t s);

// ---- pos_repair_group.hip: the listed columns of many stored files recomputed from the others, hashed
// and folded into their trees in one pass.  The host builds the tables of a staging group
// (pos_repair_group_host.cpp); tiles, workgroups and waves are the ingest's records, a wave's columns
// being columns of the job's erasure list.
//   job    the first n_rows rows of the enc - n_bad columns that are not listed, packed in column order
//          [enc - n_bad][rows_pad] canonical 8-byte words at byte offset img of the group's arena (a
//          multiple of 16; rows_pad = n_rows rounded up to even); cmap (enc int32 at byte offset cmap):
//          k >= 0 for the k-th listed column, -1 - q for packed column q; the list itself (n_bad uint32)
//          at byte offset bad; with has_tree the enc digests of the columns as they stand at byte offset
//          leaves, and for a tree_only job (one routed to the single-file entry, whose tree alone is
//          built here: no rows, no chunks) its n_bad repaired digests at byte offset dig_in.  lambda
//          (enc elements from element lam0 of tabs, the listed positions unused) and the inverse table
//          (n_bad elements from element dinv0) are the locator launch's; the repaired columns are
//          [n_bad][rows_pad] canonical words at byte offset rep of the repaired arena; the chaining value
//          of (chunk, listed column k) is slot cv0 + chunk * n_bad + k of cvs; the repaired digests are
//          [dig0, dig0 + n_bad) of digests, the row flags [row0, row0 + n_rows) of flags and the tree
//          the 2 enc - 1 digests from digest tree0 of trees.
struct PosRepairJob {
  uint64_t img, cmap, bad, leaves, dig_in, lam0, dinv0, rep, cv0, dig0, row0, tree0;
  uint32_t pre, log_enc, n_rows, rows_pad, n_chunks, n_bad, has_tree, tree_only;
};
constexpr uint8_t POS_REPAIR_ROW_DEGREE = 1;    // flags[row]: a coefficient at or past pre + n_bad is not zero
constexpr uint8_t POS_REPAIR_ROW_NONCANON = 2;  // flags[row]: a word of a column that is not listed is not < p
// The launches of a staging group, at most four, in one profiling region (pos_group_repair):
// k_group_repair_locators and k_group_repair_trees with a workgroup per job, k_group_repair_rows over
// n_wgs workgroups with lds_bytes of LDS each (none when no job has a row), k_group_repair_chunks over
// n_waves waves (4 per workgroup; none when nothing is listed).  With tree_only_group only the last one
// runs.  tw: pos_ingest_twiddles.  max_chunks as pos_group_ingest; n_wgs, n_waves / 4 and n_jobs stay
// below 2^24.
hipError_t pos_group_repair(const uint8_t *arena, const PosRepairJob *jobs, size_t n_jobs, const PosIngestTile *tiles,
                            const PosIngestWg *wgs, size_t n_wgs, size_t lds_bytes, const PosIngestWave *waves,
                            size_t n_waves, size_t max_chunks, bool tree_only_group, const uint32_t *tw, uint32_t *tabs,
                            uint8_t *rep, uint32_t *cvs, uint8_t *flags, uint8_t *digests, uint8_t *trees,
                            hipStream_t s);
// k_group_repair_locators alone, a workgroup per job (the grouped locate's first launch: it needs
// lambda; the inverse table is written too and not read)
hipError_t pos_group_repair_locators(const uint8_t *arena, const PosRepairJob *jobs, size_t n_jobs, const uint32_t *tw,
                                     uint32_t *tabs, hipStream_t s);

// ---- pos_locate_group.hip: the damaged columns of many stored files named by the rows themselves --
// Reed-Solomon error location by syndromes, Berlekamp-Massey and a root search -- in one
// pass.  A staging group is the grouped repair's (PosRepairJob with the known columns as
// the listed ones, tiles and workgroups; no waves, leaves or trees) plus one record per job of where its
// rows' syndromes, position masks and column statuses go:
//   synd0   element of the syndrome arena where row 0's N = enc - pre - n_bad syndromes S_0 .. S_{N-1}
//           stand (8-byte words, fully reduced; row r at synd0 + r N; written for dirty rows only);
//   mask0   64-bit word of the mask arena where row 0's enc-bit position mask starts (row r at mask0 +
//           r max(1, enc / 64); bit c = the root search found stored position c; written for the rows
//           Berlekamp-Massey gave a candidate for, read for the located rows only);
//   col0    the first of the job's enc bytes of col_status.
struct PosLocateJob {
  uint64_t synd0, mask0, col0, reserved;
};
// LDS of a k_group_locate_bm workgroup (one wave, one row) for a group whose longest row has enc_max
// points: the row's syndromes, later C zero-padded for the root search (enc_max elements), and C, B and
// the next B of at most N / 2 + 1 <= enc_max / 2 coefficients each.
constexpr size_t pos_locate_bm_lds(size_t enc_max) { return (enc_max + 3 * (enc_max / 2)) * 8; }
// The launches of a staging group, at most four, in one profiling region (pos_group_locate):
// k_group_repair_locators (only with any_listed), k_group_locate_rows over n_wgs workgroups with lds_rows
// of LDS each, k_group_locate_bm with a one-wave workgroup per row slot of the n_tiles tiles and lds_bm of
// LDS (both none when no job has a row), k_group_locate_cols with a workgroup per job.  flags[row]: the
// repair's row flags; rstat[row] = 0 codeword, 1 located, 2 not locatable; col_status[col0 + c] = 0, 1
// (some located row names c) or 3 (listed).  Every byte of flags, rstat and col_status has one writer and
// nothing is cleared first.  tw: pos_ingest_twiddles.
hipError_t pos_group_locate(const uint8_t *arena, const PosRepairJob *jobs, const PosLocateJob *ljobs, size_t n_jobs,
                            const PosIngestTile *tiles, size_t n_tiles, const PosIngestWg *wgs, size_t n_wgs,
                            size_t lds_rows, size_t lds_bm, bool any_listed, const uint32_t *tw, uint32_t *tabs,
                            uint64_t *synd, uint64_t *masks, uint8_t *flags, uint8_t *rstat, uint8_t *col_status,
                            hipStream_t s);

}  // namespace lcpc
