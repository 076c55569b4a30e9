/*
 * lcpc_mi.h -- C ABI of liblcpc_mi.so, the MI355X-native lcpc-2d commit / prove / verify
 * row-encoding path.
 *
 * This is the drop-in boundary for the reference's LcEncoding trait and LcCommit /
 * LcEvalProof API (TrevorGKann/lcpc_proof_of_storage, lcpc-2d/src/lib.rs).  Each entry point
 * names the reference interface it replaces (file:line).  A Rust FFI shim (see
 * INTEGRATION.md) passes `&mut [F]` as `uint64_t*` after a size/alignment check: field
 * elements cross the boundary as `limbs(field)` little-endian u64 words holding ff_derive's
 * internal Montgomery form, bit-identical to the reference's `struct FtX([u64; N])`.
 *
 * Conventions
 *   - every function returns lcpc_status (0 = OK) unless it returns a size/bool; on error
 *     lcpc_last_error() returns a thread-local message;
 *   - "host" pointers are caller-owned CPU memory; "device" pointers are HIP device memory
 *     of the current device; handles own their device buffers;
 *   - handles may be used from several threads: each call leases a HIP stream from a
 *     per-device pool (commits / encodes, prove, and the latency-side calls each have their own
 *     pool; all streams run at one priority unless LCPC_PRIORITY_STREAMS=1), so independent
 *     calls, e.g. commitments of different objects, overlap on the device.  That holds for the
 *     handles a call only reads -- lcpc_encoding (the reference's rayon workers encode rows of
 *     one encoding at once), lcpc_commit (prove, open_column) and the proof handles (verify) --
 *     and for the stateless entry points.  tests/test_gpu_threads.py holds it up: 16 host threads
 *     in one process on one encoding, one commitment and one proof handle and on the stored-file
 *     entry points, every result compared with the CPU oracle, under the default stream mode and
 *     LCPC_STREAM_MODE=serial; tests/cpp/test_pool_threads.cpp runs the device block cache's
 *     ordering logic from 8 threads under ThreadSanitizer.
 *     Handles that carry the state of a call in progress are NOT for concurrent use of one
 *     instance (distinct instances are independent): lcpc_transcript (the sponge, or the caller's
 *     callbacks), lcpc_column_digests and lcpc_pos_writer (rows and chaining values accumulated
 *     between update / push calls), lcpc_pos_chunk_cache (its update entry points rewrite the
 *     cached values in place), and lcpc_sharded_commit / lcpc_comm (one collective call at a time).
 * No torch / HIP types appear in the signatures; `void *stream` is an optional hipStream_t.
 */
#ifndef LCPC_MI_H
#define LCPC_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: the PoS column chunk-CV cache (lcpc_pos_chunk_cache_*); 3: R-S erasure decoding, scrub and
 * repair of stored files (lcpc_rs_*, lcpc_pos_scrub_porenc, lcpc_pos_repair_columns).  The R-S
 * error location block (lcpc_rs_locate_*, lcpc_rs_decode_rows, lcpc_pos_locate_porenc) is additive
 * within version 3: new symbols only, nothing existing changed.  So is the digest block (lcpc_digest,
 * lcpc_encoding_set_digest, lcpc_commit_digest and the *_d functions): every existing symbol keeps
 * its signature and its BLAKE3 meaning.  So is the update-audit block (lcpc_eval_poly*,
 * lcpc_pos_eval_poly_bytes*, lcpc_pos_left_multiply_bytes*, lcpc_pos_update_rows,
 * lcpc_pos_update_evaluation).  So are the diagnostics added since (lcpc_selftest_field_op,
 * lcpc_selftest_recombine, lcpc_selftest_twiddle_words, lcpc_selftest_ntt_rows, lcpc_selftest_spmm, lcpc_selftest_reed_solomon).
 * So is the batched stored-file audit (lcpc_pos_left_multiply_bytes_many*, lcpc_pos_left_multiply_many_kernel,
 * lcpc_selftest_recombine63).  So are the grouped stored-file audits (lcpc_pos_left_multiply_bytes_grouped*,
 * lcpc_pos_group_plan, lcpc_field_to_montgomery).  So is the grouped check of stored-file audit
 * responses (lcpc_pos_audit_job, lcpc_pos_verify_evaluations_grouped, lcpc_pos_verify_tile,
 * lcpc_pos_verify_group_plan).  So is the grouped ingest of small files (lcpc_pos_ingest_job,
 * lcpc_pos_encode_files_grouped, lcpc_pos_ingest_tile, lcpc_pos_ingest_plan).  So is the grouped scrub of
 * stored files (lcpc_pos_scrub_job, lcpc_pos_scrub_files_grouped, lcpc_pos_scrub_plan).  So is the grouped
 * repair of stored files (lcpc_pos_repair_job, lcpc_pos_repair_files_grouped, lcpc_pos_repair_plan).  So is the
 * grouped locate of stored files (lcpc_pos_locate_job, lcpc_pos_locate_files_grouped). */
#define LCPC_ABI_VERSION 3

typedef enum lcpc_status {
  LCPC_OK = 0,
  /* ProverError (lcpc-2d/src/lib.rs:113-132) */
  LCPC_PROVER_TOO_BIG = 1,
  LCPC_PROVER_ENCODE = 2,
  LCPC_PROVER_COMMIT = 3,
  LCPC_PROVER_COLUMN_NUMBER = 4,
  LCPC_PROVER_OUTER_TENSOR = 5,
  /* VerifierError (lcpc-2d/src/lib.rs:139-167) */
  LCPC_VERIFIER_NUM_COL_OPENS = 10,
  LCPC_VERIFIER_COLUMN_PATH = 11,
  LCPC_VERIFIER_COLUMN_EVAL = 12,
  LCPC_VERIFIER_COLUMN_DEGREE = 13,
  LCPC_VERIFIER_OUTER_TENSOR = 14,
  LCPC_VERIFIER_INNER_TENSOR = 15,
  LCPC_VERIFIER_ENCODING_DIMS = 16,
  LCPC_VERIFIER_ENCODE = 17,
  /* fffft::FFTError (encode's Err type, lcpc-ligero-pc/src/lib.rs:159) */
  LCPC_FFT_NOT_POWER_OF_TWO = 20,
  LCPC_FFT_TOO_BIG = 21,
  LCPC_FFT_WRONG_SIZE_PRECOMP = 22,
  /* boundary-level failures (the Rust code panics / asserts here) */
  LCPC_ERR_INVALID_ARG = 30,
  LCPC_ERR_DEVICE = 31,
  LCPC_ERR_OUT_OF_MEMORY = 32,
  LCPC_ERR_NO_DEVICE = 33,
  LCPC_ERR_UNSUPPORTED = 34,
  /* a caller-owned transcript's callback (lcpc_transcript_ops) returned non-zero */
  LCPC_ERR_TRANSCRIPT = 35,
  /* erasure decoding: more erasures than the code's redundancy, or the surviving positions are
   * not those of a codeword (no reference counterpart) */
  LCPC_ERR_UNRECOVERABLE = 36
} lcpc_status;

typedef enum lcpc_field {
  LCPC_FT63 = 0,      /* lcpc-test-fields/src/lib.rs:18-22; PoS WriteableFt63 (same p) */
  LCPC_FT127 = 1,     /* lcpc-test-fields/src/lib.rs:41-45 */
  LCPC_FT191 = 2,     /* lcpc-test-fields/src/lib.rs:53-57 (24-byte elements: row shards cut at chunks 2 mod 3) */
  LCPC_FT255 = 3,     /* lcpc-test-fields/src/lib.rs:65-69 */
  LCPC_FT253_192 = 4  /* proof-of-storage/src/fields/ft253_192.rs:6-10 (big-endian repr) */
} lcpc_field;

/* The commitment's digest: the reference's type parameter D: Digest of LcCommit<D, E>, LcRoot<D, E>,
 * LcColumn<D, E> and LcEvalProof<D, E> (lcpc-2d/src/lib.rs:174-191).  All four have 32-byte outputs,
 * so no buffer of this ABI changes size with D.  Keccak-256 is SHA3-256's permutation and rate with
 * the pre-standard padding byte 0x01 instead of 0x06 (the EVM's keccak256). */
typedef enum lcpc_digest {
  LCPC_DIGEST_BLAKE3 = 0,    /* blake3::Hasher (the default; the only D of the proof-of-storage paths) */
  LCPC_DIGEST_SHA256 = 1,    /* sha2::Sha256 */
  LCPC_DIGEST_SHA3_256 = 2,  /* sha3::Sha3_256 */
  LCPC_DIGEST_KECCAK256 = 3  /* sha3::Keccak256 */
} lcpc_digest;

typedef struct lcpc_encoding lcpc_encoding;
typedef struct lcpc_commit lcpc_commit;
typedef struct lcpc_proof lcpc_proof;
typedef struct lcpc_transcript lcpc_transcript;

/* ------------------------------------------------------------------ library */
int lcpc_abi_version(void);
const char *lcpc_last_error(void);
/* Selects the HIP device used by handles created afterwards on this thread. */
lcpc_status lcpc_set_device(int device);
int lcpc_device_count(void);
/* u64 limbs per element (1, 2, 3, 4, 4); 0 for an unknown field */
int lcpc_field_limbs(lcpc_field f);
/* NUM_BITS of the field (SizedField::CLOG2, lcpc-2d/src/lib.rs:69-72) */
int lcpc_field_num_bits(lcpc_field f);
/* n draws of Field::random(&mut ChaCha20Rng::seed_from_u64(seed)) (ff_derive / rand_chacha):
 * the synthetic-input generator of the tests and benches (lcpc-test-fields random_coeffs,
 * lcpc-test-fields/src/lib.rs:86-108, with a seeded instead of a thread RNG). Host only. */
lcpc_status lcpc_field_random(lcpc_field f, uint64_t seed, uint64_t *out, size_t n);

/* ------------------------------------------------------------------ parameters
 * n_degree_tests (lcpc-2d/src/lib.rs:642-645), log2 (:857-859) */
size_t lcpc_n_degree_tests(size_t lambda, size_t len, size_t flog2);
size_t lcpc_log2(size_t v);
/* LigeroEncodingRho::_n_col_opens (lcpc-ligero-pc/src/lib.rs:61-64) */
size_t lcpc_ligero_n_col_opens(size_t rho_num, size_t rho_den);
/* LigeroEncodingRho::_get_dims (lcpc-ligero-pc/src/lib.rs:70-112); LCPC_PROVER_TOO_BIG when
 * the Rust function returns None */
lcpc_status lcpc_ligero_get_dims(lcpc_field f, size_t rho_num, size_t rho_den, size_t len,
                                 size_t *n_rows, size_t *n_per_row, size_t *n_cols);

/* ------------------------------------------------------------------ LcEncoding
 * Ligero: LigeroEncodingRho::{new, new_ml, new_from_dims} (lcpc-ligero-pc/src/lib.rs:121-148) */
lcpc_status lcpc_ligero_new(lcpc_field f, size_t rho_num, size_t rho_den, size_t len,
                            lcpc_encoding **out);
lcpc_status lcpc_ligero_new_ml(lcpc_field f, size_t rho_num, size_t rho_den, size_t n_vars,
                               lcpc_encoding **out);
lcpc_status lcpc_ligero_new_from_dims(lcpc_field f, size_t rho_num, size_t rho_den,
                                      size_t n_per_row, size_t n_cols, lcpc_encoding **out);
/* An R-S (fft_io) encoding with explicit soundness parameters, as the lcpc-2d test encoding
 * (lcpc-2d/src/tests.rs:23-121: N_COL_OPENS = 128, 2 degree tests). */
lcpc_status lcpc_rs_encoding_new(lcpc_field f, size_t n_per_row, size_t n_cols,
                                 size_t n_col_opens, size_t n_degree_tests, lcpc_encoding **out);
/* Brakedown: SdigEncodingS<F, SdigCodeK> (lcpc-brakedown-pc/src/lib.rs:40-176), code = K in
 * 1..6 (codespec.rs:169-232; the crate's default SdigEncoding is code 3).  The random expander
 * matrices are matgen::generate(n_per_row, seed) (matgen.rs:28-52), drawn bit-exactly. */
size_t lcpc_sdig_n_col_opens(int code);                       /* _n_col_opens :57-61 */
/* the n_per_row SdigEncodingS::new would choose for `len` coefficients (:103-110, :69-99) */
lcpc_status lcpc_sdig_get_n_per_row(lcpc_field f, int code, size_t len, size_t *n_per_row);
lcpc_status lcpc_sdig_new(lcpc_field f, int code, size_t len, uint64_t seed,
                          lcpc_encoding **out);                /* new :103-110 */
lcpc_status lcpc_sdig_new_ml(lcpc_field f, int code, size_t n_vars, uint64_t seed,
                             lcpc_encoding **out);             /* new_ml :114-123 */
lcpc_status lcpc_sdig_new_from_dims(lcpc_field f, int code, size_t n_per_row, size_t n_cols,
                                    uint64_t seed, lcpc_encoding **out); /* :126-137 */
/* 0 = Reed-Solomon / fft_io (Ligero), 1 = SDIG expander code (Brakedown) */
int lcpc_encoding_kind(const lcpc_encoding *e);
/* nonzeros of all SDIG precode + postcode matrices (0 for R-S encodings) */
size_t lcpc_encoding_matrix_nnz(const lcpc_encoding *e);
void lcpc_encoding_free(lcpc_encoding *e);
lcpc_field lcpc_encoding_field(const lcpc_encoding *e);
/* LcEncoding::get_dims / dims_ok / get_n_col_opens / get_n_degree_tests (lib.rs:94-104) */
void lcpc_encoding_get_dims(const lcpc_encoding *e, size_t len, size_t *n_rows, size_t *n_per_row,
                            size_t *n_cols);
int lcpc_encoding_dims_ok(const lcpc_encoding *e, size_t n_per_row, size_t n_cols);
size_t lcpc_encoding_n_col_opens(const lcpc_encoding *e);
size_t lcpc_encoding_n_degree_tests(const lcpc_encoding *e);
size_t lcpc_encoding_n_per_row(const lcpc_encoding *e);
size_t lcpc_encoding_n_cols(const lcpc_encoding *e);
/* Which kernel encodes rows of 2^15-point Ft63 rate-1/2 encodings (the proof-of-storage default
 * dims; no effect on any other encoding): AUTO (default) = the one-pass row kernel for file images
 * (lcpc_pos_commit_bytes_device) and the four-step pair for element rows, the measured choices
 * (DESIGN.md §4); FOURSTEP / ONEPASS force one kernel for both.  Results are identical either way.
 * No reference counterpart (fffft has one FFT).  Configuration, not a runtime switch: call it
 * right after creating the encoding, before any commit / encode / prove uses it (the setting is
 * read without synchronisation by concurrent calls on the encoding). */
#define LCPC_ROW_KERNEL_AUTO 0
#define LCPC_ROW_KERNEL_FOURSTEP 1
#define LCPC_ROW_KERNEL_ONEPASS 2
lcpc_status lcpc_encoding_set_row_kernel(lcpc_encoding *e, int kernel);
/* 1 if lcpc_commit_new_device under e hashes the column leaves inside the encode's second pass
 * instead of in a pass of its own over the codeword (whole rows, BLAKE3, device-resident
 * coefficients; Ft127 encodings whose second pass is 2^8 points long, that is n_cols 2^15 .. 2^16),
 * else 0.  Fixed when the encoding is made: a build with -DLCPC_NTT_LEAF_FUSE=0 has no such pass,
 * and LCPC_NTT_LEAF_FUSE=0 in the environment at creation keeps that encoding on the separate
 * pass.  Commitments are bit-identical either way.  Host only; no reference counterpart. */
int lcpc_encoding_leaf_fuse(const lcpc_encoding *e);
/* "BLAKE3", "SHA-256", "SHA3-256", "Keccak-256"; NULL for an unknown value.  Host only. */
const char *lcpc_digest_name(lcpc_digest d);
/* The digest D of everything made or checked under e: with D substituted, merkleize (lcpc-2d/src/
 * lib.rs:720-734) hashes leaf j = D(32 zero bytes || to_repr(comm[0][j]) || .. || to_repr(comm[n_rows-1][j]))
 * (hash_columns :736-775) and node = D(left || right) (:777-815), and verify_column_path (:985-1012)
 * checks against them.  lcpc_commit_new* build the tree with it, lcpc_prove* / lcpc_check_comm need
 * a commitment of the same digest (else LCPC_ERR_INVALID_ARG), and lcpc_verify* take it from e: the
 * verifier, not the proof, says which digest the root belongs to.  The prover's transcript absorbs
 * no digest (:1057, :1075-1077, :1096-1104), so a proof under another D differs from the BLAKE3
 * proof of the same polynomial and transcript only in its Merkle paths.  Configuration, with
 * lcpc_encoding_set_row_kernel's contract: set right after creation, read without synchronisation.
 * BLAKE3-only, because the reference fixes PoSCommit = LcCommit<Blake3, ..> (proof-of-storage/src/
 * lib.rs:21) and the sharded engine exchanges BLAKE3 chunk chaining values: lcpc_pos_commit_bytes*,
 * lcpc_pos_commit_eval_bytes_device, lcpc_pos_columns, lcpc_shard_new* and lcpc_sharded_* return
 * LCPC_ERR_UNSUPPORTED, naming the digest, for an encoding set to another one; the stored-file
 * formats, the chunk-CV cache and lcpc_column_digests_* take no encoding and are BLAKE3. */
lcpc_status lcpc_encoding_set_digest(lcpc_encoding *e, lcpc_digest d);
lcpc_digest lcpc_encoding_digest(const lcpc_encoding *e);
/* Pre-allocates the calling thread's page-locked staging for lcpc_prove on commitments of
 * n_rows rows under e (host only).  Optional: a thread's first prove otherwise pays the
 * hipHostMalloc.  No reference counterpart (rayon threads have no device staging). */
lcpc_status lcpc_prepare_thread(const lcpc_encoding *e, size_t n_rows);
/* Pre-allocates into the device pool the buffers and streams of `count` concurrent
 * commit + prove calls on `len` coefficients under e (otherwise the first calls at a new
 * concurrency pay hipMalloc / hipStreamCreate).  Optional. */
lcpc_status lcpc_reserve(const lcpc_encoding *e, size_t len, size_t count);
/* LcEncoding::encode (lcpc-2d/src/lib.rs:92; Ligero: fft_io_pc, lcpc-ligero-pc/src/lib.rs:
 * 162-164): in place on `len` elements (must equal n_cols) of host memory. */
lcpc_status lcpc_encode(const lcpc_encoding *e, uint64_t *inp, size_t len);
/* Batched encode of n_rows host rows (row r at rows + r * row_stride limbs-elements). */
lcpc_status lcpc_encode_rows(const lcpc_encoding *e, uint64_t *rows, size_t n_rows,
                             size_t row_stride);
/* Device batched encode: row r reads n_valid (<= n_cols) coefficients at
 * d_src + r * src_stride (elements), treats the rest of the row as zero, and writes n_cols
 * encoded elements at d_dst + r * dst_stride (>= n_cols).  Asynchronous on `stream`; with
 * stream == NULL it runs on a pooled stream and returns when the rows are written. */
lcpc_status lcpc_encode_rows_device(const lcpc_encoding *e, const void *d_src, size_t src_stride,
                                    size_t n_valid, void *d_dst, size_t dst_stride,
                                    size_t n_rows, void *stream);

/* ------------------------------------------------------------------ LcCommit
 * LcCommit::commit (lcpc-2d/src/lib.rs:314-316 -> commit :651-700).  The commitment (coeffs,
 * encoded matrix, Merkle hashes) stays resident in HBM; `len` elements of host memory.  The rows
 * cross PCIe in ~8 MiB blocks on a copy stream, each block encoded as soon as it has landed;
 * page-locked memory (hipHostMalloc / hipHostRegister) is read by the DMA engine directly,
 * pageable memory (a Rust Vec) through the HIP runtime's own pageable path, block by block. */
lcpc_status lcpc_commit_new(const lcpc_encoding *e, const uint64_t *coeffs, size_t len,
                            lcpc_commit **out);
/* 1 if the calling thread's last host-input commit read a page-locked source directly, 0 if it
 * took the pageable path (diagnostic) */
int lcpc_last_upload_pinned(void);
/* Same with the coefficients already in device memory (no PCIe transfer). */
lcpc_status lcpc_commit_new_device(const lcpc_encoding *e, const void *d_coeffs, size_t len,
                                   lcpc_commit **out);
void lcpc_commit_free(lcpc_commit *c);
/* LcCommit::get_root (:291-296) */
lcpc_status lcpc_commit_get_root(const lcpc_commit *c, uint8_t root[32]);
size_t lcpc_commit_n_rows(const lcpc_commit *c);      /* get_n_rows   :309-311 */
size_t lcpc_commit_n_cols(const lcpc_commit *c);      /* get_n_cols   :304-306 */
size_t lcpc_commit_n_per_row(const lcpc_commit *c);   /* get_n_per_row :299-301 */
size_t lcpc_commit_n_hashes(const lcpc_commit *c);
/* the digest its tree was built with (the encoding's at commit time, or from_parts_d's) */
lcpc_digest lcpc_commit_digest(const lcpc_commit *c);
/* LcCommit's serde Deserialize (WrappedLcCommit, lib.rs:193-229): a commitment from its fields --
 * comm (n_rows x n_cols) and coeffs (n_rows x n_per_row) as row-major Montgomery limbs, the
 * n_hashes = 2 next_pow2(n_cols) - 1 digests in commit order (root last) -- loaded into HBM so
 * prove / open_column run on it.  Other sizes: LCPC_ERR_INVALID_ARG. */
lcpc_status lcpc_commit_from_parts(lcpc_field f, size_t n_rows, size_t n_cols, size_t n_per_row,
                                   const uint64_t *comm, const uint64_t *coeffs, const uint8_t *hashes,
                                   size_t n_hashes, lcpc_commit **out);
/* The same for an LcCommit<D, E>: the hashes were made with digest d (the serialized fields do not
 * say which; they are digest-agnostic for 32-byte outputs).  lcpc_commit_from_parts is d = BLAKE3. */
lcpc_status lcpc_commit_from_parts_d(lcpc_digest d, lcpc_field f, size_t n_rows, size_t n_cols, size_t n_per_row,
                                     const uint64_t *comm, const uint64_t *coeffs, const uint8_t *hashes,
                                     size_t n_hashes, lcpc_commit **out);
/* copies of the public fields comm / coeffs / hashes (:180-190) to host memory */
lcpc_status lcpc_commit_copy_comm(const lcpc_commit *c, uint64_t *out);
lcpc_status lcpc_commit_copy_coeffs(const lcpc_commit *c, uint64_t *out);
lcpc_status lcpc_commit_copy_hashes(const lcpc_commit *c, uint8_t *out);
/* device views (valid while the handle lives).  The encoded matrix is row-major [n_rows][n_cols]
 * for Ligero and element-major [n_cols][n_rows] for SDIG (lcpc_commit_col_major() == 1), where
 * every Merkle leaf is one contiguous column; copy_comm always returns the row-major layout. */
int lcpc_commit_col_major(const lcpc_commit *c);
/* 1 if the device codeword (lcpc_commit_device_comm) holds canonical values rather than
 * Montgomery words (R-S / Ligero commitments: the encode writes them so, and the Merkle leaves
 * hash canonical bytes); copy_comm and the opened columns are Montgomery either way. */
int lcpc_commit_comm_canonical(const lcpc_commit *c);
const void *lcpc_commit_device_comm(const lcpc_commit *c);
const void *lcpc_commit_device_coeffs(const lcpc_commit *c);
/* check_comm (:703-718) */
lcpc_status lcpc_check_comm(const lcpc_commit *c, const lcpc_encoding *e);
/* open_column (:818-855): n_rows elements + log2(n_cols) digests */
lcpc_status lcpc_open_column(const lcpc_commit *c, size_t column, uint64_t *col_out,
                             uint8_t *path_out);

/* ------------------------------------------------------------------ merlin::Transcript
 * (merlin 2.0; used by prove/verify at lcpc-2d/src/lib.rs:901,934,1057,1075-1077,1096-1104) */
lcpc_transcript *lcpc_transcript_new(const uint8_t *label, size_t label_len);
lcpc_transcript *lcpc_transcript_clone(const lcpc_transcript *t);
void lcpc_transcript_free(lcpc_transcript *t);
void lcpc_transcript_append_message(lcpc_transcript *t, const uint8_t *label, size_t label_len,
                                    const uint8_t *msg, size_t msg_len);
/* append_message(label, msgs + i * msg_len) for i < n_msgs (host bytes): the prover's per-element
 * absorption (lcpc-2d/src/lib.rs:1075-1077, 1096-1098) in one call */
void lcpc_transcript_append_messages(lcpc_transcript *t, const uint8_t *label, size_t label_len,
                                     const uint8_t *msgs, size_t msg_len, size_t n_msgs);
void lcpc_transcript_challenge_bytes(lcpc_transcript *t, const uint8_t *label, size_t label_len,
                                     uint8_t *dest, size_t dest_len);
/* A caller-owned transcript.  The reference's prove / verify take the CALLER's transcript,
 * `tr: &mut merlin::Transcript` (lcpc-2d/src/lib.rs:319-326, 547-556), and the caller keeps using
 * it afterwards (proof-of-storage/src/tests.rs:223-233, main.rs:47-57; lcpc-2d/src/tests.rs:318-413
 * continues one transcript over two proofs).  A handle made by lcpc_transcript_from_ops forwards
 * every absorb and squeeze of prove / verify -- in the reference's order, the only state being the
 * caller's -- to these functions:
 *   append_message(ctx, label, msg)          = Transcript::append_message   (merlin 2.0)
 *   append_messages(ctx, label, msgs, l, n)  = append_message(label, msgs + i * l) for i < n, the
 *       prover's per-coefficient absorption (:1075-1077, 1096-1098) in one call; may be NULL
 *       (then append_message is called n times)
 *   challenge_bytes(ctx, label, dest, n)     = Transcript::challenge_bytes
 * Labels are always one of "$l//DT", "$l//PR", "$l//PE", "$l//CO" (macros.rs:29-36), so a Rust
 * shim can map them back to its &'static [u8] constants.  Callbacks run on the calling thread,
 * inside the prove / verify call, and the callbacks of one call are never concurrent -- also in
 * lcpc_sharded_commit_prove_many, whose worker pool runs only the library's own transcripts
 * (tests/test_gpu_transcript_ops.py records the thread of every callback); 0 = success,
 * anything else makes the call return LCPC_ERR_TRANSCRIPT (a sharded prove still completes its exchanges first).  The handle holds no
 * transcript state of its own: lcpc_transcript_clone refuses it (NULL). */
typedef struct lcpc_transcript_ops {
  void *ctx;
  int (*append_message)(void *ctx, const uint8_t *label, size_t label_len, const uint8_t *msg,
                        size_t msg_len);
  int (*append_messages)(void *ctx, const uint8_t *label, size_t label_len, const uint8_t *msgs,
                         size_t msg_len, size_t n_msgs);
  int (*challenge_bytes)(void *ctx, const uint8_t *label, size_t label_len, uint8_t *dest,
                         size_t dest_len);
} lcpc_transcript_ops;
/* NULL (lcpc_last_error) if append_message or challenge_bytes is missing; ops is copied */
lcpc_transcript *lcpc_transcript_from_ops(const lcpc_transcript_ops *ops);
/* the first non-zero callback return seen by an ops transcript (0: none, or not an ops handle) */
int lcpc_transcript_status(const lcpc_transcript *t);

/* ------------------------------------------------------------------ LcEvalProof
 * LcCommit::prove (lcpc-2d/src/lib.rs:319-326 -> prove :1034-1123).  outer_tensor: host,
 * outer_len elements. */
lcpc_status lcpc_prove(const lcpc_commit *c, const uint64_t *outer_tensor, size_t outer_len,
                       const lcpc_encoding *e, lcpc_transcript *tr, lcpc_proof **out);
void lcpc_proof_free(lcpc_proof *p);
size_t lcpc_proof_n_cols(const lcpc_proof *p);          /* LcEvalProof::get_n_cols :537-539 */
size_t lcpc_proof_n_per_row(const lcpc_proof *p);       /* get_n_per_row :542-544 */
size_t lcpc_proof_n_rows(const lcpc_proof *p);
size_t lcpc_proof_n_degree_tests(const lcpc_proof *p);
size_t lcpc_proof_n_col_opens(const lcpc_proof *p);
size_t lcpc_proof_path_len(const lcpc_proof *p);
lcpc_field lcpc_proof_field(const lcpc_proof *p);
lcpc_status lcpc_proof_copy_p_eval(const lcpc_proof *p, uint64_t *out);
lcpc_status lcpc_proof_copy_p_random(const lcpc_proof *p, size_t i, uint64_t *out);
/* k-th opened column (LcColumn, :424-433): values (n_rows) and Merkle path (path_len x 32 B) */
lcpc_status lcpc_proof_copy_column(const lcpc_proof *p, size_t k, uint64_t *col, uint8_t *path);
/* Rebuild a proof from its public fields (e.g. after deserialisation, :591-610). */
lcpc_status lcpc_proof_from_parts(lcpc_field f, size_t n_cols, size_t n_per_row, size_t n_rows,
                                  size_t n_degree_tests, size_t n_col_opens, size_t path_len,
                                  const uint64_t *p_eval, const uint64_t *p_random,
                                  const uint64_t *cols, const uint8_t *paths, lcpc_proof **out);
/* LcEvalProof::verify (:547-556 -> verify :862-982); *eval_out = the evaluation (limbs). */
lcpc_status lcpc_verify(const uint8_t root[32], const uint64_t *outer_tensor, size_t outer_len,
                        const uint64_t *inner_tensor, size_t inner_len, const lcpc_proof *p,
                        const lcpc_encoding *e, lcpc_transcript *tr, uint64_t *eval_out);
/* lcpc_prove / lcpc_verify driving the caller's transcript through ops for this one call: the
 * drop-in for LcCommit::prove(&self, outer, enc, tr: &mut Transcript) (lib.rs:319-326) and
 * LcEvalProof::verify(.., tr: &mut Transcript) (:547-556) -- see lcpc_transcript_ops above */
lcpc_status lcpc_prove_ops(const lcpc_commit *c, const uint64_t *outer_tensor, size_t outer_len,
                           const lcpc_encoding *e, const lcpc_transcript_ops *ops, lcpc_proof **out);
lcpc_status lcpc_verify_ops(const uint8_t root[32], const uint64_t *outer_tensor, size_t outer_len,
                            const uint64_t *inner_tensor, size_t inner_len, const lcpc_proof *p,
                            const lcpc_encoding *e, const lcpc_transcript_ops *ops, uint64_t *eval_out);

/* ------------------------------------------------------------------ batched evaluation proofs
 * NO COUNTERPART IN THE REFERENCE.  Additive within LCPC_ABI_VERSION 3.  One commitment opened at
 * n_evals points with one set of degree tests and one set of column openings.  Transcript order:
 * the degree tests exactly as lcpc_prove runs them; p_eval_0 .. p_eval_(n_evals - 1) in order, each
 * coefficient under "$l//PE"; then the column challenge.  Every claim is absorbed before the
 * columns are drawn, so each opened column checks all of them and a false claim survives with the
 * probability it has in a single proof.  With n_evals = 1 the proof parts and the transcript's end
 * state are those of lcpc_prove / lcpc_verify, byte for byte.
 * The row combinations of one call go through a kernel that takes any number of tensors up to
 * LCPC_BATCH_MAX_TENSORS, which also bounds n_evals. */
#define LCPC_BATCH_MAX_TENSORS 4096
typedef struct lcpc_batch_proof lcpc_batch_proof;
/* outers: host, n_evals tensors of outer_len elements each, row-major.  n_evals == 0 or above the
 * bound: LCPC_ERR_INVALID_ARG; a commitment of another digest than e's: LCPC_ERR_INVALID_ARG;
 * outer_len != n_rows: LCPC_PROVER_OUTER_TENSOR; the other errors are lcpc_prove's. */
lcpc_status lcpc_prove_batch(const lcpc_commit *c, const uint64_t *outers, size_t n_evals, size_t outer_len,
                             const lcpc_encoding *e, lcpc_transcript *tr, lcpc_batch_proof **out);
/* inners: n_evals tensors of inner_len elements; evals_out (may be NULL): n_evals elements,
 * evals_out[j] = <inners_j, p_eval_j>.  Per opened column the checks fail in the reference's order:
 * ColumnDegree, then ColumnEval (for any j; lcpc_last_error names the first failing j), then
 * ColumnPath.  n_evals == 0 or above the bound: LCPC_ERR_INVALID_ARG; a proof that holds another
 * number of evaluations than n_evals: LCPC_VERIFIER_OUTER_TENSOR; the other argument errors are
 * lcpc_verify's. */
lcpc_status lcpc_verify_batch(const uint8_t root[32], const uint64_t *outers, size_t n_evals, size_t outer_len,
                              const uint64_t *inners, size_t inner_len, const lcpc_batch_proof *p,
                              const lcpc_encoding *e, lcpc_transcript *tr, uint64_t *evals_out);
/* the same over the caller's transcript for this one call (see lcpc_prove_ops) */
lcpc_status lcpc_prove_batch_ops(const lcpc_commit *c, const uint64_t *outers, size_t n_evals, size_t outer_len,
                                 const lcpc_encoding *e, const lcpc_transcript_ops *ops, lcpc_batch_proof **out);
lcpc_status lcpc_verify_batch_ops(const uint8_t root[32], const uint64_t *outers, size_t n_evals, size_t outer_len,
                                  const uint64_t *inners, size_t inner_len, const lcpc_batch_proof *p,
                                  const lcpc_encoding *e, const lcpc_transcript_ops *ops, uint64_t *evals_out);
void lcpc_batch_proof_free(lcpc_batch_proof *p);
size_t lcpc_batch_proof_n_evals(const lcpc_batch_proof *p);
size_t lcpc_batch_proof_n_cols(const lcpc_batch_proof *p);
size_t lcpc_batch_proof_n_per_row(const lcpc_batch_proof *p);
size_t lcpc_batch_proof_n_rows(const lcpc_batch_proof *p);
size_t lcpc_batch_proof_n_degree_tests(const lcpc_batch_proof *p);
size_t lcpc_batch_proof_n_col_opens(const lcpc_batch_proof *p);
size_t lcpc_batch_proof_path_len(const lcpc_batch_proof *p);
lcpc_field lcpc_batch_proof_field(const lcpc_batch_proof *p);
/* j-th evaluation vector (n_per_row elements), i-th degree-test vector, k-th opened column */
lcpc_status lcpc_batch_proof_copy_p_eval(const lcpc_batch_proof *p, size_t j, uint64_t *out);
lcpc_status lcpc_batch_proof_copy_p_random(const lcpc_batch_proof *p, size_t i, uint64_t *out);
lcpc_status lcpc_batch_proof_copy_column(const lcpc_batch_proof *p, size_t k, uint64_t *col, uint8_t *path);
/* p_evals: n_evals x n_per_row elements; the other arrays as lcpc_proof_from_parts */
lcpc_status lcpc_batch_proof_from_parts(lcpc_field f, size_t n_cols, size_t n_per_row, size_t n_rows,
                                        size_t n_degree_tests, size_t n_col_opens, size_t path_len,
                                        size_t n_evals, const uint64_t *p_evals, const uint64_t *p_random,
                                        const uint64_t *cols, const uint8_t *paths, lcpc_batch_proof **out);
/* out[t][c] = sum_r tensors[t][r] * coeffs[r][c] on host arrays for any 1 <= n_tensors <=
 * LCPC_BATCH_MAX_TENSORS (else LCPC_ERR_INVALID_ARG): the many-tensor row-combination kernel by
 * itself.  Every out[t] equals lcpc_collapse_columns of tensor t, bit for bit. */
lcpc_status lcpc_collapse_columns_many(lcpc_field f, const uint64_t *coeffs, size_t n_rows, size_t n_per_row,
                                       const uint64_t *tensors, size_t n_tensors, uint64_t *out);
/* tensors per chunk (one pass over the coefficient matrix each) in that kernel for field f: 16, 8,
 * 5, 4, 4 for Ft63 .. Ft253_192; Ft127's matrix-core kernel also takes 8.  0: no such field. */
int lcpc_collapse_many_chunk(lcpc_field f);

/* ------------------------------------------------------------------ free functions */
/* collapse_columns (lcpc-2d/src/lib.rs:1126-1154) on host arrays: poly[c] += ... is computed
 * as poly = sum_r tensor[r] * coeffs[r][c] for c < n_per_row */
lcpc_status lcpc_collapse_columns(lcpc_field f, const uint64_t *coeffs, const uint64_t *tensor,
                                  uint64_t *poly, size_t n_rows, size_t n_per_row);
/* merkle_tree (lcpc-2d/src/lib.rs:777-790): ins has n_ins = 2^k digests, outs n_ins - 1 */
lcpc_status lcpc_merkle_tree(const uint8_t *ins, size_t n_ins, uint8_t *outs);
/* verify_column_path (:985-1012) and verify_column_value (:1015-1030): 1 = ok, 0 = fail */
int lcpc_verify_column_path(lcpc_field f, const uint64_t *col, size_t n_rows,
                            const uint8_t *path, size_t path_len, size_t col_num,
                            const uint8_t root[32]);
int lcpc_verify_column_value(lcpc_field f, const uint64_t *col, const uint64_t *tensor,
                             size_t n_rows, const uint64_t *poly_eval);
/* leaf digests of every column of a host matrix (hash_columns, :736-775) */
lcpc_status lcpc_hash_columns(lcpc_field f, const uint64_t *comm, size_t n_rows, size_t n_cols,
                              uint8_t *out);
/* merkle_tree, verify_column_path and hash_columns with D = d (the names above are d = BLAKE3) */
lcpc_status lcpc_merkle_tree_d(lcpc_digest d, const uint8_t *ins, size_t n_ins, uint8_t *outs);
int lcpc_verify_column_path_d(lcpc_digest d, lcpc_field f, const uint64_t *col, size_t n_rows,
                              const uint8_t *path, size_t path_len, size_t col_num,
                              const uint8_t root[32]);
lcpc_status lcpc_hash_columns_d(lcpc_digest d, lcpc_field f, const uint64_t *comm, size_t n_rows, size_t n_cols,
                                uint8_t *out);

/* ------------------------------------------------------------------ proof-of-storage producers
 * (proof-of-storage/src; the field is WriteableFt63 = LCPC_FT63's modulus and arithmetic) */
/* DataField::from_byte_vec for WriteableFt63 (fields/data_field.rs:38-46, writable_ft63.rs:
 * 35-40): each 7 little-endian data bytes (the last chunk zero padded) become one element whose
 * RAW u64 limb holds them (no Montgomery conversion).  *n_out = ceil(n_bytes / 7). */
lcpc_status lcpc_pos_bytes_to_field(const uint8_t *bytes, size_t n_bytes, uint64_t *out,
                                    size_t *n_out);
/* same on device buffers (8-byte aligned); asynchronous on `stream` (NULL: synchronous) */
lcpc_status lcpc_pos_bytes_to_field_device(const void *d_bytes, size_t n_bytes, void *d_out,
                                           void *stream);
/* The server's commitment to a file image in device memory: DataField::from_byte_vec then
 * LcCommit::commit (lcpc_online.rs:80-239, networking/server.rs:670-730), the same commitment as
 * lcpc_pos_bytes_to_field_device + lcpc_commit_new_device on ceil(n_bytes / 7) elements.  At the
 * default PoS dims (2^14 -> 2^15 Ft63 rows, 16-byte-aligned image) the bytes are unpacked inside
 * the one-pass encode (no element image in HBM); elsewhere they are packed first.  The image must
 * be 8-byte aligned; WriteableFt63 (LCPC_FT63) encodings only. */
lcpc_status lcpc_pos_commit_bytes_device(const lcpc_encoding *e, const void *d_bytes, size_t n_bytes,
                                         lcpc_commit **out);
/* The same commitment from a file image in HOST memory -- what the server has after reading the
 * file from disk on every proof request (networking/server.rs:670-679): the image crosses PCIe in
 * blocks of whole rows, and at the default dims each block is unpacked and encoded by the
 * one-pass kernel as soon as it has landed (page-locked or pageable, as lcpc_commit_new).  Any
 * alignment. */
lcpc_status lcpc_pos_commit_bytes(const lcpc_encoding *e, const uint8_t *bytes, size_t n_bytes,
                                  lcpc_commit **out);
/* DataField::field_vec_to_byte_vec truncated to expected_len (data_field.rs:57-62,
 * fields.rs:115-121) */
lcpc_status lcpc_pos_field_to_bytes(const uint64_t *elems, size_t n, uint8_t *out,
                                    size_t expected_len);
/* get_aspect_ratio_default_from_field_len + get_soundness_from_matrix_dims
 * (networking/server.rs:1139-1170) */
void lcpc_pos_default_dims(size_t field_len, size_t *n_per_row, size_t *n_cols,
                           size_t *soundness);
/* get_column_indicies_from_random_seed (networking/client.rs:443-456): ChaCha8Rng +
 * IteratorRandom::choose_multiple; *n_out = min(amount, max_index) */
lcpc_status lcpc_pos_column_indices(uint64_t seed, size_t amount, size_t max_index,
                                    uint64_t *out, size_t *n_out);
/* form_side_vectors_for_polynomial_evaluation_from_point (lcpc_online.rs:603-627):
 * right = [1, x, ..., x^(n_cols-1)], left = [1, x^n_cols, ..., x^((n_rows-1) n_cols)] */
lcpc_status lcpc_pos_side_vectors(lcpc_field f, const uint64_t *x, size_t n_rows, size_t n_cols,
                                  uint64_t *left, uint64_t *right);
/* verifiable_polynomial_evaluation (lcpc_online.rs:454-484): out[j] = sum_r left[r] comm[r][j]
 * over the ENCODED matrix (n_cols outputs; row-major commitments) */
lcpc_status lcpc_pos_eval_encoded(const lcpc_commit *c, const uint64_t *left, size_t n_rows,
                                  uint64_t *out);
/* One proof-of-storage request's GPU half in one call: lcpc_pos_commit_bytes_device on the
 * device file image, then verifiable_polynomial_evaluation with `left` (n_rows elements, the
 * commitment's row count) into eval_out (n_cols elements) -- the server's sequence
 * (networking/server.rs:670-730: convert_file_data_to_commit, then lcpc_online.rs:454-484).
 * The same commitment and the same values as the two calls.  The evaluation rides on the leaf
 * hashing's pass over the codeword (each thread sums its (chunk, column)'s rows) instead of a
 * second pass over it. */
lcpc_status lcpc_pos_commit_eval_bytes_device(const lcpc_encoding *e, const void *d_bytes, size_t n_bytes,
                                              const uint64_t *left, size_t n_rows, uint64_t *eval_out,
                                              lcpc_commit **out);
/* decode_row (lcpc_online.rs:568-574) = fffft ifft_oi on each of n_rows rows of len = 2^k
 * elements (in place); FFTError codes on bad lengths */
lcpc_status lcpc_ifft_oi_rows(lcpc_field f, uint64_t *rows, size_t n_rows, size_t len);
/* open_column (lcpc-2d/src/lib.rs:818-855) for n columns at once (server_retreive_columns,
 * lcpc_online.rs:241-247): cols_out n x n_rows elements, paths_out n x log2(n_cols) x 32 B */
lcpc_status lcpc_open_columns(const lcpc_commit *c, const uint64_t *idx, size_t n,
                              uint64_t *cols_out, uint8_t *paths_out);
/* CommitRequestType::ColumnsWithoutPath / Leaves (lcpc_online.rs:144-224): encode `len`
 * elements with e and return the requested columns (n x n_rows) and / or their BLAKE3 leaf
 * digests (n x 32 B) without building the Merkle tree; either output may be NULL */
/* PoS client verification (lcpc_online.rs:251-452):
 * hash_column_to_digest / hash_field_vec_to_digest for n_cols columns stored one after another
 * ([n_cols][n_rows] elements) -> n_cols x 32 B */
lcpc_status lcpc_hash_field_columns(lcpc_field f, const uint64_t *cols, size_t n_rows, size_t n_cols,
                                    uint8_t *out);
/* client_online_verify_column_paths_without_full_columns (:280-318): ok[k] = 1 iff leaf digest
 * k with its path (path_len x 32 B) hashes up to root at column idx[k] */
lcpc_status lcpc_verify_leaf_paths(const uint8_t *leaves, const uint8_t *paths, size_t n,
                                   size_t path_len, const uint64_t *idx, const uint8_t root[32],
                                   uint8_t *ok);
/* verify_column_value (lcpc-2d/src/lib.rs:1014-1030) batched, and the check of
 * verify_proper_partial_polynomial_evaluation (:487-516): ok[k] = 1 iff
 * sum_r tensor[r] cols[k][r] == values[idx[k]] (cols [n][n_rows]) */
lcpc_status lcpc_verify_column_values(lcpc_field f, const uint64_t *cols, size_t n, size_t n_rows,
                                      const uint64_t *tensor, const uint64_t *values,
                                      size_t n_values, const uint64_t *idx, uint8_t *ok);
lcpc_status lcpc_pos_columns(const lcpc_encoding *e, const uint64_t *elems, size_t len,
                             const uint64_t *idx, size_t n, uint64_t *cols_out,
                             uint8_t *leaves_out);

/* ------------------------------------------------------------------ PoS update audits
 * The evaluation request that follows an edit, an append or a reshape (messages: networking/
 * shared.rs:90-129, 165-188; server: networking/server.rs:833-906, 963-1077; client checks:
 * networking/client.rs:755-827, 1009-1135, 1273-1420).  Additive within version 3.  Elements are
 * Montgomery limbs as everywhere; a file image is WriteableFt63, 7 bytes per element, and its
 * entries are BLAKE3-only like the other PoS entries (LCPC_ERR_UNSUPPORTED for another digest). */
/* evaluate_field_polynomial_at_point[_with_elevated_degree] (fields.rs:160-186):
 * out = sum_{i<n} coeffs[i] x^(i + degree_offset), one element; n = 0 gives zero; x^0 = 1 also for
 * x = 0.  One streaming pass over the coefficients, no power vector. */
lcpc_status lcpc_eval_poly(lcpc_field f, const uint64_t *coeffs, size_t n, const uint64_t *x,
                           uint64_t degree_offset, uint64_t *out);
/* the same from device coefficients (8-byte aligned) */
lcpc_status lcpc_eval_poly_device(lcpc_field f, const void *d_coeffs, size_t n, const uint64_t *x,
                                  uint64_t degree_offset, uint64_t *out);
/* the same over convert_byte_vec_to_field_elements_vec(bytes) (fields.rs:109-112): ceil(n_bytes / 7)
 * coefficients read straight from the bytes, no element image.  Host bytes of any alignment go up in
 * blocks of LCPC_POS_EVAL_STAGE_BYTES, each block evaluated as it lands, elevated by the index of its
 * first element. */
#define LCPC_POS_EVAL_STAGE_BYTES ((size_t)7 << 20)
lcpc_status lcpc_pos_eval_poly_bytes(const uint8_t *bytes, size_t n_bytes, const uint64_t *x,
                                     uint64_t degree_offset, uint64_t *out);
/* the same from a device file image (8-byte aligned) */
lcpc_status lcpc_pos_eval_poly_bytes_device(const void *d_bytes, size_t n_bytes, const uint64_t *x,
                                            uint64_t degree_offset, uint64_t *out);
/* left_multiply_unencoded_matrix_by_vector (file_handler.rs:614-638) without an element image:
 * out[c] = sum_r left[r] M[r][c], c < pre, over the file's rows of pre elements (the last row zero
 * padded); n_left must be the row count ceil(ceil(n_bytes / 7) / pre), else LCPC_ERR_INVALID_ARG.
 * pre a power of two >= 8 reads the bytes directly; other widths pack first. */
lcpc_status lcpc_pos_left_multiply_bytes(const uint8_t *bytes, size_t n_bytes, size_t pre,
                                         const uint64_t *left, size_t n_left, uint64_t *out);
lcpc_status lcpc_pos_left_multiply_bytes_device(const void *d_bytes, size_t n_bytes, size_t pre,
                                                const uint64_t *left, size_t n_left, uint64_t *out);
/* The same for n_vecs vectors in one pass over the image (batched audits of a stored file: m
 * evaluation points, one read of the file, one set of opened columns):
 *   out[t pre + c] = sum_r lefts[t n_left + r] M[r][c],   1 <= n_vecs <= LCPC_BATCH_MAX_TENSORS,
 * bit for bit n_vecs calls of lcpc_pos_left_multiply_bytes.  n_left must be the file's row count;
 * argument rules and status codes are those of the single entry, reported before any device work
 * (a NULL pointer, n_bytes or pre of 0, n_vecs outside its range, a wrong n_left, a device image
 * that is not 8-byte aligned: LCPC_ERR_INVALID_ARG; no device: LCPC_ERR_NO_DEVICE).
 * The host entry takes bytes of any alignment: the image goes up once, in blocks of whole rows near
 * 8 MiB, each block contracted as it lands and the blocks' partial sums folded at the end. */
lcpc_status lcpc_pos_left_multiply_bytes_many(const uint8_t *bytes, size_t n_bytes, size_t pre,
                                              const uint64_t *lefts, size_t n_vecs, size_t n_left, uint64_t *out);
lcpc_status lcpc_pos_left_multiply_bytes_many_device(const void *d_bytes, size_t n_bytes, size_t pre,
                                                     const uint64_t *lefts, size_t n_vecs, size_t n_left,
                                                     uint64_t *out);
/* The kernel the two entries above run for (pre, n_vecs), a pure function of its arguments and of
 * LCPC_NO_MFMA (read once per process).  0: pre is no power of two >= 8 -- the image is packed to
 * elements first, then lcpc_collapse_columns_many's kernel;  1: the VALU kernel on the bytes
 * (pre < 64, fewer than 16 vectors, LCPC_NO_MFMA=1);  2: the int8 matrix cores on the bytes (pre >= 64
 * and at least 16 vectors, where they measured faster).  No device needed. */
int lcpc_pos_left_multiply_many_kernel(size_t pre, size_t n_vecs);
/* Grouped audits: lcpc_pos_left_multiply_bytes for n_jobs files in one call (a server's queue of
 * audits over different files, most of them small).  Job j is the image bytes[j] of n_bytes[j] bytes
 * with rows of pre[j] elements; its left vector is the next n_rows_j = ceil(ceil(n_bytes[j] / 7) / pre[j])
 * words of lefts, its result the next pre[j] words of out:
 *   out_j[c] = sum_r left_j[r] M_j[r][c].
 * BIT-IDENTITY: out_j is word for word what lcpc_pos_left_multiply_bytes(bytes[j], n_bytes[j], pre[j],
 * left_j, n_rows_j, .) returns, for every job that call accepts (field sums are exact: neither the
 * grouping nor a job's row split shows).
 * PADDING is per image: job j is read through (bytes[j], n_bytes[j]) alone and zero padded past its
 * own end; the bytes that follow an image in an arena belong to the next file and never enter.
 * Host images may have any alignment.  Consecutive jobs are staged at 8-byte aligned offsets of a
 * device arena in staging groups of at most LCPC_POS_GROUP_STAGE_BYTES image bytes (and bounded job,
 * row and column counts), one upload and one contraction launch (plus one fold launch for the jobs
 * split in rows) per group, each group contracted as it lands: the launches are O(groups), never
 * O(n_jobs), and the device memory in use is the arena plus the largest single file.  A job larger
 * than a staging group, or with pre no power of two >= 8, goes through lcpc_pos_left_multiply_bytes'
 * own path inside the same call (it ends the group before it).
 * Errors, before any device work: a NULL pointer, n_jobs = 0, a job with n_bytes or pre of 0, n_left_total
 * != sum n_rows_j, n_out_total != sum pre[j]: LCPC_ERR_INVALID_ARG; no device: LCPC_ERR_NO_DEVICE.
 * Threading as every entry: a stream of its own per call. */
#define LCPC_POS_GROUP_STAGE_BYTES ((size_t)32 << 20)
lcpc_status lcpc_pos_left_multiply_bytes_grouped(const uint8_t *const *bytes, const size_t *n_bytes, const size_t *pre,
                                                 size_t n_jobs, const uint64_t *lefts, size_t n_left_total,
                                                 uint64_t *out, size_t n_out_total);
/* The same over one device arena the caller owns: job j is the n_bytes[j] bytes at d_arena +
 * offsets[j], offsets[j] a multiple of 8 (else LCPC_ERR_INVALID_ARG; d_arena itself 8-byte aligned).
 * No byte outside [offsets[j], offsets[j] + n_bytes[j]) enters job j's value, whatever the arena holds
 * there.  Nothing is staged but the launches' tables; the groups are those of the host entry. */
lcpc_status lcpc_pos_left_multiply_bytes_grouped_device(const void *d_arena, const size_t *offsets,
                                                        const size_t *n_bytes, const size_t *pre, size_t n_jobs,
                                                        const uint64_t *lefts, size_t n_left_total, uint64_t *out,
                                                        size_t n_out_total);
/* Host-only, no device (like lcpc_pos_read_plan): the work list of the launches the two entries above
 * make for these jobs, a pure function of its arguments (and of LCPC_POS_GROUP_BYTES, a test seam read
 * at every call that can only lower the staging group's size).  A tile is rows [row_lo, row_hi) x
 * 56-byte runs [run_lo, run_hi) of one job, a lane per run; `launch` counts the grouped launches from
 * 0 and `wave` the waves of a launch (4 per workgroup): the tiles of one wave share a row count and a
 * width.  A job routed to the single-file path has one record with launch = LCPC_POS_GROUP_SINGLE,
 * wave = 0, over all its rows and its ceil(pre / 8) runs.  Every (job, row, run) is in exactly one
 * record.  Writes at most cap records to tiles (may be NULL with cap 0), the count needed to *n_tiles
 * and the number of grouped launches to *n_launches (either may be NULL). */
typedef struct lcpc_pos_group_tile {
  uint64_t job, row_lo, row_hi, run_lo, run_hi;
  uint32_t launch, wave;
} lcpc_pos_group_tile;
#define LCPC_POS_GROUP_SINGLE 0xffffffffu
lcpc_status lcpc_pos_group_plan(const size_t *n_bytes, const size_t *pre, size_t n_jobs, lcpc_pos_group_tile *tiles,
                                size_t cap, size_t *n_tiles, size_t *n_launches);
/* Host-only: out[i] = (in[i] R) mod p, the Montgomery word of any 64-bit value in[i] (canonical or
 * not), R = 2^64; f must be LCPC_FT63 (else LCPC_ERR_UNSUPPORTED).  in == out is allowed.  What a
 * server does to the canonical column values of a `.porenc` before it sends them. */
lcpc_status lcpc_field_to_montgomery(lcpc_field f, const uint64_t *in, uint64_t *out, size_t n);

/* ---- PoS grouped check of audit responses (the client side of the grouped audits) ----
 * NO COUNTERPART IN THE REFERENCE.  Additive within LCPC_ABI_VERSION 3.  An auditor that holds the
 * roots of many stored files checks a queue of plain audit responses -- per file the server's result
 * vector and the opened columns with their Merkle paths -- together.  Job j passes (verdict[j] = 0)
 * iff every opened column hashes, through its path, to root and the result vector, decoded (ifft_oi),
 * cut to pre coefficients, zero padded and re-encoded, equals sum_r left[r] col_k[r] at every idx[k],
 * left = [1, x^pre, x^(2 pre), ...] for x = point; values[j] = <dec[:pre], [1, x, x^2, ...]>, the file
 * polynomial's value at the point.  A Merkle path that does not lead to root is verdict 1; paths that
 * pass and a column value that disagrees is verdict 2 (paths first, then values).  values[j] is
 * written for every job and means something only where verdict[j] == 0.  A bad response is a verdict,
 * never an error status, and never changes another job's verdict or value.
 * EQUALITY: verdict and value are what the single sequence (lcpc_hash_field_columns,
 * lcpc_verify_leaf_paths, lcpc_pos_side_vectors, lcpc_ifft_oi_rows, the dot, lcpc_encode,
 * lcpc_verify_column_values) gives for that response, the value word for word.  cols and result are
 * untrusted 64-bit words and are not range checked, as there; point is a field element in Montgomery
 * form.  Ft63 and BLAKE3 only; the entry takes no encoding, so no other digest can reach it.
 * Consecutive jobs fill staging groups of at most LCPC_POS_GROUP_STAGE_BYTES bytes of columns (and
 * at most 2^16 jobs and 2^16 columns, which bounds the paths); a group's columns (each at a 16-byte aligned stride),
 * paths, roots, indices, left vectors and tables go up in one copy from one of two page-locked blocks
 * and are checked in two launches, the next group gathered meanwhile.  The result vectors take one
 * decode per distinct enc and one encode per distinct (pre, enc) for the whole call.  The launches
 * never grow with n_jobs.  A job whose columns exceed a group (or number more than 2^16) ends the group
 * before it and goes through the single sequence inside the same call.
 * Errors, before any device work: a NULL pointer (idx, cols and paths may be NULL where n_cols == 0),
 * n_jobs = 0, pre, enc or file_len of 0, enc no power of two or enc <= pre (the dims every stored file
 * has: EncodedFileWriter's, e.g. 24 / 32), an idx that is not strictly
 * increasing or not below enc: LCPC_ERR_INVALID_ARG; enc beyond the field's two-adicity:
 * LCPC_FFT_TOO_BIG; no device: LCPC_ERR_NO_DEVICE.  Threading as every entry: a stream of its own per call. */
typedef struct lcpc_pos_audit_job {
  const uint8_t *root;    /* 32 B, the root the client holds */
  size_t file_len, pre, enc;
  uint64_t point;         /* the evaluation point, the word lcpc_pos_side_vectors takes */
  const uint64_t *idx;    /* n_cols opened column indices, strictly increasing, < enc */
  size_t n_cols;
  const uint64_t *cols;   /* [n_cols][n_rows] Montgomery words, n_rows = rows of file_len at pre */
  const uint8_t *paths;   /* n_cols x log2(enc) x 32 B */
  const uint64_t *result; /* enc words: the server's result vector */
} lcpc_pos_audit_job;
lcpc_status lcpc_pos_verify_evaluations_grouped(const lcpc_pos_audit_job *jobs, size_t n_jobs, uint8_t *verdict,
                                                uint64_t *values);
/* Host-only, no device (like lcpc_pos_group_plan): the work list of the first launch of each staging
 * group the entry above makes for jobs of these file lengths, pre and opened-column counts, a pure function
 * of its arguments (and of LCPC_POS_GROUP_BYTES, the test seam that can only lower the group's size).
 * A record is columns [col_lo, col_hi) (at most 64, a lane each) of one job and one 1-KiB chunk of their
 * leaf messages: one wave; `launch` counts the groups that launch from 0, `wave` the waves of a launch
 * (4 per workgroup).  A job routed to the single sequence has one record per chunk over all its columns
 * with launch = LCPC_POS_GROUP_SINGLE, wave = 0.  Every (job, column, chunk) is in exactly one record;
 * a job with n_cols = 0 has none.  Writes at most cap records to tiles (may be NULL with cap 0), the
 * count needed to *n_tiles and the number of launching groups to *n_launches (either may be NULL).
 * Errors: a NULL array, n_jobs = 0, a file_len or pre of 0: LCPC_ERR_INVALID_ARG. */
typedef struct lcpc_pos_verify_tile {
  uint64_t job, col_lo, col_hi, chunk;
  uint32_t launch, wave;
} lcpc_pos_verify_tile;
lcpc_status lcpc_pos_verify_group_plan(const size_t *file_len, const size_t *pre, const size_t *n_cols, size_t n_jobs,
                                       lcpc_pos_verify_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches);
/* Host-only, no device (like lcpc_pos_update_chunk_range): the rows an update touches.  The
 * reference's edit and append handlers (networking/server.rs:963-1077) each pick their "original
 * rows" differently and disagree with their clients; this is the one rule that replaces them.
 * An update writes `len` bytes at `offset` into a file of old_len bytes, offset <= old_len
 * (offset == old_len is an append; offset + len > old_len extends the file).
 * *row_lo = offset / (7 pre);  *row_hi = one past the last row of the NEW file that holds a
 * changed byte;  [*old_lo, *old_hi) = the OLD file's bytes of those rows, clipped to old_len
 * (empty for an append that starts a fresh row).  len == 0 or offset > old_len: INVALID_ARG. */
lcpc_status lcpc_pos_update_rows(size_t old_len, size_t offset, size_t len, size_t pre,
                                 size_t *row_lo, size_t *row_hi, size_t *old_lo, size_t *old_hi);
/* One update audit's GPU half (networking/server.rs:833-906, 963-1077): both images are committed
 * (lcpc_pos_commit_eval_bytes_device each, left = [1, x^pre, x^2pre, ...] over the commitment's rows,
 * its own pre), and both sets of columns are opened with paths.  For a reshape the two images are
 * the same pointer, the encodings differ, and *expected_eval (else NULL) = the file polynomial at x.
 * result_* : n_cols elements; cols_* : n_idx x n_rows; paths_* : n_idx x log2(n_cols) x 32 B. */
lcpc_status lcpc_pos_update_evaluation(
    const lcpc_encoding *e_old, const void *d_old, size_t n_old,
    const lcpc_encoding *e_new, const void *d_new, size_t n_new, const uint64_t *x,
    const uint64_t *idx_old, size_t n_idx_old, const uint64_t *idx_new, size_t n_idx_new,
    uint64_t *result_old, uint64_t *cols_old, uint8_t *paths_old, uint8_t root_old[32],
    uint64_t *result_new, uint64_t *cols_new, uint8_t *paths_new, uint8_t root_new[32],
    uint64_t *expected_eval);

/* ------------------------------------------------------------------ PoS encoded files
 * (proof-of-storage/src/lcpc_online/encoded_file_{writer,reader}.rs, WriteableFt63).
 * A `.porenc` image is column-major: column c holds row_capacity elements starting at byte
 * c * row_capacity * 8, each the 8-byte little-endian canonical repr (F::WRITTEN_BYTES_WIDTH,
 * field_vec_to_raw_bytes, data_field.rs:24,62-70); rows past rows_written are not touched (zero in
 * a fresh set_len file).  A `.portree` image is MerkleTree::to_bytes: the 2 enc - 1 digests
 * leaves || parents, root last (merkle_tree.rs:14-27,61-63).  Callers pass mmaps of the files. */
/* EncodedFileWriter::convert_unencoded_file (encoded_file_writer.rs:134-231): the data's 7-byte
 * elements in rows of pre, each row zero padded and Ligero-encoded to enc elements, written to
 * porenc; tree = the Merkle tree of the column digests (ColumnDigestAccumulator,
 * column_digest_accumulator.rs:62-118).  *rows_written = ceil(ceil(n_bytes / 7) / pre) and
 * row_capacity must be >= it (the reference writer allocates 2 * rows, :77-80). */
lcpc_status lcpc_pos_encode_file(const uint8_t *data, size_t n_bytes, size_t pre, size_t enc,
                                 size_t row_capacity, uint8_t *porenc, uint8_t *tree,
                                 size_t *rows_written);
/* same, processing at most batch_rows rows per GPU pass (rounded to whole 1-KiB column-digest
 * chunks; 0 = automatic, about 4 GiB of device memory per pass) */
lcpc_status lcpc_pos_encode_file_batched(const uint8_t *data, size_t n_bytes, size_t pre, size_t enc,
                                         size_t row_capacity, uint8_t *porenc, uint8_t *tree,
                                         size_t *rows_written, size_t batch_rows);
/* ---- PoS grouped ingest: many small files encoded, hashed and folded to trees in one pass ----
 * NO COUNTERPART IN THE REFERENCE (its server takes one upload per request, networking/server.rs:
 * 396-433).  Additive within LCPC_ABI_VERSION 3.  The step before the grouped audits and the grouped
 * check: a queue of (raw image, pre, enc) jobs becomes stored files and roots with a number of launches
 * that does not grow with the number of files.
 * EQUALITY: for every job, rows_written, rows [0, rows_written) of every column of porenc, tree and root
 * are byte for byte what lcpc_pos_encode_file(data, n_bytes, pre, enc, row_capacity, ...) produces, and
 * cvs is what lcpc_pos_writer_copy_cvs returns for a finalized writer over the same file.  Elements of
 * porenc at rows >= rows_written are not touched.  Every output pointer may be NULL (porenc with
 * row_capacity 0): nothing of that kind is returned for the job, and a call in which no job has a porenc
 * copies no encoded word back to the host (a client that only needs the roots).
 * PADDING is per image: job j is read through (data, n_bytes) alone and zero padded past its own end;
 * host images may have any alignment.  A job with n_bytes == 0 is legal: zero rows, every leaf BLAKE3 of
 * 32 zero bytes.
 * STAGING: consecutive jobs form a staging group of at most LCPC_POS_GROUP_STAGE_BYTES of images (8-byte
 * aligned offsets; LCPC_POS_GROUP_BYTES, the test seam, can only lower it), at most four times that in
 * encoded bytes (sum rows * enc * 8, rows rounded up to even), at most LCPC_POS_INGEST_MAX_JOBS jobs,
 * LCPC_POS_INGEST_MAX_ROWS rows, LCPC_POS_INGEST_MAX_TILES tiles and LCPC_POS_INGEST_MAX_TREE_BYTES of
 * trees.  One page-locked block per group (images and tables) goes up in one copy and the outputs come
 * back into it; two blocks alternate, and the host scatters a group's columns into the jobs' porenc
 * while the next group runs.  A group takes at most LCPC_POS_INGEST_LAUNCHES_PER_GROUP kernel launches,
 * whatever the number of jobs or of distinct enc, all inside one profiling region (pos_group_ingest).
 * ROUTING: a job with enc > LCPC_POS_INGEST_MAX_ENC, or whose image or encoded bytes alone exceed a
 * group, or whose columns have more than 2^16 1-KiB chunks, ends the group before it and goes through
 * lcpc_pos_encode_file's own path inside the same call.  Every 1 <= pre < enc <= 1024 is grouped.
 * Errors, before any device work and before any output byte is written: a NULL jobs, n_jobs == 0,
 * data == NULL with n_bytes > 0, pre == 0, enc no power of two or enc <= pre, porenc with row_capacity <
 * the job's rows, porenc == NULL with row_capacity != 0: LCPC_ERR_INVALID_ARG; enc beyond the field's
 * two-adicity: LCPC_FFT_TOO_BIG; no device: LCPC_ERR_NO_DEVICE.  Ft63 and BLAKE3 only; the entry takes no
 * encoding, so no other digest can reach it.  Threading as every entry: a stream of its own per call. */
#define LCPC_POS_INGEST_MAX_ENC ((size_t)1024)  /* rows of more points take the single path (8 rows: 64 KiB of LDS) */
#define LCPC_POS_INGEST_MAX_JOBS ((size_t)1 << 16)
#define LCPC_POS_INGEST_MAX_ROWS ((size_t)1 << 23)
#define LCPC_POS_INGEST_MAX_TILES ((size_t)1 << 20)
#define LCPC_POS_INGEST_MAX_TREE_BYTES ((size_t)64 << 20)
#define LCPC_POS_INGEST_LAUNCHES_PER_GROUP 3    /* encode, chunk chaining values, leaves and trees */
#define LCPC_POS_INGEST_TILE_ROWS ((size_t)8)   /* rows of a full tile of the encode launch */
typedef struct lcpc_pos_ingest_job {
  const uint8_t *data;  /* raw image; may be NULL iff n_bytes == 0 */
  size_t n_bytes;
  size_t pre, enc;      /* 1 <= pre < enc, enc a power of two */
  uint8_t *porenc;      /* column-major image of row_capacity rows, or NULL with row_capacity 0 */
  size_t row_capacity;
  uint8_t *tree;        /* (2 enc - 1) x 32 B, MerkleTree::to_bytes, or NULL */
  uint8_t *root;        /* 32 B, or NULL */
  uint8_t *cvs;         /* lcpc_leaf_n_chunks(LCPC_FT63, rows) x enc x 32 B, [chunk][column], or NULL */
  size_t rows_written;  /* out */
} lcpc_pos_ingest_job;
lcpc_status lcpc_pos_encode_files_grouped(lcpc_pos_ingest_job *jobs, size_t n_jobs);
/* Host-only, no device (like lcpc_pos_group_plan): the work list of the encode launch of each staging
 * group the entry above makes for jobs of these sizes and dims, a pure function of its arguments (and of
 * LCPC_POS_GROUP_BYTES).  A record is a tile: rows [row_lo, row_hi) of one job, at most
 * LCPC_POS_INGEST_TILE_ROWS of them; `launch` counts the staging groups from 0 and `workgroup` the
 * workgroups of the group's encode launch: the tiles of a workgroup share enc.  A routed job has one
 * record with launch = LCPC_POS_GROUP_SINGLE, workgroup = 0, over all its rows.  Every (job, row) is in
 * exactly one record; a job with zero rows has none (it still belongs to a group).  Writes at most cap
 * records to tiles (may be NULL with cap 0), the count needed to *n_tiles and the number of staging
 * groups to *n_launches (either may be NULL).  Errors: a NULL array, n_jobs == 0, and pre / enc as above. */
typedef struct lcpc_pos_ingest_tile {
  uint64_t job, row_lo, row_hi;
  uint32_t launch, workgroup;
} lcpc_pos_ingest_tile;
lcpc_status lcpc_pos_ingest_plan(const size_t *n_bytes, const size_t *pre, const size_t *enc, size_t n_jobs,
                                 lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches);
/* ---- PoS grouped scrub: many stored files checked against leaves, tree and row code in one pass ----
 * NO COUNTERPART IN THE REFERENCE (verify_all_files_agree, file_handler.rs:505-541, is per file and can
 * only say "trees differ").  Additive within LCPC_ABI_VERSION 3.  The triage of a scrubber that walks a
 * whole store: which of these files need the per-file locate or repair?  A queue of (stored image, stored
 * digests, expected root) jobs is answered with a number of launches that does not grow with the number
 * of files; lcpc_pos_locate_porenc, lcpc_pos_repair_columns and the Berlekamp-Massey locator stay what
 * they are and are reached only for the files with a finding.
 * EQUALITY: for every job,
 *   col_status, digests, n_bad   are byte for byte what lcpc_pos_scrub_porenc over (porenc, enc,
 *       rows_written, row_capacity, tree as leaves) returns: 0 the column's digest equals its stored
 *       leaf, 1 it differs, 2 the column holds an element that is not < p (its digest written as zeros).
 *       With tree == NULL the compare is skipped: 0 or 2 only, digests still filled.  The status is
 *       decided on the device against the caller's leaves; the library's digests are never compared with
 *       themselves.  Rows at and past rows_written are never read;
 *   tree_consistent   1 iff tree_digests == 2 enc - 1 and every stored parent is the BLAKE3 node hash of
 *       its two STORED children, which by induction from the leaves up is MerkleTree::new(the first enc
 *       digests) == tree; 0 otherwise; LCPC_POS_SCRUB_NOT_EVALUATED for tree_digests 0 or enc;
 *   root_ok           stored root == expected_root; LCPC_POS_SCRUB_NOT_EVALUATED without a whole tree or
 *       without an expected_root;
 *   n_dirty_rows      the number of rows r < rows_written whose enc stored elements are not the
 *       evaluations of a polynomial of degree < pre.  For a job without a status-2 column this is exactly
 *       *n_dirty_rows of lcpc_pos_locate_porenc with no known_bad.  A job with a status-2 column reports
 *       LCPC_POS_SCRUB_ROWS_UNCHECKED: it has a finding anyway, and the per-file path treats such
 *       columns as erasures; the grouped pass masks nothing.
 * A job with rows_written == 0 is legal: the digests of zero rows, n_dirty_rows = 0.
 * STAGING: consecutive jobs form a staging group of at most LCPC_POS_GROUP_STAGE_BYTES of packed image
 * (LCPC_POS_GROUP_BYTES, the test seam, can only lower it; also bounded as the ingest's groups in jobs,
 * rows, tiles and tree bytes).  The host packs, per column, only the first rows_written elements (rounded
 * up to even, the pad word zero): the slack up to row_capacity never crosses the bus.  Stored digests,
 * expected roots and tables go up in the same copy; flags, statuses, dirty bytes and (where a job asks)
 * digests come back in one.  Two page-locked blocks alternate: the host packs group g + 1 while g runs.
 * A group takes at most LCPC_POS_SCRUB_LAUNCHES_PER_GROUP kernel launches, whatever the number of jobs
 * or of distinct enc, all inside one profiling region (pos_group_scrub).
 * ROUTING: a job with enc > LCPC_POS_SCRUB_MAX_ENC, or whose packed image alone exceeds a group, or whose
 * columns have more than 2^16 1-KiB chunks, ends the group before it and is answered inside the same
 * call by lcpc_pos_scrub_porenc and the dirty-row count of lcpc_pos_locate_porenc (its stored tree by
 * the group's third launch alone), to the same equalities.
 * Errors, before any device work and before any output byte is written: a NULL jobs, n_jobs == 0, a
 * NULL col_status, porenc == NULL with rows_written > 0, rows_written > row_capacity, pre == 0, enc no
 * power of two or enc <= pre, tree_digests not 0, enc or 2 enc - 1, tree NULL with tree_digests != 0 or
 * the reverse: LCPC_ERR_INVALID_ARG; enc beyond the field's two-adicity: LCPC_FFT_TOO_BIG; no device:
 * LCPC_ERR_NO_DEVICE.  Ft63 and BLAKE3 only.  Threading as every entry: a stream of its own per call. */
#define LCPC_POS_SCRUB_MAX_ENC ((size_t)1024)  /* as LCPC_POS_INGEST_MAX_ENC: 8 rows = 64 KiB of LDS */
#define LCPC_POS_SCRUB_TILE_ROWS ((size_t)8)   /* rows of a full tile of the row-check launch */
#define LCPC_POS_SCRUB_LAUNCHES_PER_GROUP 3    /* row check, chunk chaining values, leaves + status + tree check */
#define LCPC_POS_SCRUB_NOT_EVALUATED ((uint8_t)0xFF)
#define LCPC_POS_SCRUB_ROWS_UNCHECKED ((size_t)-1)
typedef struct lcpc_pos_scrub_job {
  const uint8_t *porenc;        /* column-major image, layout of lcpc_pos_encode_file; NULL iff rows_written == 0 */
  size_t pre, enc, rows_written, row_capacity;
  const uint8_t *tree;          /* stored digests, or NULL */
  size_t tree_digests;          /* 0 (tree NULL), enc (leaves only) or 2 enc - 1 (the whole .portree) */
  const uint8_t *expected_root; /* 32 B, or NULL */
  uint8_t *col_status;          /* enc bytes, out, required */
  uint8_t *digests;             /* enc x 32 B, out, may be NULL */
  size_t n_bad;                 /* out: non-zero status bytes */
  size_t n_dirty_rows;          /* out */
  uint8_t tree_consistent;      /* out: 1 / 0 / LCPC_POS_SCRUB_NOT_EVALUATED */
  uint8_t root_ok;              /* out: 1 / 0 / LCPC_POS_SCRUB_NOT_EVALUATED */
} lcpc_pos_scrub_job;
lcpc_status lcpc_pos_scrub_files_grouped(lcpc_pos_scrub_job *jobs, size_t n_jobs);
/* Host-only, no device (like lcpc_pos_ingest_plan): the work list of the row-check launch of each staging
 * group the entry above makes for jobs of these row counts and dims, a pure function of its arguments
 * (and of LCPC_POS_GROUP_BYTES).  A record is a tile: rows [row_lo, row_hi) of one job, at most
 * LCPC_POS_SCRUB_TILE_ROWS of them; `launch` counts the staging groups from 0 and `workgroup` the
 * workgroups of the group's row-check launch: the tiles of a workgroup share enc.  A routed job has one
 * record with launch = LCPC_POS_GROUP_SINGLE, workgroup = 0, over all its rows.  Every (job, row) is in
 * exactly one record; a job with zero rows has none (it still belongs to a group).  Outputs and errors as
 * lcpc_pos_ingest_plan. */
lcpc_status lcpc_pos_scrub_plan(const size_t *rows_written, const size_t *pre, const size_t *enc, size_t n_jobs,
                                lcpc_pos_ingest_tile *tiles, size_t cap, size_t *n_tiles, size_t *n_launches);
/* ---- PoS grouped repair: the damaged columns of many stored files recomputed, hashed and folded into
 * their trees in one pass ----
 * NO COUNTERPART IN THE REFERENCE.  Additive within LCPC_ABI_VERSION 3.  The leg after a scrub: every file
 * with a finding went through lcpc_pos_repair_columns on its own.  Here a queue of (stored image, erasure
 * set, leaves) jobs is answered with a number of launches that does not grow with the number of files.
 * EQUALITY: for every job, status, cols_out and digests_out are byte for byte what
 * lcpc_pos_repair_columns(porenc, pre, enc, rows_written, row_capacity, bad_cols, n_bad, ...) returns and
 * writes; tree_out / root_out are MerkleTree::new over `leaves` with the entries of bad_cols replaced by
 * the repaired digests.
 * VERDICTS are per job: one job's failure never fails the call and never touches a neighbour's outputs.
 * status is LCPC_ERR_UNRECOVERABLE when n_bad > enc - pre (that job does no device work), when some row
 * is no codeword on the columns that are not listed (checked whenever n_bad < enc - pre), or when a
 * column that is not listed holds a word that is not < p.  The data outputs of a failed job are
 * unspecified.  n_bad == 0 is the consistency check alone; rows_written == 0 is legal (the digests of
 * zero rows).  LISTED COLUMNS ARE NEVER READ, neither by the host packing nor by a kernel: what they
 * hold, and whether their pages can be read at all, cannot matter.
 * STAGING: consecutive jobs form a staging group of at most LCPC_POS_GROUP_STAGE_BYTES of image
 * (rows_written rounded up to even, times enc, times 8: the packed columns and the repaired ones;
 * LCPC_POS_GROUP_BYTES, the test seam, can only lower it; also bounded as the ingest's groups in jobs,
 * rows, tiles and tree bytes).  Only the first rows_written elements of the columns that are not listed
 * cross the bus, with the leaves, the lists and the tables in the same copy; flags, digests and trees come
 * back in one, the repaired columns (where a job wants them) in a second.  Two page-locked blocks
 * alternate: the host packs group g + 1 and scatters group g - 1 while g runs.  A group takes at most
 * LCPC_POS_REPAIR_LAUNCHES_PER_GROUP kernel launches, whatever the number of jobs or of distinct enc, all
 * inside one profiling region (pos_group_repair).
 * ROUTING: a job with enc > LCPC_POS_REPAIR_MAX_ENC, or whose image alone exceeds a group, or whose columns
 * have more than 2^16 1-KiB chunks, ends the group before it and goes through lcpc_pos_repair_columns
 * inside the same call (its tree by the group's last launch alone), to the same equalities.
 * Errors, before any device work and before any output byte is written: a NULL jobs, n_jobs == 0,
 * porenc == NULL with rows_written > 0, rows_written > row_capacity, pre == 0, enc no power of two or
 * enc <= pre, bad_cols NULL with n_bad > 0, a column index >= enc, a duplicate index, tree_out or root_out
 * without leaves: LCPC_ERR_INVALID_ARG; enc beyond the field's two-adicity: LCPC_FFT_TOO_BIG; no device:
 * LCPC_ERR_NO_DEVICE.  Ft63 and BLAKE3 only.  Threading as every entry: a stream of its own per call. */
#define LCPC_POS_REPAIR_MAX_ENC ((size_t)1024)  /* as LCPC_POS_INGEST_MAX_ENC: 8 rows = 64 KiB of LDS */
#define LCPC_POS_REPAIR_TILE_ROWS ((size_t)8)   /* rows of a full tile of the row launch */
#define LCPC_POS_REPAIR_LAUNCHES_PER_GROUP 4    /* locators, rows, chunk chaining values, leaves + tree */
typedef struct lcpc_pos_repair_job {
  const uint8_t *porenc;     /* column-major image (lcpc_pos_encode_file's layout); NULL iff rows_written == 0 */
  size_t pre, enc, rows_written, row_capacity;
  const uint64_t *bad_cols;  /* the erasure set: n_bad distinct columns < enc; never read from the image */
  size_t n_bad;
  const uint8_t *leaves;     /* enc x 32 B digests of the columns as they stand (e.g. the scrub's), or NULL */
  uint8_t *cols_out;         /* n_bad x rows_written x 8 B, as lcpc_pos_repair_columns, or NULL */
  uint8_t *digests_out;      /* n_bad x 32 B, or NULL */
  uint8_t *tree_out;         /* (2 enc - 1) x 32 B: MerkleTree::new(leaves with bad_cols' entries replaced by the
                                repaired digests); needs leaves; or NULL */
  uint8_t *root_out;         /* 32 B, needs leaves; or NULL */
  lcpc_status status;        /* out: LCPC_OK or LCPC_ERR_UNRECOVERABLE, this job's own verdict */
} lcpc_pos_repair_job;
lcpc_status lcpc_pos_repair_files_grouped(lcpc_pos_repair_job *jobs, size_t n_jobs);
/* Host-only, no device (like lcpc_pos_scrub_plan): the work list of the row launch of each staging group
 * the entry above makes for jobs of these row counts, dims and erasure counts, a pure function of its
 * arguments (and of LCPC_POS_GROUP_BYTES), under lcpc_pos_scrub_plan's rules.  A job with
 * n_bad > enc - pre or with zero rows has no record; `launch` counts the staging groups that launch.
 * Outputs and errors as lcpc_pos_scrub_plan. */
lcpc_status lcpc_pos_repair_plan(const size_t *rows_written, const size_t *pre, const size_t *enc,
                                 const size_t *n_bad, size_t n_jobs, lcpc_pos_ingest_tile *tiles,
                                 size_t cap, size_t *n_tiles, size_t *n_launches);
/* ---- PoS grouped locate: the damaged columns of many stored files named by their own rows in one pass
 * (Reed-Solomon syndromes, Berlekamp-Massey and a root search, as lcpc_pos_locate_porenc) ----
 * NO COUNTERPART IN THE REFERENCE.  Additive within LCPC_ABI_VERSION 3.  The leg for a store whose
 * `.portree` cannot say where the damage is: every such file went through lcpc_pos_locate_porenc on its
 * own.  Here a queue of (stored image, known-bad columns) jobs is answered with a number of launches that
 * does not grow with the number of files.
 * EQUALITY: for every job, col_status, the three counters and status are byte for byte what
 * lcpc_pos_locate_porenc(porenc, pre, enc, rows_written, row_capacity, known_bad, n_known, ...) returns
 * and writes (a job whose status is not LCPC_OK has its other outputs left as they were, as that entry
 * leaves them).  row_status has no per-file counterpart: 0 the row is a codeword on the columns that are
 * not listed, 1 its wrong positions were located, 2 it is no codeword and cannot say where.
 * VERDICTS are per job: one job's failure never fails the call and never touches a neighbour's outputs.
 * status is LCPC_ERR_UNRECOVERABLE when n_known > enc - pre (that job does no device work), or when the
 * known columns and the columns that hold a word that is not < p together exceed enc - pre.
 * n_known == enc - pre leaves no syndromes: every row is status 0.  rows_written == 0 is legal.  KNOWN
 * COLUMNS ARE NEVER READ, neither by the host packing nor by a kernel.
 * STAGING, GROUPS: exactly the grouped repair's, with known_bad as the listed columns: the same cut, the
 * same tables, the same two alternating page-locked blocks; row statuses, column statuses and row flags
 * come back in one copy.  The syndromes of the dirty rows (at most the packed image's size) and the rows'
 * position masks stay on the device.  A group takes at most LCPC_POS_LOCATE_LAUNCHES_PER_GROUP kernel
 * launches, whatever the number of jobs or of distinct enc, all inside one profiling region
 * (pos_group_locate).  NO PLAN ENTRY of its own: the work list of a group's row launch is
 * lcpc_pos_repair_plan's with n_bad = n_known.
 * ROUTING: a job with enc > LCPC_POS_LOCATE_MAX_ENC, or whose image alone exceeds a group, or whose columns
 * have more than 2^16 1-KiB chunks, ends the group before it and goes through lcpc_pos_locate_porenc
 * inside the same call.  So does, after the last group, a job one of whose columns that are not listed
 * holds a word that is not < p (status 2 in col_status): that entry names such columns and takes them as
 * erasures.  The row_status of a job answered that way is LCPC_POS_LOCATE_ROW_NOT_EVALUATED throughout.
 * Errors, before any device work and before any output byte is written: a NULL jobs, n_jobs == 0,
 * porenc == NULL with rows_written > 0, rows_written > row_capacity, pre == 0, enc no power of two or
 * enc <= pre, col_status NULL, known_bad NULL with n_known > 0, a column index >= enc, a duplicate index:
 * LCPC_ERR_INVALID_ARG; enc beyond the field's two-adicity: LCPC_FFT_TOO_BIG; no device:
 * LCPC_ERR_NO_DEVICE.  Ft63 and BLAKE3 only.  Threading as every entry: a stream of its own per call. */
#define LCPC_POS_LOCATE_MAX_ENC ((size_t)1024)  /* as LCPC_POS_REPAIR_MAX_ENC */
#define LCPC_POS_LOCATE_LAUNCHES_PER_GROUP 4    /* locators, rows + syndromes, Berlekamp-Massey + roots, columns */
#define LCPC_POS_LOCATE_ROW_NOT_EVALUATED 0xff  /* row_status of a job lcpc_pos_locate_porenc answered */
typedef struct lcpc_pos_locate_job {
  const uint8_t *porenc;     /* column-major image (lcpc_pos_encode_file's layout); NULL iff rows_written == 0 */
  size_t pre, enc, rows_written, row_capacity;
  const uint64_t *known_bad; /* erasures: n_known distinct columns < enc; never read, host or device */
  size_t n_known;
  uint8_t *col_status;       /* enc bytes, out, required: 0 / 1 / 2 / 3 as lcpc_pos_locate_porenc */
  uint8_t *row_status;       /* rows_written bytes, out, may be NULL: 0 codeword, 1 located, 2 not locatable */
  size_t n_bad_cols, n_dirty_rows, n_unlocatable_rows; /* out */
  lcpc_status status;        /* out: LCPC_OK, or LCPC_ERR_UNRECOVERABLE (known + non-canonical > enc - pre) */
} lcpc_pos_locate_job;
lcpc_status lcpc_pos_locate_files_grouped(lcpc_pos_locate_job *jobs, size_t n_jobs);
/* The streaming writer itself: EncodedFileWriter::new (:40-105; porenc = the preallocated
 * image of row_capacity rows, batch_rows as above), push_bytes (:233-262), and
 * finalize_to_column_digest / _to_commit / _to_merkle_tree (:452-501): digests = the enc column
 * digests, tree = MerkleTree::to_bytes; either may be NULL.  Rows are encoded and written as
 * soon as the data is known to continue past them, the last ones at finalize.  When the file
 * must grow, the caller re-lays it out (EncodedFileReader::set_new_capacity, reader.rs:348-381)
 * and passes the new image with set_target.  porenc = NULL with row_capacity = 0 is a digest-only
 * writer: the rows are encoded and hashed into the column digests but written nowhere
 * (RowGeneratorIter::get_column_digests / convert_to_commit_root over a byte stream,
 * row_generator_iter.rs:29-41, 68-77; ColumnDigestAccumulator, column_digest_accumulator.rs:62-118). */
typedef struct lcpc_pos_writer lcpc_pos_writer;
lcpc_status lcpc_pos_writer_new(size_t pre, size_t enc, uint8_t *porenc, size_t row_capacity,
                                size_t batch_rows, lcpc_pos_writer **out);
void lcpc_pos_writer_free(lcpc_pos_writer *w);
lcpc_status lcpc_pos_writer_set_target(lcpc_pos_writer *w, uint8_t *porenc, size_t row_capacity);
size_t lcpc_pos_writer_rows_written(const lcpc_pos_writer *w);
lcpc_status lcpc_pos_writer_push_bytes(lcpc_pos_writer *w, const uint8_t *bytes, size_t n);
lcpc_status lcpc_pos_writer_finalize(lcpc_pos_writer *w, uint8_t *digests, uint8_t *tree,
                                     size_t *rows_written, size_t *bytes_of_data);
/* ColumnDigestAccumulator<Blake3, F> with ColumnsToCareAbout::All (column_digest_accumulator.rs:
 * 17-118; the server's upload path, server.rs:433, and RowGeneratorIter): column digests of a
 * matrix pushed a batch of encoded rows at a time (row-major, width elements each, Montgomery
 * limbs as everywhere else).  Each column's digest is BLAKE3(32 zero bytes || repr of its elements),
 * hashed on the GPU in 1-KiB chunks as they complete, so memory stays one batch of rows.  finalize
 * writes the width digests (get_column_digests) and / or the Merkle tree (finalize_to_merkle_tree:
 * 2 width - 1 digests, root last; width a power of two >= 2); either may be NULL.  Fields whose
 * elements tile a chunk (not Ft191).  ColumnsToCareAbout::Only is not offered: the reference's
 * update checks the row length against the tracked count and indexes the digests by column
 * number (:63-84), so it only works when it equals All, and no caller uses it. */
typedef struct lcpc_column_digests lcpc_column_digests;
/* batch_rows: rows buffered before a GPU pass hashes their complete chunks (0 = about 256 MiB) */
lcpc_status lcpc_column_digests_new(lcpc_field f, size_t width, size_t batch_rows,
                                    lcpc_column_digests **out);
void lcpc_column_digests_free(lcpc_column_digests *a);
size_t lcpc_column_digests_width(const lcpc_column_digests *a);      /* get_width :58-60 */
lcpc_status lcpc_column_digests_update(lcpc_column_digests *a, const uint64_t *rows, size_t n_rows);
lcpc_status lcpc_column_digests_finalize(lcpc_column_digests *a, uint8_t *digests, uint8_t *tree);
/* EncodedFileReader::process_file_to_merkle_tree (encoded_file_reader.rs:328-346).
 * LCPC_ERR_INVALID_ARG if an element is not canonical (from_repr(..).unwrap() panics there). */
lcpc_status lcpc_pos_porenc_tree(const uint8_t *porenc, size_t enc, size_t rows_written,
                                 size_t row_capacity, uint8_t *tree);
/* FileHandler::reencode_row (file_handler.rs:380-402) for a range of rows: bytes are the raw
 * data of rows [row_lo, row_lo + ceil(n_bytes / (7 pre))) (the last row may be short and is
 * zero-padded); each row is packed, encoded and written into the column-major .porenc image
 * (column stride row_capacity), as replace_encoded_row does (encoded_file_reader.rs:255-315).
 * edit_bytes / append_bytes (:279-366) re-encode the touched rows this way. */
lcpc_status lcpc_pos_reencode_rows(const uint8_t *bytes, size_t n_bytes, size_t pre, size_t enc,
                                   size_t row_lo, uint8_t *porenc, size_t row_capacity);
/* EncodedFileReader::get_unencoded_row_bytes / decode_to_target_file (encoded_file_reader.rs:
 * 59-91) for rows [row_lo, row_hi): (row_hi - row_lo) * pre * 7 bytes into out */
lcpc_status lcpc_pos_decode_porenc(const uint8_t *porenc, size_t pre, size_t enc,
                                   size_t row_capacity, size_t row_lo, size_t row_hi,
                                   uint8_t *out);

/* ------------------------------------------------------------------ PoS column chunk-CV cache
 * Incremental Merkle updates of a stored file (no counterpart in the reference, whose edit_bytes /
 * append_bytes rehash the whole .porenc; the trees are the same bit for bit).  A column digest is
 * BLAKE3(32 zero bytes || the column's rows_written 8-byte elements): a tree over 1-KiB chunks,
 * where a chunk's chaining value (CV) depends only on its bytes, its chunk counter and whether it
 * is the message's only chunk (the ROOT flag).  Chunk 0 covers rows [0, 124), chunk c >= 1 rows
 * [128 c - 4, 128 c + 124) (lcpc_leaf_chunk_first_row).  The cache keeps every column's CVs in
 * device memory, [chunk][column] x 32 bytes (the layout lcpc_pos_writer computes them in); an
 * update rereads and rehashes only the chunks an edit or append changed, and the digests and tree
 * are one fold of the cache that leaves it intact.  WriteableFt63 only, like the file layer. */
typedef struct lcpc_pos_chunk_cache lcpc_pos_chunk_cache;
/* Host-only (no device): the chunks [*chunk_lo, *chunk_hi) an update must rehash when rows
 * [row_lo, row_hi) changed and the row count went from old_rows to new_rows >= old_rows: the
 * chunks holding those rows, and on growth everything from min(chunk of row_lo, the old last
 * chunk) -- whose length changes, or which loses ROOT if it was the only chunk -- through the new
 * last chunk.  A shrinking row count or row_hi > new_rows is LCPC_ERR_INVALID_ARG; nothing to do
 * gives an empty range. */
lcpc_status lcpc_pos_update_chunk_range(size_t old_rows, size_t new_rows, size_t row_lo,
                                        size_t row_hi, size_t *chunk_lo, size_t *chunk_hi);
/* One full pass over the image (the cost of lcpc_pos_porenc_tree), keeping the CVs.
 * LCPC_ERR_INVALID_ARG if an element is not canonical, as lcpc_pos_porenc_tree. */
lcpc_status lcpc_pos_chunk_cache_from_porenc(const uint8_t *porenc, size_t enc, size_t rows_written,
                                             size_t row_capacity, lcpc_pos_chunk_cache **out);
/* From saved CVs: lcpc_leaf_n_chunks(LCPC_FT63, rows_written) * enc * 32 bytes, [chunk][column]. */
lcpc_status lcpc_pos_chunk_cache_from_cvs(const uint8_t *cvs, size_t enc, size_t rows_written,
                                          lcpc_pos_chunk_cache **out);
void lcpc_pos_chunk_cache_free(lcpc_pos_chunk_cache *c);
size_t lcpc_pos_chunk_cache_enc(const lcpc_pos_chunk_cache *c);
size_t lcpc_pos_chunk_cache_rows(const lcpc_pos_chunk_cache *c);
size_t lcpc_pos_chunk_cache_n_chunks(const lcpc_pos_chunk_cache *c);
/* CVs of chunks [chunk_lo, chunk_hi): (chunk_hi - chunk_lo) * enc * 32 bytes */
lcpc_status lcpc_pos_chunk_cache_copy_cvs(const lcpc_pos_chunk_cache *c, size_t chunk_lo,
                                          size_t chunk_hi, uint8_t *out);
/* Rows [row_lo, row_hi) of the image changed and the file now has new_rows_written rows (>= the
 * cache's): the chunks of lcpc_pos_update_chunk_range are reread from the image (enc strided
 * slices through page-locked staging) and rehashed, the cache growing by whole chunk rows; the
 * range is reported (either pointer may be NULL).  On any error, a non-canonical element
 * (LCPC_ERR_INVALID_ARG) included, the cache is unchanged. */
lcpc_status lcpc_pos_chunk_cache_update(lcpc_pos_chunk_cache *c, const uint8_t *porenc,
                                        size_t row_capacity, size_t row_lo, size_t row_hi,
                                        size_t new_rows_written, size_t *chunk_lo, size_t *chunk_hi);
/* The same with the image read from the open file fd (pread of the affected slices) instead of a
 * mapping: mapping and unmapping a multi-GB .porenc costs more than an update's 1 KiB per column.
 * A file that ends before a slice is LCPC_ERR_INVALID_ARG. */
lcpc_status lcpc_pos_chunk_cache_update_fd(lcpc_pos_chunk_cache *c, int fd, size_t row_capacity,
                                           size_t row_lo, size_t row_hi, size_t new_rows_written,
                                           size_t *chunk_lo, size_t *chunk_hi);
/* The enc column digests and / or MerkleTree::to_bytes (2 enc - 1 digests) from the cache; either
 * may be NULL; layouts of lcpc_pos_writer_finalize. */
lcpc_status lcpc_pos_chunk_cache_tree(const lcpc_pos_chunk_cache *c, uint8_t *digests, uint8_t *tree);
/* After lcpc_pos_writer_finalize: the writer's chunk count and its n_chunks * enc * 32 bytes of
 * CVs, so a new file gets its cache without a second pass over the image. */
size_t lcpc_pos_writer_n_chunks(const lcpc_pos_writer *w);
lcpc_status lcpc_pos_writer_copy_cvs(const lcpc_pos_writer *w, uint8_t *out);
/* lcpc_leaves_from_cvs by the cache's non-clobbering fold (one thread per column, a register stack
 * of subtree roots): the same leaves; cvs_after (optional) receives the device copy of the CVs as
 * the fold left it, which equals cvs. */
lcpc_status lcpc_leaves_fold_cvs(const uint8_t *cvs, size_t n_chunks, size_t n_cols, uint8_t *leaves,
                                 uint8_t *cvs_after);

/* ------------------------------------------------------------------ PoS checkable reads
 * Reading bytes [byte_start, byte_end) of a stored file so that the client can check them against
 * the 32-byte root it keeps (no counterpart in the reference: RequestFileRow, networking/server.rs:
 * 474-493, answers with bytes the client must trust, or the client downloads the whole file and
 * recommits it, client.rs:306-429).  Additive within version 3; WriteableFt63 and BLAKE3 only.
 *
 * Two messages, IN THIS ORDER -- the order is a soundness condition, not a convention:
 *   1. the client asks for the range and receives the raw bytes of the whole rows that cover it,
 *      [row_lo * 7 pre, min(row_hi * 7 pre, file_len));
 *   2. ONLY THEN the client draws the column indices (strictly increasing, < enc) and sends them;
 *      the server answers with one opening per column.
 * A server that knows the columns before it sends the rows can interpolate a wrong row that agrees
 * with the committed one at all of them (fewer than pre columns are opened).
 *
 * A column's leaf is BLAKE3(32 zero bytes || its rows_written 8-byte elements), a left-balanced tree
 * over n = lcpc_leaf_n_chunks(LCPC_FT63, rows_written) 1-KiB chunks.  An opening covers only the
 * chunks [chunk_lo, chunk_hi) that hold the rows read:
 *   segment  the column's elements of rows [seg_row_lo, seg_row_hi) -- the rows of those chunks,
 *            clipped to rows_written -- as 8-byte canonical reprs, the bytes of the `.porenc`;
 *   covers   walk the tree from the root [0, n); a node [lo, hi) of more than one chunk splits at
 *            lo + (the largest power of two < hi - lo).  A node disjoint from [chunk_lo, chunk_hi)
 *            contributes its chaining value (never with ROOT) and is not descended; a node inside
 *            the range contributes nothing; any other node is descended, left then right.  The
 *            covers are those values in walk order: none when n = 1 or the range is every chunk,
 *            at most 2 log2(n) otherwise;
 *   path     the column's Merkle path, as everywhere.
 * The client rebuilds each leaf from the segment's chunk CVs (their true chunk counters) and the
 * covers, ROOT on the last parent (a one-chunk leaf carries ROOT on the chunk), checks the paths
 * with lcpc_verify_leaf_paths, and checks the rows against the segments: with a private random u over
 * rows [row_lo, row_hi) (zero on the segment's other rows), v = u^T M over the received bytes
 * (lcpc_pos_left_multiply_bytes) and Enc(v), every opened column j must have
 * Enc(v)[j] = sum_r u_r segment_j[r].  If the committed rows are codewords, a wrong row differs from
 * the committed one in at least enc - pre + 1 columns; u keeps the difference non-zero except with
 * probability 1/p, and each column, drawn after the rows were sent, misses it with probability at
 * most pre / enc. */
/* Host-only, no device.  rows = ceil(ceil(file_len / 7) / pre) and rb = 7 pre:
 * *row_lo = byte_start / rb, *row_hi = ceil(byte_end / rb); [*chunk_lo, *chunk_hi) = the chunks
 * that hold those rows; [*seg_row_lo, *seg_row_hi) = the rows of those chunks clipped to rows;
 * *n_cover = the number of cover nodes, and cover_nodes[2 j], cover_nodes[2 j + 1] = the chunk range
 * [lo, hi) of cover j in order.  Any result pointer may be NULL; cover_cap = the pairs cover_nodes
 * has room for (128 is enough for any size_t; too few is LCPC_ERR_INVALID_ARG).
 * byte_start >= byte_end, byte_end > file_len or pre == 0: LCPC_ERR_INVALID_ARG. */
lcpc_status lcpc_pos_read_plan(size_t file_len, size_t byte_start, size_t byte_end, size_t pre,
                               size_t *row_lo, size_t *row_hi, size_t *chunk_lo, size_t *chunk_hi,
                               size_t *seg_row_lo, size_t *seg_row_hi, size_t *n_cover,
                               size_t *cover_nodes, size_t cover_cap);
/* The server's cover values for the columns idx[0..n_idx) (each < enc) opened on chunks
 * [chunk_lo, chunk_hi): covers_out[n_idx][n_cover][32], from the chunk-CV cache, which is only read.
 * An empty range or chunk_hi past the cache's chunks: LCPC_ERR_INVALID_ARG. */
lcpc_status lcpc_pos_segment_covers_from_cache(const lcpc_pos_chunk_cache *cache, const uint64_t *idx,
                                               size_t n_idx, size_t chunk_lo, size_t chunk_hi,
                                               uint8_t *covers_out);
/* The same bytes without a cache, from the opened columns themselves: cols[n_idx][rows_written]
 * canonical 8-byte elements as the `.porenc` holds them.  An element that is not < p is
 * LCPC_ERR_INVALID_ARG (as lcpc_pos_porenc_tree). */
lcpc_status lcpc_pos_segment_covers_from_columns(const uint64_t *cols, size_t rows_written, size_t n_idx,
                                                 size_t chunk_lo, size_t chunk_hi, uint8_t *covers_out);
/* The client's side: leaves_out[n_idx][32] rebuilt from segs[n_idx][seg_rows] (canonical 8-byte
 * elements, seg_rows = seg_row_hi - seg_row_lo of the plan) and covers[n_idx][n_cover][32].
 * weights: NULL, or seg_rows elements (Montgomery limbs) u_r for the segment's rows; then
 * dots_out[k] = sum_r weights[r] segs[k][r] (Montgomery limbs, summed in the pass that hashes the
 * segments).  dots_out is NULL iff weights is.  A segment element that is not < p is a verdict, not
 * an error: canonical_ok[k] = 0 (else 1), the call still returns LCPC_OK, and leaf and dot of that
 * column are unspecified.  n_cover that is not the plan's count for (rows_written, chunk_lo,
 * chunk_hi), chunk_hi past the column's chunks or an empty range: LCPC_ERR_INVALID_ARG. */
lcpc_status lcpc_pos_segment_leaves(const uint64_t *segs, size_t n_idx, size_t rows_written,
                                    size_t chunk_lo, size_t chunk_hi, const uint8_t *covers,
                                    size_t n_cover, const uint64_t *weights, uint8_t *leaves_out,
                                    uint64_t *dots_out, uint8_t *canonical_ok);

/* ------------------------------------------------------------------ row shards (multi-GPU)
 * One process per GPU holds rows [row0, row0 + n_shard_rows) of an n_rows x n_per_row Ligero
 * coefficient matrix.  With the exchanges done by the caller (lcpc_proof_of_storage_amd/
 * shard.py over RCCL: chaining values by column block, subtree roots, partial row sums,
 * challenge broadcasts) these reproduce commit (lcpc-2d/src/lib.rs:651-815) and prove
 * (:1034-1123) bit for bit.  Shard boundaries must fall on BLAKE3 chunk boundaries of the leaf
 * message (32 zero bytes || column): lcpc_leaf_chunk_first_row gives them. */
typedef struct lcpc_shard lcpc_shard;
size_t lcpc_leaf_n_chunks(lcpc_field f, size_t n_rows);          /* 1-KiB chunks per leaf */
size_t lcpc_leaf_chunk_first_row(lcpc_field f, size_t chunk);    /* first row of chunk */
lcpc_status lcpc_shard_new(const lcpc_encoding *e, const uint64_t *coeffs, size_t row0,
                           size_t n_shard_rows, size_t n_rows_total, lcpc_shard **out);
/* same with the shard's coefficient rows already in device memory */
lcpc_status lcpc_shard_new_device(const lcpc_encoding *e, const void *d_coeffs, size_t row0,
                                  size_t n_shard_rows, size_t n_rows_total, lcpc_shard **out);
void lcpc_shard_free(lcpc_shard *s);
/* chaining values of leaf chunks [chunk_lo, chunk_hi) of every column: out[chunk][col][32] */
lcpc_status lcpc_shard_chunk_cvs(const lcpc_shard *s, size_t chunk_lo, size_t chunk_hi,
                                 uint8_t *out);
/* leaf digests from all n_chunks chaining values of n_cols columns ([chunk][col][32]) */
lcpc_status lcpc_leaves_from_cvs(const uint8_t *cvs, size_t n_chunks, size_t n_cols,
                                 uint8_t *leaves);
/* partial collapse_columns over the shard's rows; tensors: n_tensors x n_shard_rows */
lcpc_status lcpc_shard_collapse(const lcpc_shard *s, const uint64_t *tensors, size_t n_tensors,
                                uint64_t *out);
/* the shard's rows of columns idx[]: out[k][r] (n x n_shard_rows elements) */
lcpc_status lcpc_shard_gather_columns(const lcpc_shard *s, const uint64_t *idx, size_t n,
                                      uint64_t *out);
/* out[i] = sum_k vecs[k][i] mod p */
lcpc_status lcpc_field_sum(lcpc_field f, const uint64_t *vecs, size_t n_vecs, size_t len,
                           uint64_t *out);
/* Device-resident variants for exchanges over RCCL (shard.py with the "nccl" backend): the
 * exchanged buffers are device pointers (torch tensors); host memory only for idx and the
 * folded row combination the transcript absorbs.  Same semantics as the host forms above. */
lcpc_status lcpc_shard_chunk_cvs_device(const lcpc_shard *s, size_t chunk_lo, size_t chunk_hi,
                                        void *d_out);
/* leaf digests of n_cols (a power of two) columns from d_cvs [chunk][col][32] (clobbered) and
 * their Merkle tree: d_hashes = leaves || level 1 || ... || root (2 n_cols - 1 digests) */
lcpc_status lcpc_leaves_tree_device(void *d_cvs, size_t n_chunks, size_t n_cols, void *d_hashes);
lcpc_status lcpc_shard_collapse_device(const lcpc_shard *s, const void *d_tensors,
                                       size_t n_tensors, void *d_out);
lcpc_status lcpc_shard_gather_columns_device(const lcpc_shard *s, const uint64_t *idx, size_t n,
                                             void *d_out);
lcpc_status lcpc_field_sum_device(lcpc_field f, const void *d_vecs, size_t n_vecs, size_t len,
                                  uint64_t *out);
/* the Fiat-Shamir steps of prove: degree-test tensor ("$l//DT" -> ChaCha20 -> Field::random,
 * lib.rs:1056-1062), absorbing field elements as their repr (lib.rs:1075-1077, 1096-1098) and
 * the column choice ("$l//CO" -> ChaCha20 -> Uniform(0, n_cols), lib.rs:1101-1110) */
lcpc_status lcpc_challenge_tensor(lcpc_transcript *tr, lcpc_field f, size_t n, uint64_t *out);
lcpc_status lcpc_transcript_append_field_elems(lcpc_transcript *tr, const uint8_t *label,
                                               size_t label_len, lcpc_field f,
                                               const uint64_t *elems, size_t n);
lcpc_status lcpc_challenge_columns(lcpc_transcript *tr, size_t n_cols, size_t n, uint64_t *out);

/* ------------------------------------------------------------------ communicators (multi-GPU)
 * One process per GPU.  A row-sharded commitment (below) moves its chaining values, subtree
 * digests, challenge vectors, partial row combinations and opened-column pieces through an
 * lcpc_comm: RCCL over xGMI (librccl.so.1, loaded at first use; every exchange is a device-side
 * send / recv on device buffers), or collectives the caller supplies (a host transport: the
 * tests, or several ranks sharing one GPU, which RCCL refuses).  All ranks must make the same
 * sequence of sharded calls on a comm, one at a time per comm.  Replaces the exchanges that
 * lcpc-2d's rayon row loop never needed (lcpc-2d/src/lib.rs:677-682 encodes rows in parallel on
 * one host; here the rows live on several GPUs). */
typedef struct lcpc_comm lcpc_comm;
#define LCPC_COMM_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: rank 0 makes the id and hands it to the other ranks out of band */
lcpc_status lcpc_comm_rccl_unique_id(uint8_t id[LCPC_COMM_UNIQUE_ID_BYTES]);
/* ncclCommInitRank on the calling thread's device (lcpc_set_device); collective */
lcpc_status lcpc_comm_rccl_new(const uint8_t id[LCPC_COMM_UNIQUE_ID_BYTES], int nranks, int rank,
                               lcpc_comm **out);
/* Caller-supplied collectives on DEVICE buffers of the current device.  The library drains the
 * work producing a buffer before the call and expects the data in place when it returns;
 * 0 = success.  all_gather: d_recv = the nranks ranks' `bytes`-byte buffers in rank order.
 * all_to_all_v: d_send holds send_bytes[k] bytes for rank k back to back, d_recv receives
 * recv_bytes[k] bytes from rank k back to back.  broadcast: root's d_buf to every rank. */
typedef struct lcpc_comm_ops {
  void *user;
  int (*all_gather)(void *user, const void *d_send, void *d_recv, size_t bytes);
  int (*all_to_all_v)(void *user, const void *d_send, const size_t *send_bytes, void *d_recv,
                      const size_t *recv_bytes);
  int (*broadcast)(void *user, void *d_buf, size_t bytes, int root);
} lcpc_comm_ops;
lcpc_status lcpc_comm_from_ops(const lcpc_comm_ops *ops, int nranks, int rank, lcpc_comm **out);
int lcpc_comm_nranks(const lcpc_comm *c);
int lcpc_comm_rank(const lcpc_comm *c);
int lcpc_comm_is_rccl(const lcpc_comm *c);
void lcpc_comm_free(lcpc_comm *c);

/* ------------------------------------------------------------------ row-sharded commitments
 * One Ligero or Brakedown commitment whose n_rows coefficient rows are split over the comm's ranks
 * (SURVEY.md §8e), reproducing commit (lcpc-2d/src/lib.rs:651-815) and prove (:1034-1123) bit
 * for bit.  Rank g encodes rows [row0_g, row0_g + n_g) -- cut on BLAKE3 chunk boundaries of the
 * leaf message -- and the chaining values of its chunks of every column; an all-to-all by column
 * block gives rank k the leaves and subtree of block k; an all-gather of the subtrees gives
 * every rank the whole Merkle tree (the bytes of lcpc_commit_copy_hashes).  prove runs the
 * Merlin transcript on one `root` rank: it broadcasts each challenge vector, gathers the ranks'
 * partial row combinations and folds them mod p (RCCL has no mod-p reduction), then gathers the
 * opened columns' row pieces.  Needs a power-of-two rank count of at most next_pow2(n_cols).
 * Rows are cut where a 1 KiB chunk starts on an element boundary (every chunk for 8/16/32-byte
 * elements, every third for Ft191).  Brakedown shards are element-major ([n_cols][rows], the
 * rows encoded independently, lcpc-brakedown-pc/src/encode.rs:36-94); the tree's leaves past
 * n_cols are zero digests, as in the single-GPU commit. */
/* the rows of rank `rank` */
lcpc_status lcpc_sharded_rows(lcpc_field f, size_t n_rows, int nranks, int rank, size_t *row0,
                              size_t *n_shard_rows);
typedef struct lcpc_sharded_commit lcpc_sharded_commit;
/* collective: d_rows = this rank's n_shard_rows zero-padded coefficient rows (n_per_row
 * elements each) in device memory; n_rows = the whole matrix's row count */
lcpc_status lcpc_sharded_commit_new_device(const lcpc_encoding *e, const void *d_rows, size_t n_rows,
                                           lcpc_comm *comm, lcpc_sharded_commit **out);
void lcpc_sharded_commit_free(lcpc_sharded_commit *c);
lcpc_status lcpc_sharded_commit_get_root(const lcpc_sharded_commit *c, uint8_t root[32]);
size_t lcpc_sharded_commit_n_hashes(const lcpc_sharded_commit *c);
lcpc_status lcpc_sharded_commit_copy_hashes(const lcpc_sharded_commit *c, uint8_t *out);
/* collective prove (:1034-1123): outer = the n_rows-element outer tensor (host, every rank);
 * on rank `root`, tr is the transcript and *out receives the proof; elsewhere tr is ignored
 * (may be NULL) and *out is set to NULL */
lcpc_status lcpc_sharded_prove(lcpc_sharded_commit *c, const uint64_t *outer, size_t outer_len,
                               const lcpc_encoding *e, lcpc_transcript *tr, int root,
                               lcpc_proof **out);
/* Collective proof-of-storage request on a row-sharded file commitment (networking/server.rs:
 * 652-737; the file's WriteableFt63 rows split over the ranks as above): on rank `root`,
 * eval_out (n_cols elements) = verifiable_polynomial_evaluation (proof-of-storage/src/
 * lcpc_online.rs:454-484), sum_r left[r] comm[r][j] over the ENCODED matrix -- the ranks'
 * partial sums over their rows gathered and folded mod p -- and cols_out / paths_out the n_open
 * requested columns (whole columns [k][n_rows], Montgomery, as lcpc_open_columns) with their
 * Merkle paths.  left (n_rows elements) and idx (n_open) are host inputs on every rank; outputs
 * are written on `root` only (NULL skips one).  Replaces lcpc_pos_eval_encoded +
 * lcpc_open_columns (lcpc_online.rs:454-484, 226-247) for one file committed over several GPUs. */
lcpc_status lcpc_sharded_pos_request(lcpc_sharded_commit *c, const uint64_t *left, size_t n_rows,
                                     const uint64_t *idx, size_t n_open, int root,
                                     uint64_t *eval_out, uint64_t *cols_out, uint8_t *paths_out);
/* Pipelined commit + prove of n_polys row-sharded polynomials (a proof-of-storage server's
 * objects, the bench's steps): polynomial i reads this rank's rows at d_rows[i] and is proved on
 * rank i % nranks, whose transcript is make_transcript(user, i, root_i) (the library frees it);
 * proofs[i] is set there and NULL elsewhere (proofs may be NULL: proofs are dropped), roots
 * (optional) gets every root on every rank.  Up to `depth` polynomials are in flight; the
 * exchanges of different polynomials go out in one fixed order on every rank (two RCCL groups per
 * pipeline tick: the stages with no host wait, then the tensor and column-index broadcasts that
 * wait on a transcript), `lag` ticks apart wherever the root rank absorbs a row combination into
 * its transcript (0: automatic). */
typedef lcpc_transcript *(*lcpc_make_transcript_fn)(void *user, size_t i, const uint8_t root[32]);
lcpc_status lcpc_sharded_commit_prove_many(const lcpc_encoding *e, const void *const *d_rows,
                                           size_t n_polys, size_t n_rows, const uint64_t *outer,
                                           lcpc_comm *comm, lcpc_make_transcript_fn make_transcript,
                                           void *user, size_t lag, lcpc_proof **proofs,
                                           uint8_t *roots);

/* Pre-populates this rank's device pool, page-locked staging and stream pool with what
 * lcpc_sharded_commit_prove_many(n_polys, lag) keeps in flight at once (every polynomial in
 * the pipeline holds its own rows, codeword, exchange and proof buffers), so the first call
 * at a new depth does not pay for hipMalloc / hipHostMalloc / stream creation inside it.  The
 * counterpart of lcpc_reserve for the sharded driver; no exchange. */
lcpc_status lcpc_sharded_reserve(const lcpc_encoding *e, size_t n_rows, lcpc_comm *comm,
                                 size_t n_polys, size_t lag);
/* Host-only (no device): the point-to-point transfers rank `rank` issues, in order, in every
 * exchange group of lcpc_sharded_commit_prove_many(n_polys, lag) -- the exact list run_group
 * hands RCCL as ncclSend / ncclRecv between ncclGroupStart / ncclGroupEnd.  Lets a single host
 * check that every rank's groups match (each send p -> q of n bytes meets a receive on q from p of
 * n bytes at the same position of the pair's sequence: no deadlock, right byte counts) for any
 * rank count without a GPU.  These exchanges replace nothing in the reference (its rows never
 * leave one host, lcpc-2d/src/lib.rs:677-682, 736-815); stage numbers: 0 chaining values,
 * 1 subtrees, 2 + 2r / 3 + 2r round r's tensor broadcast / partial gather, 2 + 2 rounds column
 * indices, 3 + 2 rounds opened columns (rounds = max(n_degree_tests, 1)).  A record's `tick` is
 * its exchange group: 2t + 0 / 2t + 1 for pipeline tick t's two groups.  *n_out = the record
 * count; LCPC_ERR_INVALID_ARG if it exceeds cap (out may be NULL with cap 0 to size). */
typedef struct lcpc_p2p_record {
  uint32_t tick, pos, poly, stage;
  int32_t is_send, peer;
  uint64_t bytes;
} lcpc_p2p_record;
lcpc_status lcpc_sharded_p2p_schedule(lcpc_field f, size_t n_rows, size_t n_per_row, size_t n_cols,
                                      size_t n_degree_tests, size_t n_col_opens, int nranks, int rank,
                                      size_t n_polys, size_t lag, lcpc_p2p_record *out, size_t cap,
                                      size_t *n_out);

/* ------------------------------------------------------------------ R-S erasure decoding, scrub, repair
 * NO COUNTERPART IN THE REFERENCE.  Its decode_row is a plain ifft_oi over the whole stored row
 * (lcpc_online.rs:568-574: one flipped byte corrupts the row's pre x 7 decoded bytes) and
 * FileHandler::verify_all_files_agree (file_handler.rs:505-541) can only say "trees differ".  A
 * stored file is Reed-Solomon encoded at rate <= 1/2 and column-major, so damage lands in few
 * columns, the `.portree` leaves say which, and a row of len evaluations of a polynomial of degree
 * < n_per_row is determined by any n_per_row of them: up to len - n_per_row damaged columns are
 * recomputed from the others.  With L(x) = prod_{j erased} (x - x_j): the surviving evaluations
 * times L(x_c) are those of P = f L (zero at the erased positions, which are never read), ifft_oi
 * gives P's coefficients -- all zero from index n_per_row + n_erased on, or the row is no codeword
 * -- and f(x_j) = P'(x_j) / L'(x_j) at the erased positions, one fft_io of the formal derivative.
 * Two transforms per row, as one decode plus one re-encode.  Existing entry points, file formats
 * and trees are unchanged. */
/* Host only (no device): the len evaluation points in codeword order, Montgomery limbs
 * (len x limbs u64): position c of an encoded row is f(out[c]), i.e. out = fft_io of the
 * polynomial x, under the switches of lcpc_fft_convention.h the library was built with.
 * LCPC_FFT_NOT_POWER_OF_TWO / LCPC_FFT_TOO_BIG for a bad length. */
lcpc_status lcpc_rs_domain_points(lcpc_field f, size_t len, uint64_t *out);
/* rows: n_rows x len elements (host, row-major, Montgomery, as lcpc_ifft_oi_rows), codewords of
 * messages of n_per_row coefficients whose positions erased[0..n_erased) are unknown (never read:
 * they may hold anything).  Fills those positions of every row in place with fully reduced
 * Montgomery values; every other limb keeps its bits.  LCPC_ERR_INVALID_ARG: an index >= len, a
 * duplicate index, n_per_row outside [1, len).  LCPC_ERR_UNRECOVERABLE: n_erased > len - n_per_row,
 * or some row's surviving positions are not those of a codeword (checked whenever n_erased <
 * len - n_per_row); no row is written then.  n_erased == 0 is that consistency check alone.  Rows
 * go through the device in batches of bounded size.  All five fields. */
lcpc_status lcpc_rs_erasure_decode_rows(lcpc_field f, uint64_t *rows, size_t n_rows, size_t len,
                                        size_t n_per_row, const uint64_t *erased, size_t n_erased);
/* The damage locator of a stored `.porenc` image (layout: lcpc_pos_encode_file): each column's
 * first rows_written elements hashed as lcpc_pos_porenc_tree does and compared on the device with
 * leaves (enc x 32 B, e.g. the head of the `.portree`).  status[c] = 0: the digest equals the leaf;
 * 1: it differs; 2: the column holds an element that is not < p (its digest is then written as
 * zeros).  Unlike lcpc_pos_porenc_tree a non-canonical element is a finding, not an error.  digests
 * (enc x 32 B) may be NULL; *n_bad (may be NULL) = the number of non-zero status bytes.  Rows past
 * rows_written are not looked at. */
lcpc_status lcpc_pos_scrub_porenc(const uint8_t *porenc, size_t enc, size_t rows_written,
                                  size_t row_capacity, const uint8_t *leaves, uint8_t *digests,
                                  uint8_t *status, size_t *n_bad);
/* Recomputes the columns bad_cols[0..n_bad) of the image from its other columns, which alone are
 * read.  The image is const: the caller decides what to write.  Any output may be NULL:
 *   cols_out     n_bad x rows_written x 8 B: column k = the canonical little-endian elements of
 *                column bad_cols[k], as they belong in the image;
 *   digests_out  n_bad x 32 B: their column digests (leaves), accumulated over the row batches as
 *                chunk chaining values like the writer's;
 *   data_out     rows_written x pre x 7 B: the decoded file (lcpc_pos_decode_porenc of the
 *                completed rows): the read-only recovery path for a download from a damaged replica.
 * Errors as lcpc_rs_erasure_decode_rows with len = enc, n_per_row = pre; LCPC_ERR_UNRECOVERABLE also
 * when a column that is not listed holds a non-canonical element.  The outputs are undefined after
 * an error. */
lcpc_status lcpc_pos_repair_columns(const uint8_t *porenc, size_t pre, size_t enc, size_t rows_written,
                                    size_t row_capacity, const uint64_t *bad_cols, size_t n_bad,
                                    uint8_t *cols_out, uint8_t *digests_out, uint8_t *data_out);

/* ------------------------------------------------------------------ R-S error location by syndromes
 * NO COUNTERPART IN THE REFERENCE.  Additive within LCPC_ABI_VERSION 3.  The erasure decoder above
 * must be told which positions are damaged; these entry points find them from the row alone.  With
 * the known erasures masked as above, the coefficients of P at index k' = n_per_row + n_erased and
 * above -- the ones the degree check tests for zero -- are the power sums S_i = sum_{c wrong}
 * a_c x_c^-i, i < N = len - k'.  Inversion-free Berlekamp-Massey finds their shortest recurrence;
 * its connection polynomial C(z) = prod (1 - z / x_c) has the evaluation points of the wrong
 * positions as its roots, so one forward transform of C's zero-padded coefficients has its zeros
 * exactly there.  Unique whenever 2 t <= N for t wrong positions.  The evaluation points are the
 * forward plan's table under lcpc_fft_convention.h, as for the erasure decoder. */
/* The largest number of wrong positions per row that can be located for field f (the
 * Berlekamp-Massey kernel keeps its polynomials in LDS); at least 256 for every field.  Host only. */
size_t lcpc_rs_locate_max_errors(lcpc_field f);

/* rows as lcpc_rs_erasure_decode_rows (host, row-major, Montgomery; erased positions never read).
 * row_status[r] = 0: the surviving positions are those of a codeword; 1: located; 2: not locatable
 * (more than (len - n_per_row - n_erased)/2 wrong positions, or more than the cap).
 * row_n_errors (n_rows, may be NULL), err_mask (n_rows x len bytes, may be NULL: 1 at the located
 * positions of status-1 rows), col_any (len bytes, may be NULL: OR over status-1 rows).
 * A status-2 row is a finding: the call returns LCPC_OK.  Argument errors as the erasure decoder;
 * n_erased > len - n_per_row: LCPC_ERR_UNRECOVERABLE.  n_erased == len - n_per_row leaves no
 * syndromes: every row is status 0.  Nothing in rows is written. */
lcpc_status lcpc_rs_locate_errors_rows(lcpc_field f, const uint64_t *rows, size_t n_rows, size_t len,
                                       size_t n_per_row, const uint64_t *erased, size_t n_erased,
                                       uint8_t *row_status, uint32_t *row_n_errors, uint8_t *err_mask,
                                       uint8_t *col_any);

/* Errors-and-erasures correction in place: the located and the erased positions of every row get
 * fully reduced Montgomery values, every other limb keeps its bits.  Any status-2 row:
 * LCPC_ERR_UNRECOVERABLE, no row written, row_status (may be NULL) still filled.  The values come
 * from the erasure decoder with the known and the located positions as the erasure set; consecutive
 * rows share one set while its size fits len - n_per_row. */
lcpc_status lcpc_rs_decode_rows(lcpc_field f, uint64_t *rows, size_t n_rows, size_t len,
                                size_t n_per_row, const uint64_t *erased, size_t n_erased,
                                uint8_t *row_status);

/* A `.porenc` image: col_status[c] = 0 nothing found, 1 a wrong element located in at least one row,
 * 2 holds an element that is not < p (treated as an erasure while the rest is located), 3 listed
 * in known_bad (never read).  *n_bad_cols = the number of non-zero status bytes, *n_dirty_rows = the
 * rows that are not codewords on the columns read, *n_unlocatable_rows those among them whose wrong
 * elements could not be located (their columns are NOT in col_status): > 0 is a finding (LCPC_OK).
 * Known plus non-canonical columns > enc - pre: LCPC_ERR_UNRECOVERABLE.  Row batches as
 * lcpc_pos_repair_columns (LCPC_POS_REPAIR_BATCH_ROWS).  The counters may be NULL. */
lcpc_status lcpc_pos_locate_porenc(const uint8_t *porenc, size_t pre, size_t enc, size_t rows_written,
                                   size_t row_capacity, const uint64_t *known_bad, size_t n_known,
                                   uint8_t *col_status, size_t *n_bad_cols, size_t *n_dirty_rows,
                                   size_t *n_unlocatable_rows);

/* ------------------------------------------------------------------ diagnostics
 * On-device check of the stream-ordered buffer pool the commit / prove / shard paths share
 * (no reference counterpart: its buffers are host Vecs).  Each round releases a 1 MiB block
 * while a writer that spins spin_us before storing still owns it, takes the same block on
 * another stream and overwrites it at once: *violations counts words the late writer clobbered
 * across the pool's fences (two fenced rounds per round: writer on the allocating stream, writer
 * on a second stream), *control_violations the same for one unfenced control round (expected
 * non-zero when the streams run concurrently), *reused the takes that returned the same block.
 * spin_us <= 100000. */
lcpc_status lcpc_selftest_pool_ordering(int rounds, uint32_t spin_us, uint64_t *violations,
                                        uint64_t *control_violations, uint64_t *reused);

/* LCPC_POOL_POISON=<0..255> (the environment, read once per process) fills every device block
 * of the pool over its whole rounded size, and every page-locked staging block, with that byte
 * before its owner sees it: a result must not depend on what a block held before.  This call
 * takes one pool block of `bytes` (> 0) as the library's own code does -- on a stream of the pool
 * when with_stream != 0, with none otherwise -- copies back its first and last byte and releases
 * it.  *enabled = 1 when the switch is set (both bytes are then the poison, for a fresh block and
 * for a recycled one), 0 when it is not (the bytes are whatever the block held: no claim). */
lcpc_status lcpc_selftest_pool_poison(size_t bytes, int with_stream, int *enabled, uint8_t *first,
                                      uint8_t *last);

/* The field primitives every kernel is built from (csrc/field.hpp) and the Ft127 matrix-core
 * digit recombination (csrc/collapse_mfma.hpp), one call per GPU thread: raw words in, raw words
 * out, NO range check on the values -- the caller owns the domain, which is the point: a test
 * can put p - 1, 2p - 1 or an all-ones limb pattern into both operands of one product.  An element
 * is the field's limbs as everywhere else; a, b and out are host pointers.  R = 2^(64 limbs). */
typedef enum lcpc_selftest_op {
  LCPC_SELFTEST_ADD = 0,           /* fe_add: a + b mod p                    (a, b < p) */
  LCPC_SELFTEST_SUB = 1,           /* fe_sub: a - b mod p                    (a, b < p) */
  LCPC_SELFTEST_ADD_2P = 2,        /* fe_add_2p: a + b, minus 2p if >= 2p    (a, b < 2p) */
  LCPC_SELFTEST_SUB_2P = 3,        /* fe_sub_2p: a - b, plus 2p if negative  (a, b < 2p) */
  LCPC_SELFTEST_REDUCE_2P = 4,     /* fe_reduce_2p: a mod p                  (a < 2p); b unused */
  LCPC_SELFTEST_SUB_LAZY = 5,      /* fe_sub_lazy: a - b + p mod R           (a, b < p) */
  LCPC_SELFTEST_MUL_SUB_LAZY = 6,  /* fe_mul(fe_sub_lazy(a[2i], a[2i+1]), b[i]): a holds 2n elements */
  LCPC_SELFTEST_MUL = 7,           /* fe_mul (product scanning): a b R^-1 mod p  (a < 2p, b < p) */
  LCPC_SELFTEST_MUL_CIOS = 8,      /* fe_mul_cios: the same                  (a, b < p) */
  LCPC_SELFTEST_SQR = 9,           /* fe_sqr: a a R^-1 mod p; b unused */
  LCPC_SELFTEST_MUL_LAZY = 10,     /* fe_mul_lazy: (a b + m p) / R, no final subtraction (a < 2p, b < p) */
  LCPC_SELFTEST_DOT = 11,          /* fe_dot<k>: sum_q a[ik+q] b[ik+q] R^-1 mod p: a, b hold n k elements */
  LCPC_SELFTEST_FROM_MONT = 12,    /* fe_from_mont (product scanning): a R^-1 mod p; b unused */
  LCPC_SELFTEST_FROM_MONT_GENERIC = 13, /* fe_from_mont_generic: (a + m p) / R for any a < R; b unused */
  LCPC_SELFTEST_TO_MONT = 14,      /* fe_to_mont: a R mod p; b unused */
  LCPC_SELFTEST_REPR_WORDS = 15,   /* fe_repr_words: to_repr of a Montgomery value as u32 words; b unused */
  LCPC_SELFTEST_CANON_REPR_WORDS = 16, /* fe_canon_repr_words: the same of a canonical value; b unused */
  LCPC_SELFTEST_IS_CANONICAL = 17, /* fe_is_canonical: out = 1 if a < p else 0 (any a < R); b unused */
  LCPC_SELFTEST_POW = 18,          /* fe_pow(a, e), e = the low 64 bits of b[i] */
  LCPC_SELFTEST_BALANCED_DIGITS = 19, /* Ft127 only: the 16 int8 digits of a < p, digit j in byte j; b unused */
  LCPC_SELFTEST_MUL_TW = 20,       /* Ft127 only: fe_mul_tw(a[i], W), W = the 2 limbs elements b[2 limbs i ..], the
                                      word-expanded constant of w (lcpc_selftest_twiddle_words): a w + m p
                                      over 2^64, in [0, 2p)               (a < 2p, every W_j < p) */
  LCPC_SELFTEST_N_OPS = 21
} lcpc_selftest_op;

/* The largest k of LCPC_SELFTEST_DOT for a field (fe_dot_kmax: k p < R); 0 for an unknown field. */
int lcpc_selftest_fe_dot_kmax(lcpc_field f);

/* out[i] = op(a[i], b[i]) for i < n.  k is fe_dot's number of products (1 for every other op).
 * LCPC_ERR_INVALID_ARG, before the device is touched: an unknown field or op, k < 1 or
 * k > lcpc_selftest_fe_dot_kmax(f), LCPC_SELFTEST_BALANCED_DIGITS or _MUL_TW on another field than Ft127,
 * a NULL a or out, a NULL b where the op reads b. */
lcpc_status lcpc_selftest_field_op(lcpc_field f, int op, int k, const uint64_t *a, const uint64_t *b,
                                   uint64_t *out, size_t n);

/* out[i] (an Ft127 element) = recombine_redc of the 16 digit-position accumulators y[16 i ..]:
 * (sum_u y_u 2^(8u)) R^-1 mod p, fully reduced, for |y_u| < 2^27.  NULL y or out:
 * LCPC_ERR_INVALID_ARG. */
lcpc_status lcpc_selftest_recombine(const int32_t *y, uint64_t *out, size_t n);

/* out[i] (an Ft63 element) = recombine_redc63 (csrc/pos_eval_mfma.hpp) of the 8 digit-position
 * accumulators y[8 i ..]: (sum_u y_u 2^(8u)) R^-1 mod p, fully reduced, for |y_u| <= 2^26.  NULL y or
 * out: LCPC_ERR_INVALID_ARG. */
lcpc_status lcpc_selftest_recombine63(const int32_t *y, uint64_t *out, size_t n);

/* The word-expanded table entries the Ft127 encode passes multiply by (csrc/field.hpp, fe_mul_tw):
 * for each of the n Montgomery values tw[i] = w R mod p (< p), out holds 2 limbs elements,
 * out[2 limbs i + j] = w 2^(32 (j + 2)) mod p, fully reduced, made by the kernel that fills a
 * plan's table.  LCPC_ERR_INVALID_ARG: another field than Ft127, a NULL tw or out. */
lcpc_status lcpc_selftest_twiddle_words(lcpc_field f, const uint64_t *tw, uint64_t *out, size_t n);

/* The row transform under every encode, commit and decode, called directly: n_rows rows of
 * 2^log_n points on a plan made for the call.  Row r reads the n_valid leading elements at
 * src + r src_stride (the rest of the row counts as zero) and writes 2^log_n elements at
 * dst + r dst_stride, fffft::fft_io's output (Montgomery words; canonical words with canon = 1).
 * inverse = 1 takes the inverse plan's root, omega^-1 -- the inner transform of ifft_oi, without
 * its reordering and its 2^-log_n.  copy (optional, may be NULL): row r's n_valid inputs are also
 * written to copy + r copy_stride, as the commit paths keep their coefficient matrix.  Strides are
 * in elements; src, dst and copy are host buffers of n_rows whole strides.  All three are uploaded
 * whole before the transform, and dst and copy downloaded whole after it, so every element the
 * kernels do not write -- the gap after each row, copy beyond n_valid -- returns as the caller set
 * it, and whatever src holds beyond n_valid is on the device for the kernels to (not) read.
 * n_valid <= 2^(log_n - 1) runs the
 * half-zero variant of the first pass, as rate-1/2 rows do.
 * LCPC_ERR_INVALID_ARG, before the device is touched: an unknown field, a NULL src or dst,
 * log_n < 0, canon together with inverse, n_valid > 2^log_n, src_stride or copy_stride < n_valid,
 * dst_stride < 2^log_n.  LCPC_ERR_UNSUPPORTED, before the device is touched and before the
 * lengths are looked at: log_n above the field's range (24 for Ft63 and Ft127, 22 for Ft191,
 * Ft255 and Ft253_192). */
lcpc_status lcpc_selftest_ntt_rows(lcpc_field f, int log_n, int inverse, const uint64_t *src,
                                   size_t src_stride, size_t n_valid, uint64_t *dst, size_t dst_stride,
                                   size_t n_rows, uint64_t *copy, size_t copy_stride, int canon);

/* One sparse level of the Brakedown encode, y = M x, on a matrix of the caller's: for every output
 * j < m_rows and every row b in [b0, b0 + nb), y[j][b] = sum_k val[k] x[idx[k]][b] R^-1 mod p over
 * k in [ptr[j], ptr[j + 1]) (Montgomery products, as the encode computes them).  The matrix is CSR
 * by output: ptr has m_rows + 1 entries, every idx is below m_cols, val holds the field's limbs per
 * nonzero -- raw words with NO range check, as lcpc_selftest_field_op: the caller owns the domain.
 * x = [m_cols][R] and y = [m_rows][R] are element-major (element j of row b at j R + b), host
 * buffers.  The matrix goes to the device by the upload every encoding's levels take, the Ft127
 * matrix-core form (nonzeros padded to groups of 4) included, and the launch is the encode's own
 * dispatch.  y is uploaded whole before it and downloaded whole after it: rows outside
 * [b0, b0 + nb) return as the caller set them.
 * path 0: the kernel an encoding would run -- the int8 matrix cores for Ft127 unless LCPC_NO_MFMA
 * is set or some output has more than 512 nonzeros (then the VALU kernel for the whole matrix),
 * the VALU kernel for every other field.  path 1: the VALU kernel.  *used_mfma = 1 if the
 * matrix-core kernel ran, else 0.
 * LCPC_ERR_INVALID_ARG, before the device is touched: an unknown field, a NULL pointer, a path
 * other than 0 or 1, R or m_rows above 2^32 - 1, b0 + nb > R, ptr[0] != 0, a ptr that decreases,
 * an idx >= m_cols.  nb = 0 or m_rows = 0: LCPC_OK, nothing written (*used_mfma = 0). */
lcpc_status lcpc_selftest_spmm(lcpc_field f, size_t m_rows, size_t m_cols, const uint32_t *ptr,
                               const uint32_t *idx, const uint64_t *val, const uint64_t *x, uint64_t *y,
                               size_t R, size_t b0, size_t nb, int path, int *used_mfma);

/* The Reed-Solomon step at the bottom of the Brakedown recursion (encode::reed_solomon), launched
 * as the encode launches it: out[k][b] = sum_(j < m) in[j][b] (k + 1)^j mod p for k < n_out and
 * the rows b in [b0, b0 + nb).  in = [m][R] and out = [n_out][R], element-major host buffers of
 * Montgomery words (in < p; no range check).  out is uploaded whole first: rows outside the range
 * return as the caller set them.  m = 0 writes zeros.
 * LCPC_ERR_INVALID_ARG, before the device is touched: an unknown field, a NULL in or out, R, m or
 * n_out above 2^32 - 1, b0 + nb > R.  nb = 0 or n_out = 0: LCPC_OK, nothing written. */
lcpc_status lcpc_selftest_reed_solomon(lcpc_field f, const uint64_t *in, size_t m, uint64_t *out,
                                       size_t n_out, size_t R, size_t b0, size_t nb);

/* ------------------------------------------------------------------ kernel timing
 * HIP-event timing of every kernel launch on the handle streams (off by default). */
void lcpc_prof_enable(int enable);
void lcpc_prof_reset(void);
/* accumulated milliseconds and launch count for a kernel name (0 if never launched) */
int lcpc_prof_get(const char *name, double *total_ms, uint64_t *count);
/* newline-separated kernel names seen so far; returns the full length */
size_t lcpc_prof_names(char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LCPC_MI_H */
