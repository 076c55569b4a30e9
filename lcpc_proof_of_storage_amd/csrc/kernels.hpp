// kernels.hpp -- host-side launchers of the gfx950 kernels (internal to liblcpc_mi.so).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/lcpc_fft_convention.h"

namespace lcpc {

// LCPC_POOL_POISON=<0..255> (read once per process; -1 when unset or out of range): every device
// block and staging block the library hands to itself is filled with that byte first, so a word
// that a kernel or a memset was meant to write and did not shows in the results whatever the
// block held before (tests/test_gpu_pool_poison.py).  Off by default: one flag test per block.
inline int pool_poison() {
  static const int v = [] {
    const char *e = std::getenv("LCPC_POOL_POISON");
    if (!e || !*e) return -1;
    char *end = nullptr;
    const long x = std::strtol(e, &end, 10);
    return (*end || x < 0 || x > 255) ? -1 : (int)x;
  }();
  return v;
}
// The fill itself.  On stream s when given; without one the fill has completed on return
// (hipMemset on device memory may return before it has run, so the null stream is drained).
inline hipError_t pool_poison_fill(void *p, size_t bytes, hipStream_t s) {
  const int v = pool_poison();
  if (v < 0 || !p || !bytes) return hipSuccess;
  if (s) return hipMemsetAsync(p, v, bytes, s);
  const hipError_t e = hipMemsetAsync(p, v, bytes, nullptr);
  return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
}
// hipMalloc for the blocks that do not come from a Device's pool (plan tables, the sharded
// engine's temporaries): the same fill, completed on return.
inline hipError_t device_malloc(void **p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  return e == hipSuccess ? pool_poison_fill(*p, bytes, nullptr) : e;
}
template <class T>
inline hipError_t device_malloc(T **p, size_t bytes) {
  return device_malloc(reinterpret_cast<void **>(p), bytes);
}

// Bytes per element of field `fid` (8, 16, 24, 32) and 32-bit words per element.
int field_words(int fid);
inline int field_bytes(int fid) { return 4 * field_words(fid); }
bool field_gpu_supported(int fid);

// ------------------------------------------------------------------ NTT (Ligero encode)
// fffft::fft_io semantics on rows of length n = 2^log_n: out[bitrev(j)] = sum_i in[i] w^(ij),
// w = ROOT_OF_UNITY^(2^(S - log_n)).  Two passes (four-step):
//   pass A: 2^l1-point DIF down each of the 2^l2 columns of the row viewed as [2^l1][2^l2],
//           input zero-padded past n_valid, then the inter-pass twiddle w^(c * bitrev(t'));
//   pass B: 2^l2-point DIF along each contiguous block.
// LCPC_NO_MFMA=1: VALU kernels instead of the int8 matrix-core ones (A/B runs; identical results)
bool no_mfma();

struct NttPlan {
  int fid = -1;
  int log_n = 0, l1 = 0, l2 = 0;
  // an ifft_oi plan (its rows are the inner DIF of the inverse: never reordered by ntt_rows)
  bool inverse = false;
  uint32_t *d_tw = nullptr;        // w^e, e in [0, n): n elements (Montgomery)
  uint32_t *d_tw_canon = nullptr;  // forward plans: the same values' canonical words (below)
  // pass A's inter-pass twiddles w^(c * bitrev_l1(t)) laid out [t][c] (t < 2^l1, c < 2^l2): the
  // lanes of a pass-A store are adjacent columns c, so their twiddle loads are contiguous (from
  // the flat table they were c * bitrev(t) apart, one cache line per lane); log_n > 12 only
  uint32_t *d_tw2 = nullptr;
  uint32_t *d_tw2_canon = nullptr;  // forward plans: canonical words
  // Ft127, log_n > 12 (LCPC_NTT_TW4, ntt_v2.hpp): the word-expanded sub-FFT twiddles of the passes
  // that multiply by them (field.hpp, fe_mul_tw), N elements per entry, entry e = W(w^(e << l2)),
  // e < 2^(l1-1) (pass A's 2^l1-point DIF), then at ntt_tw4_b() entry e = W(w^(e << l1)),
  // e < 2^(l2-1) (pass B's).  Only what a block stages in LDS is kept, so the table is 64
  // (2^(l1-1) + 2^(l2-1)) bytes whatever the row length.  A pass longer than 2^NTT_TW4_MAX_L points
  // keeps the one-element twiddles (its part is empty).  Inverse plans get the table too: they
  // run the same kernels.
  uint32_t *d_tw4 = nullptr;
  // which kernel encodes the PoS-dims rows (2^15-point Ft63, rate 1/2): LCPC_ROW_KERNEL_AUTO (the
  // measured choice: the one-pass kernel for file images, the four-step pair for element rows),
  // _FOURSTEP or _ONEPASS (lcpc_encoding_set_row_kernel)
  int row_kernel = 0;
  // the persistent passes' grid (ntt_v2.hpp, LCPC_NTT_PERSIST): the blocks the device holds at
  // once, blocks per CU at the kernels' LDS / VGPR footprint times the CU count, taken once at
  // plan init; 0 where the plan's passes have no persistent form (they launch one workgroup per
  // tile).  LCPC_NTT_PERSIST_GRID=<n> in the environment at plan init gives the grid instead
  // (persist_grid_forced: taken as it stands, not rounded to the column groups); any grid is
  // correct, the tests walk small ones.
  size_t persist_grid = 0;
  bool persist_grid_forced = false;
  // whether a whole commitment's encode may end in the pass B that also hashes the column leaves
  // (ntt_rows_leaf_cvs): forward Ft127 plans whose pass B has the fused kernel's length, in a build
  // that has the kernel (LCPC_NTT_LEAF_FUSE, ntt_v2.hpp); LCPC_NTT_LEAF_FUSE=0 in the environment
  // at plan init clears it for that plan
  bool leaf_fuse = false;
};
// the longest sub-FFT whose block stages word-expanded twiddles: 2^(L-1) entries of 64 bytes beside
// the tile (16 KiB at L = 9; at L = 12 the table alone would be 128 KiB of a CU's 160)
constexpr int NTT_TW4_MAX_L = 9;
inline size_t ntt_tw4_entries(int l) { return l <= NTT_TW4_MAX_L ? (size_t)1 << (l - 1) : 0; }
inline const uint32_t *ntt_tw4_b(const NttPlan &p) {  // pass B's part of d_tw4 (Ft127: 16 words per entry)
  return p.d_tw4 + ntt_tw4_entries(p.l1) * 16;
}
// out[e][i] = the word-expanded constant's element i of the Montgomery value tw[e * stride],
// e < count (Ft127 only; hipErrorInvalidValue otherwise)
hipError_t ntt_tw4_table(int fid, const uint32_t *tw, size_t stride, size_t count, uint32_t *out, hipStream_t s);
// the [t][c] table above for a pass-A split l1 from a flat table tw (n = 2^log_n elements)
hipError_t ntt_tw2_table(int fid, const uint32_t *tw, int log_n, int l1, uint32_t *out, hipStream_t s);
// the longest row a plan can be made for is 2^ntt_max_log_n(fid); beyond it ntt_plan_init returns
// hipErrorInvalidValue before it allocates anything
int ntt_max_log_n(int fid);
hipError_t ntt_plan_init(NttPlan &p, int fid, int log_n, bool inverse, hipStream_t s);
void ntt_plan_free(NttPlan &p);
// rows r in [0, n_rows): in = src + r * src_stride (elements), n_valid leading elements
// (rest zero); out = dst + r * dst_stride (n elements).  src may alias dst only if
// src_stride == dst_stride and n_valid == n (in-place full-length transform).
// copy (optional): the n_valid input coefficients of row r are also written to
// copy + r * copy_stride by the first pass, which reads them anyway (commit keeps its own
// coefficient matrix without a separate device-to-device copy).
// canon_out: the outputs are written in canonical form instead of Montgomery form.  The
// transform is linear, so pass A multiplies by w^e R^-1 -- whose Montgomery words are the
// canonical words of w^e (d_tw_canon) -- at no extra cost, and every output's Montgomery words
// become its canonical value: commitments hash their codeword without a per-element
// conversion (the Merkle leaves are over canonical bytes).
// Forward plans follow include/lcpc_fft_convention.h: with LCPC_FFT_OUTPUT_BITREV = 0 the rows are
// reordered to natural order after the transform (bitrev_rows_inplace).
hipError_t ntt_rows(const NttPlan &p, const uint32_t *src, size_t src_stride, size_t n_valid,
                    uint32_t *dst, size_t dst_stride, size_t n_rows, hipStream_t s,
                    uint32_t *copy = nullptr, size_t copy_stride = 0, bool canon_out = false);
// ntt_rows with canon_out for ALL n_rows rows of a row-major commitment at once, whose second pass
// also leaves the BLAKE3 chunk chaining values of the column leaves (leaf_hashes' messages over
// the canonical codeword) in cvs[chunk][col], leaf_n_chunks(fid, n_rows) x 2^log_n values of 8
// words, the layout leaf_chunk_cvs writes with blk = 0: leaves_from_cvs turns them into the leaves
// (a one-chunk message's value is already the leaf), and no kernel reads the codeword back.
// Only where ntt_rows_leaf_ok says so (the plan's leaf_fuse, canonical output, rows n_cols apart);
// hipErrorInvalidValue otherwise.
bool ntt_rows_leaf_ok(const NttPlan &p, size_t dst_stride, bool canon_out);
hipError_t ntt_rows_leaf_cvs(const NttPlan &p, const uint32_t *src, size_t src_stride, size_t n_valid,
                             uint32_t *dst, size_t dst_stride, size_t n_rows, hipStream_t s, uint32_t *copy,
                             size_t copy_stride, uint32_t *cvs);
// m[r][j] <-> m[r][bitrev_log_n(j)] in place, rows r < n_rows of stride `stride` elements
hipError_t bitrev_rows_inplace(int fid, uint32_t *m, size_t stride, int log_n, size_t n_rows, hipStream_t s);
// The proof-of-storage file image encoded straight into a commitment (ntt_row1.hpp BYTES): row r
// = WriteableFt63 elements [n_per_row r, n_per_row (r + 1)) of the n_bytes-byte image, 7 bytes per
// element (zero padded); canonical output, the coefficient matrix written to copy.  Only at the
// one-pass kernel's shape (ntt_rows_pos_bytes_ok), 16-byte-aligned bytes.
bool ntt_rows_pos_bytes_ok(const NttPlan &p, size_t n_per_row);
bool ntt_row1_bytes(const NttPlan &p);  // whether the file-image commit takes the one-pass kernel (p.row_kernel)
hipError_t ntt_rows_pos_bytes(const NttPlan &p, const uint8_t *bytes, size_t n_bytes, uint32_t *dst,
                              size_t dst_stride, size_t n_rows, hipStream_t s, uint32_t *copy, size_t copy_stride);

// ------------------------------------------------------------------ BLAKE3 / Merkle
// leaf[j] = BLAKE3(32 zero bytes || repr(m[0][j]) || ... || repr(m[n_rows-1][j]))
// for j in [0, n_cols); m is row-major with row stride `stride` elements.
// canon: the matrix holds canonical values (ntt_rows canon_out) instead of Montgomery form.
size_t leaf_hash_scratch_bytes(int fid, size_t n_rows, size_t n_cols);
hipError_t leaf_hashes(int fid, const uint32_t *m, size_t n_rows, size_t n_cols, size_t stride,
                       uint8_t *leaves, void *scratch, hipStream_t s, bool canon = false);
// Row shards: chaining values of chunks [chunk_lo, chunk_hi) of every column's leaf message
// (messages of n_rows rows in total) from a row-major shard m holding rows [row0, ...);
// cvs[(chunk - chunk_lo) * n_cols + col] (8 words), or with blk > 0 the exchange layout
// cvs[((col / blk) * (chunk_hi - chunk_lo) + chunk - chunk_lo) * blk + col % blk].  Chunk c starts
// at message byte 1024 c.  col_stride: elements between columns (1: row-major m; the shard's row
// count with stride 1: an element-major [n_cols][rows] shard).
size_t leaf_n_chunks(int fid, size_t n_rows);
hipError_t leaf_chunk_cvs(int fid, const uint32_t *m, size_t row0, size_t n_rows, size_t n_cols,
                          size_t stride, size_t chunk_lo, size_t chunk_hi, uint32_t *cvs,
                          hipStream_t s, bool canon = false, size_t blk = 0, size_t col_stride = 1);
// leaf digests from all n_chunks chaining values ([chunk][col] layout; cvs is clobbered)
hipError_t leaves_from_cvs(uint32_t *cvs, size_t n_cols, int n_chunks, uint8_t *leaves,
                           hipStream_t s);
// the same leaves, bit for bit, with cvs left untouched (a chunk-CV cache that outlives the fold):
// one thread per column and one launch, a register stack of subtree roots (n_chunks <= 2^20)
hipError_t leaves_fold_cvs(const uint32_t *cvs, size_t n_cols, size_t n_chunks, uint8_t *leaves,
                           hipStream_t s);
// Chunk-CV cache of column-major canonical files: chaining values of chunks [chunk_lo, chunk_hi) of
// n_cols column messages (n_rows rows in total) from slices [col][col_elems] of little-endian
// canonical elements that hold only those chunks' rows (from lcpc_leaf_chunk_first_row(chunk_lo)
// on; the message's last chunk may be short).  col_elems: elements between columns, at least the
// slice's rows, with col_elems * N a multiple of 4 words.  The value of (chunk, col) is written to
// cvs[((chunk - cv_chunk0) * cv_stride + col) * 8]: cvs is a [chunk][cv_stride columns] array whose
// first chunk row is chunk cv_chunk0 <= chunk_lo (0: the cache itself), offset to the first of
// these columns; a one-chunk message's value carries ROOT; *bad |= 1 if an element is not < p.
// Fields whose element tiles a block.
hipError_t leaf_chunk_cvs_slices(int fid, const uint32_t *slices, size_t col_elems, size_t n_rows,
                                 size_t n_cols, size_t chunk_lo, size_t chunk_hi, uint32_t *cvs,
                                 size_t cv_chunk0, size_t cv_stride, uint32_t *bad, hipStream_t s);
// leaf_hashes of a canonical row-major codeword that also writes each (chunk, column)'s share of
// u^T Enc(M): partials[chunk][col] = sum over the chunk's rows r of left[r] * m[r][col]
// (Montgomery left, canonical results; leaf_n_chunks(fid, n_rows) x n_cols elements).  Fields
// whose element tiles a BLAKE3 block only (leaf_eval_fusable).
bool leaf_eval_fusable(int fid);
hipError_t leaf_hashes_eval(int fid, const uint32_t *m, size_t n_rows, size_t n_cols, size_t stride,
                            uint8_t *leaves, void *scratch, const uint32_t *left, uint32_t *partials,
                            hipStream_t s);
// same, for a [column][row] matrix (opened columns of a proof)
hipError_t leaf_hashes_cols(int fid, const uint32_t *cols, size_t n_rows, size_t n_cols,
                            uint8_t *leaves, void *scratch, hipStream_t s, bool canon = false);
// hashes = [leaves (np2) | level 1 (np2/2) | ... | root]; fills every level above the leaves
hipError_t merkle_tree(uint8_t *hashes, size_t np2, hipStream_t s);
// generic Merkle over ins (n_ins = outs + 1 nodes, power of two) -> outs
hipError_t merkle_tree_io(const uint8_t *ins, size_t n_ins, uint8_t *outs, hipStream_t s);
// row shards: G subtrees of 2B - 1 digests (column block g, levels leaves..root, B a power of
// two) into levels 0..log2(B) of the whole tree of G B leaves ([leaves | level 1 | ...] layout)
hipError_t assemble_subtrees(const uint8_t *subs, size_t B, size_t G, uint8_t *tree, hipStream_t s);

// ------------------------------------------------------------------ checkable reads (pos_read.hip)
// A column opened on the chunk range [chunk_lo, chunk_hi) of its n_chunks-chunk leaf message: the
// leaf is rebuilt from the chunk CVs of the range and the CVs of the subtrees that cover the rest.
// Which nodes those are depends only on (n_chunks, chunk_lo, chunk_hi), so the host flattens
// BLAKE3's left-balanced tree, pruned at the covers and at the nodes inside the range, into a
// post-order program that every column runs on a register stack of chaining values:
//   COVER  push covers[col][a]
//   CHUNKS push the subtree over the range's chunk CVs [a, a + b) (indices from chunk_lo)
//   GROUPS the same over b group nodes from group a of group_cvs (groups of READ_GROUP chunks,
//          aligned, are whole subtrees: the argument of blake3.hip's k_leaf_merge_groups)
//   MERGE  pop right and left, push their parent
// root: the last parent this op makes carries ROOT (the program's last op only).
constexpr int READ_GROUP = 8;
enum : uint32_t { READ_OP_COVER = 0, READ_OP_CHUNKS = 1, READ_OP_GROUPS = 2, READ_OP_MERGE = 3 };
struct ReadOp {
  uint32_t kind, root;
  uint64_t a, b;
};
// covers[(k * n_cover + j) * 32] = the CV of the subtree over chunks [nodes[2 j], nodes[2 j + 1]) of
// column idx[k] (k with idx null) of cvs, a [chunk][cv_stride columns] array of chunk CVs that is
// only read.  One thread per (column, node); never ROOT (a cover is never the whole tree).
// n_chunks <= 2^20.
hipError_t read_cover_values(const uint32_t *cvs, size_t cv_stride, size_t n_chunks, const uint64_t *idx,
                             size_t n_idx, const uint64_t *nodes, size_t n_cover, uint8_t *covers, hipStream_t s);
// leaf_chunk_cvs_slices for n_idx segments (rows from row0 = the first row of chunk_lo on) that also
// sums partials[(chunk - chunk_lo) * n_idx + k] = sum of weights[r - row0] * element r over the
// chunk's rows (Montgomery weights, canonical sums) and flags the columns, bad_cols[k] = 1, that hold
// an element not < p.  cvs[(chunk - chunk_lo) * n_idx + k].
hipError_t read_segment_chunks(int fid, const uint32_t *segs, size_t col_elems, size_t n_rows, size_t n_idx,
                               size_t chunk_lo, size_t chunk_hi, uint32_t *cvs, const uint32_t *weights,
                               uint32_t *partials, uint32_t *bad_cols, hipStream_t s);
// group_cvs[g * n_idx + k] = the node over chunks [first + 8 g, min(first + 8 g + 8, chunk_end)) of
// seg_cvs (whose chunk row 0 is chunk chunk_lo), g < n_groups: one thread per (column, group)
hipError_t read_segment_groups(const uint32_t *seg_cvs, size_t n_idx, size_t chunk_lo, size_t first,
                               size_t chunk_end, size_t n_groups, uint32_t *group_cvs, hipStream_t s);
// leaves[k] = the program's result for column k; n_chunks (<= 2^20) sizes the stack
hipError_t read_segment_leaves(const uint32_t *seg_cvs, const uint32_t *group_cvs, const uint8_t *covers,
                               size_t n_idx, size_t n_cover, size_t n_chunks, const ReadOp *ops, size_t n_ops,
                               uint8_t *leaves, hipStream_t s);

// ------------------------------------------------------------------ other digests (digest.hip)
// The commitment's digest D (lcpc_digest): BLAKE3 goes to the functions above, SHA-256 and the
// Keccak-f[1600] sponge (SHA3-256, Keccak-256: one kernel, the padding byte a parameter) to
// digest.hip's one-lane-per-column kernels.  Same arguments and layouts as the BLAKE3 functions;
// scratch is used by BLAKE3 only (leaf_hash_scratch_bytes).  gather_paths, gather_columns and
// assemble_subtrees are digest-agnostic.
enum { DIGEST_BLAKE3 = 0, DIGEST_SHA256 = 1, DIGEST_SHA3_256 = 2, DIGEST_KECCAK256 = 3 };
bool digest_valid(int digest);
hipError_t leaf_hashes_d(int digest, int fid, const uint32_t *m, size_t n_rows, size_t n_cols, size_t stride,
                         uint8_t *leaves, void *scratch, hipStream_t s, bool canon = false);
hipError_t leaf_hashes_cols_d(int digest, int fid, const uint32_t *cols, size_t n_rows, size_t n_cols,
                              uint8_t *leaves, void *scratch, hipStream_t s, bool canon = false);
hipError_t merkle_tree_d(int digest, uint8_t *hashes, size_t np2, hipStream_t s);
hipError_t path_checks_d(int digest, const uint8_t *leaves, const uint8_t *paths, size_t n, size_t path_len,
                         const uint64_t *idx, const uint8_t *root, uint32_t *flags, hipStream_t s);

// ------------------------------------------------------------------ prover helpers
// out[t][c] = sum_r tensors[t][r] * coeffs[r][c]   (t < n_tensors, c < n_per_row)
size_t collapse_scratch_bytes(int fid, size_t n_rows, size_t n_per_row, int n_tensors);
hipError_t collapse_rows(int fid, const uint32_t *coeffs, size_t n_rows, size_t n_per_row,
                         const uint32_t *tensors, int n_tensors, uint32_t *out, void *scratch,
                         hipStream_t s);
// The same for any 1 <= n_tensors <= COLLAPSE_MANY_MAX_TENSORS (batched evaluation proofs): the
// tensors go through the VALU kernel in chunks of collapse_many_chunk(fid) accumulators per thread,
// one read of the coefficient matrix per chunk; Ft127 from 5 tensors on takes the int8 matrix-core
// kernel in chunks of 8 (LCPC_NO_MFMA=1: the VALU kernel).  Results are bit-identical to collapse_rows.
constexpr size_t COLLAPSE_MANY_MAX_TENSORS = 4096;
int collapse_many_chunk(int fid);
size_t collapse_many_scratch_bytes(int fid, size_t n_rows, size_t n_per_row, size_t n_tensors);
hipError_t collapse_rows_many(int fid, const uint32_t *coeffs, size_t n_rows, size_t n_per_row,
                              const uint32_t *tensors, size_t n_tensors, uint32_t *out, void *scratch,
                              hipStream_t s);
// out[c] = sum_k vecs[k][c] (n_vecs vectors of len elements)
hipError_t collapse_fold_rows(int fid, const uint32_t *vecs, size_t n_vecs, size_t len, uint32_t *out,
                              hipStream_t s);
// cols[k][r] = m[r][idx[k]] (m row-major) or m[idx[k]][r] (col_major); canon: m holds
// canonical values and the gathered columns are converted to Montgomery form;
// paths[k][i] = sibling digests of leaf idx[k]
hipError_t gather_columns(int fid, const uint32_t *m, size_t n_rows, size_t n_cols,
                          const uint64_t *idx, size_t n_idx, uint32_t *cols, hipStream_t s,
                          bool col_major = false, bool canon = false);
hipError_t gather_paths(const uint8_t *hashes, size_t n_hashes, const uint64_t *idx,
                        size_t n_idx, size_t path_len, uint8_t *paths, hipStream_t s);

// ------------------------------------------------------------------ verifier helpers
// dots[k][t] = sum_r tensors[t][r] * cols[k][r]; ok[k] bit t set iff dots == enc[t][idx[k]]
hipError_t column_checks(int fid, const uint32_t *cols, size_t n_cols_open, size_t n_rows,
                         const uint32_t *tensors, int n_tensors, const uint32_t *encs,
                         size_t enc_len, const uint64_t *idx, uint32_t *flags, hipStream_t s);
// path[k] check against root: flags[k] = 1 iff the Merkle path of leaf k verifies
hipError_t path_checks(const uint8_t *leaves, const uint8_t *paths, size_t n, size_t path_len,
                       const uint64_t *idx, const uint8_t *root, uint32_t *flags,
                       hipStream_t s);
// out = sum_i a[i] * b[i]
hipError_t dot(int fid, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out,
               void *scratch, hipStream_t s);
// out[j] = sum_i a[j][i] * b[j][i] for j < n_vecs (vectors of n elements): one workgroup per j
hipError_t dot_many(int fid, const uint32_t *a, const uint32_t *b, size_t n, size_t n_vecs, uint32_t *out,
                    hipStream_t s);
// elementwise Montgomery <-> canonical conversion (device); with bad non-null, canonical
// inputs that are not < p set *bad = 1
hipError_t convert(int fid, const uint32_t *in, uint32_t *out, size_t n, bool to_mont,
                   hipStream_t s, uint32_t *bad = nullptr);
// bytes (a multiple of 8, 8-byte aligned pointers) copied by a kernel on stream s; either side
// may be device-mapped page-locked host memory (over_link: then a capped grid)
hipError_t copy_words(void *dst, const void *src, size_t bytes, hipStream_t s, bool over_link = true);
// chunk-local self-test entry: out = a * b elementwise (Montgomery)
hipError_t mul_elementwise(int fid, const uint32_t *a, const uint32_t *b, uint32_t *out,
                           size_t n, hipStream_t s);

// ------------------------------------------------------------------ R-S erasure decoding (erasure.hip)
// Rows of n = 2^log_n evaluations with the positions erased[0..n_erased) missing.  tw is a FORWARD
// plan's d_tw (the evaluation points follow include/lcpc_fft_convention.h).  The caller has checked
// the indices (each < n, no duplicates).
// slot[c] = j if c == erased[j], else -1; lambda[c] = prod_{j} (x_c - x_erased[j]) for c not erased
// (0 at the erased c); dinv[j] = 1 / prod_{i != j} (x_erased[j] - x_erased[i]).  Montgomery.
hipError_t erasure_locator(int fid, const uint32_t *tw, int log_n, const uint32_t *erased, size_t n_erased,
                           int32_t *slot, uint32_t *lambda, uint32_t *dinv, hipStream_t s);
// dscale[k] = (k + 1) / n for k < n (Montgomery) from the canonical words of n^-1
hipError_t erasure_dscale(int fid, int log_n, const uint32_t *inv_n_canon_words, uint32_t *dscale, hipStream_t s);
// out[r][.] = in[r][c] * lambda[c] (0 at the erased c, which are not read), laid out as the natural-
// order input of the inverse plan's ntt_rows (the opening reorder of ifft_oi folded in)
hipError_t erasure_masked_rows(int fid, const uint32_t *in, uint32_t *out, int log_n, size_t n_rows,
                               const int32_t *slot, const uint32_t *lambda, hipStream_t s);
// the same from a column-major batch src[c][r] (r < B) of canonical elements (a `.porenc` slice; Ft63
// only): transposed, converted to Montgomery form, masked.  plain (optional): the unmasked Montgomery
// rows plain[r][c] at the columns that are not erased.  *bad = 1 if a column that is read holds an
// element that is not < p; erased columns are never read.
hipError_t erasure_masked_cols(int fid, const uint32_t *src, size_t B, int log_n, uint32_t *out, uint32_t *plain,
                               const int32_t *slot, const uint32_t *lambda, uint32_t *bad, hipStream_t s);
// h = the inverse plan's output of the masked rows (bit-reversed, unscaled coefficients of P):
// out[r][k] = (k + 1) p_{k+1} / n, natural order, ready for the forward plan; *flag = 1 if a
// coefficient p_k, k >= deg_bound (>= 1), is not zero
hipError_t erasure_deriv(int fid, const uint32_t *h, uint32_t *out, int log_n, size_t n_rows, const uint32_t *dscale,
                         size_t deg_bound, uint32_t *flag, hipStream_t s);
// e = the forward plan's output of erasure_deriv's rows: v(r, j) = e[r][erased[j]] * dinv[j] to
// vals[r][j] and (optional) cm[j][r], canonical words if canon, else Montgomery; rows (optional):
// rows[r][erased[j]] = v in Montgomery form (completes erasure_masked_cols' plain rows)
hipError_t erasure_fill(int fid, const uint32_t *e, int log_n, size_t n_rows, const uint32_t *erased, size_t n_erased,
                        const uint32_t *dinv, uint32_t *vals, uint32_t *cm, uint32_t *rows, bool canon,
                        hipStream_t s);
// col_bad[c] = 1 (never cleared here) if column c of cols[c][r], r < n_rows, canonical words, holds
// an element that is not < p
hipError_t scrub_col_canon(int fid, const uint32_t *cols, size_t n_rows, size_t n_cols, uint32_t *col_bad,
                           hipStream_t s);
// status[c] = 2 if col_bad[c] (digest c is then zeroed), else 0 / 1: digest c equals / differs from leaf c
hipError_t scrub_status(uint8_t *digests, const uint8_t *leaves, const uint32_t *col_bad, size_t n_cols,
                        uint8_t *status, hipStream_t s);

// ------------------------------------------------------------------ R-S error location (rs_locate.hip)
// h = the inverse plan's output of masked rows (as erasure_deriv takes it), deg_bound = n_per_row +
// n_erased, n_synd = n - deg_bound syndromes per row.
// the largest recurrence length Berlekamp-Massey keeps in LDS for field fid (>= 256)
size_t rs_locate_cap(int fid);
// row_flag[r] = 1 (never cleared here) if a coefficient at index >= deg_bound of row r is not zero
hipError_t rs_locate_scan(int fid, const uint32_t *h, int log_n, size_t n_rows, size_t deg_bound, uint8_t *row_flag,
                          hipStream_t s);
// synd[d][i] = coefficient deg_bound + i of row dirty[d], natural order, fully reduced
hipError_t rs_locate_gather(int fid, const uint32_t *h, int log_n, const uint32_t *dirty, size_t n_dirty,
                            size_t deg_bound, size_t n_synd, uint32_t *synd, hipStream_t s);
// coef[d][0..n) = the connection polynomial of synd[d] zero-padded (natural order, the forward plan's
// input), bm_len[d] = its degree L; >= 0xfffffffe and zeros when L would pass min(cap, n_synd / 2)
hipError_t rs_locate_bm(int fid, const uint32_t *synd, size_t n_dirty, size_t n_synd, int log_n, uint32_t *coef,
                        uint32_t *bm_len, hipStream_t s);
// e = the forward plan's output of coef: mask[d][c] = 1 where e[d][c] is zero, n_zero[d] their number,
// on_erased[d] = 1 if one of them is an erased position (slot[c] >= 0)
hipError_t rs_locate_zeros(int fid, const uint32_t *e, int log_n, size_t n_dirty, const int32_t *slot, uint8_t *mask,
                           uint32_t *n_zero, uint32_t *on_erased, hipStream_t s);
// dstatus[d] = row_status[dirty[d]] = 1 (located: bm_len[d] zeros, none erased) or 2; row_n_errors[dirty[d]]
// = the number of located positions; mask rows of status 2 are cleared, the others ORed into col_any[c]
hipError_t rs_locate_finish(const uint32_t *dirty, size_t n_dirty, int log_n, const uint32_t *bm_len,
                            const uint32_t *n_zero, const uint32_t *on_erased, uint8_t *dstatus, uint8_t *mask,
                            uint8_t *row_status, uint32_t *row_n_errors, uint8_t *col_any, hipStream_t s);

}  // namespace lcpc
