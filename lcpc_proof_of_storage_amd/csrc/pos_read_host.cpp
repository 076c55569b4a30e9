// pos_read_host.cpp -- checkable reads of a stored file (no counterpart in the reference, whose
// RequestFileRow answers with bytes the client cannot check, networking/server.rs:474-493): the plan
// of a byte range, the cover values a server sends with a column opened on a chunk range, and the
// client's rebuild of the leaves from segments and covers.  DESIGN.md §5e.
#include "pos_internal.hpp"

namespace {

using Nodes = std::vector<std::pair<size_t, size_t>>;

size_t pos_first_row(size_t chunk) { return lcpc_leaf_chunk_first_row(LCPC_FT63, chunk); }

// BLAKE3's left-balanced tree over chunks [lo, hi), pruned against the range [c_lo, c_hi): a node
// disjoint from the range is a cover, a node inside it is a run of the segment's own chunk CVs,
// any other node is the parent of its two children (split at the largest power of two below its
// size).  covers: the disjoint nodes in walk order; ops (optional): the post-order program of
// kernels.hpp.  A node of 8 chunks or more starts on a multiple of 8 (a node's first chunk is a
// multiple of its size rounded up to a power of two), so with `groups` such a run is taken a group
// node at a time, g0 being the first group read_segment_groups folds.
void read_walk(size_t lo, size_t hi, size_t c_lo, size_t c_hi, bool root, bool groups, size_t g0, Nodes &covers,
               std::vector<ReadOp> *ops) {
  if (hi <= c_lo || lo >= c_hi) {
    if (ops) ops->push_back(ReadOp{READ_OP_COVER, 0, covers.size(), 0});
    covers.emplace_back(lo, hi);
    return;
  }
  if (c_lo <= lo && hi <= c_hi) {
    if (!ops) return;
    if (groups && hi - lo >= (size_t)READ_GROUP)
      ops->push_back(ReadOp{READ_OP_GROUPS, root, lo / READ_GROUP - g0, (hi - lo + READ_GROUP - 1) / READ_GROUP});
    else
      ops->push_back(ReadOp{READ_OP_CHUNKS, root, lo - c_lo, hi - lo});
    return;
  }
  size_t half = 1;
  while (2 * half < hi - lo) half *= 2;
  read_walk(lo, lo + half, c_lo, c_hi, false, groups, g0, covers, ops);
  read_walk(lo + half, hi, c_lo, c_hi, false, groups, g0, covers, ops);
  if (ops) ops->push_back(ReadOp{READ_OP_MERGE, root, 0, 0});
}

lcpc_status read_chunk_range_check(size_t n_chunks, size_t chunk_lo, size_t chunk_hi) {
  if (chunk_lo >= chunk_hi) return fail(LCPC_ERR_INVALID_ARG, "read: empty chunk range");
  if (chunk_hi > n_chunks) return fail(LCPC_ERR_INVALID_ARG, "read: chunk_hi past the column's chunks");
  if (n_chunks > ((size_t)1 << 20)) return fail(LCPC_ERR_UNSUPPORTED, "read: columns of more than 2^20 chunks");
  return LCPC_OK;
}

// [n][rows] tightly packed 8-byte elements -> device columns col_elems (even, >= rows) apart
lcpc_status upload_columns(DBuf &d, Device *dev, const uint64_t *cols, size_t n, size_t rows, size_t col_elems,
                           hipStream_t s) {
  HIP_TRY(d.alloc(dev, n * col_elems * POS_WB));
  HIP_TRY(hipMemcpy2DAsync(d.p, col_elems * POS_WB, cols, rows * POS_WB, rows * POS_WB, n, hipMemcpyHostToDevice, s));
  return LCPC_OK;
}

// covers_out from a device [chunk][cv_stride] array of chunk CVs (idx null: column k is opened column k)
lcpc_status cover_values(Device *dev, hipStream_t s, const uint32_t *cvs, size_t cv_stride, size_t n_chunks,
                         const uint64_t *idx, size_t n_idx, const Nodes &covers, uint8_t *covers_out) {
  if (covers.empty() || !n_idx) return LCPC_OK;
  std::vector<uint64_t> flat;
  for (const auto &c : covers) {
    flat.push_back(c.first);
    flat.push_back(c.second);
  }
  lcpc_status st;
  DBuf dn, di, dc;
  if ((st = upload(dev, dn, flat.data(), flat.size() * 8))) return st;
  if (idx && (st = upload(dev, di, idx, n_idx * 8))) return st;
  HIP_TRY(dc.alloc(dev, n_idx * covers.size() * 32));
  HIP_TRY(read_cover_values(cvs, cv_stride, n_chunks, idx ? di.as<uint64_t>() : nullptr, n_idx, dn.as<uint64_t>(),
                            covers.size(), dc.as<uint8_t>(), s));
  HIP_TRY(hipMemcpyAsync(covers_out, dc.p, n_idx * covers.size() * 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_read_plan(size_t file_len, size_t byte_start, size_t byte_end, size_t pre, size_t *row_lo,
                               size_t *row_hi, size_t *chunk_lo, size_t *chunk_hi, size_t *seg_row_lo,
                               size_t *seg_row_hi, size_t *n_cover, size_t *cover_nodes, size_t cover_cap) {
  if (byte_start >= byte_end || byte_end > file_len || !pre)
    return fail(LCPC_ERR_INVALID_ARG, "read: byte_start >= byte_end, byte_end > file_len or pre == 0");
  if (pre > SIZE_MAX / POS_DB || byte_end > SIZE_MAX - POS_DB * pre)
    return fail(LCPC_ERR_INVALID_ARG, "read: range overflows");
  const size_t rb = POS_DB * pre;
  const size_t rows = ((file_len + POS_DB - 1) / POS_DB + pre - 1) / pre;
  const size_t n_chunks = leaf_n_chunks(POS_FID, rows);
  const size_t r_lo = byte_start / rb, r_hi = (byte_end + rb - 1) / rb;
  const size_t c_lo = (32 + r_lo * POS_WB) / 1024, c_hi = (32 + (r_hi - 1) * POS_WB) / 1024 + 1;
  Nodes covers;
  read_walk(0, n_chunks, c_lo, c_hi, true, false, 0, covers, nullptr);
  if (cover_nodes && covers.size() > cover_cap)
    return fail(LCPC_ERR_INVALID_ARG, "read: cover_cap is smaller than the number of cover nodes");
  if (row_lo) *row_lo = r_lo;
  if (row_hi) *row_hi = r_hi;
  if (chunk_lo) *chunk_lo = c_lo;
  if (chunk_hi) *chunk_hi = c_hi;
  if (seg_row_lo) *seg_row_lo = pos_first_row(c_lo);
  if (seg_row_hi) *seg_row_hi = c_hi == n_chunks ? rows : pos_first_row(c_hi);
  if (n_cover) *n_cover = covers.size();
  if (cover_nodes)
    for (size_t j = 0; j < covers.size(); j++) {
      cover_nodes[2 * j] = covers[j].first;
      cover_nodes[2 * j + 1] = covers[j].second;
    }
  return LCPC_OK;
}

lcpc_status lcpc_pos_segment_covers_from_cache(const lcpc_pos_chunk_cache *cache, const uint64_t *idx, size_t n_idx,
                                               size_t chunk_lo, size_t chunk_hi, uint8_t *covers_out) {
  if (!cache) return fail(LCPC_ERR_INVALID_ARG, "null cache");
  lcpc_status st = read_chunk_range_check(cache->n_chunks, chunk_lo, chunk_hi);
  if (st) return st;
  if (!idx && n_idx) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  for (size_t k = 0; k < n_idx; k++)
    if (idx[k] >= cache->enc) return fail(LCPC_ERR_INVALID_ARG, "column index out of range");
  Nodes covers;
  read_walk(0, cache->n_chunks, chunk_lo, chunk_hi, true, false, 0, covers, nullptr);
  if (covers.empty() || !n_idx) return LCPC_OK;
  if (!covers_out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  Device *dev = cache->dev;
  Lease lease(dev, POOL_HIGH);
  HIP_TRY(hipSetDevice(dev->id));
  return cover_values(dev, lease.s, cache->cvs.as<uint32_t>(), cache->enc, cache->n_chunks, idx, n_idx, covers,
                      covers_out);
}

lcpc_status lcpc_pos_segment_covers_from_columns(const uint64_t *cols, size_t rows_written, size_t n_idx,
                                                 size_t chunk_lo, size_t chunk_hi, uint8_t *covers_out) {
  if (!rows_written) return fail(LCPC_ERR_INVALID_ARG, "read: a file without rows");
  const size_t n_chunks = leaf_n_chunks(POS_FID, rows_written);
  lcpc_status st = read_chunk_range_check(n_chunks, chunk_lo, chunk_hi);
  if (st) return st;
  if (!cols && n_idx) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  Nodes covers;
  read_walk(0, n_chunks, chunk_lo, chunk_hi, true, false, 0, covers, nullptr);
  if (!covers_out && n_idx && !covers.empty()) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_idx) return LCPC_OK;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev, POOL_HIGH);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  // every chunk CV of the opened columns (the existing column-major chunk kernel, which also checks
  // the elements), then the same fold as from the cache
  const size_t col_elems = rows_written + (rows_written & 1);
  DBuf dcols, dcvs;
  BadFlag bad;
  if ((st = bad.init(dev, s)) || (st = upload_columns(dcols, dev, cols, n_idx, rows_written, col_elems, s))) return st;
  HIP_TRY(dcvs.alloc(dev, n_chunks * n_idx * 32));
  for (size_t c0 = 0; c0 < n_chunks; c0 += 65535)  // (one launch hashes at most 65535 chunks)
    HIP_TRY(leaf_chunk_cvs_slices(POS_FID, dcols.as<uint32_t>() + (pos_first_row(c0) * POS_WB) / 4, col_elems,
                                  rows_written, n_idx, c0, std::min(n_chunks, c0 + 65535), dcvs.as<uint32_t>(), 0,
                                  n_idx, bad.p(), s));
  if ((st = bad.read_back(s))) return st;
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = bad.verdict())) return st;
  return cover_values(dev, s, dcvs.as<uint32_t>(), n_idx, n_chunks, nullptr, n_idx, covers, covers_out);
}

lcpc_status lcpc_pos_segment_leaves(const uint64_t *segs, size_t n_idx, size_t rows_written, size_t chunk_lo,
                                    size_t chunk_hi, const uint8_t *covers, size_t n_cover, const uint64_t *weights,
                                    uint8_t *leaves_out, uint64_t *dots_out, uint8_t *canonical_ok) {
  if (!rows_written) return fail(LCPC_ERR_INVALID_ARG, "read: a file without rows");
  const size_t n_chunks = leaf_n_chunks(POS_FID, rows_written);
  lcpc_status st = read_chunk_range_check(n_chunks, chunk_lo, chunk_hi);
  if (st) return st;
  if ((weights == nullptr) != (dots_out == nullptr))
    return fail(LCPC_ERR_INVALID_ARG, "read: weights and dots_out go together");
  // the program of this range; a short segment folds chunk by chunk (as launch_leaf_merge's one pass)
  const size_t n_seg = chunk_hi - chunk_lo;
  const bool groups = n_seg > 2 * (size_t)READ_GROUP;
  const size_t g0 = (chunk_lo + READ_GROUP - 1) / READ_GROUP;
  const size_t g1 = chunk_hi == n_chunks ? (n_chunks + READ_GROUP - 1) / READ_GROUP : chunk_hi / READ_GROUP;
  const size_t n_groups = groups && g1 > g0 ? g1 - g0 : 0;
  Nodes nodes;
  std::vector<ReadOp> ops;
  read_walk(0, n_chunks, chunk_lo, chunk_hi, true, groups, g0, nodes, &ops);
  if (n_cover != nodes.size()) return fail(LCPC_ERR_INVALID_ARG, "read: n_cover is not the plan's cover count");
  if ((!segs || !leaves_out || !canonical_ok || (!covers && n_cover)) && n_idx)
    return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!n_idx) return LCPC_OK;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev, POOL_HIGH);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const size_t seg_lo = pos_first_row(chunk_lo), seg_hi = chunk_hi == n_chunks ? rows_written : pos_first_row(chunk_hi);
  const size_t seg_rows = seg_hi - seg_lo, col_elems = seg_rows + (seg_rows & 1);
  DBuf dsegs, dw, dcov, dops, dcvs, dgroups, dpart, dbad, dleaves, ddots;
  if ((st = upload_columns(dsegs, dev, segs, n_idx, seg_rows, col_elems, s))) return st;
  if (weights) {
    if ((st = upload(dev, dw, weights, seg_rows * POS_WB))) return st;
  } else {  // the pass sums either way: zero weights
    HIP_TRY(dw.alloc(dev, seg_rows * POS_WB));
    HIP_TRY(hipMemsetAsync(dw.p, 0, seg_rows * POS_WB, s));
  }
  if (n_cover && (st = upload(dev, dcov, covers, n_idx * n_cover * 32))) return st;
  if ((st = upload(dev, dops, ops.data(), ops.size() * sizeof(ReadOp)))) return st;
  HIP_TRY(dcvs.alloc(dev, n_seg * n_idx * 32));
  HIP_TRY(dpart.alloc(dev, n_seg * n_idx * POS_WB));
  HIP_TRY(dgroups.alloc(dev, n_groups * n_idx * 32));
  HIP_TRY(dbad.alloc(dev, n_idx * 4));
  HIP_TRY(dleaves.alloc(dev, n_idx * 32));
  HIP_TRY(ddots.alloc(dev, n_idx * POS_WB));
  HIP_TRY(hipMemsetAsync(dbad.p, 0, n_idx * 4, s));
  HIP_TRY(read_segment_chunks(POS_FID, dsegs.as<uint32_t>(), col_elems, rows_written, n_idx, chunk_lo, chunk_hi,
                              dcvs.as<uint32_t>(), dw.as<uint32_t>(), dpart.as<uint32_t>(), dbad.as<uint32_t>(), s));
  HIP_TRY(read_segment_groups(dcvs.as<uint32_t>(), n_idx, chunk_lo, g0 * READ_GROUP, chunk_hi, n_groups,
                              dgroups.as<uint32_t>(), s));
  HIP_TRY(read_segment_leaves(dcvs.as<uint32_t>(), dgroups.as<uint32_t>(), dcov.as<uint8_t>(), n_idx, n_cover, n_chunks,
                              dops.as<ReadOp>(), ops.size(), dleaves.as<uint8_t>(), s));
  std::vector<uint32_t> bad(n_idx);
  HIP_TRY(hipMemcpyAsync(leaves_out, dleaves.p, n_idx * 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(bad.data(), dbad.p, n_idx * 4, hipMemcpyDeviceToHost, s));
  if (dots_out) {
    // the chunks' shares summed; canonical sums of canonical elements, handed back as Montgomery
    // limbs like every element of this interface
    HIP_TRY(collapse_fold_rows(POS_FID, dpart.as<uint32_t>(), n_seg, n_idx, ddots.as<uint32_t>(), s));
    HIP_TRY(convert(POS_FID, ddots.as<uint32_t>(), ddots.as<uint32_t>(), n_idx, true, s));
    HIP_TRY(hipMemcpyAsync(dots_out, ddots.p, n_idx * POS_WB, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t k = 0; k < n_idx; k++) canonical_ok[k] = bad[k] ? 0 : 1;
  return LCPC_OK;
}

}  // extern "C"
