// pos_files_host.cpp -- stored proof-of-storage files: the streaming writer, re-encode, tree and
// decode of an encoded image, the column chunk-CV cache and the column-digest accumulator.
#include "pos_internal.hpp"

// The `.porenc` / `.portree` formats of proof-of-storage/src/lcpc_online.
// The whole data path (byte packing, Ligero encode, canonical conversion + transpose to the
// column-major file layout, BLAKE3 column digests, Merkle tree) runs on the GPU in row batches
// that end on BLAKE3 chunk boundaries of the column messages, so each batch contributes whole
// chunk chaining values and the file streams through bounded device memory.  The host only
// moves bytes between the caller's buffers (typically mmaps of the files) and page-locked
// staging, with the copies of one batch overlapping the GPU work of the next.

// EncodedFileWriter (encoded_file_writer.rs:24-38): bytes arrive in pushes; whole batches of
// rows are encoded once the data provably continues past them (so no chunk they close can be
// a column message's last chunk), the rest at finalize when the row count is known.
struct lcpc_pos_writer {
  std::unique_ptr<lcpc_encoding> e;
  size_t pre = 0, enc = 0, row_capacity = 0;
  uint8_t *porenc = nullptr;
  size_t cpb = 1, bmax = 1;        // chunks per batch, rows per batch (at most)
  size_t rows_done = 0, chunks_done = 0, bytes_received = 0;
  bool finalized = false;
  Pinned pend;                     // data bytes from row rows_done on (page-locked)
  size_t pend_len = 0;
  std::vector<uint8_t> cvs;        // [chunk][column] chaining values of the chunks done
  size_t buf_rows = 0;             // rows the batch buffers below hold (grown on demand)
  DBuf dbytes, coeffs, comm, dout, dcv;
  Pinned stg[2];
  Events ev;
};

namespace {

size_t pos_row_bytes(const lcpc_pos_writer *w) { return w->pre * POS_DB; }

lcpc_status writer_append(lcpc_pos_writer *w, const uint8_t *bytes, size_t n) {
  if (!n) return LCPC_OK;
  if (w->pend_len + n > w->pend.n) {
    Pinned bigger;
    if (!bigger.get(w->e->dev, std::max(w->pend_len + n, std::max<size_t>(1 << 20, 2 * w->pend.n))))
      return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    par_memcpy(bigger.b(), w->pend.b(), w->pend_len);
    std::swap(w->pend.p, bigger.p);
    std::swap(w->pend.n, bigger.n);
    std::swap(w->pend.d, bigger.d);
  }
  par_memcpy(w->pend.b() + w->pend_len, bytes, n);
  w->pend_len += n;
  return LCPC_OK;
}

// Encode chunks [chunks_done, c_end) (rows from pend), n_rows_cv = the row count the chunk
// chaining values are computed for (exact at finalize; any larger-than-covered count before).
lcpc_status writer_run(lcpc_pos_writer *w, size_t c_end, size_t n_rows_cv, size_t n_rows_max) {
  if (c_end <= w->chunks_done) return LCPC_OK;
  const int fid = POS_FID;
  const size_t pre = w->pre, enc = w->enc, rb = pos_row_bytes(w);
  Device *dev = w->e->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  for (auto *b : {&w->dbytes, &w->coeffs, &w->comm, &w->dout, &w->dcv}) b->s = s;
  lcpc_status st;
  struct Pending {
    int slot = -1;
    size_t r0 = 0, rows = 0;
  } pend;
  auto scatter = [&](const Pending &p) -> lcpc_status {
    if (p.slot < 0) return LCPC_OK;
    HIP_TRY(hipEventSynchronize(w->ev.e[p.slot]));
    scatter_slices(w->porenc, w->row_capacity, 0, enc, p.r0, p.rows, p.rows * POS_WB, w->stg[p.slot].b());
    return LCPC_OK;
  };
  const size_t pend_row0 = w->rows_done;
  // batch buffers sized for the largest batch of this run (small files stay small)
  const size_t need_rows = std::min(w->bmax, std::max<size_t>(1, n_rows_max - std::min(n_rows_max, pend_row0)));
  if (need_rows > w->buf_rows) {
    HIP_TRY(w->dbytes.alloc(dev, need_rows * pre * POS_DB + 64));
    HIP_TRY(w->coeffs.alloc(dev, need_rows * pre * POS_WB));
    HIP_TRY(w->comm.alloc(dev, need_rows * enc * POS_WB));
    HIP_TRY(w->dout.alloc(dev, need_rows * enc * POS_WB));
    for (auto &x : w->stg)
      if (!x.get(dev, need_rows * enc * POS_WB)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    w->buf_rows = need_rows;
  }
  // chaining values land in w->cvs by async copies: no reallocation while they are queued
  w->cvs.reserve(c_end * w->enc * 32);
  const ChunkBatches batches{leaf_n_chunks(fid, n_rows_cv), w->cpb, n_rows_max, c_end};
  int k = 0;
  for (size_t c_lo = w->chunks_done; c_lo < c_end; c_lo += w->cpb, k++) {
    const auto [r0, B, c_hi] = batches.at(c_lo);
    if (B > w->buf_rows) return fail(LCPC_ERR_INVALID_ARG, "internal: batch larger than its buffers");
    if (B) {
      if (w->porenc && r0 + B > w->row_capacity) return fail(LCPC_ERR_INVALID_ARG, "row capacity exceeded");
      // rows r0..r0+B are data bytes [rb (r0 - pend_row0), ...) of pend (the last may be short)
      const size_t b0 = (r0 - pend_row0) * rb;
      const size_t b1 = std::min(w->pend_len, b0 + B * rb);
      // (digest-only writers keep no image: nothing is transposed for them)
      if ((st = pack_encode_batch(w->e.get(), w->pend.b() + b0, b1 - b0, B, w->dbytes, w->coeffs, w->comm,
                                  w->porenc ? &w->dout : nullptr, s)))
        return st;
    }
    // column-digest chunks of these rows (ColumnDigestAccumulator::update, :62-87)
    HIP_TRY(leaf_chunk_cvs(fid, w->comm.as<uint32_t>(), r0, n_rows_cv, enc, enc, c_lo, c_hi,
                           w->dcv.as<uint32_t>(), s, true));
    const size_t cv_bytes = (c_hi - c_lo) * enc * 32;
    const size_t cv_off = w->cvs.size();
    w->cvs.resize(cv_off + cv_bytes);
    HIP_TRY(hipMemcpyAsync(w->cvs.data() + cv_off, w->dcv.p, cv_bytes, hipMemcpyDeviceToHost, s));
    if (B && w->porenc) {
      const int slot = k & 1;
      HIP_TRY(hipMemcpyAsync(w->stg[slot].p, w->dout.p, B * enc * POS_WB, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipEventRecord(w->ev.e[slot], s));
      if ((st = scatter(pend))) return st;  // overlaps this batch's GPU work
      pend = Pending{slot, r0, B};
    }
    w->chunks_done = c_hi;
    w->rows_done = r0 + B;
  }
  if ((st = scatter(pend))) return st;
  HIP_TRY(hipStreamSynchronize(s));
  for (auto *b : {&w->dbytes, &w->coeffs, &w->comm, &w->dout, &w->dcv}) b->settle();
  const size_t used = std::min(w->pend_len, (w->rows_done - pend_row0) * rb);
  std::memmove(w->pend.b(), w->pend.b() + used, w->pend_len - used);
  w->pend_len -= used;
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_writer_new(size_t pre, size_t enc, uint8_t *porenc, size_t row_capacity,
                                size_t batch_rows, lcpc_pos_writer **out) {
  lcpc_status st = pos_dims_check(pre, enc);
  if (st) return st;
  if (!out || (!porenc && row_capacity)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  lcpc_encoding *ep = nullptr;
  if ((st = make_rs_encoding(POS_FID, pre, enc, 0, 0, &ep))) return st;
  auto w = std::make_unique<lcpc_pos_writer>();
  w->e.reset(ep);
  w->pre = pre;
  w->enc = enc;
  w->porenc = porenc;
  w->row_capacity = row_capacity;
  size_t want = batch_rows;
  if (!want) want = std::max<size_t>(POS_ROWS_PER_CHUNK, pos_stage_bytes() / (enc * POS_WB));
  w->cpb = std::max<size_t>(1, want / POS_ROWS_PER_CHUNK);
  w->bmax = w->cpb * POS_ROWS_PER_CHUNK;
  Device *dev = w->e->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  HIP_TRY(w->dcv.alloc(dev, w->cpb * enc * 32));
  HIP_TRY(w->ev.init());
  HIP_TRY(hipStreamSynchronize(lease.s));
  for (auto *b : {&w->dbytes, &w->coeffs, &w->comm, &w->dout, &w->dcv}) b->settle();
  *out = w.release();
  return LCPC_OK;
}

void lcpc_pos_writer_free(lcpc_pos_writer *w) { delete w; }

lcpc_status lcpc_pos_writer_set_target(lcpc_pos_writer *w, uint8_t *porenc, size_t row_capacity) {
  // after the caller grew the file (EncodedFileReader::set_new_capacity layout, :348-381)
  if (!w || (!porenc && row_capacity)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (row_capacity < w->rows_done) return fail(LCPC_ERR_INVALID_ARG, "row_capacity < rows written");
  w->porenc = porenc;
  w->row_capacity = row_capacity;
  return LCPC_OK;
}

size_t lcpc_pos_writer_rows_written(const lcpc_pos_writer *w) { return w ? w->rows_done : 0; }

lcpc_status lcpc_pos_writer_push_bytes(lcpc_pos_writer *w, const uint8_t *bytes, size_t n) {
  // push_bytes (encoded_file_writer.rs:233-262)
  if (!w || (!bytes && n)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (w->finalized) return fail(LCPC_ERR_INVALID_ARG, "writer already finalized");
  lcpc_status st;
  const size_t rb = pos_row_bytes(w);
  // large pushes are taken a batch at a time, so the staging stays about a batch
  const size_t step = std::max<size_t>(1, w->bmax * rb);
  for (size_t off = 0; off < n || (n == 0 && off == 0); off += step) {
    const size_t m = std::min(step, n - off);
    if ((st = writer_append(w, bytes + off, m))) return st;
    w->bytes_received += m;
    // whole batches whose rows are followed by at least one more full row
    const size_t full_rows = w->rows_done + w->pend_len / rb;
    size_t c_end = w->chunks_done;
    while (lcpc_leaf_chunk_first_row(LCPC_FT63, c_end + w->cpb) < full_rows) c_end += w->cpb;
    if (c_end > w->chunks_done &&
        (st = writer_run(w, c_end, full_rows, lcpc_leaf_chunk_first_row(LCPC_FT63, c_end))))
      return st;
    if (n == 0) break;
  }
  return LCPC_OK;
}

lcpc_status lcpc_pos_writer_finalize(lcpc_pos_writer *w, uint8_t *digests, uint8_t *tree,
                                     size_t *rows_written, size_t *bytes_of_data) {
  // finalize_to_column_digest / _to_commit / _to_merkle_tree (encoded_file_writer.rs:452-501):
  // digests = the enc column digests, tree = MerkleTree::to_bytes (2 enc - 1 digests); either
  // may be NULL
  if (!w) return fail(LCPC_ERR_INVALID_ARG, "null writer");
  if (w->finalized) return fail(LCPC_ERR_INVALID_ARG, "writer already finalized");
  const size_t rb = pos_row_bytes(w);
  const size_t n_rows = w->rows_done + (w->pend_len + rb - 1) / rb;
  if (w->porenc && n_rows > w->row_capacity) return fail(LCPC_ERR_INVALID_ARG, "row capacity exceeded");
  const int fid = POS_FID;
  const size_t n_chunks = leaf_n_chunks(fid, n_rows);
  lcpc_status st = writer_run(w, n_chunks, n_rows, n_rows);
  if (st) return st;
  w->finalized = true;
  const size_t enc = w->enc;
  Device *dev = w->e->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  DBuf dc, hashes;
  if ((st = upload(dev, dc, w->cvs.data(), w->cvs.size()))) return st;
  HIP_TRY(hashes.alloc(dev, (2 * enc - 1) * 32));
  HIP_TRY(leaves_from_cvs(dc.as<uint32_t>(), enc, (int)n_chunks, hashes.as<uint8_t>(), s));
  if (tree) {
    HIP_TRY(merkle_tree(hashes.as<uint8_t>(), enc, s));
    HIP_TRY(hipMemcpyAsync(tree, hashes.p, (2 * enc - 1) * 32, hipMemcpyDeviceToHost, s));
  }
  if (digests) HIP_TRY(hipMemcpyAsync(digests, hashes.p, enc * 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (rows_written) *rows_written = w->rows_done;
  if (bytes_of_data) *bytes_of_data = w->bytes_received;
  return LCPC_OK;
}

lcpc_status lcpc_pos_encode_file_batched(const uint8_t *data, size_t n_bytes, size_t pre, size_t enc,
                                         size_t row_capacity, uint8_t *porenc, uint8_t *tree,
                                         size_t *rows_written, size_t batch_rows) {
  lcpc_status st = pos_dims_check(pre, enc);
  if (st) return st;
  if (!tree || (!data && n_bytes)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  const size_t n_rows = ((n_bytes + POS_DB - 1) / POS_DB + pre - 1) / pre;
  if (rows_written) *rows_written = n_rows;
  if (row_capacity < n_rows) return fail(LCPC_ERR_INVALID_ARG, "row_capacity < rows to write");
  lcpc_pos_writer *w = nullptr;
  if ((st = lcpc_pos_writer_new(pre, enc, porenc, row_capacity, batch_rows, &w))) return st;
  std::unique_ptr<lcpc_pos_writer> guard(w);
  if ((st = lcpc_pos_writer_push_bytes(w, data, n_bytes))) return st;
  return lcpc_pos_writer_finalize(w, nullptr, tree, rows_written, nullptr);
}

lcpc_status lcpc_pos_encode_file(const uint8_t *data, size_t n_bytes, size_t pre, size_t enc,
                                 size_t row_capacity, uint8_t *porenc, uint8_t *tree,
                                 size_t *rows_written) {
  return lcpc_pos_encode_file_batched(data, n_bytes, pre, enc, row_capacity, porenc, tree, rows_written, 0);
}

lcpc_status lcpc_pos_reencode_rows(const uint8_t *bytes, size_t n_bytes, size_t pre, size_t enc,
                                   size_t row_lo, uint8_t *porenc, size_t row_capacity) {
  // FileHandler::reencode_row / EncodedFileReader::replace_row_with_decoded_bytes +
  // replace_encoded_row (file_handler.rs:380-402, encoded_file_reader.rs:196-315) for the rows
  // [row_lo, row_lo + ceil(n_bytes / (7 pre))): pack each row's bytes (the last row may be
  // short: zero-padded), encode, and write the canonical repr into the column-major image at
  // column stride row_capacity.  Batches of rows go through the GPU like the writer's.
  lcpc_status st = pos_dims_check(pre, enc);
  if (st) return st;
  if ((!bytes || !porenc) && n_bytes) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  const size_t rb = pre * POS_DB;
  const size_t n_rows = (n_bytes + rb - 1) / rb;
  if (!n_rows) return LCPC_OK;
  if (row_lo + n_rows > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "rows beyond row_capacity");
  lcpc_encoding *ep = nullptr;
  if ((st = make_rs_encoding(POS_FID, pre, enc, 0, 0, &ep))) return st;
  std::unique_ptr<lcpc_encoding> eg(ep);
  Device *dev = ep->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const size_t bmax = std::min(n_rows, std::max<size_t>(1, pos_stage_bytes() / (enc * POS_WB)));
  DBuf dbytes, coeffs, comm, dout;
  for (auto *b : {&dbytes, &coeffs, &comm, &dout}) b->s = s;
  HIP_TRY(dbytes.alloc(dev, bmax * rb + 64));
  HIP_TRY(coeffs.alloc(dev, bmax * pre * POS_WB));
  HIP_TRY(comm.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(dout.alloc(dev, bmax * enc * POS_WB));
  Pinned stg;
  if (!stg.get(dev, bmax * enc * POS_WB)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  for (size_t r0 = 0; r0 < n_rows; r0 += bmax) {
    const size_t B = std::min(bmax, n_rows - r0);
    const size_t b0 = r0 * rb, b1 = std::min(n_bytes, b0 + B * rb);
    if ((st = pack_encode_batch(ep, bytes + b0, b1 - b0, B, dbytes, coeffs, comm, &dout, s))) return st;
    HIP_TRY(hipMemcpyAsync(stg.p, dout.p, B * enc * POS_WB, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    scatter_slices(porenc, row_capacity, 0, enc, row_lo + r0, B, B * POS_WB, stg.b());
  }
  for (auto *b : {&dbytes, &coeffs, &comm, &dout}) b->settle();
  return LCPC_OK;
}

lcpc_status lcpc_pos_porenc_tree(const uint8_t *porenc, size_t enc, size_t rows_written,
                                 size_t row_capacity, uint8_t *tree) {
  // EncodedFileReader::process_file_to_merkle_tree (encoded_file_reader.rs:328-346): every
  // column's first rows_written elements, hashed after the 32-byte zero block
  if (enc < 2 || (enc & (enc - 1))) return fail(LCPC_ERR_INVALID_ARG, "encoded width must be a power of 2 (>= 2)");
  if (!tree || (!porenc && rows_written)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (rows_written > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "rows_written > row_capacity");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const int fid = POS_FID;
  const size_t cpb = column_block_cols(enc, rows_written * POS_WB, pos_stage_bytes());
  DBuf hashes, scratch[2];
  BadFlag bad;
  HIP_TRY(hashes.alloc(dev, (2 * enc - 1) * 32));
  for (auto &x : scratch) HIP_TRY(x.alloc(dev, leaf_hash_scratch_bytes(fid, rows_written, cpb)));
  if ((st = bad.init(dev, s))) return st;
  const ImageSrc img{porenc, -1, row_capacity};
  st = for_column_blocks(dev, s, img, enc, cpb, 0, rows_written, rows_written,
                         [&](uint32_t *d_cols, size_t c0, size_t nc, int slot) -> lcpc_status {
                           if (rows_written)
                             HIP_TRY(convert(fid, d_cols, d_cols, nc * rows_written, true, s, bad.p()));
                           HIP_TRY(leaf_hashes_cols(fid, d_cols, rows_written, nc, hashes.as<uint8_t>() + c0 * 32,
                                                    scratch[slot].p, s));
                           return LCPC_OK;
                         });
  if (st) return st;
  HIP_TRY(merkle_tree(hashes.as<uint8_t>(), enc, s));
  if ((st = bad.read_back(s))) return st;
  HIP_TRY(hipMemcpyAsync(tree, hashes.p, (2 * enc - 1) * 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return bad.verdict();
}

lcpc_status lcpc_pos_decode_porenc(const uint8_t *porenc, size_t pre, size_t enc, size_t row_capacity,
                                   size_t row_lo, size_t row_hi, uint8_t *out) {
  // EncodedFileReader::get_unencoded_row_bytes / decode_to_target_file (encoded_file_reader.rs:
  // 59-91): gather each row's enc elements from the columns, decode_row (ifft_oi), keep the
  // first pre coefficients, 7 data bytes each
  lcpc_status st = pos_dims_check(pre, enc);
  if (st) return st;
  if (row_lo > row_hi || row_hi > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "row range");
  const size_t n = row_hi - row_lo;
  if (!n) return LCPC_OK;
  if (!porenc || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const int fid = POS_FID;
  const int log_n = (int)log2_np2(enc);
  InversePlan inverse;
  if ((st = inverse.init(fid, log_n, s))) return st;
  const size_t bmax = std::max<size_t>(1, std::min(n, pos_stage_bytes() / (enc * POS_WB)));
  DBuf a, b, dbytes;
  BadFlag bad;
  HIP_TRY(a.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(b.alloc(dev, bmax * enc * POS_WB));
  HIP_TRY(dbytes.alloc(dev, bmax * pre * POS_DB + 64));
  if ((st = bad.init(dev, s))) return st;
  const ImageSrc img{porenc, -1, row_capacity};
  Pinned stg[2], ostg[2];
  Events in_ev, out_ev;
  HIP_TRY(in_ev.init());
  HIP_TRY(out_ev.init());
  for (int i = 0; i < 2; i++)
    if (!stg[i].get(dev, bmax * enc * POS_WB) || !ostg[i].get(dev, bmax * pre * POS_DB))
      return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  struct Done {
    int slot = -1;
    size_t r0 = 0, rows = 0;
  } done;
  auto copy_out = [&](const Done &d) -> lcpc_status {
    if (d.slot < 0) return LCPC_OK;
    HIP_TRY(hipEventSynchronize(out_ev.e[d.slot]));
    par_memcpy(out + (d.r0 - row_lo) * pre * POS_DB, ostg[d.slot].b(), d.rows * pre * POS_DB);
    return LCPC_OK;
  };
  int k = 0;
  for (size_t r0 = row_lo; r0 < row_hi; r0 += bmax, k++) {
    const size_t B = std::min(row_hi, r0 + bmax) - r0;
    const int slot = k & 1;
    HIP_TRY(in_ev.reuse(k));  // its last upload has left it
    gather_slices(img, 0, enc, r0, B, B * POS_WB, stg[slot].b());
    HIP_TRY(hipMemcpyAsync(a.p, stg[slot].p, enc * B * POS_WB, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(in_ev.e[slot], s));
    // [enc][B] canonical -> [B][enc] Montgomery (get_encoded_row + raw_bytes_to_field_vec)
    HIP_TRY(transpose_elems(fid, a.as<uint32_t>(), enc, B, B, B, b.as<uint32_t>(), enc, s, TR_TO_MONT,
                            bad.p()));
    uint32_t *x = nullptr, *y = nullptr;  // the decoded rows, and the buffer that is free again
    if ((st = ifft_oi_device(inverse.plan, fid, log_n, b.as<uint32_t>(), a.as<uint32_t>(), B, s, &x, &y))) return st;
    if ((st = decode_rows_to_bytes(x, y, pre, enc, B, dbytes.as<uint8_t>(), s))) return st;
    HIP_TRY(out_ev.reuse(k));
    HIP_TRY(hipMemcpyAsync(ostg[slot].p, dbytes.p, B * pre * POS_DB, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(out_ev.e[slot], s));
    if ((st = copy_out(done))) return st;  // overlaps this batch's GPU work
    done = Done{slot, r0, B};
  }
  if ((st = copy_out(done))) return st;
  if ((st = bad.read_back(s))) return st;
  HIP_TRY(hipStreamSynchronize(s));
  return bad.verdict();
}

}  // extern "C"

// Column chunk-CV cache of a stored file: the chaining value of every 1-KiB BLAKE3 chunk of every
// column message (32 zero bytes || the column's rows_written canonical elements), [chunk][column],
// kept in device memory.  A chunk's value depends only on its bytes, its counter and whether it is
// the message's only chunk, so after an edit or an append only the chunks whose rows, length or
// one-chunk flag changed are read from the image and rehashed; the column digests are one
// non-clobbering fold of the cache (leaves_fold_cvs) and the tree follows as everywhere else.
// (struct lcpc_pos_chunk_cache: pos_internal.hpp; the checkable read opens columns from it too.)

namespace {

size_t pos_chunk_of_row(size_t row) { return (32 + row * POS_WB) / 1024; }

lcpc_status pos_update_chunk_range(size_t old_rows, size_t new_rows, size_t row_lo, size_t row_hi,
                                   size_t *chunk_lo, size_t *chunk_hi) {
  if (new_rows < old_rows) return fail(LCPC_ERR_INVALID_ARG, "a stored file's row count cannot shrink");
  if (row_lo > row_hi || row_hi > new_rows) return fail(LCPC_ERR_INVALID_ARG, "row range");
  size_t lo = 0, hi = 0;
  if (row_lo < row_hi) {
    lo = pos_chunk_of_row(row_lo);
    hi = pos_chunk_of_row(row_hi - 1) + 1;
  }
  if (new_rows > old_rows) {
    // the old last chunk changes length (or, the only chunk so far, loses ROOT); every later one is new
    const size_t old_last = leaf_n_chunks(POS_FID, old_rows) - 1;
    lo = row_lo < row_hi ? std::min(lo, old_last) : old_last;
    hi = leaf_n_chunks(POS_FID, new_rows);
  }
  *chunk_lo = lo;
  *chunk_hi = hi;
  return LCPC_OK;
}

// Chunks [c_lo, c_hi) of every column of the image (messages of n_rows rows) hashed into dst, a
// device [chunk][enc] array whose first chunk row is chunk c_lo: only those chunks' rows are read,
// enc strided slices staged through page-locked memory a block of columns at a time, each block's
// host copy overlapping the previous block's upload and hashing.  Returns with the stream drained,
// and an error if an element is not < p.  The image is the mapping porenc or, with fd >= 0, the open
// file fd read with pread.
lcpc_status cache_hash_chunks(Device *dev, hipStream_t s, const uint8_t *porenc, int fd, size_t enc,
                              size_t row_capacity, size_t n_rows, size_t c_lo, size_t c_hi, uint32_t *dst) {
  const int fid = POS_FID;
  const size_t n_chunks = leaf_n_chunks(fid, n_rows);
  const size_t r_lo = std::min(n_rows, lcpc_leaf_chunk_first_row((lcpc_field)fid, c_lo));
  const size_t r_hi = c_hi == n_chunks ? n_rows : lcpc_leaf_chunk_first_row((lcpc_field)fid, c_hi);
  const size_t R = r_hi - r_lo;
  const size_t col_elems = R + (R & 1);  // 16-byte aligned slices (the kernel masks the pad)
  const ImageSrc img{porenc, fd, row_capacity};
  BadFlag bad;
  lcpc_status st = bad.init(dev, s);
  if (st) return st;
  const size_t cpb = column_block_cols(enc, col_elems * POS_WB, pos_stage_bytes());
  st = for_column_blocks(dev, s, img, enc, cpb, r_lo, R, col_elems, [&](uint32_t *d_cols, size_t c0, size_t nc, int) -> lcpc_status {
    HIP_TRY(leaf_chunk_cvs_slices(fid, d_cols, col_elems, n_rows, nc, c_lo, c_hi, dst + c0 * 8, c_lo, enc, bad.p(), s));
    return LCPC_OK;
  });
  if (st || (st = bad.read_back(s))) return st;
  HIP_TRY(hipStreamSynchronize(s));
  return bad.verdict();
}

lcpc_status cache_check_enc(size_t enc) {
  if (enc < 2 || (enc & (enc - 1))) return fail(LCPC_ERR_INVALID_ARG, "encoded width must be a power of 2 (>= 2)");
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_pos_update_chunk_range(size_t old_rows, size_t new_rows, size_t row_lo, size_t row_hi,
                                        size_t *chunk_lo, size_t *chunk_hi) {
  if (!chunk_lo || !chunk_hi) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  return pos_update_chunk_range(old_rows, new_rows, row_lo, row_hi, chunk_lo, chunk_hi);
}

size_t lcpc_pos_writer_n_chunks(const lcpc_pos_writer *w) {
  return w && w->finalized ? w->chunks_done : 0;
}

lcpc_status lcpc_pos_writer_copy_cvs(const lcpc_pos_writer *w, uint8_t *out) {
  if (!w || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!w->finalized) return fail(LCPC_ERR_INVALID_ARG, "writer not finalized");
  std::memcpy(out, w->cvs.data(), w->cvs.size());
  return LCPC_OK;
}

lcpc_status lcpc_pos_chunk_cache_from_porenc(const uint8_t *porenc, size_t enc, size_t rows_written,
                                             size_t row_capacity, lcpc_pos_chunk_cache **out) {
  lcpc_status st = cache_check_enc(enc);
  if (st) return st;
  if (!out || (!porenc && rows_written)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (rows_written > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "rows_written > row_capacity");
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  auto c = std::make_unique<lcpc_pos_chunk_cache>();
  c->dev = dev;
  c->enc = enc;
  c->rows = rows_written;
  c->n_chunks = c->cap_chunks = leaf_n_chunks(POS_FID, rows_written);
  HIP_TRY(c->cvs.alloc(dev, c->cap_chunks * enc * 32));
  if ((st = cache_hash_chunks(dev, s, porenc, -1, enc, row_capacity, rows_written, 0, c->n_chunks, c->cvs.as<uint32_t>())))
    return st;
  c->cvs.settle();
  *out = c.release();
  return LCPC_OK;
}

lcpc_status lcpc_pos_chunk_cache_from_cvs(const uint8_t *cvs, size_t enc, size_t rows_written,
                                          lcpc_pos_chunk_cache **out) {
  lcpc_status st = cache_check_enc(enc);
  if (st) return st;
  if (!out || !cvs) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  auto c = std::make_unique<lcpc_pos_chunk_cache>();
  c->dev = dev;
  c->enc = enc;
  c->rows = rows_written;
  c->n_chunks = c->cap_chunks = leaf_n_chunks(POS_FID, rows_written);
  if ((st = upload(dev, c->cvs, cvs, c->n_chunks * enc * 32))) return st;
  HIP_TRY(hipStreamSynchronize(lease.s));
  c->cvs.settle();
  *out = c.release();
  return LCPC_OK;
}

void lcpc_pos_chunk_cache_free(lcpc_pos_chunk_cache *c) { delete c; }
size_t lcpc_pos_chunk_cache_enc(const lcpc_pos_chunk_cache *c) { return c ? c->enc : 0; }
size_t lcpc_pos_chunk_cache_rows(const lcpc_pos_chunk_cache *c) { return c ? c->rows : 0; }
size_t lcpc_pos_chunk_cache_n_chunks(const lcpc_pos_chunk_cache *c) { return c ? c->n_chunks : 0; }

lcpc_status lcpc_pos_chunk_cache_copy_cvs(const lcpc_pos_chunk_cache *c, size_t chunk_lo, size_t chunk_hi,
                                          uint8_t *out) {
  if (!c) return fail(LCPC_ERR_INVALID_ARG, "null cache");
  if (chunk_lo > chunk_hi || chunk_hi > c->n_chunks) return fail(LCPC_ERR_INVALID_ARG, "chunk range");
  if (chunk_lo == chunk_hi) return LCPC_OK;
  if (!out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  Lease lease(c->dev);
  HIP_TRY(hipSetDevice(c->dev->id));
  HIP_TRY(hipMemcpyAsync(out, c->cvs.as<uint8_t>() + chunk_lo * c->enc * 32, (chunk_hi - chunk_lo) * c->enc * 32,
                         hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

static lcpc_status chunk_cache_update(lcpc_pos_chunk_cache *c, const uint8_t *porenc, int fd, size_t row_capacity,
                                      size_t row_lo, size_t row_hi, size_t new_rows_written, size_t *chunk_lo,
                                      size_t *chunk_hi) {
  if (!c) return fail(LCPC_ERR_INVALID_ARG, "null cache");
  size_t c_lo = 0, c_hi = 0;
  lcpc_status st = pos_update_chunk_range(c->rows, new_rows_written, row_lo, row_hi, &c_lo, &c_hi);
  if (st) return st;
  if (new_rows_written > row_capacity) return fail(LCPC_ERR_INVALID_ARG, "rows_written > row_capacity");
  if (!porenc && fd < 0 && new_rows_written) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (chunk_lo) *chunk_lo = c_lo;
  if (chunk_hi) *chunk_hi = c_hi;
  if (c_lo == c_hi) return LCPC_OK;
  Device *dev = c->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const size_t enc = c->enc, new_chunks = leaf_n_chunks(POS_FID, new_rows_written);
  // rehash into a side buffer: the cache is touched only once every element has passed the check
  DBuf fresh;
  HIP_TRY(fresh.alloc(dev, (c_hi - c_lo) * enc * 32));
  if ((st = cache_hash_chunks(dev, s, porenc, fd, enc, row_capacity, new_rows_written, c_lo, c_hi, fresh.as<uint32_t>())))
    return st;
  if (new_chunks > c->cap_chunks) {  // grow by whole chunk rows (doubling, so appends stay amortised)
    const size_t cap = std::max(new_chunks, 2 * c->cap_chunks);
    DBuf bigger;
    HIP_TRY(bigger.alloc(dev, cap * enc * 32));
    HIP_TRY(hipMemcpyAsync(bigger.p, c->cvs.p, c->n_chunks * enc * 32, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    bigger.settle();
    c->cvs = std::move(bigger);
    c->cap_chunks = cap;
  }
  HIP_TRY(hipMemcpyAsync(c->cvs.as<uint8_t>() + c_lo * enc * 32, fresh.p, (c_hi - c_lo) * enc * 32,
                         hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  c->rows = new_rows_written;
  c->n_chunks = new_chunks;
  return LCPC_OK;
}

lcpc_status lcpc_pos_chunk_cache_update(lcpc_pos_chunk_cache *c, const uint8_t *porenc, size_t row_capacity,
                                        size_t row_lo, size_t row_hi, size_t new_rows_written, size_t *chunk_lo,
                                        size_t *chunk_hi) {
  return chunk_cache_update(c, porenc, -1, row_capacity, row_lo, row_hi, new_rows_written, chunk_lo, chunk_hi);
}

lcpc_status lcpc_pos_chunk_cache_update_fd(lcpc_pos_chunk_cache *c, int fd, size_t row_capacity, size_t row_lo,
                                           size_t row_hi, size_t new_rows_written, size_t *chunk_lo,
                                           size_t *chunk_hi) {
  if (fd < 0) return fail(LCPC_ERR_INVALID_ARG, "file descriptor");
  return chunk_cache_update(c, nullptr, fd, row_capacity, row_lo, row_hi, new_rows_written, chunk_lo, chunk_hi);
}

lcpc_status lcpc_pos_chunk_cache_tree(const lcpc_pos_chunk_cache *c, uint8_t *digests, uint8_t *tree) {
  if (!c) return fail(LCPC_ERR_INVALID_ARG, "null cache");
  Device *dev = c->dev;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const size_t enc = c->enc;
  DBuf hashes;
  HIP_TRY(hashes.alloc(dev, (2 * enc - 1) * 32));
  HIP_TRY(leaves_fold_cvs(c->cvs.as<uint32_t>(), enc, c->n_chunks, hashes.as<uint8_t>(), s));
  if (tree) {
    HIP_TRY(merkle_tree(hashes.as<uint8_t>(), enc, s));
    HIP_TRY(hipMemcpyAsync(tree, hashes.p, (2 * enc - 1) * 32, hipMemcpyDeviceToHost, s));
  }
  if (digests) HIP_TRY(hipMemcpyAsync(digests, hashes.p, enc * 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LCPC_OK;
}

lcpc_status lcpc_leaves_fold_cvs(const uint8_t *cvs, size_t n_chunks, size_t n_cols, uint8_t *leaves,
                                 uint8_t *cvs_after) {
  if ((!cvs || !leaves) && n_cols) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (n_chunks == 0) return fail(LCPC_ERR_INVALID_ARG, "n_chunks");
  if (!n_cols) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf dc, dl;
  if ((st = upload(dev, dc, cvs, n_chunks * n_cols * 32))) return st;
  HIP_TRY(dl.alloc(dev, n_cols * 32));
  HIP_TRY(leaves_fold_cvs(dc.as<uint32_t>(), n_cols, n_chunks, dl.as<uint8_t>(), lease.s));
  HIP_TRY(hipMemcpyAsync(leaves, dl.p, n_cols * 32, hipMemcpyDeviceToHost, lease.s));
  if (cvs_after) HIP_TRY(hipMemcpyAsync(cvs_after, dc.p, n_chunks * n_cols * 32, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

}  // extern "C"

// ColumnDigestAccumulator<Blake3, F> with ColumnsToCareAbout::All (column_digest_accumulator.rs:
// 17-118): encoded rows pushed one batch at a time; every column's message is the 32 zero bytes
// then the repr of its elements, hashed in 1-KiB BLAKE3 chunks on the GPU as soon as a chunk is
// complete and the message is known to continue past it (so no chunk is hashed as the only one).
struct lcpc_column_digests {
  Device *dev = nullptr;
  int fid = 0;
  size_t width = 0, chunks_done = 0, rows_in = 0, batch_rows = 0;
  std::vector<uint64_t> pend;  // rows from leaf_chunk_first_row(chunks_done) on
  std::vector<uint8_t> cvs;    // [chunk][column] chaining values of the chunks done
  bool finalized = false;
};

namespace {

constexpr size_t ACC_BATCH_BYTES = (size_t)256 << 20;  // default rows per GPU pass: about this much input

// hash chunks [a->chunks_done, c_end) of messages n_rows_cv rows long (exact, or any count past
// the covered rows while the message continues) from the pending rows
lcpc_status acc_run(lcpc_column_digests *a, size_t c_end, size_t n_rows_cv) {
  if (c_end <= a->chunks_done) return LCPC_OK;
  const int fid = a->fid;
  const size_t nl = (size_t)field_bytes(fid) / 8, w = a->width;
  const size_t r0 = lcpc_leaf_chunk_first_row((lcpc_field)fid, a->chunks_done);
  const size_t r1 = std::min(a->rows_in, lcpc_leaf_chunk_first_row((lcpc_field)fid, c_end));
  Lease lease(a->dev);
  HIP_TRY(hipSetDevice(a->dev->id));
  DBuf drows, dcv;
  lcpc_status st;
  if ((st = upload(a->dev, drows, a->pend.data(), (r1 - r0) * w * nl * 8))) return st;
  HIP_TRY(dcv.alloc(a->dev, (c_end - a->chunks_done) * w * 32));
  HIP_TRY(leaf_chunk_cvs(fid, drows.as<uint32_t>(), r0, n_rows_cv, w, w, a->chunks_done, c_end,
                         dcv.as<uint32_t>(), lease.s));
  const size_t off = a->cvs.size();
  a->cvs.resize(off + (c_end - a->chunks_done) * w * 32);
  HIP_TRY(hipMemcpyAsync(a->cvs.data() + off, dcv.p, (c_end - a->chunks_done) * w * 32, hipMemcpyDeviceToHost,
                         lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  a->pend.erase(a->pend.begin(), a->pend.begin() + (r1 - r0) * w * nl);
  a->chunks_done = c_end;
  return LCPC_OK;
}

}  // namespace

extern "C" {

lcpc_status lcpc_column_digests_new(lcpc_field f, size_t width, size_t batch_rows, lcpc_column_digests **out) {
  if (!out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (!valid_field(f) || !field_gpu_supported(f)) return fail(LCPC_ERR_UNSUPPORTED, "field");
  if (992 % field_bytes(f)) return fail(LCPC_ERR_UNSUPPORTED, "elements that straddle BLAKE3 chunks (Ft191)");
  if (!width) return fail(LCPC_ERR_INVALID_ARG, "width must be > 0");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  auto a = std::make_unique<lcpc_column_digests>();
  a->dev = dev;
  a->fid = f;
  a->width = width;
  a->batch_rows = batch_rows ? batch_rows : std::max<size_t>(1, ACC_BATCH_BYTES / (width * field_bytes(f)));
  *out = a.release();
  return LCPC_OK;
}

void lcpc_column_digests_free(lcpc_column_digests *a) { delete a; }

size_t lcpc_column_digests_width(const lcpc_column_digests *a) { return a ? a->width : 0; }

lcpc_status lcpc_column_digests_update(lcpc_column_digests *a, const uint64_t *rows, size_t n_rows) {
  // update (:62-87), for n_rows encoded rows of `width` elements at once
  if (!a || (!rows && n_rows)) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (a->finalized) return fail(LCPC_ERR_INVALID_ARG, "accumulator already finalized");
  const size_t nl = (size_t)field_bytes(a->fid) / 8, w = a->width;
  a->pend.insert(a->pend.end(), rows, rows + n_rows * w * nl);
  a->rows_in += n_rows;
  // chunks that end at or before the last row but one: complete, and not their column's last
  size_t c_end = a->chunks_done;
  while (lcpc_leaf_chunk_first_row((lcpc_field)a->fid, c_end + 1) < a->rows_in) c_end++;
  const size_t r0 = lcpc_leaf_chunk_first_row((lcpc_field)a->fid, a->chunks_done);
  if (lcpc_leaf_chunk_first_row((lcpc_field)a->fid, c_end) - r0 < a->batch_rows) return LCPC_OK;  // keep buffering
  return acc_run(a, c_end, a->rows_in);
}

lcpc_status lcpc_column_digests_finalize(lcpc_column_digests *a, uint8_t *digests, uint8_t *tree) {
  // get_column_digests (:89-96) into digests (width x 32 B), and / or finalize_to_merkle_tree
  // (:109-118) into tree (MerkleTree::to_bytes: 2 width - 1 digests, root last; width a power
  // of two >= 2, MerkleTree::new's requirement); either may be NULL
  if (!a) return fail(LCPC_ERR_INVALID_ARG, "null accumulator");
  if (a->finalized) return fail(LCPC_ERR_INVALID_ARG, "accumulator already finalized");
  const size_t w = a->width;
  if (tree && (w < 2 || (w & (w - 1)))) return fail(LCPC_ERR_INVALID_ARG, "Input needs to be a power of two, at least two.");
  // With no rows pushed every column's message is the 32-byte zero prefix alone: one chunk of one
  // 32-byte block with ROOT, so each digest is BLAKE3(32 zero bytes), as the reference's untouched
  // hashers give.  acc_run covers it: its upload of zero rows is an allocation only and the chunk
  // kernel loads no element of a zero-row message.
  const size_t n_chunks = leaf_n_chunks(a->fid, a->rows_in);
  lcpc_status st = acc_run(a, n_chunks, a->rows_in);
  if (st) return st;
  a->finalized = true;
  Lease lease(a->dev);
  HIP_TRY(hipSetDevice(a->dev->id));
  DBuf dc, hashes;
  if ((st = upload(a->dev, dc, a->cvs.data(), a->cvs.size()))) return st;
  HIP_TRY(hashes.alloc(a->dev, (2 * w - 1) * 32));
  HIP_TRY(leaves_from_cvs(dc.as<uint32_t>(), w, (int)n_chunks, hashes.as<uint8_t>(), lease.s));
  if (tree) {
    HIP_TRY(merkle_tree(hashes.as<uint8_t>(), w, lease.s));
    HIP_TRY(hipMemcpyAsync(tree, hashes.p, (2 * w - 1) * 32, hipMemcpyDeviceToHost, lease.s));
  }
  if (digests) HIP_TRY(hipMemcpyAsync(digests, hashes.p, w * 32, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

}  // extern "C"

