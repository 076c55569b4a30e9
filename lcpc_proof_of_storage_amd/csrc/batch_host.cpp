// batch_host.cpp -- batched evaluation proofs: one commitment opened at n_evals points.
//
// The degree tests run once, every evaluation vector is absorbed, and only then are the columns
// drawn, so one set of column openings checks all of them.  Every claim is fixed before the
// column challenge, so a false p_eval_j survives the openings with the probability it has in a
// single proof.  NO COUNTERPART IN THE REFERENCE (its prove / verify, lcpc-2d/src/lib.rs:862-982
// and :1034-1123, take one outer tensor); with n_evals = 1 the proof parts and the transcript are
// those of lcpc_prove / lcpc_verify.
#include "host_internal.hpp"

static_assert(LCPC_BATCH_MAX_TENSORS == COLLAPSE_MANY_MAX_TENSORS, "header bound = kernel bound");

int lcpc_collapse_many_chunk(lcpc_field f) { return valid_field(f) ? collapse_many_chunk(f) : 0; }

lcpc_status lcpc_collapse_columns_many(lcpc_field f, const uint64_t *coeffs, size_t n_rows, size_t n_per_row,
                                       const uint64_t *tensors, size_t n_tensors, uint64_t *out) {
  if (!valid_field(f)) return fail(LCPC_ERR_INVALID_ARG, "field");
  if (n_tensors == 0 || n_tensors > LCPC_BATCH_MAX_TENSORS)
    return fail(LCPC_ERR_INVALID_ARG, "n_tensors must be in [1, LCPC_BATCH_MAX_TENSORS]");
  if (!coeffs || !tensors || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const int wb = field_bytes(f);
  DBuf dc, dt, dp, scratch;
  if ((st = upload(dev, dc, coeffs, n_rows * n_per_row * wb))) return st;
  if ((st = upload(dev, dt, tensors, n_tensors * n_rows * wb))) return st;
  HIP_TRY(dp.alloc(dev, n_tensors * n_per_row * wb));
  HIP_TRY(scratch.alloc(dev, collapse_many_scratch_bytes(f, n_rows, n_per_row, n_tensors)));
  HIP_TRY(collapse_rows_many(f, dc.as<uint32_t>(), n_rows, n_per_row, dt.as<uint32_t>(), n_tensors,
                             dp.as<uint32_t>(), scratch.p, lease.s));
  HIP_TRY(hipMemcpyAsync(out, dp.p, n_tensors * n_per_row * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

lcpc_status lcpc_prove_batch(const lcpc_commit *c, const uint64_t *outers, size_t n_evals, size_t outer_len,
                             const lcpc_encoding *e, lcpc_transcript *tr, lcpc_batch_proof **out) {
  prof::HostScope hs_total("host_prove_batch_total");
  if (!c || !e || !tr || !out) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (n_evals == 0 || n_evals > LCPC_BATCH_MAX_TENSORS)
    return fail(LCPC_ERR_INVALID_ARG, "n_evals must be in [1, LCPC_BATCH_MAX_TENSORS]");
  lcpc_status st = lcpc_check_comm(c, e);
  if (st) return st;
  if (outer_len != c->n_rows || !outers) return fail(LCPC_PROVER_OUTER_TENSOR, "ProverError::OuterTensor");
  Device *dev = c->dev;
  Lease lease(dev, POOL_PROVER);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;
  const int fid = c->fid, wb = field_bytes(fid), limbs = wb / 8;
  const size_t nr = c->n_rows, np = c->n_per_row, ndt = e->n_degree_tests, nco = e->n_col_opens, m = n_evals;
  auto p = std::make_unique<lcpc_batch_proof>();
  p->fid = fid;
  p->n_cols = c->n_cols;
  p->n_per_row = np;
  p->n_rows = nr;
  p->ndt = ndt;
  p->nco = nco;
  p->path_len = log2_np2(c->n_cols);
  p->n_evals = m;
  p->p_random.resize(ndt * np * limbs);
  p->p_evals.resize(m * np * limbs);
  uint8_t *h_prand = (uint8_t *)p->p_random.data();
  uint8_t *h_tens = (uint8_t *)t_pin[PIN_TENSOR].get(nr * wb);
  uint8_t *h_erepr = (uint8_t *)t_pin[PIN_PEVAL].get(m * np * wb);
  if (!h_tens || !h_erepr) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");

  // The outer tensors are known now: all m row combinations, their copy into the proof and their
  // canonical bytes are queued ahead of the first degree test, whose GPU round trip they share.
  // The absorption of the m vectors below is then host work alone.
  DBuf douters, devals, ecanon, mscratch;
  if ((st = upload(dev, douters, outers, m * nr * wb))) return st;
  HIP_TRY(devals.alloc(dev, m * np * wb));
  HIP_TRY(mscratch.alloc(dev, collapse_many_scratch_bytes(fid, nr, np, m)));
  HIP_TRY(collapse_rows_many(fid, c->coeffs.as<uint32_t>(), nr, np, douters.as<uint32_t>(), m,
                             devals.as<uint32_t>(), mscratch.p, s));
  HIP_TRY(d2h(p->p_evals.data(), devals.p, m * np * wb, s));
  if (void *hd = host_dev_ptr(h_erepr)) {
    HIP_TRY(convert(fid, devals.as<uint32_t>(), (uint32_t *)hd, m * np, false, s));
  } else {
    HIP_TRY(ecanon.alloc(dev, m * np * wb));
    HIP_TRY(convert(fid, devals.as<uint32_t>(), ecanon.as<uint32_t>(), m * np, false, s));
    HIP_TRY(hipMemcpyAsync(h_erepr, ecanon.p, m * np * wb, hipMemcpyDeviceToHost, s));
  }

  // degree tests, as lcpc_prove runs them (lib.rs:1056-1083)
  DBuf dtens, dres, scratch;
  HIP_TRY(dtens.alloc(dev, nr * wb));
  HIP_TRY(dres.alloc(dev, np * wb));
  HIP_TRY(scratch.alloc(dev, collapse_scratch_bytes(fid, nr, np, 1)));
  std::vector<uint64_t> tensor;
  const uint8_t *repr = nullptr;
  for (size_t i = 0; i < ndt; i++) {
    challenge_tensor(*tr, fid, nr, tensor);
    if ((st = transcript_status(tr))) return st;
    std::memcpy(h_tens, tensor.data(), nr * wb);
    HIP_TRY(h2d(dtens.p, h_tens, nr * wb, s));
    HIP_TRY(collapse_rows(fid, c->coeffs.as<uint32_t>(), nr, np, dtens.as<uint32_t>(), 1, dres.as<uint32_t>(),
                          scratch.p, s));
    HIP_TRY(d2h(h_prand + i * np * wb, dres.p, np * wb, s));
    if ((st = to_repr_host(dev, fid, dres.as<uint32_t>(), np, &repr))) return st;  // syncs the stream
    tr->append_messages(LABEL_PR, 6, repr, wb, np);
    if ((st = transcript_status(tr))) return st;
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (fid == LCPC_FT253_192)  // big-endian repr, as to_repr_host
    for (size_t i = 0; i < m * np; i++) std::reverse(h_erepr + i * wb, h_erepr + (i + 1) * wb);
  for (size_t j = 0; j < m; j++) {
    tr->append_messages(LABEL_PE, 6, h_erepr + j * np * wb, wb, np);
    if ((st = transcript_status(tr))) return st;
  }

  // columns, drawn after every evaluation vector is fixed (lib.rs:1101-1115)
  challenge_columns(*tr, c->n_cols, nco, p->col_idx);
  if ((st = transcript_status(tr))) return st;
  p->cols.resize(nco * nr * limbs);
  p->paths.resize(nco * p->path_len * 32);
  uint8_t *h_idx = (uint8_t *)t_pin[PIN_PATHS].get(std::max<size_t>(1, nco * 8));
  if (!h_idx) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
  std::memcpy(h_idx, p->col_idx.data(), nco * 8);
  DBuf didx, dcols, dpaths;
  HIP_TRY(didx.alloc(dev, nco * 8));
  if (nco) HIP_TRY(h2d(didx.p, h_idx, nco * 8, s));
  HIP_TRY(dcols.alloc(dev, nco * nr * wb));
  HIP_TRY(dpaths.alloc(dev, nco * p->path_len * 32));
  HIP_TRY(gather_columns(fid, c->comm.as<uint32_t>(), nr, c->n_cols, didx.as<uint64_t>(), nco, dcols.as<uint32_t>(),
                         s, c->col_major, c->canon));
  HIP_TRY(gather_paths(c->hashes.as<uint8_t>(), c->n_hashes, didx.as<uint64_t>(), nco, p->path_len,
                       dpaths.as<uint8_t>(), s));
  if (nco) {
    HIP_TRY(d2h(p->cols.data(), dcols.p, nco * nr * wb, s));
    if (p->path_len) HIP_TRY(d2h(p->paths.data(), dpaths.p, nco * p->path_len * 32, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  *out = p.release();
  return LCPC_OK;
}

void lcpc_batch_proof_free(lcpc_batch_proof *p) { delete p; }
size_t lcpc_batch_proof_n_evals(const lcpc_batch_proof *p) { return p->n_evals; }
size_t lcpc_batch_proof_n_cols(const lcpc_batch_proof *p) { return p->n_cols; }
size_t lcpc_batch_proof_n_per_row(const lcpc_batch_proof *p) { return p->n_per_row; }
size_t lcpc_batch_proof_n_rows(const lcpc_batch_proof *p) { return p->n_rows; }
size_t lcpc_batch_proof_n_degree_tests(const lcpc_batch_proof *p) { return p->ndt; }
size_t lcpc_batch_proof_n_col_opens(const lcpc_batch_proof *p) { return p->nco; }
size_t lcpc_batch_proof_path_len(const lcpc_batch_proof *p) { return p->path_len; }
lcpc_field lcpc_batch_proof_field(const lcpc_batch_proof *p) { return (lcpc_field)p->fid; }

lcpc_status lcpc_batch_proof_copy_p_eval(const lcpc_batch_proof *p, size_t j, uint64_t *out) {
  if (j >= p->n_evals) return fail(LCPC_ERR_INVALID_ARG, "evaluation index");
  const size_t n = p->n_per_row * (field_bytes(p->fid) / 8);
  std::memcpy(out, p->p_evals.data() + j * n, n * 8);
  return LCPC_OK;
}
lcpc_status lcpc_batch_proof_copy_p_random(const lcpc_batch_proof *p, size_t i, uint64_t *out) {
  if (i >= p->ndt) return fail(LCPC_ERR_INVALID_ARG, "degree test index");
  const size_t n = p->n_per_row * (field_bytes(p->fid) / 8);
  std::memcpy(out, p->p_random.data() + i * n, n * 8);
  return LCPC_OK;
}
lcpc_status lcpc_batch_proof_copy_column(const lcpc_batch_proof *p, size_t k, uint64_t *col, uint8_t *path) {
  if (k >= p->nco) return fail(LCPC_ERR_INVALID_ARG, "column index");
  const size_t n = p->n_rows * (field_bytes(p->fid) / 8);
  if (col) std::memcpy(col, p->cols.data() + k * n, n * 8);
  if (path && p->path_len) std::memcpy(path, p->paths.data() + k * p->path_len * 32, p->path_len * 32);
  return LCPC_OK;
}

lcpc_status lcpc_batch_proof_from_parts(lcpc_field f, size_t n_cols, size_t n_per_row, size_t n_rows, size_t ndt,
                                        size_t nco, size_t path_len, size_t n_evals, const uint64_t *p_evals,
                                        const uint64_t *p_random, const uint64_t *cols, const uint8_t *paths,
                                        lcpc_batch_proof **out) {
  if (!valid_field(f) || !out) return fail(LCPC_ERR_INVALID_ARG, "field / out");
  if (n_evals == 0 || n_evals > LCPC_BATCH_MAX_TENSORS || !p_evals)
    return fail(LCPC_ERR_INVALID_ARG, "n_evals must be in [1, LCPC_BATCH_MAX_TENSORS]");
  auto p = std::make_unique<lcpc_batch_proof>();
  const size_t limbs = field_info(f).limbs;
  p->fid = f;
  p->n_cols = n_cols;
  p->n_per_row = n_per_row;
  p->n_rows = n_rows;
  p->ndt = ndt;
  p->nco = nco;
  p->path_len = path_len;
  p->n_evals = n_evals;
  p->p_evals.assign(p_evals, p_evals + n_evals * n_per_row * limbs);
  if (ndt) p->p_random.assign(p_random, p_random + ndt * n_per_row * limbs);
  if (nco) p->cols.assign(cols, cols + nco * n_rows * limbs);
  if (nco && path_len) p->paths.assign(paths, paths + nco * path_len * 32);
  *out = p.release();
  return LCPC_OK;
}

lcpc_status lcpc_verify_batch(const uint8_t root[32], const uint64_t *outers, size_t n_evals, size_t outer_len,
                              const uint64_t *inners, size_t inner_len, const lcpc_batch_proof *p,
                              const lcpc_encoding *e, lcpc_transcript *tr, uint64_t *evals_out) {
  if (!root || !p || !e || !tr || !outers || !inners) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (n_evals == 0 || n_evals > LCPC_BATCH_MAX_TENSORS)
    return fail(LCPC_ERR_INVALID_ARG, "n_evals must be in [1, LCPC_BATCH_MAX_TENSORS]");
  const size_t nco = e->n_col_opens, m = n_evals;
  if (nco != p->nco || nco == 0) return fail(LCPC_VERIFIER_NUM_COL_OPENS, "VerifierError::NumColOpens");
  const size_t nr = p->n_rows, nc = p->n_cols, np = p->n_per_row;
  if (inner_len != np) return fail(LCPC_VERIFIER_INNER_TENSOR, "VerifierError::InnerTensor");
  if (outer_len != nr) return fail(LCPC_VERIFIER_OUTER_TENSOR, "VerifierError::OuterTensor");
  if (p->n_evals != m)
    return fail(LCPC_VERIFIER_OUTER_TENSOR, "VerifierError::OuterTensor: the proof holds " +
                                                std::to_string(p->n_evals) + " evaluations, the call " +
                                                std::to_string(m));
  if (encoding_dims_ok(e, np, nc) != LCPC_OK || p->fid != e->fid)
    return fail(LCPC_VERIFIER_ENCODING_DIMS, "VerifierError::EncodingDims");
  const size_t ndt = e->n_degree_tests, nt = ndt + m;
  if (p->ndt != ndt) return fail(LCPC_VERIFIER_ENCODING_DIMS, "proof has a different number of degree tests");
  const int fid = e->fid, wb = field_bytes(fid), limbs = wb / 8;
  Device *dev = e->dev;
  Lease lease(dev, POOL_HIGH);
  HIP_TRY(hipSetDevice(dev->id));
  hipStream_t s = lease.s;

  // rows [p_random (ndt) | p_eval (m)] of n_per_row elements: one encode and one conversion to
  // repr bytes for all of them (neither depends on the transcript)
  DBuf dtens, denc, dvec, didx, dcols, dpaths, dleaves, dflags, dpflags, scratch, dinner, dout, droot;
  HIP_TRY(dvec.alloc(dev, nt * np * wb));
  HIP_TRY(denc.alloc(dev, nt * nc * wb));
  HIP_TRY(h2d(dvec.p, p->p_random.data(), ndt * np * wb, s));
  HIP_TRY(h2d(dvec.as<uint8_t>() + ndt * np * wb, p->p_evals.data(), m * np * wb, s));
  lcpc_status st = encode_rows_any(e, dvec.as<uint32_t>(), np, np, denc.as<uint32_t>(), nc, nt, s);
  if (st) return st;
  const uint8_t *repr = nullptr;
  if ((st = to_repr_host(dev, fid, dvec.as<uint32_t>(), nt * np, &repr))) return st;
  std::vector<uint64_t> tensor, tensors(ndt * nr * limbs);
  for (size_t i = 0; i < ndt; i++) {
    challenge_tensor(*tr, fid, nr, tensor);
    std::memcpy(tensors.data() + i * nr * limbs, tensor.data(), nr * wb);
    tr->append_messages(LABEL_PR, 6, repr + i * np * wb, wb, np);
    if ((st = transcript_status(tr))) return st;
  }
  for (size_t j = 0; j < m; j++) {
    tr->append_messages(LABEL_PE, 6, repr + (ndt + j) * np * wb, wb, np);
    if ((st = transcript_status(tr))) return st;
  }
  std::vector<uint64_t> idx;
  challenge_columns(*tr, nc, nco, idx);
  if ((st = transcript_status(tr))) return st;

  // tensors [degree tests (ndt) | outers (m)], one column_checks launch over all of them
  HIP_TRY(dtens.alloc(dev, nt * nr * wb));
  if (ndt) HIP_TRY(hipMemcpyAsync(dtens.p, tensors.data(), ndt * nr * wb, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(dtens.as<uint8_t>() + ndt * nr * wb, outers, m * nr * wb, hipMemcpyHostToDevice, s));
  if ((st = upload(dev, didx, idx.data(), nco * 8))) return st;
  if ((st = upload(dev, dcols, p->cols.data(), nco * nr * wb))) return st;
  if ((st = upload(dev, dpaths, p->paths.data(), nco * p->path_len * 32))) return st;
  if ((st = upload(dev, droot, root, 32))) return st;
  HIP_TRY(dflags.alloc(dev, nco * nt * 4));
  HIP_TRY(dpflags.alloc(dev, nco * 4));
  HIP_TRY(dleaves.alloc(dev, nco * 32));
  HIP_TRY(scratch.alloc(dev, leaf_hash_scratch_bytes(fid, nr, nco)));
  HIP_TRY(column_checks(fid, dcols.as<uint32_t>(), nco, nr, dtens.as<uint32_t>(), (int)nt, denc.as<uint32_t>(), nc,
                        didx.as<uint64_t>(), dflags.as<uint32_t>(), s));
  HIP_TRY(leaf_hashes_cols_d(e->digest, fid, dcols.as<uint32_t>(), nr, nco, dleaves.as<uint8_t>(), scratch.p, s));
  HIP_TRY(path_checks_d(e->digest, dleaves.as<uint8_t>(), dpaths.as<uint8_t>(), nco, p->path_len,
                        didx.as<uint64_t>(), droot.as<uint8_t>(), dpflags.as<uint32_t>(), s));
  std::vector<uint32_t> flags(nco * nt), pflags(nco);
  HIP_TRY(hipMemcpyAsync(flags.data(), dflags.p, flags.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(pflags.data(), dpflags.p, pflags.size() * 4, hipMemcpyDeviceToHost, s));
  // final inner products <inner_j, p_eval_j> (lib.rs:977-981): one workgroup per evaluation
  if ((st = upload(dev, dinner, inners, m * np * wb))) return st;
  HIP_TRY(dout.alloc(dev, m * wb));
  HIP_TRY(dot_many(fid, dinner.as<uint32_t>(), dvec.as<uint32_t>() + ndt * np * limbs * 2, np, m,
                   dout.as<uint32_t>(), s));
  std::vector<uint64_t> ev(m * limbs);
  HIP_TRY(hipMemcpyAsync(ev.data(), dout.p, m * wb, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // per column, in the reference's order (lib.rs:953-974): degree tests, evaluations, path
  for (size_t k = 0; k < nco; k++) {
    for (size_t i = 0; i < ndt; i++)
      if (!flags[k * nt + i]) return fail(LCPC_VERIFIER_COLUMN_DEGREE, "VerifierError::ColumnDegree");
    for (size_t j = 0; j < m; j++)
      if (!flags[k * nt + ndt + j])
        return fail(LCPC_VERIFIER_COLUMN_EVAL, "VerifierError::ColumnEval (evaluation " + std::to_string(j) + ")");
    if (!pflags[k]) return fail(LCPC_VERIFIER_COLUMN_PATH, "VerifierError::ColumnPath");
  }
  if (evals_out) std::memcpy(evals_out, ev.data(), m * wb);
  return LCPC_OK;
}

lcpc_status lcpc_prove_batch_ops(const lcpc_commit *c, const uint64_t *outers, size_t n_evals, size_t outer_len,
                                 const lcpc_encoding *e, const lcpc_transcript_ops *ops, lcpc_batch_proof **out) {
  if (!ops || !ops->append_message || !ops->challenge_bytes)
    return fail(LCPC_ERR_INVALID_ARG, "transcript ops need append_message and challenge_bytes");
  lcpc_transcript tr(*ops);
  return lcpc_prove_batch(c, outers, n_evals, outer_len, e, &tr, out);
}
lcpc_status lcpc_verify_batch_ops(const uint8_t root[32], const uint64_t *outers, size_t n_evals, size_t outer_len,
                                  const uint64_t *inners, size_t inner_len, const lcpc_batch_proof *p,
                                  const lcpc_encoding *e, const lcpc_transcript_ops *ops, uint64_t *evals_out) {
  if (!ops || !ops->append_message || !ops->challenge_bytes)
    return fail(LCPC_ERR_INVALID_ARG, "transcript ops need append_message and challenge_bytes");
  lcpc_transcript tr(*ops);
  return lcpc_verify_batch(root, outers, n_evals, outer_len, inners, inner_len, p, e, &tr, evals_out);
}
