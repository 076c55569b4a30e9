// selftest_field.hip -- the primitives of field.hpp and the Ft127 digit recombination of
// collapse_mfma.hpp, one call per thread, raw words in and raw words out.
//
// The product reaches these functions only through whole pipelines (encode, commit, collapse),
// whose data is random: a carry fold dropped where fips_free_mask should have kept it, a lazy
// residue that leaves [0, 2p), a digit accumulator near 2^27 show only on operands chosen for
// them.  These entries let a test choose the operands (tests/test_gpu_field_ops.py, against
// Python integers).  The kernels call the functions the product's kernels call; nothing is
// restated here, and no value is range-checked: the caller owns the domain.
#include "collapse_mfma.hpp"
#include "host_internal.hpp"

namespace lcpc_host {
namespace {

constexpr int DOT_KMAX_ALL = 8;  // the largest fe_dot_kmax of any field (Ft253_192)

int dot_kmax(int fid) {
  return dispatch_field(fid, []<class F>() { return fe_dot_kmax<F>(); });
}

// elements of a / of b that one output reads
int a_per_out(int op, int k) { return op == LCPC_SELFTEST_MUL_SUB_LAZY ? 2 : op == LCPC_SELFTEST_DOT ? k : 1; }
int b_per_out(int fid, int op, int k) {
  return op == LCPC_SELFTEST_DOT ? k : op == LCPC_SELFTEST_MUL_TW ? field_words(fid) : 1;
}
bool unary(int op) {
  switch (op) {
    case LCPC_SELFTEST_REDUCE_2P:
    case LCPC_SELFTEST_SQR:
    case LCPC_SELFTEST_FROM_MONT:
    case LCPC_SELFTEST_FROM_MONT_GENERIC:
    case LCPC_SELFTEST_TO_MONT:
    case LCPC_SELFTEST_REPR_WORDS:
    case LCPC_SELFTEST_CANON_REPR_WORDS:
    case LCPC_SELFTEST_IS_CANONICAL:
    case LCPC_SELFTEST_BALANCED_DIGITS: return true;
    default: return false;
  }
}

template <class F, int OP, int K>
__global__ __launch_bounds__(256) void k_field_op(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                  uint32_t *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<F> r = fe_zero<F>();
  if constexpr (OP == LCPC_SELFTEST_ADD) {
    r = fe_add<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_SUB) {
    r = fe_sub<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_ADD_2P) {
    r = fe_add_2p<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_SUB_2P) {
    r = fe_sub_2p<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_REDUCE_2P) {
    r = fe_reduce_2p<F>(fe_load<F>(a, i));
  } else if constexpr (OP == LCPC_SELFTEST_SUB_LAZY) {
    r = fe_sub_lazy<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_MUL_SUB_LAZY) {
    r = fe_mul<F>(fe_sub_lazy<F>(fe_load<F>(a, 2 * i), fe_load<F>(a, 2 * i + 1)), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_MUL) {
    r = fe_mul<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_MUL_CIOS) {
    r = fe_mul_cios<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_SQR) {
    r = fe_sqr<F>(fe_load<F>(a, i));
  } else if constexpr (OP == LCPC_SELFTEST_MUL_LAZY) {
    r = fe_mul_lazy<F>(fe_load<F>(a, i), fe_load<F>(b, i));
  } else if constexpr (OP == LCPC_SELFTEST_DOT) {
    Fe<F> x[K], w[K];
#pragma unroll
    for (int q = 0; q < K; q++) {
      x[q] = fe_load<F>(a, i * K + q);
      w[q] = fe_load<F>(b, i * K + q);
    }
    r = fe_dot<F, K>(x, w);
  } else if constexpr (OP == LCPC_SELFTEST_FROM_MONT) {
    r = fe_from_mont<F>(fe_load<F>(a, i));
  } else if constexpr (OP == LCPC_SELFTEST_FROM_MONT_GENERIC) {
    r = fe_from_mont_generic<F>(fe_load<F>(a, i));
  } else if constexpr (OP == LCPC_SELFTEST_TO_MONT) {
    r = fe_to_mont<F>(fe_load<F>(a, i));
  } else if constexpr (OP == LCPC_SELFTEST_REPR_WORDS) {
    fe_repr_words<F>(fe_load<F>(a, i), r.v);
  } else if constexpr (OP == LCPC_SELFTEST_CANON_REPR_WORDS) {
    fe_canon_repr_words<F>(fe_load<F>(a, i), r.v);
  } else if constexpr (OP == LCPC_SELFTEST_IS_CANONICAL) {
    r.v[0] = fe_is_canonical<F>(fe_load<F>(a, i)) ? 1u : 0u;
  } else if constexpr (OP == LCPC_SELFTEST_POW) {
    const Fe<F> e = fe_load<F>(b, i);
    r = fe_pow<F>(fe_load<F>(a, i), (uint64_t)e.v[0] | ((uint64_t)e.v[1] << 32));
  } else if constexpr (OP == LCPC_SELFTEST_MUL_TW) {
    if constexpr (F::ID == 1) {
      Fe<F> W[F::N];
#pragma unroll
      for (int q = 0; q < F::N; q++) W[q] = fe_load<F>(b, i * F::N + q);
      r = fe_mul_tw<F>(fe_load<F>(a, i), W);
    }
  } else if constexpr (OP == LCPC_SELFTEST_BALANCED_DIGITS) {
    if constexpr (F::N == 4) {
      const Fe<F> x = fe_load<F>(a, i);
      const cmfma::v4i d = cmfma::balanced_digits(x.v[0], x.v[1], x.v[2], x.v[3]);
      r.v[0] = (uint32_t)d.x;
      r.v[1] = (uint32_t)d.y;
      r.v[2] = (uint32_t)d.z;
      r.v[3] = (uint32_t)d.w;
    }
  }
  fe_store<F>(out, i, r);
}

__global__ __launch_bounds__(256) void k_recombine(const int *__restrict__ y, uint32_t *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int Y[16];
#pragma unroll
  for (int u = 0; u < 16; u++) Y[u] = y[i * 16 + u];
  fe_store<Ft127>(out, i, cmfma::recombine_redc<Ft127>(Y));
}

template <class F, int OP, int K = 1>
hipError_t launch(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n, hipStream_t s) {
  hipLaunchKernelGGL((k_field_op<F, OP, K>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, out, n);
  return hipGetLastError();
}

template <class F, int K>
hipError_t launch_dot(int k, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n, hipStream_t s) {
  if constexpr (K > fe_dot_kmax<F>()) {
    return hipErrorInvalidValue;
  } else {
    if (k == K) return launch<F, LCPC_SELFTEST_DOT, K>(a, b, out, n, s);
    return launch_dot<F, K + 1>(k, a, b, out, n, s);
  }
}

template <class F, int OP>
hipError_t launch_op(int op, int k, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n, hipStream_t s) {
  if constexpr (OP >= LCPC_SELFTEST_N_OPS) {
    return hipErrorInvalidValue;
  } else {
    if (op != OP) return launch_op<F, OP + 1>(op, k, a, b, out, n, s);
    if constexpr (OP == LCPC_SELFTEST_DOT)
      return launch_dot<F, 1>(k, a, b, out, n, s);
    else
      return launch<F, OP>(a, b, out, n, s);
  }
}

}  // namespace
}  // namespace lcpc_host

using namespace lcpc_host;

extern "C" int lcpc_selftest_fe_dot_kmax(lcpc_field f) { return valid_field(f) ? dot_kmax(f) : 0; }

extern "C" lcpc_status lcpc_selftest_field_op(lcpc_field f, int op, int k, const uint64_t *a, const uint64_t *b,
                                              uint64_t *out, size_t n) {
  static_assert(DOT_KMAX_ALL >= fe_dot_kmax<Ft63>() && DOT_KMAX_ALL >= fe_dot_kmax<Ft127>() &&
                    DOT_KMAX_ALL >= fe_dot_kmax<Ft191>() && DOT_KMAX_ALL >= fe_dot_kmax<Ft255>() &&
                    DOT_KMAX_ALL >= fe_dot_kmax<Ft253_192>(),
                "launch_dot's range");
  if (!valid_field(f)) return fail(LCPC_ERR_INVALID_ARG, "field");
  if (op < 0 || op >= LCPC_SELFTEST_N_OPS) return fail(LCPC_ERR_INVALID_ARG, "op");
  if (op == LCPC_SELFTEST_BALANCED_DIGITS && f != LCPC_FT127) return fail(LCPC_ERR_INVALID_ARG, "balanced_digits: Ft127");
  if (op == LCPC_SELFTEST_MUL_TW && f != LCPC_FT127) return fail(LCPC_ERR_INVALID_ARG, "mul_tw: Ft127");
  if (k < 1 || k > dot_kmax(f)) return fail(LCPC_ERR_INVALID_ARG, "k outside [1, fe_dot_kmax]");
  if (!a || !out || (!b && !unary(op))) return fail(LCPC_ERR_INVALID_ARG, "null operand or output");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  if (!n) return LCPC_OK;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const size_t wb = field_bytes(f);
  DBuf da, db, dout;
  if ((st = upload(dev, da, a, n * a_per_out(op, k) * wb))) return st;
  if (!unary(op) && (st = upload(dev, db, b, n * b_per_out(f, op, k) * wb))) return st;
  HIP_TRY(dout.alloc(dev, n * wb));
  HIP_TRY(dispatch_field(f, [&]<class F>() {
    return launch_op<F, 0>(op, k, da.as<uint32_t>(), db.as<uint32_t>(), dout.as<uint32_t>(), n, lease.s);
  }));
  HIP_TRY(hipMemcpyAsync(out, dout.p, n * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

extern "C" lcpc_status lcpc_selftest_recombine(const int32_t *y, uint64_t *out, size_t n) {
  if (!y || !out) return fail(LCPC_ERR_INVALID_ARG, "null accumulators or output");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  if (!n) return LCPC_OK;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  DBuf dy, dout;
  if ((st = upload(dev, dy, y, n * 16 * sizeof(int32_t)))) return st;
  HIP_TRY(dout.alloc(dev, n * 16));
  hipLaunchKernelGGL(k_recombine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, lease.s, dy.as<int>(),
                     dout.as<uint32_t>(), n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, dout.p, n * 16, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

extern "C" lcpc_status lcpc_selftest_twiddle_words(lcpc_field f, const uint64_t *tw, uint64_t *out, size_t n) {
  if (f != LCPC_FT127) return fail(LCPC_ERR_INVALID_ARG, "twiddle_words: Ft127");
  if (!tw || !out) return fail(LCPC_ERR_INVALID_ARG, "null twiddles or output");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  if (!n) return LCPC_OK;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const size_t wb = field_bytes(f), nw = (size_t)field_words(f);
  DBuf dtw, dout;
  if ((st = upload(dev, dtw, tw, n * wb))) return st;
  HIP_TRY(dout.alloc(dev, n * nw * wb));
  HIP_TRY(lcpc::ntt_tw4_table(f, dtw.as<uint32_t>(), 1, n, dout.as<uint32_t>(), lease.s));
  HIP_TRY(hipMemcpyAsync(out, dout.p, n * nw * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}
