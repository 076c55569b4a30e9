// erasure.hip -- Reed-Solomon erasure decoding around the two NTT directions (no counterpart in
// the reference: its decode_row is a plain ifft_oi and cannot use the code's redundancy).
//
// A row of n evaluations f(x_c) of a polynomial of degree < n_per_row, with the positions E erased
// (|E| <= n - n_per_row).  With L(x) = prod_{j in E} (x - x_j):
//   k_locator      lambda_c = L(x_c) for c not in E, 1 / L'(x_j) for j in E (one-off per call)
//   k_masked_*     g_c = y_c lambda_c (0 at E): the evaluations of P = f L, deg P < n_per_row + |E|
//   (ntt_rows, inverse plan: P's coefficients, bit-reversed and unscaled)
//   k_deriv        p'_k = (k + 1) p_{k+1} / n in natural order -- the closing bitrev_scale of ifft_oi
//                  with the derivative folded in -- and the check that p_k = 0 for
//                  k >= n_per_row + |E| (free redundancy whenever |E| < n - n_per_row)
//   (ntt_rows, forward plan: P'(x_c))
//   k_fill         f(x_j) = P'(x_j) / L'(x_j) for j in E   (P' = f' L + f L' and L(x_j) = 0)
// The evaluation point of codeword position c comes from the forward plan's twiddle table w^e and
// the switches of include/lcpc_fft_convention.h: x_c = w^bitrev(c) for bit-reversed output, w^c
// for natural output (rs_point_index).  Erased positions are never read.
//
//   k_col_canon / k_scrub_status   the damage locator of stored files: a canonicity flag per column
//                  of a column-major slice, then status per column from its digest and its leaf.
#include "field.hpp"
#include "kernels.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

__device__ __forceinline__ size_t bitrev_n(size_t i, int log_n) {
  return log_n ? (size_t)(__builtin_bitreverse64((uint64_t)i) >> (64 - log_n)) : 0;
}
// exponent e with x_c = w^e (w the forward plan's root); an involution on [0, n) either way, and
// also where codeword position c sits in the natural-order input of the inverse plan
__device__ __forceinline__ size_t rs_point_index(size_t c, int log_n) {
#if LCPC_FFT_OUTPUT_BITREV
  return bitrev_n(c, log_n);
#else
  return c;
#endif
}

__global__ __launch_bounds__(256) void k_slot_set(const uint32_t *__restrict__ erased, size_t n_erased,
                                                  int32_t *__restrict__ slot) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_erased) slot[erased[t]] = (int32_t)t;
}

// One thread per evaluation point; the erased points stream through LDS in tiles of 256.
template <class F>
__global__ __launch_bounds__(256) void k_locator(const uint32_t *__restrict__ tw, int log_n,
                                                 const uint32_t *__restrict__ erased, size_t n_erased,
                                                 const int32_t *__restrict__ slot, uint32_t *__restrict__ lambda,
                                                 uint32_t *__restrict__ dinv) {
  __shared__ Fe<F> s_x[256];
  __shared__ uint32_t s_idx[256];
  const int tid = threadIdx.x;
  const size_t n = (size_t)1 << log_n;
  const size_t c = (size_t)blockIdx.x * blockDim.x + tid;
  const bool active = c < n;
  const Fe<F> xc = active ? fe_load<F>(tw, rs_point_index(c, log_n)) : fe_zero<F>();
  Fe<F> acc = fe_one<F>();
  for (size_t base = 0; base < n_erased; base += 256) {
    __syncthreads();
    if (base + tid < n_erased) {
      const uint32_t j = erased[base + tid];
      s_idx[tid] = j;
      s_x[tid] = fe_load<F>(tw, rs_point_index(j, log_n));
    }
    __syncthreads();
    const int m = (int)(n_erased - base < 256 ? n_erased - base : 256);
    if (active) {
      for (int k = 0; k < m; k++)
        if (s_idx[k] != (uint32_t)c) acc = fe_mul<F>(acc, fe_sub<F>(xc, s_x[k]));
    }
  }
  if (!active) return;
  const int32_t sl = slot[c];
  if (sl >= 0) {
    fe_store<F>(dinv, (size_t)sl, fe_inv_fermat<F>(acc));
    fe_store<F>(lambda, c, fe_zero<F>());
  } else {
    fe_store<F>(lambda, c, acc);
  }
}

// dscale[k] = (k + 1) / n (Montgomery), k < n
template <class F>
__global__ __launch_bounds__(256) void k_dscale(Fe<F> inv_n_canon, size_t n, uint32_t *__restrict__ dscale) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  Fe<F> kk = fe_zero<F>();
  kk.v[0] = (uint32_t)(k + 1);  // n <= 2^24
  fe_store<F>(dscale, k, fe_mul<F>(fe_to_mont<F>(inv_n_canon), fe_to_mont<F>(kk)));
}

// out[r][rs_point_index(c)] = in[r][c] * lambda[c], 0 at the erased c (never read)
template <class F>
__global__ __launch_bounds__(256) void k_masked_rows(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                     int log_n, size_t n_rows, const int32_t *__restrict__ slot,
                                                     const uint32_t *__restrict__ lambda) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)1 << log_n;
  if (t >= n * n_rows) return;
  const size_t r = t >> log_n, c = t & (n - 1);
  Fe<F> v = fe_zero<F>();
  if (slot[c] < 0) v = fe_mul<F>(fe_load<F>(in, t), fe_load<F>(lambda, c));
  fe_store<F>(out, r * n + rs_point_index(c, log_n), v);
}

// A column-major batch src[c][r] (c < n, r < B, canonical) to rows: out[r][rs_point_index(c)] =
// mont(src[c][r]) * lambda[c], 0 at the erased c, whose columns are never read; plain (optional)
// gets the unmasked Montgomery rows plain[r][c] (erased positions left for k_fill).  *bad |= 1
// if a column that is read holds an element that is not < p.  32 x 32 tiles in OUTPUT coordinates:
// the loads are runs of 32 rows of one column, the stores runs of 32 adjacent output positions.
template <class F>
__global__ __launch_bounds__(256) void k_masked_cols(const uint32_t *__restrict__ src, size_t B, int log_n,
                                                     uint32_t *__restrict__ out, uint32_t *__restrict__ plain,
                                                     const int32_t *__restrict__ slot,
                                                     const uint32_t *__restrict__ lambda, uint32_t *__restrict__ bad) {
  __shared__ Fe<F> tile[32][33];
  __shared__ Fe<F> ptile[32][33];
  const size_t n = (size_t)1 << log_n;
  const size_t nd = (n + 31) / 32;  // a 1-D grid of tiles: d-tiles fastest
  const size_t d0 = ((size_t)blockIdx.x % nd) * 32, r0 = ((size_t)blockIdx.x / nd) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const size_t d = d0 + i, r = r0 + tx;
    if (d < n && r < B) {
      const size_t c = rs_point_index(d, log_n);
      Fe<F> v = fe_zero<F>(), pv = fe_zero<F>();
      if (slot[c] < 0) {
        const Fe<F> y = fe_load<F>(src, c * B + r);
        if (!fe_is_canonical<F>(y)) {
          *bad = 1;
        } else {
          pv = fe_to_mont<F>(y);
          v = fe_mul<F>(pv, fe_load<F>(lambda, c));
        }
      }
      tile[i][tx] = v;
      if (plain) ptile[i][tx] = pv;
    }
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const size_t r = r0 + i, d = d0 + tx;
    if (d < n && r < B) {
      fe_store<F>(out, r * n + d, tile[tx][i]);
      if (plain) {
        const size_t c = rs_point_index(d, log_n);
        if (slot[c] < 0) fe_store<F>(plain, r * n + c, ptile[tx][i]);
      }
    }
  }
}

// h[r][bitrev(k)] = n p_k (the inverse plan's output).  out[r][k] = p_{k+1} (k + 1) / n, 0 at
// k = n - 1; *flag = 1 if some p_k != 0 with k >= deg_bound (deg_bound >= 1).
template <class F>
__global__ __launch_bounds__(256) void k_deriv(const uint32_t *__restrict__ h, uint32_t *__restrict__ out, int log_n,
                                               size_t n_rows, const uint32_t *__restrict__ dscale, size_t deg_bound,
                                               uint32_t *__restrict__ flag) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)1 << log_n;
  if (t >= n * n_rows) return;
  const size_t r = t >> log_n, k = t & (n - 1);
  Fe<F> v = fe_zero<F>();
  if (k + 1 < n) {
    const Fe<F> p = fe_load<F>(h, r * n + bitrev_n(k + 1, log_n));
    if (k + 1 >= deg_bound && !fe_is_zero<F>(p)) *flag = 1;
    v = fe_mul<F>(p, fe_load<F>(dscale, k));
  }
  fe_store<F>(out, t, v);
}

// v = e[r][erased[j]] / L'(x_j): vals[r][j] (canonical if CANON), cm[j][r] (optional, column-major)
// and rows[r][erased[j]] (optional, Montgomery: the completed rows)
template <class F, bool CANON>
__global__ __launch_bounds__(256) void k_fill(const uint32_t *__restrict__ e, int log_n, size_t n_rows,
                                              const uint32_t *__restrict__ erased, size_t n_erased,
                                              const uint32_t *__restrict__ dinv, uint32_t *__restrict__ vals,
                                              uint32_t *__restrict__ cm, uint32_t *__restrict__ rows) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * n_erased) return;
  const size_t r = t / n_erased, j = t - r * n_erased;
  const size_t c = erased[j];
  const Fe<F> v = fe_mul<F>(fe_load<F>(e, ((size_t)r << log_n) + c), fe_load<F>(dinv, j));
  if (rows) fe_store<F>(rows, ((size_t)r << log_n) + c, v);
  const Fe<F> o = CANON ? fe_from_mont<F>(v) : v;
  fe_store<F>(vals, t, o);
  if (cm) fe_store<F>(cm, j * n_rows + r, o);
}

// col_bad[c] = 1 if column c of cols[c][r] (r < n_rows, canonical words) holds an element >= p
template <class F>
__global__ __launch_bounds__(256) void k_col_canon(const uint32_t *__restrict__ cols, size_t n_rows, size_t n_cols,
                                                   uint32_t *__restrict__ col_bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * n_cols) return;
  if (!fe_is_canonical<F>(fe_load<F>(cols, t))) col_bad[t / n_rows] = 1;
}

// status[c] = 2 (digest zeroed) if col_bad[c], else 0 / 1 as digest c equals / differs from leaf c
__global__ __launch_bounds__(256) void k_scrub_status(uint32_t *__restrict__ digests, const uint32_t *__restrict__ leaves,
                                                      const uint32_t *__restrict__ col_bad, size_t n_cols,
                                                      uint8_t *__restrict__ status) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cols) return;
  if (col_bad[c]) {
    for (int i = 0; i < 8; i++) digests[8 * c + i] = 0;
    status[c] = 2;
    return;
  }
  uint32_t o = 0;
  for (int i = 0; i < 8; i++) o |= digests[8 * c + i] ^ leaves[8 * c + i];
  status[c] = o ? 1 : 0;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t erasure_locator(int fid, const uint32_t *tw, int log_n, const uint32_t *erased, size_t n_erased,
                           int32_t *slot, uint32_t *lambda, uint32_t *dinv, hipStream_t s) {
  const size_t n = (size_t)1 << log_n;
  hipError_t e = hipMemsetAsync(slot, 0xff, n * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  if (n_erased) {
    hipLaunchKernelGGL(k_slot_set, dim3(blocks_for(n_erased)), dim3(256), 0, s, erased, n_erased, slot);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  prof::Scope ps("erasure_locator", s);
  return dispatch_field(fid, [&]<class F>() {
    hipLaunchKernelGGL((k_locator<F>), dim3(blocks_for(n)), dim3(256), 0, s, tw, log_n, erased, n_erased, slot,
                       lambda, dinv);
    return hipGetLastError();
  });
}

hipError_t erasure_dscale(int fid, int log_n, const uint32_t *inv_n_canon_words, uint32_t *dscale, hipStream_t s) {
  const size_t n = (size_t)1 << log_n;
  return dispatch_field(fid, [&]<class F>() {
    Fe<F> inv{};
    for (int i = 0; i < F::N; i++) inv.v[i] = inv_n_canon_words[i];
    hipLaunchKernelGGL((k_dscale<F>), dim3(blocks_for(n)), dim3(256), 0, s, inv, n, dscale);
    return hipGetLastError();
  });
}

hipError_t erasure_masked_rows(int fid, const uint32_t *in, uint32_t *out, int log_n, size_t n_rows,
                               const int32_t *slot, const uint32_t *lambda, hipStream_t s) {
  const size_t total = ((size_t)1 << log_n) * n_rows;
  if (!total) return hipSuccess;
  prof::Scope ps("erasure_masked_load", s);
  return dispatch_field(fid, [&]<class F>() {
    hipLaunchKernelGGL((k_masked_rows<F>), dim3(blocks_for(total)), dim3(256), 0, s, in, out, log_n, n_rows, slot,
                       lambda);
    return hipGetLastError();
  });
}

hipError_t erasure_masked_cols(int fid, const uint32_t *src, size_t B, int log_n, uint32_t *out, uint32_t *plain,
                               const int32_t *slot, const uint32_t *lambda, uint32_t *bad, hipStream_t s) {
  if (!B) return hipSuccess;
  if (fid != 0) return hipErrorInvalidValue;  // the file layer's field (WriteableFt63)
  const size_t n = (size_t)1 << log_n;
  const size_t tiles = ((n + 31) / 32) * ((B + 31) / 32);
  if (tiles > 0x7fffffffu) return hipErrorInvalidValue;
  prof::Scope ps("erasure_masked_load", s);
  hipLaunchKernelGGL((k_masked_cols<Ft63>), dim3((unsigned)tiles), dim3(256), 0, s, src, B, log_n, out, plain, slot,
                     lambda, bad);
  return hipGetLastError();
}

hipError_t erasure_deriv(int fid, const uint32_t *h, uint32_t *out, int log_n, size_t n_rows, const uint32_t *dscale,
                         size_t deg_bound, uint32_t *flag, hipStream_t s) {
  const size_t total = ((size_t)1 << log_n) * n_rows;
  if (!total) return hipSuccess;
  prof::Scope ps("erasure_deriv", s);
  return dispatch_field(fid, [&]<class F>() {
    hipLaunchKernelGGL((k_deriv<F>), dim3(blocks_for(total)), dim3(256), 0, s, h, out, log_n, n_rows, dscale,
                       deg_bound, flag);
    return hipGetLastError();
  });
}

hipError_t erasure_fill(int fid, const uint32_t *e, int log_n, size_t n_rows, const uint32_t *erased, size_t n_erased,
                        const uint32_t *dinv, uint32_t *vals, uint32_t *cm, uint32_t *rows, bool canon,
                        hipStream_t s) {
  const size_t total = n_rows * n_erased;
  if (!total) return hipSuccess;
  prof::Scope ps("erasure_fill", s);
  return dispatch_field(fid, [&]<class F>() {
    if (canon)
      hipLaunchKernelGGL((k_fill<F, true>), dim3(blocks_for(total)), dim3(256), 0, s, e, log_n, n_rows, erased,
                         n_erased, dinv, vals, cm, rows);
    else
      hipLaunchKernelGGL((k_fill<F, false>), dim3(blocks_for(total)), dim3(256), 0, s, e, log_n, n_rows, erased,
                         n_erased, dinv, vals, cm, rows);
    return hipGetLastError();
  });
}

hipError_t scrub_col_canon(int fid, const uint32_t *cols, size_t n_rows, size_t n_cols, uint32_t *col_bad,
                           hipStream_t s) {
  const size_t total = n_rows * n_cols;
  if (!total) return hipSuccess;
  prof::Scope ps("scrub_col_canon", s);
  return dispatch_field(fid, [&]<class F>() {
    hipLaunchKernelGGL((k_col_canon<F>), dim3(blocks_for(total)), dim3(256), 0, s, cols, n_rows, n_cols, col_bad);
    return hipGetLastError();
  });
}

hipError_t scrub_status(uint8_t *digests, const uint8_t *leaves, const uint32_t *col_bad, size_t n_cols,
                        uint8_t *status, hipStream_t s) {
  if (!n_cols) return hipSuccess;
  hipLaunchKernelGGL(k_scrub_status, dim3(blocks_for(n_cols)), dim3(256), 0, s, (uint32_t *)digests,
                     (const uint32_t *)leaves, col_bad, n_cols, status);
  return hipGetLastError();
}

}  // namespace lcpc
