// pos_eval.hip -- the two streaming evaluations of an update audit (proof-of-storage/src).
//
//   k_poly_eval       evaluate_field_polynomial_at_point[_with_elevated_degree] (fields.rs:160-186):
//                     sum_{i<n} c_i x^(i + d), the coefficients an element array of any field or a
//                     WriteableFt63 file image read 7 bytes per element (k_pack7's rule), with no
//                     power vector and no element image in memory.
//   k_left_mul_bytes  left_multiply_unencoded_matrix_by_vector (file_handler.rs:614-638): u^T M
//                     straight from the file image.
//   k_left_mul_bytes_many / pmfma::k_left_mul_mfma   the same for many vectors in one pass over the
//                     image (batched audits): TT accumulator sets per thread on the
//                     VALU, or the int8 matrix cores (pos_eval_mfma.hpp).
//
// All arithmetic is exact field arithmetic on Montgomery words (a packed byte element is its raw
// limb, as everywhere on the proof-of-storage path), so the order of summation does not show.
//
// k_poly_eval: a block owns a tile of EVAL_T = 2048 coefficients, 8 per thread.  Each thread runs
// Horner over its 8 in registers and multiplies the result by y^t, y the step between adjacent
// threads, from a 256-entry table built once per launch (k_eval_setup, with the Horner step, x^T
// and x^d); the products are then summed: across the wave through shuffles, the four waves once
// through LDS.  (Combining the threads with powers by squaring instead, v_t += y^(2^s) v_(t + 2^s),
// costs six products per thread where the table costs one: 0.285 against 0.233 ms for the 1 GiB
// image)  The block's value (times x^d) is one partial; the same kernel over the
// partials with x' = x^T reduces them level by level to one element.
//   bytes:    thread t owns the 56-byte run t of the tile (k_pack7's LDS staging: coalesced 16-byte
//             loads), elements 8t..8t+7, inner step x, y = x^8;
//   elements: lane t owns elements t, t + 256, ... of the tile (adjacent lanes, adjacent elements:
//             coalesced), inner step x^256, y = x.
#include <algorithm>

#include "field.hpp"
#include "kernels.hpp"
#include "pos.hpp"
#include "pos_bytes.hpp"
#include "pos_eval_mfma.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

constexpr int EVAL_T = POS_EVAL_TILE;
static_assert(EVAL_T == PACK_EL && EVAL_T == 8 * 256, "a tile is 256 threads x 8 coefficients = one k_pack7 block");
// a launch's table: the thread's Horner step (bytes: x, elements: x^256), x^T (the next level's
// point), x^d, then y^t for t < 256 (bytes: y = x^8, elements: y = x)
constexpr int TAB_STEP = 0, TAB_XT = 1, TAB_XD = 2, TAB_Y = 3, EVAL_TAB = TAB_Y + 256;

// 256 threads
template <class F>
__global__ void k_eval_setup(const uint32_t *__restrict__ x, size_t xi, uint64_t d, int bytes,
                             uint32_t *__restrict__ tab) {
  const int t = threadIdx.x;
  const Fe<F> v = fe_load<F>(x, xi);
  fe_store<F>(tab, TAB_Y + t, fe_pow<F>(v, (uint64_t)(bytes ? 8 * t : t)));
  if (t == 0) {
    fe_store<F>(tab, TAB_STEP, bytes ? v : fe_pow<F>(v, 256));
    fe_store<F>(tab, TAB_XT, fe_pow<F>(v, (uint64_t)EVAL_T));
    fe_store<F>(tab, TAB_XD, fe_pow<F>(v, d));
  }
}

template <class F>
__device__ __forceinline__ Fe<F> fe_shfl_down(const Fe<F> &a, int o) {
  Fe<F> r;
#pragma unroll
  for (int i = 0; i < F::N; i++) r.v[i] = __shfl_down(a.v[i], o, 64);
  return r;
}

template <class F, bool BYTES>
__global__ __launch_bounds__(256) void k_poly_eval(const void *__restrict__ src, size_t n, size_t n_bytes,
                                                   const uint32_t *__restrict__ tab, uint32_t *__restrict__ out) {
  __shared__ __align__(16) uint32_t s_w[4 * F::N];
  const int tid = threadIdx.x;
  Fe<F> c[8];
  if constexpr (BYTES) {
    static_assert(F::N == 2, "a file image holds WriteableFt63 elements");
    __shared__ __align__(16) uint64_t s_in[PACK_BYTES / 8];
    const uint8_t *bytes = static_cast<const uint8_t *>(src);
    const size_t bb = (size_t)blockIdx.x * PACK_BYTES;
    uint64_t q[7];
    // (the API guarantees 8-byte images; the 16-byte loads need 16-byte alignment)
    if ((((uintptr_t)bytes) & 15) == 0 && bb + PACK_BYTES <= n_bytes) {
      const uint4 *g = reinterpret_cast<const uint4 *>(bytes + bb);
      uint4 *si = reinterpret_cast<uint4 *>(s_in);
#pragma unroll
      for (int i = tid; i < PACK_BYTES / 16; i += 256) si[i] = g[i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 7; i++) q[i] = s_in[7 * tid + i];
    } else {
      pack7_load_run(bytes, n_bytes, bb + 56 * (size_t)tid, q);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint64_t e = pack7_elem(q, k);
      c[k].v[0] = (uint32_t)e;
      c[k].v[1] = (uint32_t)(e >> 32);
    }
  } else {
    const uint32_t *el = static_cast<const uint32_t *>(src);
    const size_t e0 = (size_t)blockIdx.x * EVAL_T + tid;
#pragma unroll
    for (int j = 0; j < 8; j++) c[j] = e0 + 256 * j < n ? fe_load<F>(el, e0 + 256 * j) : fe_zero<F>();
  }
  const Fe<F> xs = fe_load<F>(tab, TAB_STEP);
  Fe<F> v = c[7];
#pragma unroll
  for (int k = 6; k >= 0; k--) v = fe_add<F>(fe_mul<F>(v, xs), c[k]);
  v = fe_mul<F>(v, fe_load<F>(tab, TAB_Y + tid));
  // lane 0 of a wave ends with the wave's sum (a lane past the wave's end returns the caller's own
  // value, which only lanes that lane 0 never reads pick up)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fe_add<F>(v, fe_shfl_down<F>(v, o));
  if ((tid & 63) == 0) fe_store<F>(s_w, tid >> 6, v);
  __syncthreads();
  if (tid == 0) {
    Fe<F> t = fe_load<F>(s_w, 0);
#pragma unroll
    for (int w = 1; w < 4; w++) t = fe_add<F>(t, fe_load<F>(s_w, w));
    fe_store<F>(out, blockIdx.x, fe_mul<F>(t, fe_load<F>(tab, TAB_XD)));
  }
}

// out = (sum_{b < nb} vals[b]) * x^d   (the block values of a host image staged in blocks)
template <class F>
__global__ void k_eval_sum_scale(const uint32_t *__restrict__ vals, size_t nb, const uint32_t *__restrict__ x,
                                 uint64_t d, uint32_t *__restrict__ out) {
  Fe<F> t = fe_zero<F>();
  for (size_t b = 0; b < nb; b++) t = fe_add<F>(t, fe_load<F>(vals, b));
  fe_store<F>(out, 0, fe_mul<F>(t, fe_pow<F>(fe_load<F>(x, 0), d)));
}

// partial[y][8g + k] = sum over rows r of split y of left[r] * M[r][8g + k]; thread (y, g) walks
// its rows' 56-byte runs g, fe_dot_kmax rows per lazy reduction
template <class F>
__global__ __launch_bounds__(256) void k_left_mul_bytes(const uint8_t *__restrict__ bytes, size_t n_bytes, size_t pre,
                                                        size_t n_rows, size_t rows_per, size_t n_split,
                                                        const uint32_t *__restrict__ left,
                                                        uint32_t *__restrict__ partials) {
  static_assert(F::N == 2, "a file image holds WriteableFt63 elements");
  constexpr int K = fe_dot_kmax<F>() < 4 ? fe_dot_kmax<F>() : 4;
  const size_t n_runs = pre / 8;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t g = t % n_runs, y = t / n_runs;
  if (y >= n_split) return;
  const size_t r0 = y * rows_per, r1 = r0 + rows_per < n_rows ? r0 + rows_per : n_rows;
  const size_t row_b = 7 * pre;
  Fe<F> acc[8];
#pragma unroll
  for (int k = 0; k < 8; k++) acc[k] = fe_zero<F>();
  size_t r = r0;
  for (; r + K <= r1; r += K) {
    uint64_t q[K][7];
    Fe<F> a[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      pack7_load_run(bytes, n_bytes, (r + j) * row_b + 56 * g, q[j]);
      a[j] = fe_load<F>(left, r + j);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      Fe<F> b[K];
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint64_t e = pack7_elem(q[j], k);
        b[j].v[0] = (uint32_t)e;
        b[j].v[1] = (uint32_t)(e >> 32);
      }
      acc[k] = fe_add<F>(acc[k], fe_dot<F, K>(a, b));
    }
  }
  for (; r < r1; r++) {
    uint64_t q[7];
    pack7_load_run(bytes, n_bytes, r * row_b + 56 * g, q);
    const Fe<F> a = fe_load<F>(left, r);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint64_t e = pack7_elem(q, k);
      Fe<F> b;
      b.v[0] = (uint32_t)e;
      b.v[1] = (uint32_t)(e >> 32);
      acc[k] = fe_add<F>(acc[k], fe_mul<F>(a, b));
    }
  }
#pragma unroll
  for (int k = 0; k < 8; k++) fe_store<F>(partials, y * pre + 8 * g + k, acc[k]);
}

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// k_left_mul_bytes for many vectors: blockIdx.y = a chunk of TT vectors, each with its own
// accumulators, so a run of the image is loaded once per chunk.  lefts[t left_stride + r];
// partial[(y n_vecs + t) pre + 8g + k].  A short last chunk computes on clamped vector indices and
// stores only the vectors that exist.
constexpr int LEFT_MANY_TT = 4;

template <class F, int TT>
__global__ __launch_bounds__(256) void k_left_mul_bytes_many(const uint8_t *__restrict__ bytes, size_t n_bytes,
                                                             size_t pre, size_t n_rows, size_t rows_per,
                                                             size_t n_split, const uint32_t *__restrict__ lefts,
                                                             size_t left_stride, size_t n_vecs,
                                                             uint32_t *__restrict__ partials) {
  static_assert(F::N == 2, "a file image holds WriteableFt63 elements");
  constexpr int K = fe_dot_kmax<F>() < 2 ? fe_dot_kmax<F>() : 2;
  const size_t n_runs = pre / 8;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t g = t % n_runs, y = t / n_runs;
  if (y >= n_split) return;
  const size_t t0 = (size_t)blockIdx.y * TT;
  const size_t r0 = y * rows_per, r1 = r0 + rows_per < n_rows ? r0 + rows_per : n_rows;
  const size_t row_b = 7 * pre;
  const uint32_t *lv[TT];
#pragma unroll
  for (int v = 0; v < TT; v++) lv[v] = lefts + 2 * (t0 + v < n_vecs ? t0 + v : n_vecs - 1) * left_stride;
  Fe<F> acc[TT][8];
#pragma unroll
  for (int v = 0; v < TT; v++)
#pragma unroll
    for (int k = 0; k < 8; k++) acc[v][k] = fe_zero<F>();
  size_t r = r0;
  for (; r + K <= r1; r += K) {
    uint64_t q[K][7];
    Fe<F> a[TT][K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      pack7_load_run(bytes, n_bytes, (r + j) * row_b + 56 * g, q[j]);
#pragma unroll
      for (int v = 0; v < TT; v++) a[v][j] = fe_load<F>(lv[v], r + j);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      Fe<F> b[K];
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint64_t e = pack7_elem(q[j], k);
        b[j].v[0] = (uint32_t)e;
        b[j].v[1] = (uint32_t)(e >> 32);
      }
#pragma unroll
      for (int v = 0; v < TT; v++) acc[v][k] = fe_add<F>(acc[v][k], fe_dot<F, K>(a[v], b));
    }
  }
  for (; r < r1; r++) {
    uint64_t q[7];
    pack7_load_run(bytes, n_bytes, r * row_b + 56 * g, q);
    Fe<F> a[TT];
#pragma unroll
    for (int v = 0; v < TT; v++) a[v] = fe_load<F>(lv[v], r);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint64_t e = pack7_elem(q, k);
      Fe<F> b;
      b.v[0] = (uint32_t)e;
      b.v[1] = (uint32_t)(e >> 32);
#pragma unroll
      for (int v = 0; v < TT; v++) acc[v][k] = fe_add<F>(acc[v][k], fe_mul<F>(a[v], b));
    }
  }
#pragma unroll
  for (int v = 0; v < TT; v++)
    if (t0 + v < n_vecs)
#pragma unroll
      for (int k = 0; k < 8; k++) fe_store<F>(partials, (y * n_vecs + t0 + v) * pre + 8 * g + k, acc[v][k]);
}

// corr[t] = (sum_r lefts[t left_stride + r]) * C128, the file digits' shift of the matrix-core
// kernel (pos_eval_mfma.hpp); one block of 256 threads per vector
template <class F>
__global__ __launch_bounds__(256) void k_left_many_corr(const uint32_t *__restrict__ lefts, size_t left_stride,
                                                        size_t n_rows, uint32_t *__restrict__ corr) {
  __shared__ __align__(16) uint32_t s_w[256 * F::N];
  const int tid = threadIdx.x;
  const size_t t = blockIdx.x;
  Fe<F> v = fe_zero<F>();
  for (size_t r = tid; r < n_rows; r += 256) v = fe_add<F>(v, fe_load<F>(lefts, t * left_stride + r));
  fe_store<F>(s_w, tid, v);
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) fe_store<F>(s_w, tid, fe_add<F>(fe_load<F>(s_w, tid), fe_load<F>(s_w, tid + o)));
    __syncthreads();
  }
  if (tid == 0) {
    Fe<F> c;
    c.v[0] = (uint32_t)pmfma::C128;
    c.v[1] = (uint32_t)(pmfma::C128 >> 32);
    fe_store<F>(corr, t, fe_mul<F>(fe_load<F>(s_w, 0), c));
  }
}

// out[t pre + c] = sum_y partials[(y n_vecs + t) pre + c] (+ corr[t]); blockIdx.y = t
template <class F>
__global__ __launch_bounds__(256) void k_left_many_fold(const uint32_t *__restrict__ partials, size_t n_split,
                                                        size_t pre, size_t n_vecs, const uint32_t *__restrict__ corr,
                                                        uint32_t *__restrict__ out) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (c >= pre) return;
  Fe<F> v = corr ? fe_load<F>(corr, t) : fe_zero<F>();
  for (size_t y = 0; y < n_split; y++) v = fe_add<F>(v, fe_load<F>(partials, (y * n_vecs + t) * pre + c));
  fe_store<F>(out, t * pre + c, v);
}

__global__ __launch_bounds__(256) void k_recombine63(const int *__restrict__ y, uint32_t *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int Y[8];
#pragma unroll
  for (int u = 0; u < 8; u++) Y[u] = y[i * 8 + u];
  fe_store<Ft63>(out, i, pmfma::recombine_redc63<Ft63>(Y));
}


// the row split of k_left_mul_bytes: enough threads to fill the device, each with whole rows and
// at least 8 of them (a few lazy reductions per partial it writes)
inline void left_mul_split(size_t pre, size_t n_rows, size_t *rows_per, size_t *n_split) {
  const size_t n_runs = pre / 8, want = ceil_div((size_t)1 << 18, n_runs);
  *rows_per = std::min(n_rows, std::max<size_t>(ceil_div(n_rows, want), 8));
  *n_split = ceil_div(n_rows, *rows_per);
}


constexpr int MFMA_TP = 8;  // vector pairs per chunk of the matrix-core kernel: 16 vectors

// the row split of the many-vector kernels over n_rows rows of one image piece
//   VALU: left_mul_split with the chunks counted into the threads in flight;
//   matrix cores: splits of at most MAX_SPLIT_ROWS rows, a multiple of the K step, halved while the
//   launch has fewer than 2048 waves and a split keeps at least 128 KiB of image (below that its
//   partials and their fold cost more than its waves add)
inline void left_many_split(int kernel, size_t pre, size_t n_rows, size_t n_vecs, size_t *rows_per, size_t *n_split) {
  if (kernel == POS_LEFT_MANY_MFMA) {
    const size_t waves = pre / pmfma::COLS_PER_WAVE * ceil_div(n_vecs, 2 * MFMA_TP);
    size_t rp = pmfma::MAX_SPLIT_ROWS;
    while (rp > pmfma::STEP_ROWS && ceil_div(n_rows, rp) * waves < 2048 && rp / 2 * 7 * pre >= ((size_t)128 << 10))
      rp /= 2;
    *rows_per = rp;
    *n_split = ceil_div(n_rows, rp);
    return;
  }
  const size_t n_runs = pre / 8, want = ceil_div((size_t)1 << 18, n_runs * ceil_div(n_vecs, LEFT_MANY_TT));
  *rows_per = std::min(n_rows, std::max<size_t>(ceil_div(n_rows, want), 8));
  *n_split = ceil_div(n_rows, *rows_per);
}

}  // namespace

size_t poly_eval_scratch_bytes(int fid, size_t n) {
  size_t elems = 0, levels = 0;
  for (size_t m = n; m > 1 || !levels; levels++) {
    m = ceil_div(m, EVAL_T);
    elems += m;
  }
  return (elems + levels * EVAL_TAB) * (size_t)field_bytes(fid);
}

hipError_t poly_eval(int fid, const void *src, size_t n, size_t n_bytes, const uint32_t *x, uint64_t d,
                     uint32_t *out, void *scratch, hipStream_t s) {
  if (n_bytes && (fid != 0 || n != (n_bytes + 6) / 7)) return hipErrorInvalidValue;
  if (!n) return hipMemsetAsync(out, 0, (size_t)field_bytes(fid), s);
  prof::Scope ps("pos_poly_eval", s);
  return dispatch_field(fid, [&]<class F>() -> hipError_t {
    size_t levels = 0;
    for (size_t m = n; m > 1 || !levels; levels++) m = ceil_div(m, EVAL_T);
    uint32_t *tab = static_cast<uint32_t *>(scratch);          // [level][EVAL_TAB]
    uint32_t *part = tab + levels * EVAL_TAB * F::N;           // level 0's partials, then level 1's, ...
    const void *cur = src;
    size_t m = n;
    for (size_t l = 0; l < levels; l++) {
      uint32_t *t = tab + l * EVAL_TAB * F::N;
      const bool bytes = l == 0 && n_bytes;
      if (l == 0)
        hipLaunchKernelGGL((k_eval_setup<F>), dim3(1), dim3(256), 0, s, x, (size_t)0, d, (int)bytes, t);
      else  // the partials of level l - 1 are the coefficients of a polynomial in x^T
        hipLaunchKernelGGL((k_eval_setup<F>), dim3(1), dim3(256), 0, s, t - EVAL_TAB * F::N, (size_t)TAB_XT,
                           (uint64_t)0, 0, t);
      const size_t nb = ceil_div(m, EVAL_T);
      if (nb >= ((size_t)1 << 24)) return hipErrorInvalidValue;  // (grid threads stay below 2^32)
      uint32_t *dst = nb == 1 ? out : part;
      if constexpr (F::N == 2) {
        if (bytes)
          hipLaunchKernelGGL((k_poly_eval<F, true>), dim3((unsigned)nb), dim3(256), 0, s, cur, m, n_bytes, t, dst);
        else
          hipLaunchKernelGGL((k_poly_eval<F, false>), dim3((unsigned)nb), dim3(256), 0, s, cur, m, (size_t)0, t, dst);
      } else {
        hipLaunchKernelGGL((k_poly_eval<F, false>), dim3((unsigned)nb), dim3(256), 0, s, cur, m, (size_t)0, t, dst);
      }
      cur = dst;
      part += nb * F::N;
      m = nb;
    }
    return hipGetLastError();
  });
}

hipError_t poly_eval_sum_scale(int fid, const uint32_t *vals, size_t nb, const uint32_t *x, uint64_t d,
                               uint32_t *out, hipStream_t s) {
  return dispatch_field(fid, [&]<class F>() {
    hipLaunchKernelGGL((k_eval_sum_scale<F>), dim3(1), dim3(1), 0, s, vals, nb, x, d, out);
    return hipGetLastError();
  });
}

bool pos_left_mul_bytes_ok(size_t pre) { return pre >= 8 && !(pre & (pre - 1)); }

size_t pos_left_mul_bytes_scratch_bytes(size_t pre, size_t n_rows) {
  size_t rows_per, n_split;
  left_mul_split(pre, n_rows, &rows_per, &n_split);
  return n_split * pre * 8;
}

hipError_t pos_left_mul_bytes(const uint8_t *bytes, size_t n_bytes, size_t pre, size_t n_rows, const uint32_t *left,
                              uint32_t *out, void *scratch, hipStream_t s) {
  if (!pos_left_mul_bytes_ok(pre) || !n_rows) return hipErrorInvalidValue;
  prof::Scope ps("pos_left_mul_bytes", s);
  size_t rows_per, n_split;
  left_mul_split(pre, n_rows, &rows_per, &n_split);
  const size_t blocks = ceil_div(n_split * (pre / 8), 256);
  if (blocks >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  uint32_t *partials = n_split == 1 ? out : static_cast<uint32_t *>(scratch);
  hipLaunchKernelGGL((k_left_mul_bytes<Ft63>), dim3((unsigned)blocks), dim3(256), 0, s, bytes, n_bytes, pre, n_rows,
                     rows_per, n_split, left, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n_split == 1) return e;
  return collapse_fold_rows(0, partials, n_split, pre, out, s);
}

// The matrix-core kernel from POS_LEFT_MANY_MFMA_MIN_VECS vectors on (the adoption measurement of
// DESIGN §5f); pre below one wave's 64 columns and LCPC_NO_MFMA=1 stay on the VALU kernel.
int pos_left_mul_many_kernel(size_t pre, size_t n_vecs) {
  if (!pos_left_mul_bytes_ok(pre)) return POS_LEFT_MANY_PACK;
  if (!no_mfma() && pre >= (size_t)pmfma::COLS_PER_WAVE && n_vecs >= POS_LEFT_MANY_MFMA_MIN_VECS)
    return POS_LEFT_MANY_MFMA;
  return POS_LEFT_MANY_VALU;
}

size_t pos_left_mul_many_splits(int kernel, size_t pre, size_t n_rows, size_t n_vecs) {
  size_t rows_per, n_split;
  left_many_split(kernel, pre, n_rows, n_vecs, &rows_per, &n_split);
  return n_split;
}

size_t pos_left_mul_many_prep_bytes(int kernel, size_t n_rows, size_t n_vecs) {
  if (kernel != POS_LEFT_MANY_MFMA) return 0;
  return n_vecs * ((n_rows + 1) / 2) * 128 + n_vecs * 8;
}

hipError_t pos_left_mul_many_prepare(int kernel, const uint32_t *lefts, size_t n_rows, size_t n_vecs, void *prep,
                                     hipStream_t s) {
  if (kernel != POS_LEFT_MANY_MFMA) return hipSuccess;
  using F = Ft63;
  const size_t n_pairs = (n_rows + 1) / 2, nd = n_vecs * n_pairs * 16;
  if (ceil_div(nd, 256) >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  prof::Scope ps("pos_left_mul_many_prepare", s);
  uint8_t *hdig = static_cast<uint8_t *>(prep);
  uint32_t *corr = reinterpret_cast<uint32_t *>(hdig + n_vecs * n_pairs * 128);
  hipLaunchKernelGGL((pmfma::k_left_digits<F>), dim3((unsigned)ceil_div(nd, 256)), dim3(256), 0, s, lefts, n_rows,
                     n_rows, n_pairs, n_vecs, hdig);
  hipLaunchKernelGGL((k_left_many_corr<F>), dim3((unsigned)n_vecs), dim3(256), 0, s, lefts, n_rows, n_rows, corr);
  return hipGetLastError();
}

hipError_t pos_left_mul_many_partials(int kernel, const uint8_t *bytes, size_t n_bytes, size_t pre, size_t n_rows,
                                      size_t row_base, const uint32_t *lefts, size_t n_rows_total, size_t n_vecs,
                                      const void *prep, uint32_t *partials, hipStream_t s) {
  if (kernel == POS_LEFT_MANY_PACK || !pos_left_mul_bytes_ok(pre) || !n_rows || !n_vecs ||
      n_vecs > POS_LEFT_MANY_MAX_VECS || row_base + n_rows > n_rows_total)
    return hipErrorInvalidValue;
  using F = Ft63;
  prof::Scope ps("pos_left_mul_many", s);
  size_t rows_per, n_split;
  left_many_split(kernel, pre, n_rows, n_vecs, &rows_per, &n_split);
  if (kernel == POS_LEFT_MANY_MFMA) {
    if (pre < (size_t)pmfma::COLS_PER_WAVE || (row_base & 1) || n_split >= 65536) return hipErrorInvalidValue;
    const size_t n_pairs = (n_rows_total + 1) / 2;
    const uint4 *hd = static_cast<const uint4 *>(prep) + row_base / 2 * 8;
    const dim3 grid((unsigned)ceil_div(pre, 4 * pmfma::COLS_PER_WAVE), (unsigned)n_split,
                    (unsigned)ceil_div(n_vecs, 2 * MFMA_TP));
    hipLaunchKernelGGL((pmfma::k_left_mul_mfma<F, MFMA_TP>), grid, dim3(256), 0, s, bytes, n_bytes, pre, n_rows, hd,
                       n_pairs, n_vecs, partials, rows_per);
    return hipGetLastError();
  }
  const size_t blocks = ceil_div(n_split * (pre / 8), 256);
  if (blocks >= ((size_t)1 << 24)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_left_mul_bytes_many<F, LEFT_MANY_TT>),
                     dim3((unsigned)blocks, (unsigned)ceil_div(n_vecs, LEFT_MANY_TT)), dim3(256), 0, s, bytes, n_bytes,
                     pre, n_rows, rows_per, n_split, lefts + 2 * row_base, n_rows_total, n_vecs, partials);
  return hipGetLastError();
}

hipError_t pos_left_mul_many_fold(int kernel, const uint32_t *partials, size_t n_split, size_t pre, size_t n_rows_total,
                                  size_t n_vecs, const void *prep, uint32_t *out, hipStream_t s) {
  prof::Scope ps("pos_left_mul_many_fold", s);
  const uint32_t *corr = nullptr;
  if (kernel == POS_LEFT_MANY_MFMA)
    corr = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(prep) + n_vecs * ((n_rows_total + 1) / 2) * 128);
  hipLaunchKernelGGL((k_left_many_fold<Ft63>), dim3((unsigned)ceil_div(pre, 256), (unsigned)n_vecs), dim3(256), 0, s,
                     partials, n_split, pre, n_vecs, corr, out);
  return hipGetLastError();
}

hipError_t pos_recombine63(const int *y, uint32_t *out, size_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_recombine63, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, y, out, n);
  return hipGetLastError();
}

}  // namespace lcpc
