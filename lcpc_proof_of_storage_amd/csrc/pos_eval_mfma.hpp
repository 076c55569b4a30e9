// pos_eval_mfma.hpp -- u_t^T M for many vectors straight from a WriteableFt63 file image, on the
// gfx950 int8 matrix cores (batched audits of a stored file).
//
//     out[t][c] = sum_r left_t[r] * M[r][c] R^-1 mod p       (left: Montgomery words, M: raw 56 bits)
//
// A file element is seven raw bytes b_0..b_6, M = sum_a b_a 2^(8a): its base-256 digits are already
// in memory.  The byte is used as the signed digit d_a = b_a - 128 (the byte XOR 0x80 read as
// int8), and every vector entry is expanded, as in collapse_mfma.hpp, into the 7 residues
// H[r][a] = left[r] 2^(8a) mod p in 8 balanced digits H = sum_u h[r][a][u] 2^(8u), h in [-128, 128)
// (p < 2^63 - 2^56, so H + 0x80..80 does not carry out).  Then
//
//     Y[u][c] = sum_(r, a) h[r][a][u] d_a(r, c)                        (an exact int32 GEMM)
//     sum_u Y[u][c] 2^(8u) + C128 sum_r left[r] = sum_r left[r] M[r][c]   (mod p),
//
// C128 = 0x80808080808080 = sum_a 128 2^(8a): the shift of the file digits is one field element per
// vector, the same for every column and every row split, so it is added once, after the splits are
// folded (k_left_many_fold), as the Montgomery product (sum_r left[r]) * C128.  One Montgomery
// reduction per output (recombine_redc63) turns sum_u Y[u] 2^(8u) into the field sum of Montgomery
// products, bit-identical to the VALU kernels.
//
// Bound: |h d| <= 128 * 128 = 2^14, and an accumulator of a split of at most MAX_SPLIT_ROWS = 512
// rows holds 7 products per row: |Y[u]| <= 512 * 7 * 2^14 = 2^25.81 < 2^26 = Y_BOUND.
//
// The GEMM is v_mfma_i32_16x16x64_i8.  M = 16: the 8 digit positions u of two vectors (m = 8 v + u).
// K = 64: 8 file rows x 8 slots, slot a < 7 the digit a and slot 7 zero on both operands; lane group
// g holds the rows 2g, 2g + 1 of the step (k = 16 g + 8 (r & 1) + a on both operands).  N = 16
// columns.  A lane's B fragment is two 7-byte runs 7 pre bytes apart, so a wave stages its 8 rows x
// 64 columns (8 runs of 448 bytes, each 8-byte aligned in an 8-byte aligned image) through its own
// LDS slice with coalesced 8-byte loads and cuts the fragments there; the next step's loads are in
// flight under this step's MFMAs.  One B fragment feeds the TP vector pairs of a chunk.
#pragma once
#include "field.hpp"

namespace lcpc {
namespace pmfma {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int COLS_PER_WAVE = 64, TILES = COLS_PER_WAVE / 16;
constexpr size_t MAX_SPLIT_ROWS = 512;
constexpr int Y_BOUND_LOG2 = 26;  // |Y[u]| < 2^26 (512 rows x 7 digits x 2^14 = 2^25.81)
constexpr int STEP_ROWS = 8;      // file rows per MFMA (K = 64 = 8 rows x 8 slots)
constexpr int RUN_WORDS = 7 * COLS_PER_WAVE / 8;  // a row's 64 columns: 448 bytes = 56 u64
constexpr int ROW_STRIDE = RUN_WORDS + 1;         // LDS row stride in u64
constexpr int STAGE_WORDS = STEP_ROWS * ROW_STRIDE;  // (column 63's 7 bytes end with the run: no cut reads past it)
constexpr int LOADS = STEP_ROWS * RUN_WORDS / 64;        // u64 per lane and step
static_assert(STEP_ROWS * RUN_WORDS % 64 == 0, "whole loads per lane");
constexpr uint64_t C128 = 0x0080808080808080ull;  // sum_a 128 2^(8a), a < 7

// hdig as uint4: entry ((t n_pairs + (r >> 1)) 8 + u) holds h[r][a][u] in byte 8 (r & 1) + a, byte
// 8 (r & 1) + 7 zero; rows n_rows <= r < 2 n_pairs are zero.  One thread per (t, r, a < 8).
template <class F>
__global__ __launch_bounds__(256) void k_left_digits(const uint32_t *__restrict__ lefts, size_t left_stride,
                                                     size_t n_rows, size_t n_pairs, size_t n_vecs,
                                                     uint8_t *__restrict__ hdig) {
  static_assert(F::N == 2, "Ft63 layout");
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_vecs * n_pairs * 16) return;
  const int a = (int)(g & 7);
  const size_t tr = g >> 3, t = tr / (2 * n_pairs), r = tr % (2 * n_pairs);
  uint64_t d = 0;
  if (a < 7 && r < n_rows) {
    const Fe<F> x = fe_load<F>(lefts, t * left_stride + r);
    Fe<F> pw = fe_zero<F>();  // 2^(8a) as an integer (< p), then to Montgomery form
    pw.v[a >> 2] = 1u << (8 * (a & 3));
    const Fe<F> h = fe_mul<F>(x, fe_to_mont<F>(pw));
    const uint64_t hv = ((uint64_t)h.v[1] << 32) | h.v[0];
    d = (hv + 0x8080808080808080ull) ^ 0x8080808080808080ull;  // h < p < 2^63 - 2^56: no carry out
  }
  uint8_t *o = hdig + ((t * n_pairs + (r >> 1)) * 8) * 16 + 8 * (r & 1) + a;
#pragma unroll
  for (int u = 0; u < 8; u++) o[16 * u] = (uint8_t)(d >> (8 * u));
}

// The field element of a digit-position accumulator column: (sum_u Y[u] 2^(8u)) R^-1 mod p for
// |Y[u]| <= 2^26 (Ft63, R = 2^64).
template <class F>
__device__ __forceinline__ Fe<F> recombine_redc63(const int (&Y)[8]) {
  static_assert(F::N == 2, "Ft63 layout");
  // V = sum_u Y_u 2^(8u) as S_w = sum_j Y_(4w+j) 2^(8j) (int64, |S_w| < 2^50.01), then signed carries
  int64_t S[2];
#pragma unroll
  for (int w = 0; w < 2; w++) {
    int64_t sum = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) sum += (int64_t)Y[4 * w + j] * ((int64_t)1 << (8 * j));
    S[w] = sum;
  }
  uint32_t y[2];
  int64_t carry = 0;
#pragma unroll
  for (int w = 0; w < 2; w++) {
    const int64_t v = S[w] + carry;
    y[w] = (uint32_t)v;
    carry = v >> 32;  // arithmetic
  }
  // V = y + carry 2^64 with |V| <= 2^26 (2^64 - 1) / 255 < 2^82.01; add OFF = p 2^21 (a multiple of
  // p, > 2^83.14 > |V|) so that V + OFF is nonnegative and below 2^83.7: top < 2^19.7
  constexpr uint32_t O0 = F::P[0] << 21;
  constexpr uint32_t O1 = (F::P[1] << 21) | (F::P[0] >> 11);
  constexpr uint32_t O2 = F::P[1] >> 11;
  uint32_t cc = 0;
  y[0] = __builtin_addc(y[0], O0, cc, &cc);
  y[1] = __builtin_addc(y[1], O1, cc, &cc);
  const uint32_t top = (uint32_t)(carry + (int64_t)O2 + (int64_t)cc);
  // (x + top 2^64) R^-1 = REDC(x) + top: REDC(x) lies in [0, p], so the sum is below p + 2^20 < 2p
  Fe<F> a;
  a.v[0] = y[0];
  a.v[1] = y[1];
  const Fe<F> r = fe_from_mont_generic<F>(a);
  uint32_t s[2], u[2], c = 0, br = 0;
  s[0] = __builtin_addc(r.v[0], top, c, &c);
  s[1] = __builtin_addc(r.v[1], 0u, c, &c);
#pragma unroll
  for (int i = 0; i < 2; i++) u[i] = __builtin_subc(s[i], F::P[i], br, &br);
  Fe<F> o;
#pragma unroll
  for (int i = 0; i < 2; i++) o.v[i] = br ? s[i] : u[i];
  return o;
}

// One wave = 64 columns x the split's rows x one chunk of 2 TP vectors; 4 waves per block on
// adjacent column ranges (pre a power of two >= 64: a wave has all its columns or none).
// blockIdx.y = the split, blockIdx.z = the chunk.  bytes: the image of rows 0 .. n_rows - 1
// (n_bytes bytes, 8-byte aligned, zero padded past its end); hd: the digit table at the pair of
// row 0.  partial[(split n_vecs + t) pre + c] = the split's field sum without the C128 term.
// A short last chunk runs all TP pairs on clamped vector indices and stores only the vectors that
// exist.  rows_per_split is a multiple of STEP_ROWS and at most MAX_SPLIT_ROWS.
template <class F, int TP>
__global__ __launch_bounds__(256, 2) void k_left_mul_mfma(const uint8_t *__restrict__ bytes, size_t n_bytes, size_t pre,
                                                       size_t n_rows, const uint4 *__restrict__ hd, size_t n_pairs,
                                                       size_t n_vecs, uint32_t *__restrict__ partial,
                                                       size_t rows_per_split) {
  static_assert(F::N == 2, "a file image holds WriteableFt63 elements");
  __shared__ __align__(16) uint64_t stage[4][STAGE_WORDS];
  __shared__ int red[4][TILES][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane >> 4, n = lane & 15;
  const size_t col0 = ((size_t)blockIdx.x * 4 + wave) * COLS_PER_WAVE;
  if (col0 >= pre) return;  // (whole waves; the kernel has no block barrier)
  const size_t split = blockIdx.y;
  const size_t t0 = (size_t)blockIdx.z * (2 * TP);
  const size_t r0 = split * rows_per_split;
  const size_t r1 = r0 + rows_per_split < n_rows ? r0 + rows_per_split : n_rows;
  uint64_t *sw = stage[wave];

  // the lane's vector in each pair (A row m = n: vector n >> 3, digit position n & 7), clamped
  size_t ta[TP];
#pragma unroll
  for (int p = 0; p < TP; p++) {
    const size_t t = t0 + 2 * p + (n >> 3);
    ta[p] = ((t < n_vecs ? t : n_vecs - 1) * n_pairs) * 8 + (n & 7);
  }

  v4i acc[TP][TILES];
#pragma unroll
  for (int p = 0; p < TP; p++)
#pragma unroll
    for (int k = 0; k < TILES; k++) acc[p][k] = v4i{0, 0, 0, 0};

  // word j = lane + 64 q of the step: row j / 56, u64 j % 56 of the row's run
  auto gload = [&](size_t rg, uint64_t *x) {
#pragma unroll
    for (int q = 0; q < LOADS; q++) {
      const int j = lane + 64 * q, row = j / RUN_WORDS, w = j - RUN_WORDS * row;
      const size_t off = 7 * ((rg + row) * pre + col0) + 8 * (size_t)w;
      if (off + 8 <= n_bytes) {
        x[q] = *reinterpret_cast<const uint64_t *>(bytes + off);
      } else {
        uint64_t v = 0;
        for (int b = 0; b < 8; b++)
          if (off + b < n_bytes) v |= (uint64_t)bytes[off + b] << (8 * b);
        x[q] = v;
      }
    }
  };
  auto put = [&](const uint64_t *x) {
#pragma unroll
    for (int q = 0; q < LOADS; q++) {
      const int j = lane + 64 * q, row = j / RUN_WORDS, w = j - RUN_WORDS * row;
      sw[row * ROW_STRIDE + w] = x[q];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // the 7 bytes of column col (of the wave's 64) in staged row `row`, as signed digits, slot 7 zero
  auto cut = [&](int row, int col) -> uint64_t {
    const int off = 7 * col, wi = off >> 3, sh = 8 * (off & 7);
    const uint64_t *p = sw + row * ROW_STRIDE + wi;
    uint64_t v = p[0] >> sh;
    if (sh > 8) v |= p[1] << (64 - sh);
    return (v & 0x00ffffffffffffffull) ^ C128;
  };

  uint64_t xn[LOADS];
  if (r0 < r1) {
    gload(r0, xn);
    put(xn);
  }
  for (size_t rg = r0; rg < r1; rg += STEP_ROWS) {
    const bool more = rg + STEP_ROWS < r1;
    if (more) gload(rg + STEP_ROWS, xn);  // the next step's image (HBM) under this step's MFMAs
    v4i d[TILES];
#pragma unroll
    for (int k = 0; k < TILES; k++) {
      const uint64_t e0 = cut(2 * grp, 16 * k + n), e1 = cut(2 * grp + 1, 16 * k + n);
      d[k] = v4i{(int)(uint32_t)e0, (int)(uint32_t)(e0 >> 32), (int)(uint32_t)e1, (int)(uint32_t)(e1 >> 32)};
    }
    const size_t pr = (rg >> 1) + grp;  // the lane group's row pair
    const bool ok = 2 * pr < r1;
#pragma unroll
    for (int p = 0; p < TP; p++) {
      const uint4 a = ok ? hd[ta[p] + pr * 8] : make_uint4(0, 0, 0, 0);
      const v4i av = v4i{(int)a.x, (int)a.y, (int)a.z, (int)a.w};
#pragma unroll
      for (int k = 0; k < TILES; k++) acc[p][k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, d[k], acc[p][k], 0, 0, 0);
    }
    if (more) {
      __builtin_amdgcn_wave_barrier();  // (every lane has cut its fragments)
      put(xn);
    }
  }
  // C/D layout (16x16): lane holds rows m = 4 grp + j of column n, m = 8 v + u.  Each wave turns its
  // accumulators into field elements through its own LDS slice, one pair at a time: the outputs
  // (vector v, column col0 + lane) for v = 0, 1 per lane.
  const int q = lane >> 4;
  const size_t c = col0 + lane;
  int(*rw)[16][17] = red[wave];
#pragma unroll
  for (int p = 0; p < TP; p++) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < TILES; k++) {
      rw[k][4 * grp + 0][n] = acc[p][k].x;
      rw[k][4 * grp + 1][n] = acc[p][k].y;
      rw[k][4 * grp + 2][n] = acc[p][k].z;
      rw[k][4 * grp + 3][n] = acc[p][k].w;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int v = 0; v < 2; v++) {
      int Y[8];
#pragma unroll
      for (int u = 0; u < 8; u++) Y[u] = rw[q][8 * v + u][n];
      const size_t t = t0 + 2 * p + v;
      if (t < n_vecs) fe_store<F>(partial, (split * n_vecs + t) * pre + c, recombine_redc63<F>(Y));
    }
  }
}

}  // namespace pmfma
}  // namespace lcpc
