// ntt_v2.hpp -- register-round NTT passes with one LDS exchange (gfx950).
//
// Same contract and four-step decomposition as ntt_impl.hpp (fffft::fft_io, out[bitrev(j)] =
// sum_i in[i] w^(ij)).  What changes is the data movement per workgroup:
//   pass A: round 0 of the column DIF loads its 2^R elements straight from HBM (lanes = adjacent
//           columns: coalesced row segments), rounds exchange through one padded LDS tile, and
//           the last round applies the inter-pass twiddle and stores straight to HBM (again
//           lanes = adjacent columns).  With HALFZ (n_valid <= n/2, rate-1/2 Ligero rows) the
//           upper half of every column is known zero: it is never loaded and the first stage
//           degenerates to (a, a*w) -- no add/sub.
//   pass B: round 0 loads contiguous block positions (lanes = adjacent positions), the last
//           round goes through LDS once more so the final stores are contiguous rows.
// Block size T threads, tile S x CW elements, 2^R = S*CW/T elements per thread per round.
#pragma once
#include "field.hpp"
#include "kernels.hpp"
#include "prof.hpp"

// LCPC_NTT_LAZY (default 1): butterflies keep residues in [0, 2p) (no final subtraction in the
// twiddle products), and pass B's final store reduces to [0, p).
#ifndef LCPC_NTT_LAZY
#define LCPC_NTT_LAZY 1
#endif

// LCPC_NTT_TW4 (default 1; needs LCPC_NTT_LAZY): the Ft127 passes of at most 2^NTT_TW4_MAX_L points
// multiply by word-expanded twiddles (field.hpp, fe_mul_tw: two Montgomery word-steps per product
// instead of four) staged in LDS from NttPlan::d_tw4.  0: every field takes the library product
// (tools/ab_lib.py runs one build against the other).
#ifndef LCPC_NTT_TW4
#define LCPC_NTT_TW4 1
#endif
#if !LCPC_NTT_LAZY
#undef LCPC_NTT_TW4
#define LCPC_NTT_TW4 0
#endif
// LCPC_NTT_TW4_A (default 1): 0 keeps pass A on the library product while pass B takes the
// expanded twiddles (an A/B switch: pass A answers the shorter instruction stream far less than
// pass B does).
#ifndef LCPC_NTT_TW4_A
#define LCPC_NTT_TW4_A 1
#endif

// LCPC_NTT_PERSIST (default 1): Ft127's pass A of at most 2^NTT_TW4_MAX_L points at the default
// tile shape runs as a persistent tile loop (k_pass_a_loop; pass B: LCPC_NTT_PERSIST_B) on a grid
// of the resident blocks.  0 builds the one-tile-per-workgroup kernels everywhere (tools/ab_lib.py
// runs one build against the other).
#ifndef LCPC_NTT_PERSIST
#define LCPC_NTT_PERSIST 1
#endif
// LCPC_NTT_PERSIST_B (default 0; an A/B switch under LCPC_NTT_PERSIST, as LCPC_NTT_TW4_A is under
// LCPC_NTT_TW4): 0 pass B stays on the one-tile kernel while pass A loops, 1 it loops and
// prefetches too (k_pass_b_loop).  Measured: the looping pass B is 14 % slower
// alone (0.344 against 0.302 ms) and about 1 % faster inside the pipelined bench, which is within
// twice the parent's run-to-run spread.
#ifndef LCPC_NTT_PERSIST_B
#define LCPC_NTT_PERSIST_B 0
#endif

// LCPC_NTT_LEAF_FUSE (default 1): a whole Ft127 commitment's canonical encode can end in
// k_pass_b_leaf, pass B that also hashes the column leaves' BLAKE3 chunks (ntt_rows_leaf_cvs,
// kernels.hpp).  0 builds the tree without the kernel: every commitment keeps the separate leaf
// pass (tools/ab_lib.py runs one build against the other).  LCPC_NTT_LEAF_FUSE=0 in the environment
// when a plan is made does the same for that plan (NttPlan::leaf_fuse).
#ifndef LCPC_NTT_LEAF_FUSE
#define LCPC_NTT_LEAF_FUSE 1
#endif
// LCPC_NTT_LEAF_FUSE_PF (default 0): the fused pass prefetches the next tile's round-0 loads before
// its last round and the hash (an A/B switch, as LCPC_NTT_PERSIST_B).
#ifndef LCPC_NTT_LEAF_FUSE_PF
#define LCPC_NTT_LEAF_FUSE_PF 0
#endif

#if LCPC_NTT_LEAF_FUSE
#include "blake3_dev.hpp"
#endif

namespace lcpc {
namespace ntt_v2 {

#if LCPC_NTT_LAZY
template <class F>
__device__ __forceinline__ Fe<F> NTT_MUL(const Fe<F> &a, const Fe<F> &b) { return fe_mul_lazy<F>(a, b); }
#else
template <class F>
__device__ __forceinline__ Fe<F> NTT_MUL(const Fe<F> &a, const Fe<F> &b) { return fe_mul<F>(a, b); }
#endif

// The twiddle product of the sub-FFT stages as a policy: what a block stages in LDS at `lds` for
// the HALF = 2^(LOG_S-1) twiddles of its 2^LOG_S-point DIF, and the product by entry e.
// TwLib: one Montgomery element per twiddle, from the flat table twn[e << shift]; the library product.
template <class F>
struct TwLib {
  static constexpr int ELEMS = 1;  // LDS elements per twiddle
  template <int HALF>
  static __device__ __forceinline__ void stage(Fe<F> *lds, const uint32_t *__restrict__ twn, int shift, int tid,
                                               int nt) {
    for (int e = tid; e < HALF; e += nt) lds[e] = fe_load<F>(twn, (size_t)e << shift);
  }
  template <int HALF>
  static __device__ __forceinline__ Fe<F> mul(const Fe<F> *lds, const Fe<F> &x, int e) {
    return NTT_MUL<F>(x, lds[e]);
  }
};
// TwWords: the word-expanded constant (N elements per twiddle) from the pass's compact table
// twn[e][i], staged as N planes [i][e] so that each of a product's N reads has the lane pattern
// of TwLib's one; fe_mul_tw.  The result is the class fe_mul_lazy returns, in [0, 2p).
template <class F>
struct TwWords {
  static constexpr int ELEMS = F::N;
  template <int HALF>
  static __device__ __forceinline__ void stage(Fe<F> *lds, const uint32_t *__restrict__ twn, int, int tid, int nt) {
    for (int k = tid; k < HALF * F::N; k += nt) lds[(k % F::N) * HALF + k / F::N] = fe_load<F>(twn, k);
  }
  template <int HALF>
  static __device__ __forceinline__ Fe<F> mul(const Fe<F> *lds, const Fe<F> &x, int e) {
    Fe<F> W[F::N];
#pragma unroll
    for (int i = 0; i < F::N; i++) W[i] = lds[i * HALF + e];
    return fe_mul_tw<F>(x, W);
  }
};

__device__ __forceinline__ int brev(int x, int bits) {
  return bits ? (int)(__builtin_bitreverse32((uint32_t)x) >> (32 - bits)) : 0;
}

// Stages S0 .. S0+RR-1 of the 2^LOG_S-point DIF on the K = 2^RR register elements
// x[j] = v[b + j*GL] (GL = 2^(LOG_S-S0-RR), b = b_lo + multiple of GL*K, b_lo < GL).
// HALFZ: x[j] == 0 for j >= K/2 on entry (only meaningful for S0 == 0).
template <class F, int LOG_S, int S0, int RR, bool HALFZ, class TW>
__device__ __forceinline__ void dif_regs(Fe<F> *x, int b_lo, const Fe<F> *tw) {
  constexpr int LOG_GL = LOG_S - S0 - RR;
  constexpr int GL = 1 << LOG_GL;
  constexpr int K = 1 << RR;
#pragma unroll
  for (int qq = 0; qq < RR; qq++) {
    const int s = S0 + qq;
    const int h = 1 << (RR - 1 - qq);
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (j & h) continue;
      const int jm = j & (h - 1);
      const bool triv = (LOG_GL == 0 && jm == 0);
      if (HALFZ && qq == 0) {
        const Fe<F> a = x[j];
        x[j + h] = triv ? a : TW::template mul<(1 << LOG_S) / 2>(tw, a, (b_lo + jm * GL) << s);
      } else {
        const Fe<F> a = x[j], c = x[j + h];
#if LCPC_NTT_LAZY
        // residues in [0, 2p) throughout; the final store reduces (k_pass_b)
        x[j] = fe_add_2p<F>(a, c);
        const Fe<F> d = fe_sub_2p<F>(a, c);
        x[j + h] = triv ? d : TW::template mul<(1 << LOG_S) / 2>(tw, d, (b_lo + jm * GL) << s);
#else
        x[j] = fe_add<F>(a, c);
        x[j + h] = triv ? fe_sub<F>(a, c) : TW::template mul<(1 << LOG_S) / 2>(tw, fe_sub_lazy<F>(a, c), (b_lo + jm * GL) << s);
#endif
      }
    }
  }
}

// round size for round starting at stage S0
template <int LOG_S, int R, int S0>
constexpr int rr_of() {
  return (LOG_S - S0) < R ? (LOG_S - S0) : R;
}

// middle rounds: LDS -> registers -> LDS, lanes = adjacent vectors (v fastest)
template <class F, int LOG_S, int LOG_CW, int LOG_T, int R, int S0, int LAST_S0, class TW>
__device__ __forceinline__ void mid_rounds(Fe<F> *tile, const Fe<F> *tw, int tid) {
  if constexpr (S0 < LAST_S0) {
    constexpr int RR = rr_of<LOG_S, R, S0>();
    constexpr int CW = 1 << LOG_CW, LD = CW > 1 ? CW + 1 : 1;
    constexpr int LOG_GL = LOG_S - S0 - RR;
    constexpr int GL = 1 << LOG_GL, K = 1 << RR;
    constexpr int ITEMS = (1 << (LOG_S - RR)) * CW;
    for (int item = tid; item < ITEMS; item += (1 << LOG_T)) {
      const int v = item & (CW - 1), q = item >> LOG_CW;
      const int b_lo = q & (GL - 1);
      const int b = b_lo + ((q >> LOG_GL) << (LOG_GL + RR));
      Fe<F> x[K];
#pragma unroll
      for (int j = 0; j < K; j++) x[j] = tile[(b + j * GL) * LD + v];
      dif_regs<F, LOG_S, S0, RR, false, TW>(x, b_lo, tw);
#pragma unroll
      for (int j = 0; j < K; j++) tile[(b + j * GL) * LD + v] = x[j];
    }
    __syncthreads();
    mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, S0 + RR, LAST_S0, TW>(tile, tw, tid);
  }
}

template <int LOG_S, int R>
constexpr int last_s0() {  // first stage of the last round
  int s0 = 0;
  while (LOG_S - s0 > R) s0 += R;
  return s0;
}

// CANON: the inter-pass multiplier is w^e R^-1 (the canonical words of w^e), applied to every
// element including e = 0, so the whole transform comes out scaled by R^-1 -- i.e. in canonical
// form (see ntt_rows' canon_out).  tw2: the inter-pass twiddles w^(c bitrev(t)) laid out [t][c]
// (NttPlan::d_tw2 / d_tw2_canon), so the lanes of a store (adjacent columns c) load adjacent
// twiddles; it keeps the library product under either policy (1/8 of the products).
// twn: what the policy TW stages (TwLib: the flat table; TwWords: pass A's part of d_tw4).
template <class F, int LOG_S, int LOG_CW, int LOG_T, bool HALFZ, bool CANON, class TW>
__global__ __launch_bounds__(1 << LOG_T) void k_pass_a(const uint32_t *__restrict__ src,
                                                       size_t src_stride, size_t n_valid,
                                                       uint32_t *__restrict__ dst,
                                                       size_t dst_stride,
                                                       const uint32_t *__restrict__ twn,
                                                       const uint32_t *__restrict__ tw2,
                                                       int log_n, uint32_t *__restrict__ copy,
                                                       size_t copy_stride) {
  constexpr int S = 1 << LOG_S, CW = 1 << LOG_CW, LD = CW > 1 ? CW + 1 : 1, T = 1 << LOG_T;
  constexpr int R = LOG_S + LOG_CW - LOG_T;
  static_assert(R >= 1 && R <= LOG_S, "tile / thread shape");
  constexpr int LS0 = last_s0<LOG_S, R>();
  constexpr bool ONE_ROUND = LS0 == 0;
  __shared__ __align__(16) uint32_t smem[((ONE_ROUND ? 0 : S * LD) + S / 2 * TW::ELEMS) * F::N];
  Fe<F> *tw = reinterpret_cast<Fe<F> *>(smem);
  Fe<F> *tile = tw + S / 2 * TW::ELEMS;
  const int tid = threadIdx.x;
  const int log_m = log_n - LOG_S;
  const int groups = 1 << (log_m - LOG_CW);
  const size_t row = blockIdx.x / groups;
  const size_t c0 = (size_t)(blockIdx.x % groups) << LOG_CW;
  TW::template stage<S / 2>(tw, twn, log_m, tid, T);

  const uint32_t *in = src + row * src_stride * F::N;
  uint32_t *out = dst + row * dst_stride * F::N;
  uint32_t *cp = copy ? copy + row * copy_stride * F::N : nullptr;
  // ---- round 0 straight from HBM (exactly one item per thread: ITEMS = CW * S / 2^R = T)
  {
    constexpr int RR = rr_of<LOG_S, R, 0>();
    constexpr int K = 1 << RR, LOG_GL = LOG_S - RR, GL = 1 << LOG_GL;
    const int v = tid & (CW - 1), q = tid >> LOG_CW;  // q < GL
    const size_t c = c0 + v;
    Fe<F> x[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (HALFZ && j >= K / 2) {
        x[j] = fe_zero<F>();
      } else {
        const size_t pos = c + ((size_t)(q + j * GL) << log_m);
        if (pos < n_valid) {
          x[j] = fe_load<F>(in, pos);
          if (cp) fe_store<F>(cp, pos, x[j]);  // coalesced: lanes = adjacent columns
        } else {
          x[j] = fe_zero<F>();
        }
      }
    }
    __syncthreads();  // twiddle table
    dif_regs<F, LOG_S, 0, RR, HALFZ, TW>(x, q, tw);
    if constexpr (ONE_ROUND) {
#pragma unroll
      for (int j = 0; j < K; j++) {
        const int t = q + j * GL;  // GL == 1 here
        const size_t at = c + ((size_t)t << log_m);  // (also the [t][c] twiddle's index)
        Fe<F> y = x[j];
        if (CANON || (c && t)) y = NTT_MUL<F>(y, fe_load<F>(tw2, at));  // (w^0 = 1 otherwise)
        fe_store<F>(out, at, y);
      }
      return;
    } else {
#pragma unroll
      for (int j = 0; j < K; j++) tile[(q + j * GL) * LD + v] = x[j];
    }
  }
  if constexpr (!ONE_ROUND) {
    __syncthreads();
    mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, rr_of<LOG_S, R, 0>(), LS0, TW>(tile, tw, tid);
    // ---- last round: LDS -> registers -> twiddle -> HBM
    constexpr int RR = LOG_S - LS0;
    constexpr int K = 1 << RR;
    constexpr int ITEMS = (1 << (LOG_S - RR)) * CW;
    for (int item = tid; item < ITEMS; item += T) {
      const int v = item & (CW - 1), q = item >> LOG_CW;
      const int b = q << RR;  // GL == 1
      Fe<F> x[K];
#pragma unroll
      for (int j = 0; j < K; j++) x[j] = tile[(b + j) * LD + v];
      dif_regs<F, LOG_S, LS0, RR, false, TW>(x, 0, tw);
      const size_t c = c0 + v;
#pragma unroll
      for (int j = 0; j < K; j++) {
        const int t = b + j;
        const size_t at = c + ((size_t)t << log_m);  // (also the [t][c] twiddle's index)
        Fe<F> y = x[j];
        if (CANON || (c && t)) y = NTT_MUL<F>(y, fe_load<F>(tw2, at));  // (w^0 = 1 otherwise)
        fe_store<F>(out, at, y);
      }
    }
  }
}

template <class F, int LOG_S, int LOG_CW, int LOG_T, class TW>
__global__ __launch_bounds__(1 << LOG_T) void k_pass_b(uint32_t *__restrict__ data, size_t stride,
                                                       const uint32_t *__restrict__ twn,
                                                       int log_n) {
  constexpr int S = 1 << LOG_S, CW = 1 << LOG_CW, LD = CW > 1 ? CW + 1 : 1, T = 1 << LOG_T;
  constexpr int R = LOG_S + LOG_CW - LOG_T;
  static_assert(R >= 1 && R <= LOG_S, "tile / thread shape");
  __shared__ __align__(16) uint32_t smem[(S * LD + S / 2 * TW::ELEMS) * F::N];
  Fe<F> *tw = reinterpret_cast<Fe<F> *>(smem);
  Fe<F> *tile = tw + S / 2 * TW::ELEMS;
  const int tid = threadIdx.x;
  const int log_blocks = log_n - LOG_S;
  const int groups = 1 << (log_blocks - LOG_CW);
  const size_t row = blockIdx.x / groups;
  const size_t b0 = (size_t)(blockIdx.x % groups) << LOG_CW;
  TW::template stage<S / 2>(tw, twn, log_blocks, tid, T);
  uint32_t *io = data + (row * stride + b0 * S) * F::N;
  // ---- round 0 from HBM: lanes = adjacent positions of one block
  {
    constexpr int RR = rr_of<LOG_S, R, 0>();
    constexpr int K = 1 << RR, LOG_GL = LOG_S - RR, GL = 1 << LOG_GL;
    const int q = tid & (GL - 1), v = tid >> LOG_GL;
    Fe<F> x[K];
#pragma unroll
    for (int j = 0; j < K; j++) x[j] = fe_load<F>(io, (size_t)v * S + q + j * GL);
    __syncthreads();
    dif_regs<F, LOG_S, 0, RR, false, TW>(x, q, tw);
#pragma unroll
    for (int j = 0; j < K; j++) tile[(q + j * GL) * LD + v] = x[j];
  }
  __syncthreads();
  mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, rr_of<LOG_S, R, 0>(), LOG_S, TW>(tile, tw, tid);
  for (int idx = tid; idx < S * CW; idx += T) {
    const int v = idx >> LOG_S, t = idx & (S - 1);
#if LCPC_NTT_LAZY
    fe_store<F>(io, idx, fe_reduce_2p<F>(tile[t * LD + v]));
#else
    fe_store<F>(io, idx, tile[t * LD + v]);
#endif
  }
}

// ---- persistent passes (LCPC_NTT_PERSIST): a workgroup walks tiles blockIdx.x, + gridDim.x, ...
// Same arithmetic per element as k_pass_a / k_pass_b; what a one-tile workgroup paid per tile is
// paid once per workgroup or overlapped:
//   * the sub-FFT twiddles are staged before the loop;
//   * PF: tile i+1's round-0 loads are issued into a second register set before tile i's last
//     round (same pos < n_valid predicate; none when there is no next tile), and pass A's fused
//     coefficient-copy stores go out from those registers at the top of the next iteration;
//   * TW2R (pass A): when gridDim.x is a multiple of the groups per row a workgroup's tiles differ
//     only in the row, so a thread's 2^R inter-pass twiddles are loaded once, before the loop;
//     for any other grid the launcher takes the instantiation that loads them per tile as
//     k_pass_a does.
// Tiles are independent and no workgroup waits for another, so any grid size is correct; the
// launcher sizes it to the resident blocks (NttPlan::persist_grid).
// The second launch bound keeps three 256-thread blocks per CU (168 VGPRs).
// A use of r's registers that costs no instruction: the compiler's wait for the loads that fill
// them lands here.  The loops put it before a tile's last stores: left to the first real use (the
// next tile's round 0), the wait would also count those younger stores -- s_waitcnt vmcnt(0) at
// the top of every tile, a store round trip per tile that a one-tile workgroup never waits for.
template <class F, int K>
__device__ __forceinline__ void land_loads(Fe<F> (&r)[K]) {
#pragma unroll
  for (int j = 0; j < K; j++)
#pragma unroll
    for (int i = 0; i < F::N; i++) asm volatile("" : "+v"(r[j].v[i])::"memory");
}

// TW2R needs gridDim.x to be a multiple of the groups per row (launch_a_loop sees to it).
template <class F, int LOG_S, int LOG_CW, int LOG_T, bool HALFZ, bool CANON, class TW, bool PF, bool TW2R>
__global__ __launch_bounds__(1 << LOG_T, 3) void k_pass_a_loop(const uint32_t *__restrict__ src,
                                                               size_t src_stride, size_t n_valid,
                                                               uint32_t *__restrict__ dst, size_t dst_stride,
                                                               const uint32_t *__restrict__ twn,
                                                               const uint32_t *__restrict__ tw2, int log_n,
                                                               uint32_t *__restrict__ copy, size_t copy_stride,
                                                               size_t n_tiles) {
  constexpr int S = 1 << LOG_S, CW = 1 << LOG_CW, LD = CW > 1 ? CW + 1 : 1, T = 1 << LOG_T;
  constexpr int R = LOG_S + LOG_CW - LOG_T;
  static_assert(R >= 1 && R < LOG_S, "tile / thread shape (more than one round)");
  constexpr int LS0 = last_s0<LOG_S, R>();
  constexpr int RR0 = rr_of<LOG_S, R, 0>(), K0 = 1 << RR0, GL0 = 1 << (LOG_S - RR0);
  constexpr int KL = HALFZ ? K0 / 2 : K0;  // what round 0 loads
  // last round: NIT items of KE elements per thread (NIT * KE = 2^R)
  constexpr int RRE = LOG_S - LS0, KE = 1 << RRE, NIT = 1 << (R - RRE);
  __shared__ __align__(16) uint32_t smem[(S * LD + S / 2 * TW::ELEMS) * F::N];
  Fe<F> *tw = reinterpret_cast<Fe<F> *>(smem);
  Fe<F> *tile = tw + S / 2 * TW::ELEMS;
  const int tid = threadIdx.x;
  const int log_m = log_n - LOG_S, log_g = log_m - LOG_CW;
  const size_t gmask = ((size_t)1 << log_g) - 1;
  const size_t G = gridDim.x;
  TW::template stage<S / 2>(tw, twn, log_m, tid, T);

  const int v0 = tid & (CW - 1), q0 = tid >> LOG_CW;  // round 0's item (q0 < GL0)
  auto load0 = [&](size_t tl, Fe<F> *r) {
    const uint32_t *in = src + (tl >> log_g) * src_stride * F::N;
    const size_t c = ((tl & gmask) << LOG_CW) + v0;
#pragma unroll
    for (int j = 0; j < KL; j++) {
      const size_t pos = c + ((size_t)(q0 + j * GL0) << log_m);
      r[j] = pos < n_valid ? fe_load<F>(in, pos) : fe_zero<F>();
    }
  };
  Fe<F> w2[TW2R ? K0 : 1];
  auto load_w2 = [&](size_t c0) {
#pragma unroll
    for (int i = 0; i < NIT; i++) {
      const int item = tid + i * T;
      const size_t c = c0 + (item & (CW - 1));
#pragma unroll
      for (int j = 0; j < KE; j++) {
        const int t = ((item >> LOG_CW) << RRE) + j;
        if (CANON || (c && t))
          w2[TW2R ? i * KE + j : 0] = fe_load<F>(tw2, c + ((size_t)t << log_m));
        else
          w2[TW2R ? i * KE + j : 0] = fe_zero<F>();  // (never multiplied by: w^0 = 1)
      }
    }
    land_loads<F>(w2);  // (or every tile's last round would wait as if they were still in flight)
  };
  Fe<F> nx[PF ? KL : 1];
  size_t tl = blockIdx.x;
  if constexpr (PF) {
    if (tl < n_tiles) load0(tl, nx);
  }
  if constexpr (TW2R) load_w2((tl & gmask) << LOG_CW);  // (the same columns in every tile of this workgroup)
  for (; tl < n_tiles; tl += G) {
    const size_t row = tl >> log_g, c0 = (tl & gmask) << LOG_CW;
    uint32_t *out = dst + row * dst_stride * F::N;
    // ---- round 0 from the registers the previous iteration filled (exactly one item per thread)
    Fe<F> x[K0];
    if constexpr (PF) {
#pragma unroll
      for (int j = 0; j < KL; j++) x[j] = nx[j];
    } else {
      load0(tl, x);
    }
#pragma unroll
    for (int j = KL; j < K0; j++) x[j] = fe_zero<F>();
    if (copy) {
      uint32_t *cp = copy + row * copy_stride * F::N;
#pragma unroll
      for (int j = 0; j < KL; j++) {
        const size_t pos = c0 + v0 + ((size_t)(q0 + j * GL0) << log_m);
        if (pos < n_valid) fe_store<F>(cp, pos, x[j]);  // coalesced: lanes = adjacent columns
      }
    }
    __syncthreads();  // twiddle table (first tile); the previous tile's last-round reads of `tile`
    dif_regs<F, LOG_S, 0, RR0, HALFZ, TW>(x, q0, tw);
#pragma unroll
    for (int j = 0; j < K0; j++) tile[(q0 + j * GL0) * LD + v0] = x[j];
    __syncthreads();
    mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, RR0, LS0, TW>(tile, tw, tid);
    if constexpr (PF) {
      if (tl + G < n_tiles) load0(tl + G, nx);
    }
    // ---- last round: LDS -> registers -> twiddle -> HBM
#pragma unroll
    for (int i = 0; i < NIT; i++) {
      const int item = tid + i * T;
      const int v = item & (CW - 1), b = (item >> LOG_CW) << RRE;  // GL == 1
      Fe<F> y[KE];
#pragma unroll
      for (int j = 0; j < KE; j++) y[j] = tile[(b + j) * LD + v];
      dif_regs<F, LOG_S, LS0, RRE, false, TW>(y, 0, tw);
      const size_t c = c0 + v;
#pragma unroll
      for (int j = 0; j < KE; j++) {
        const int t = b + j;
        if (CANON || (c && t)) {  // (w^0 = 1 otherwise; at is also the [t][c] twiddle's index)
          if constexpr (TW2R)
            y[j] = NTT_MUL<F>(y[j], w2[i * KE + j]);
          else
            y[j] = NTT_MUL<F>(y[j], fe_load<F>(tw2, c + ((size_t)t << log_m)));
        }
      }
      if constexpr (PF) {
        if (i == NIT - 1) land_loads<F>(nx);
      }
#pragma unroll
      for (int j = 0; j < KE; j++) fe_store<F>(out, c + ((size_t)(b + j) << log_m), y[j]);
    }
  }
}

template <class F, int LOG_S, int LOG_CW, int LOG_T, class TW, bool PF>
__global__ __launch_bounds__(1 << LOG_T, 3) void k_pass_b_loop(uint32_t *__restrict__ data, size_t stride,
                                                               const uint32_t *__restrict__ twn, int log_n,
                                                               size_t n_tiles) {
  constexpr int S = 1 << LOG_S, CW = 1 << LOG_CW, LD = CW > 1 ? CW + 1 : 1, T = 1 << LOG_T;
  constexpr int R = LOG_S + LOG_CW - LOG_T;
  static_assert(R >= 1 && R < LOG_S, "tile / thread shape (more than one round)");
  constexpr int LS0 = last_s0<LOG_S, R>();
  constexpr int RR0 = rr_of<LOG_S, R, 0>(), K0 = 1 << RR0, LOG_GL0 = LOG_S - RR0, GL0 = 1 << LOG_GL0;
  __shared__ __align__(16) uint32_t smem[(S * LD + S / 2 * TW::ELEMS) * F::N];
  Fe<F> *tw = reinterpret_cast<Fe<F> *>(smem);
  Fe<F> *tile = tw + S / 2 * TW::ELEMS;
  const int tid = threadIdx.x;
  const int log_blocks = log_n - LOG_S, log_g = log_blocks - LOG_CW;
  const size_t gmask = ((size_t)1 << log_g) - 1;
  const size_t G = gridDim.x;
  TW::template stage<S / 2>(tw, twn, log_blocks, tid, T);
  const int q0 = tid & (GL0 - 1), v0 = tid >> LOG_GL0;  // round 0: lanes = adjacent positions of one block
  auto tile_io = [&](size_t tl) { return data + ((tl >> log_g) * stride + (((tl & gmask) << LOG_CW) << LOG_S)) * F::N; };
  auto load0 = [&](size_t tl, Fe<F> *r) {
    const uint32_t *io = tile_io(tl);
#pragma unroll
    for (int j = 0; j < K0; j++) r[j] = fe_load<F>(io, (size_t)v0 * S + q0 + j * GL0);
  };
  Fe<F> nx[PF ? K0 : 1];
  size_t tl = blockIdx.x;
  if constexpr (PF) {
    if (tl < n_tiles) load0(tl, nx);
  }
  for (; tl < n_tiles; tl += G) {
    uint32_t *io = tile_io(tl);
    {
      Fe<F> x[K0];
      if constexpr (PF) {
#pragma unroll
        for (int j = 0; j < K0; j++) x[j] = nx[j];
      } else {
        load0(tl, x);
      }
      __syncthreads();  // twiddle table (first tile); the previous tile's final reads of `tile`
      dif_regs<F, LOG_S, 0, RR0, false, TW>(x, q0, tw);
#pragma unroll
      for (int j = 0; j < K0; j++) tile[(q0 + j * GL0) * LD + v0] = x[j];
    }
    __syncthreads();
    mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, RR0, LS0, TW>(tile, tw, tid);
    if constexpr (PF) {
      if (tl + G < n_tiles) load0(tl + G, nx);
    }
    mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, LS0, LOG_S, TW>(tile, tw, tid);  // the last round
    if constexpr (PF) land_loads<F>(nx);
    for (int idx = tid; idx < S * CW; idx += T) {
      const int v = idx >> LOG_S, t = idx & (S - 1);
#if LCPC_NTT_LAZY
      fe_store<F>(io, idx, fe_reduce_2p<F>(tile[t * LD + v]));
#else
      fe_store<F>(io, idx, tile[t * LD + v]);
#endif
    }
  }
}

#if LCPC_NTT_LEAF_FUSE
// ---- pass B that also hashes the column leaves (LCPC_NTT_LEAF_FUSE): the commitment's last pass
// over the codeword leaves the BLAKE3 chunk chaining values of every column, so no leaf kernel
// reads the codeword back.  16-byte elements (a "row" of a leaf message is 16 bytes: chunk k of the
// message 32 zero bytes || row 0 || row 1 ... covers rows 64k - 2 .. 64k + 61, the rows below 0
// standing for the zero prefix), T == S threads.
// A workgroup is one (chunk, block of S columns) and walks the chunk in tiles of CW rows of that
// one block from row 64k - 2 on: tile slot v of tile i is row 64k - 2 + CW i + v, so a tile is CW/4
// whole 64-byte blocks of each column's message.  Slots outside [0, n_rows) load zeros and store
// nothing; the transform of a zero row is zero words (fe_add_2p, fe_sub_2p and the twiddle
// products all map 0 to 0), which is what the prefix and the pad past the message hash as.  After
// the last round thread t holds column b S + t of the tile's CW rows, reduced to canonical words:
// it stores them (lanes = adjacent columns, as k_pass_b's final stores) and compresses them into
// the chunk's chaining value, kept in registers across the tiles.  cvs[chunk][col] (8 words) is
// k_leaf_chunks' layout; a one-chunk message's value carries ROOT (it is the leaf).
// blockIdx = chunk * blocks + b: the last chunk, the only short one, comes last.
// PF: the next tile's round-0 loads are issued before the last round and the hash.
template <class F, int LOG_S, int LOG_CW, int LOG_T, class TW, bool PF>
__global__ __launch_bounds__(1 << LOG_T, 3) void k_pass_b_leaf(uint32_t *__restrict__ data, size_t stride,
                                                               const uint32_t *__restrict__ twn, int log_n,
                                                               int n_rows, int n_chunks, uint32_t *__restrict__ cvs) {
  constexpr int S = 1 << LOG_S, CW = 1 << LOG_CW, LD = CW > 1 ? CW + 1 : 1, T = 1 << LOG_T;
  constexpr int R = LOG_S + LOG_CW - LOG_T;
  static_assert(R >= 1 && R < LOG_S, "tile / thread shape (more than one round)");
  static_assert(F::N == 4 && T == S && CW >= 4 && 64 % CW == 0, "a thread owns CW/4 whole blocks of one column");
  constexpr int LS0 = last_s0<LOG_S, R>();
  constexpr int RR0 = rr_of<LOG_S, R, 0>(), K0 = 1 << RR0, LOG_GL0 = LOG_S - RR0, GL0 = 1 << LOG_GL0;
  __shared__ __align__(16) uint32_t smem[(S * LD + S / 2 * TW::ELEMS) * F::N];
  Fe<F> *tw = reinterpret_cast<Fe<F> *>(smem);
  Fe<F> *tile = tw + S / 2 * TW::ELEMS;
  const int tid = threadIdx.x;
  const int log_blocks = log_n - LOG_S;
  const int chunk = (int)(blockIdx.x >> log_blocks);
  const size_t b = blockIdx.x & (((size_t)1 << log_blocks) - 1);
  TW::template stage<S / 2>(tw, twn, log_blocks, tid, T);
  // the chunk's rows, tiles and message blocks (the same in every thread)
  const int row_base = 64 * chunk - 2;
  const int row_end = 64 * chunk + 62 < n_rows ? 64 * chunk + 62 : n_rows;
  const int n_tiles = (row_end - row_base + CW - 1) / CW;
  const int left_words = 8 + 4 * n_rows - 256 * chunk;  // message words from this chunk on
  const int cw = left_words < 256 ? left_words : 256;
  const int nb = (cw + 15) / 16;
  uint32_t *io = data + (b << LOG_S) * F::N;  // column b S of row 0
  const int q0 = tid & (GL0 - 1), v0 = tid >> LOG_GL0;  // round 0: lanes = adjacent positions of one row's block
  auto load0 = [&](int i, Fe<F> *r) {
    const int row = row_base + CW * i + v0;
    const bool in = row >= 0 && row < n_rows;
#pragma unroll
    for (int j = 0; j < K0; j++) r[j] = in ? fe_load<F>(io + (size_t)row * stride * F::N, q0 + j * GL0) : fe_zero<F>();
  };
  uint32_t cv[8];
  b3::iv(cv);
  Fe<F> nx[PF ? K0 : 1];
  if constexpr (PF) load0(0, nx);
  for (int i = 0; i < n_tiles; i++) {
    {
      Fe<F> x[K0];
      if constexpr (PF) {
#pragma unroll
        for (int j = 0; j < K0; j++) x[j] = nx[j];
      } else {
        load0(i, x);
      }
      __syncthreads();  // twiddle table (first tile); the previous tile's final reads of `tile`
      dif_regs<F, LOG_S, 0, RR0, false, TW>(x, q0, tw);
#pragma unroll
      for (int j = 0; j < K0; j++) tile[(q0 + j * GL0) * LD + v0] = x[j];
    }
    __syncthreads();
    mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, RR0, LS0, TW>(tile, tw, tid);
    if constexpr (PF) {
      if (i + 1 < n_tiles) load0(i + 1, nx);
    }
    mid_rounds<F, LOG_S, LOG_CW, LOG_T, R, LS0, LOG_S, TW>(tile, tw, tid);  // the last round
    if constexpr (PF) land_loads<F>(nx);
    // ---- column b S + tid of the tile's rows: store, then hash
    Fe<F> y[CW];
#pragma unroll
    for (int v = 0; v < CW; v++) {
#if LCPC_NTT_LAZY
      y[v] = fe_reduce_2p<F>(tile[tid * LD + v]);
#else
      y[v] = tile[tid * LD + v];
#endif
    }
#pragma unroll
    for (int v = 0; v < CW; v++) {
      const int row = row_base + CW * i + v;
      if (row >= 0 && row < n_rows) fe_store<F>(io + (size_t)row * stride * F::N, tid, y[v]);
    }
#pragma unroll
    for (int k = 0; k < CW / 4; k++) {
      const int blk = i * (CW / 4) + k;  // block of the chunk
      if (blk < nb) {
        uint32_t msg[16];
#pragma unroll
        for (int e = 0; e < 4; e++) fe_canon_repr_words<F>(y[4 * k + e], msg + 4 * e);
        const int left = cw - 16 * blk;
        uint32_t flags = blk == 0 ? b3::CHUNK_START : 0u;
        if (blk == nb - 1) flags |= b3::CHUNK_END | (n_chunks == 1 ? b3::ROOT : 0u);
        b3::compress(cv, msg, (uint64_t)chunk, left >= 16 ? 64u : (uint32_t)(4 * left), flags);
      }
    }
  }
  b3::store8(cvs + ((((size_t)chunk << log_blocks) + b) * S + tid) * 8, cv);
}
#endif  // LCPC_NTT_LEAF_FUSE

// Blocks of `threads` threads of kernel `k` that one CU holds, from the kernel's own LDS and
// register footprint (160 KiB of LDS, 512 VGPRs per lane in granules of 8, 8 waves per SIMD).
template <class K>
int blocks_per_cu(K k, int threads) {
  hipFuncAttributes at;
  if (hipFuncGetAttributes(&at, reinterpret_cast<const void *>(k)) != hipSuccess) {
    (void)hipGetLastError();
    return 1;
  }
  const int waves = (threads + 63) / 64;
  const int regs = at.numRegs > 0 ? (at.numRegs + 7) / 8 * 8 : 8;
  int per_simd = 512 / regs;
  if (per_simd > 8) per_simd = 8;
  int n = per_simd * 4 / waves;
  if (at.sharedSizeBytes > 0 && (int)(160 * 1024 / at.sharedSizeBytes) < n) n = (int)(160 * 1024 / at.sharedSizeBytes);
  return n < 1 ? 1 : n;
}

// grid: the workgroups to launch (at most the tiles).  query: only lower *query to this
// kernel's blocks per CU (ntt_plan_init sizes NttPlan::persist_grid with it); nothing is launched.
template <class F, int LOG_S, int LOG_CW, int LOG_T, bool HALFZ, bool CANON, class TW, bool PF = true,
          bool TW2R = true>
hipError_t launch_a_loop(const uint32_t *src, size_t ss, size_t nv, uint32_t *dst, size_t ds, const uint32_t *tw,
                         int log_n, size_t n_rows, hipStream_t s, uint32_t *cp, size_t cs, const uint32_t *tw2,
                         size_t grid, int *query = nullptr) {
  auto k = k_pass_a_loop<F, LOG_S, LOG_CW, LOG_T, HALFZ, CANON, TW, PF, TW2R>;
  if (query) {
    const int b = blocks_per_cu(k, 1 << LOG_T);
    if (b < *query) *query = b;
    return hipSuccess;
  }
  const size_t tiles = n_rows << (log_n - LOG_S - LOG_CW);
  if (grid > tiles) grid = tiles;
  if constexpr (TW2R) {  // a workgroup keeps its column group only on a multiple of the groups
    if (grid & (((size_t)1 << (log_n - LOG_S - LOG_CW)) - 1))
      return launch_a_loop<F, LOG_S, LOG_CW, LOG_T, HALFZ, CANON, TW, PF, false>(src, ss, nv, dst, ds, tw, log_n, n_rows,
                                                                                s, cp, cs, tw2, grid);
  }
  prof::Scope ps("ntt_pass_a", s);
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(1 << LOG_T), 0, s, src, ss, nv, dst, ds, tw, tw2, log_n, cp, cs,
                     tiles);
  return hipGetLastError();
}

template <class F, int LOG_S, int LOG_CW, int LOG_T, class TW, bool PF = true>
hipError_t launch_b_loop(uint32_t *dst, size_t ds, const uint32_t *tw, int log_n, size_t n_rows, hipStream_t s,
                         size_t grid, int *query = nullptr) {
  auto k = k_pass_b_loop<F, LOG_S, LOG_CW, LOG_T, TW, PF>;
  if (query) {
    const int b = blocks_per_cu(k, 1 << LOG_T);
    if (b < *query) *query = b;
    return hipSuccess;
  }
  const size_t tiles = n_rows << (log_n - LOG_S - LOG_CW);
  if (grid > tiles) grid = tiles;
  prof::Scope ps("ntt_pass_b", s);
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(1 << LOG_T), 0, s, dst, ds, tw, log_n, tiles);
  return hipGetLastError();
}

template <class F, int LOG_S, int LOG_CW, int LOG_T, bool HALFZ, bool CANON, class TW>
hipError_t launch_a(const uint32_t *src, size_t ss, size_t nv, uint32_t *dst, size_t ds,
                    const uint32_t *tw, int log_n, size_t n_rows, hipStream_t s, uint32_t *cp,
                    size_t cs, const uint32_t *tw2) {
  const size_t groups = (size_t)1 << (log_n - LOG_S - LOG_CW);
  prof::Scope ps("ntt_pass_a", s);
  hipLaunchKernelGGL((k_pass_a<F, LOG_S, LOG_CW, LOG_T, HALFZ, CANON, TW>), dim3((unsigned)(n_rows * groups)),
                     dim3(1 << LOG_T), 0, s, src, ss, nv, dst, ds, tw, tw2, log_n, cp, cs);
  return hipGetLastError();
}

template <class F, int LOG_S, int LOG_CW, int LOG_T, class TW>
hipError_t launch_b(uint32_t *dst, size_t ds, const uint32_t *tw, int log_n, size_t n_rows,
                    hipStream_t s) {
  const size_t groups = (size_t)1 << (log_n - LOG_S - LOG_CW);
  prof::Scope ps("ntt_pass_b", s);
  hipLaunchKernelGGL((k_pass_b<F, LOG_S, LOG_CW, LOG_T, TW>), dim3((unsigned)(n_rows * groups)),
                     dim3(1 << LOG_T), 0, s, dst, ds, tw, log_n);
  return hipGetLastError();
}

#if LCPC_NTT_LEAF_FUSE
// One workgroup per (chunk, block of 2^LOG_S columns).  The scope keeps pass B's name, so a profile
// still sums an encode time; it now includes the leaf hashing.
template <class F, int LOG_S, int LOG_CW, int LOG_T, class TW, bool PF = LCPC_NTT_LEAF_FUSE_PF != 0>
hipError_t launch_b_leaf(uint32_t *dst, size_t ds, const uint32_t *tw, int log_n, size_t n_rows, size_t n_chunks,
                         uint32_t *cvs, hipStream_t s) {
  const size_t grid = n_chunks << (log_n - LOG_S);
  if (n_rows == 0 || n_rows > ((size_t)1 << 24) || grid > 0x7fffffffu) return hipErrorInvalidValue;
  prof::Scope ps("ntt_pass_b", s);
  hipLaunchKernelGGL((k_pass_b_leaf<F, LOG_S, LOG_CW, LOG_T, TW, PF>), dim3((unsigned)grid), dim3(1 << LOG_T), 0, s, dst,
                     ds, tw, log_n, (int)n_rows, (int)n_chunks, cvs);
  return hipGetLastError();
}
#endif

}  // namespace ntt_v2
}  // namespace lcpc
