// blake3_dev.hpp -- the BLAKE3 device primitives the leaf kernels share (blake3.hip, pos_read.hip):
// the compression function, parent nodes, 32-byte loads and stores, and the column-major chunk
// body that hashes 1-KiB chunks of [column][row] matrices through LDS.  Device code only; every
// function is inlined into the kernel that uses it.
#pragma once
#include "field.hpp"

namespace lcpc {
namespace b3 {

constexpr uint32_t IV0 = 0x6A09E667u, IV1 = 0xBB67AE85u, IV2 = 0x3C6EF372u, IV3 = 0xA54FF53Au,
                   IV4 = 0x510E527Fu, IV5 = 0x9B05688Cu, IV6 = 0x1F83D9ABu, IV7 = 0x5BE0CD19u;
enum : uint32_t { CHUNK_START = 1, CHUNK_END = 2, PARENT = 4, ROOT = 8 };

// message schedule: round r uses m[SCHED[r][i]]  (permutation 2,6,3,10,7,0,4,13,1,11,12,5,9,14,15,8)
__host__ __device__ constexpr int sched(int r, int i) {
  constexpr int P[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  int x = i;
  for (int k = 0; k < r; k++) x = P[x];
  return x;
}

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_rotateright32(x, n); }

#define B3G(a, b, c, d, mx, my)          \
  a = a + b + (mx);                      \
  d = rotr(d ^ a, 16);                   \
  c = c + d;                             \
  b = rotr(b ^ c, 12);                   \
  a = a + b + (my);                      \
  d = rotr(d ^ a, 8);                    \
  c = c + d;                             \
  b = rotr(b ^ c, 7);

// cv = first half of compress(cv, m, counter, len, flags)
__device__ __forceinline__ void compress(uint32_t cv[8], const uint32_t m[16], uint64_t counter,
                                         uint32_t block_len, uint32_t flags) {
  uint32_t s0 = cv[0], s1 = cv[1], s2 = cv[2], s3 = cv[3], s4 = cv[4], s5 = cv[5], s6 = cv[6],
           s7 = cv[7];
  uint32_t s8 = IV0, s9 = IV1, s10 = IV2, s11 = IV3;
  uint32_t s12 = (uint32_t)counter, s13 = (uint32_t)(counter >> 32), s14 = block_len, s15 = flags;
#pragma unroll
  for (int r = 0; r < 7; r++) {
    B3G(s0, s4, s8, s12, m[sched(r, 0)], m[sched(r, 1)]);
    B3G(s1, s5, s9, s13, m[sched(r, 2)], m[sched(r, 3)]);
    B3G(s2, s6, s10, s14, m[sched(r, 4)], m[sched(r, 5)]);
    B3G(s3, s7, s11, s15, m[sched(r, 6)], m[sched(r, 7)]);
    B3G(s0, s5, s10, s15, m[sched(r, 8)], m[sched(r, 9)]);
    B3G(s1, s6, s11, s12, m[sched(r, 10)], m[sched(r, 11)]);
    B3G(s2, s7, s8, s13, m[sched(r, 12)], m[sched(r, 13)]);
    B3G(s3, s4, s9, s14, m[sched(r, 14)], m[sched(r, 15)]);
  }
  cv[0] = s0 ^ s8;
  cv[1] = s1 ^ s9;
  cv[2] = s2 ^ s10;
  cv[3] = s3 ^ s11;
  cv[4] = s4 ^ s12;
  cv[5] = s5 ^ s13;
  cv[6] = s6 ^ s14;
  cv[7] = s7 ^ s15;
}

__device__ __forceinline__ void iv(uint32_t cv[8]) {
  cv[0] = IV0; cv[1] = IV1; cv[2] = IV2; cv[3] = IV3;
  cv[4] = IV4; cv[5] = IV5; cv[6] = IV6; cv[7] = IV7;
}

// BLAKE3 of a 64-byte message (one chunk, one block) = lcpc-2d Merkle node.
__device__ __forceinline__ void hash64(const uint32_t m[16], uint32_t out[8]) {
  iv(out);
  compress(out, m, 0, 64, CHUNK_START | CHUNK_END | ROOT);
}

__device__ __forceinline__ void parent_cv(const uint32_t l[8], const uint32_t r[8], bool root,
                                          uint32_t out[8]) {
  uint32_t m[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    m[i] = l[i];
    m[8 + i] = r[i];
  }
  iv(out);
  compress(out, m, 0, 64, PARENT | (root ? ROOT : 0u));
}

__device__ __forceinline__ void load8(const uint32_t *p, uint32_t v[8]) {
  const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(uint32_t *p, const uint32_t v[8]) {
  reinterpret_cast<uint4 *>(p)[0] = make_uint4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<uint4 *>(p)[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// Chunks of a column-major matrix ([column][row], a column's message words contiguous in memory:
// the SDIG commitments and the PoS column files).  Read lane-per-column, every load of a wave
// touches 64 columns n_rows * B bytes apart; here the wave loads each 64-byte block of its
// 64 columns cooperatively instead -- 4 adjacent lanes read one column's block, so a load
// instruction covers 16 columns x 64 contiguous bytes -- and hands the blocks over through LDS
// (rows padded to 80 B so the per-column reads are bank-conflict free).  Needs
// n_rows * N % 4 == 0 (16-B aligned columns); the message word w of a column is memory word w - 8
// of the column (w >= 8), and a 4-word unit lies wholly inside or outside the message.
// fuse2: a two-chunk message hashed whole by one wave (grid.y = 1, leaves written directly).
//
// SLICE (the PoS chunk-CV cache, canonical input only): m holds, per column, only the rows of the
// chunks [chunk0, chunk0 + gridDim.y) of messages n_rows rows long -- column c at m + c * col_words
// words (col_words a multiple of 4, at least the slice's words rounded up to 4), its word 0 being
// message word w_base (a multiple of 4: 8 + 2 * first row of chunk0).  n_rows may be odd there, so
// the message can end inside a 4-word unit: the words past it are zeroed.  Every element is checked
// < p (*bad set otherwise: from_repr would refuse it), and the chaining value of (chunk, col) goes
// to cvs[(chunk - cv_chunk0) * cv_stride + col] whatever n_chunks is -- straight into a
// [chunk][column] array of cv_stride columns whose first chunk row is chunk cv_chunk0 (0: the whole
// cache), cvs already offset to this launch's first column.
struct CmSlice {
  size_t col_words, w_base, cv_stride;
  int chunk0, cv_chunk0;
  uint32_t *bad;
};

// EVAL (a SLICE launch, the checkable read's segments): the pass also leaves each (chunk, column)'s
// share of a weighted column sum, partials[(chunk - cv_chunk0) * cv_stride + col] = sum over the
// chunk's rows r of weights[r - row0] * element r -- Montgomery weights and canonical elements, so
// canonical sums (what k_leaf_chunks_eval gives for row-major input).  The row of an element is the
// same for every lane, so the weight loads are uniform.  A column with an element that is not < p is
// reported on its own there, bad[col] = 1, instead of in one flag for the launch.
struct CmEval {
  const uint32_t *weights = nullptr;  // the slice's rows [row0, ...), Montgomery
  uint32_t *partials = nullptr;
  size_t row0 = 0;
};

// One chunk of one wave's 64 columns [col0, col0 + 64) of m (column c at m + c * col_words words, its
// word 0 being message word w_base): the chunk's blocks staged through the wave's LDS rows `stage`,
// the next block's loads in flight while this one compresses; cv = the chunk's chaining value (ROOT
// when n_chunks == 1).  TAIL: the message may end inside a 4-word unit (n_rows odd), the words past it
// are zeroed.  CHECK: noncanon |= an element is not < p.  EVAL: acc += sum over the chunk's rows r of
// weights[r - row0] * element r (the element as loaded; the row is the same in every lane, so a
// wave-uniform weights pointer makes the weight loads scalar).  Every caller passes wave-uniform
// arguments but for the lane's own cv / acc / noncanon.
template <class F, bool CANON, bool TAIL, bool CHECK, bool EVAL>
__device__ __forceinline__ void cm_chunk_cv(uint4 (*__restrict__ stage)[5], const uint32_t *__restrict__ m,
                                            size_t n_rows, size_t n_cols, size_t col0, size_t col_words,
                                            size_t w_base, int chunk, int n_chunks,
                                            const uint32_t *__restrict__ weights, size_t row0, uint32_t cv[8],
                                            Fe<F> &acc, bool &noncanon) {
  constexpr int N = F::N;
  constexpr int EPB = 16 / N;
  const int lane = threadIdx.x & 63;
  const size_t msg_words = 8 + n_rows * N;  // the column's message, in words
  const int unit = lane & 3, csub = lane >> 2;
  // block b (of the chunk starting at message word w0): this lane's 4 loads, unit `unit` (words
  // 4 unit .. +3) of column col0 + csub + 16 i
  auto gload = [&](size_t w0, int b, uint4 r[4]) {
    const size_t w = w0 + 16 * (size_t)b + 4 * unit;  // message word
    const bool in = w >= 8 && w < msg_words;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const size_t c = col0 + csub + 16 * i;
      r[i] = in && c < n_cols ? reinterpret_cast<const uint4 *>(m + c * col_words + (w - w_base))[0]
                              : make_uint4(0, 0, 0, 0);
      if constexpr (TAIL) {  // the message ends inside this unit (msg_words is even)
        if (w + 2 == msg_words) r[i].z = r[i].w = 0;
      }
    }
  };
  auto wave_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto lput = [&](const uint4 r[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) stage[csub + 16 * i][unit] = r[i];
    wave_sync();
  };
  const size_t w0 = (size_t)chunk * 256;
  const size_t cw = msg_words - w0 < 256 ? msg_words - w0 : 256;
  const int nb = (int)((cw + 15) / 16);
  iv(cv);
  uint4 r[4];
  gload(w0, 0, r);
  lput(r);
  for (int b = 0; b < nb; b++) {
    const bool more = b + 1 < nb;
    if (more) gload(w0, b + 1, r);
    uint32_t msg[16];
    {
      const uint4 *row = stage[lane];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint4 q = row[k];
        msg[4 * k] = q.x; msg[4 * k + 1] = q.y; msg[4 * k + 2] = q.z; msg[4 * k + 3] = q.w;
      }
    }
    wave_sync();  // every lane has read block b before block b + 1 overwrites the stage
    // element words -> repr words (Montgomery -> canonical unless CANON); the zero prefix and
    // words past the message stay zero either way (from_mont(0) = 0, and they load as zero)
#pragma unroll
    for (int k = 0; k < EPB; k++) {
      Fe<F> e;
#pragma unroll
      for (int i = 0; i < N; i++) e.v[i] = msg[k * N + i];
      if constexpr (CHECK) noncanon |= !fe_is_canonical<F>(e);  // (prefix and tail words are zero)
      if constexpr (EVAL) {
        // the element's message word and row (the same in every lane); the prefix and the pad
        // past an odd row count hold no element
        const size_t ew = w0 + 16 * (size_t)b + (size_t)k * N;
        if (ew >= 8 && ew < msg_words) acc = fe_add<F>(acc, fe_mul<F>(fe_load<F>(weights, (ew - 8) / N - row0), e));
      }
      uint32_t w[N];
      if constexpr (CANON)
        fe_canon_repr_words<F>(e, w);
      else
        fe_repr_words<F>(e, w);
#pragma unroll
      for (int i = 0; i < N; i++) msg[k * N + i] = w[i];
    }
    const size_t left = cw - 16 * (size_t)b;
    const uint32_t blen = left >= 16 ? 64u : (uint32_t)(4 * left);
    uint32_t flags = b == 0 ? CHUNK_START : 0u;
    if (b == nb - 1) flags |= CHUNK_END | (n_chunks == 1 ? ROOT : 0u);
    compress(cv, msg, (uint64_t)chunk, blen, flags);
    if (more) lput(r);
  }
}

// The leaf of one column from its n_chunks chunk chaining values cvs[0], cvs[stride], ... (32-byte
// values `stride` values apart), which are left untouched: the register stack of blake3.hip's
// k_leaf_fold_stack as a function.  level[k] = the root of a complete 2^k-chunk subtree, present iff
// bit k of the number of chunks taken so far is set; the last chunk merges with every level still
// present, lowest first, ROOT on the last parent (a one-chunk column's chaining value carries ROOT
// already).  n_chunks must be uniform over the wave: the stack is then picked over by unrolled
// compares, never indexed dynamically.  n_chunks >= 1 and n_chunks - 1 < 2^D.
template <int D>
__device__ __forceinline__ void leaf_fold_stack(const uint32_t *__restrict__ cvs, size_t stride, int n_chunks,
                                                uint32_t cv[8]) {
  uint32_t level[D][8], nxt[8];
  load8(cvs, nxt);
  for (int i = 0; i < n_chunks; i++) {
#pragma unroll
    for (int q = 0; q < 8; q++) cv[q] = nxt[q];
    if (i + 1 < n_chunks) load8(cvs + (size_t)(i + 1) * stride * 8, nxt);  // in flight over the merges
    const bool last = i + 1 == n_chunks;
    for (int k = 0; k < D; k++) {
      const bool top = (i >> (k + 1)) == 0;  // no level above k is present
      if ((i >> k) & 1) {
        uint32_t l[8], o[8];
#pragma unroll
        for (int j = 0; j < D; j++)
          if (j == k) {
#pragma unroll
            for (int q = 0; q < 8; q++) l[q] = level[j][q];
          }
        parent_cv(l, cv, last && top, o);
#pragma unroll
        for (int q = 0; q < 8; q++) cv[q] = o[q];
      } else if (!last) {
#pragma unroll
        for (int j = 0; j < D; j++)
          if (j == k) {
#pragma unroll
            for (int q = 0; q < 8; q++) level[j][q] = cv[q];
          }
        break;
      }
      if (last && top) break;
    }
  }
}

template <class F, bool CANON, bool SLICE, bool EVAL = false>
__device__ __forceinline__ void leaf_chunks_cm_body(const uint32_t *__restrict__ m, size_t n_rows, size_t n_cols,
                                                    uint32_t *__restrict__ cvs, uint8_t *__restrict__ leaves,
                                                    int n_chunks, int fuse2, const CmSlice &sl,
                                                    const CmEval &ev = CmEval{}) {
  constexpr int N = F::N;
  static_assert(16 % N == 0 && 8 % N == 0, "element must tile a BLAKE3 block");
  static_assert(!EVAL || SLICE, "the weighted sums ride on slice launches");
  __shared__ uint4 stage[4][64][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t col0 = ((size_t)blockIdx.x * 4 + wave) * 64, col = col0 + lane;
  if (col0 >= n_cols) return;  // whole waves
  const size_t col_words = SLICE ? sl.col_words : n_rows * N, w_base = SLICE ? sl.w_base : 8;
  bool noncanon = false;
  Fe<F> acc = fe_zero<F>();
  // one chunk's chaining value (cm_chunk_cv)
  auto chunk_cv = [&](int chunk, uint32_t cv[8]) {
    cm_chunk_cv<F, CANON, SLICE, SLICE, EVAL>(stage[wave], m, n_rows, n_cols, col0, col_words, w_base, chunk, n_chunks,
                                              ev.weights, ev.row0, cv, acc, noncanon);
  };
  uint32_t cv[8];
  if (fuse2) {
    // a two-chunk message (cfg4's 1184-byte leaves) whole in one wave: both chaining values in
    // registers and their ROOT parent, no scratch round trip and no merge launch
    uint32_t cv1[8], leaf[8];
    chunk_cv(0, cv);
    chunk_cv(1, cv1);
    parent_cv(cv, cv1, true, leaf);
    if (col < n_cols) store8(reinterpret_cast<uint32_t *>(leaves + 32 * col), leaf);
    return;
  }
  const int chunk = (SLICE ? sl.chunk0 : 0) + blockIdx.y;
  chunk_cv(chunk, cv);
  if (col >= n_cols) return;
  if constexpr (SLICE) {
    const size_t slot = (size_t)(chunk - sl.cv_chunk0) * sl.cv_stride + col;
    if constexpr (EVAL) {
      if (noncanon) sl.bad[col] = 1u;
      fe_store<F>(ev.partials, slot, acc);
    } else {
      if (noncanon) atomicOr(sl.bad, 1u);
    }
    store8(cvs + slot * 8, cv);
    return;
  }
  if (n_chunks == 1 && leaves) {
    store8(reinterpret_cast<uint32_t *>(leaves + 32 * col), cv);
  } else {
    store8(cvs + ((size_t)chunk * n_cols + col) * 8, cv);
  }
}

}  // namespace b3
}  // namespace lcpc
