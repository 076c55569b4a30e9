// pos_read.hip -- checkable reads of a stored file on gfx950: a column opened on a chunk range only.
//
// A column's leaf is BLAKE3(32 zero bytes || the column): a left-balanced tree over 1-KiB chunks.
// Opened on chunks [chunk_lo, chunk_hi) the column is its elements there (the segment) plus the
// chaining values of the subtrees that cover the other chunks.  The server computes those cover
// values from chunk CVs (k_cover_values); the client hashes the segments' chunks (the slice form of
// the column-major chunk kernel, with the weighted column sums of the row check riding on the same
// pass: k_segment_chunks) and folds them with the covers into the leaves (k_segment_groups,
// k_segment_leaves).
//
// Every fold here is one register stack of chaining values per thread (CvStack).  Lanes are columns
// and the tree's shape is the same for every column, so which stack level is read or written is
// uniform: the levels are picked over by unrolled compares (static register indices), never
// indexed dynamically -- the rule of blake3.hip's k_leaf_fold_stack.
#include "blake3_dev.hpp"
#include "field.hpp"
#include "kernels.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

using namespace b3;

// The values of a post-order walk that have no parent yet: `top` is the newest, level[0 .. sp) the
// ones below it, oldest first.  A tree of height h needs D >= h levels.  A push past D is dropped
// (the result is then wrong, nothing is written out of bounds); the launchers size D from the chunk
// count.
template <int D>
struct CvStack {
  uint32_t level[D][8] = {};
  uint32_t top[8] = {};
  int sp = 0;
  bool has = false;

  __device__ __forceinline__ int depth() const { return sp + (has ? 1 : 0); }

  // (The level is chosen by selects on the uniform sp, not by branches around the copies: the
  // compiler merges such branches' stores into one dynamically indexed store, which sends the
  // whole stack to scratch.)
  __device__ __forceinline__ void push(const uint32_t cv[8]) {
    const int at = has ? sp : -1;
#pragma unroll
    for (int j = 0; j < D; j++) {
#pragma unroll
      for (int q = 0; q < 8; q++) level[j][q] = j == at ? top[q] : level[j][q];
    }
    sp += has ? 1 : 0;
#pragma unroll
    for (int q = 0; q < 8; q++) top[q] = cv[q];
    has = true;
  }

  // top = parent(the value below it, top)
  __device__ __forceinline__ void merge(bool root) {
    uint32_t l[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
    sp--;
#pragma unroll
    for (int j = 0; j < D; j++) {
#pragma unroll
      for (int q = 0; q < 8; q++) l[q] = j == sp ? level[j][q] : l[q];
    }
    parent_cv(l, top, root, o);
#pragma unroll
    for (int q = 0; q < 8; q++) top[q] = o[q];
  }
};

// Pushes the root of the left-balanced tree over items 0 .. count - 1 (fetch(i, cv) loads item i):
// after item i, one merge per trailing one bit of i (BLAKE3's rule: a complete subtree merges as soon
// as its sibling is complete), and after the last item whatever is left, newest first.  The next
// item's load is in flight over the merges.  root: the last parent carries ROOT.
template <int D, class Fetch>
__device__ __forceinline__ void fold_run(CvStack<D> &st, Fetch fetch, size_t count, bool root) {
  const int base = st.depth();
  uint32_t cur[8], nxt[8];
  fetch(0, nxt);
  for (size_t i = 0; i < count; i++) {
#pragma unroll
    for (int q = 0; q < 8; q++) cur[q] = nxt[q];
    const bool last = i + 1 == count;
    if (!last) fetch(i + 1, nxt);
    st.push(cur);
    // the merges of item i, then (last item) every level this run still holds
    size_t t = i;
    while (st.depth() > base + 1 && ((t & 1) || last)) {
      st.merge(root && last && st.depth() == base + 2);
      t >>= 1;
    }
  }
}

// One thread per (column k, cover node j): the node's subtree CV from the column's chunk CVs.
template <int D>
__global__ __launch_bounds__(64) void k_cover_values(const uint32_t *__restrict__ cvs, size_t cv_stride,
                                                     const uint64_t *__restrict__ idx, size_t n_idx,
                                                     const uint64_t *__restrict__ nodes, size_t n_cover,
                                                     uint8_t *__restrict__ covers) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t j = blockIdx.y;
  if (k >= n_idx) return;
  const size_t c = idx ? (size_t)idx[k] : k;
  const size_t lo = (size_t)nodes[2 * j], hi = (size_t)nodes[2 * j + 1];
  CvStack<D> st;
  fold_run<D>(st, [&](size_t i, uint32_t cv[8]) { load8(cvs + ((lo + i) * cv_stride + c) * 8, cv); }, hi - lo,
              false);
  store8(reinterpret_cast<uint32_t *>(covers + 32 * (k * n_cover + j)), st.top);
}

// The segments' chunks [sl.chunk0, sl.chunk0 + gridDim.y): chaining values, the weighted sums' shares
// and the per-column canonical flags (blake3_dev.hpp, SLICE with EVAL).
template <class F>
__global__ __launch_bounds__(256) void k_segment_chunks(const uint32_t *__restrict__ m, size_t n_rows, size_t n_cols,
                                                        uint32_t *__restrict__ cvs, int n_chunks, CmSlice sl,
                                                        CmEval ev) {
  leaf_chunks_cm_body<F, true, true, true>(m, n_rows, n_cols, cvs, nullptr, n_chunks, 0, sl, ev);
}

// One thread per (column, group): the node over an aligned group of READ_GROUP chunks that lies
// inside the range (the last group of the message may be short).  Blocks are (group, 64 columns).
__global__ __launch_bounds__(64) void k_segment_groups(const uint32_t *__restrict__ seg_cvs, size_t n_idx,
                                                       size_t chunk_lo, size_t first, size_t chunk_end,
                                                       uint32_t *__restrict__ group_cvs) {
  const size_t k = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
  const size_t g = blockIdx.x;
  if (k >= n_idx) return;
  const size_t lo = first + (size_t)READ_GROUP * g;
  const size_t count = chunk_end - lo < (size_t)READ_GROUP ? chunk_end - lo : (size_t)READ_GROUP;
  CvStack<3> st;
  fold_run<3>(st, [&](size_t i, uint32_t cv[8]) { load8(seg_cvs + ((lo - chunk_lo + i) * n_idx + k) * 8, cv); },
              count, false);
  store8(group_cvs + (g * n_idx + k) * 8, st.top);
}

// One thread per column runs the program (kernels.hpp, ReadOp) and writes the leaf.
template <int D>
__global__ __launch_bounds__(64) void k_segment_leaves(const uint32_t *__restrict__ seg_cvs,
                                                       const uint32_t *__restrict__ group_cvs,
                                                       const uint8_t *__restrict__ covers, size_t n_idx,
                                                       size_t n_cover, const ReadOp *__restrict__ ops, int n_ops,
                                                       uint8_t *__restrict__ leaves) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_idx) return;
  CvStack<D> st;
  for (int o = 0; o < n_ops; o++) {
    const ReadOp op = ops[o];
    if (op.kind == READ_OP_MERGE) {
      st.merge(op.root != 0);
    } else if (op.kind == READ_OP_COVER) {
      uint32_t cv[8];
      load8(reinterpret_cast<const uint32_t *>(covers + 32 * (k * n_cover + (size_t)op.a)), cv);
      st.push(cv);
    } else {
      const uint32_t *src = op.kind == READ_OP_GROUPS ? group_cvs : seg_cvs;
      const size_t a = (size_t)op.a;
      fold_run<D>(st, [&](size_t i, uint32_t cv[8]) { load8(src + ((a + i) * n_idx + k) * 8, cv); }, (size_t)op.b,
                  op.root != 0);
    }
  }
  store8(reinterpret_cast<uint32_t *>(leaves + 32 * k), st.top);
}

constexpr size_t MAX_CHUNKS = (size_t)1 << 20;  // D = 20 levels

}  // namespace

hipError_t read_cover_values(const uint32_t *cvs, size_t cv_stride, size_t n_chunks, const uint64_t *idx,
                             size_t n_idx, const uint64_t *nodes, size_t n_cover, uint8_t *covers, hipStream_t s) {
  if (!n_idx || !n_cover) return hipSuccess;
  if (n_chunks > MAX_CHUNKS || n_cover > 65535) return hipErrorInvalidValue;
  prof::Scope ps("read_covers", s);
  const dim3 grid((unsigned)((n_idx + 63) / 64), (unsigned)n_cover);
  if (n_chunks <= 256)
    hipLaunchKernelGGL((k_cover_values<8>), grid, dim3(64), 0, s, cvs, cv_stride, idx, n_idx, nodes, n_cover, covers);
  else
    hipLaunchKernelGGL((k_cover_values<20>), grid, dim3(64), 0, s, cvs, cv_stride, idx, n_idx, nodes, n_cover, covers);
  return hipGetLastError();
}

hipError_t read_segment_chunks(int fid, const uint32_t *segs, size_t col_elems, size_t n_rows, size_t n_idx,
                               size_t chunk_lo, size_t chunk_hi, uint32_t *cvs, const uint32_t *weights,
                               uint32_t *partials, uint32_t *bad_cols, hipStream_t s) {
  if (n_idx == 0 || chunk_hi <= chunk_lo) return hipSuccess;
  const size_t n_chunks = leaf_n_chunks(fid, n_rows);
  if (chunk_hi > n_chunks || n_chunks > MAX_CHUNKS || !weights || !partials || !bad_cols) return hipErrorInvalidValue;
  return dispatch_field(fid, [&]<class F>() -> hipError_t {
    if constexpr (F::N == 2) {  // WriteableFt63's element: two words, first row of chunk c >= 1 is 128 c - 4
      const size_t r_lo = chunk_lo ? (256 * chunk_lo - 8) / F::N : 0;
      const size_t r_hi = chunk_hi == n_chunks ? n_rows : (256 * chunk_hi - 8) / F::N;
      CmSlice sl;
      sl.col_words = col_elems * F::N;
      sl.w_base = 8 + r_lo * F::N;
      sl.cv_stride = n_idx;
      sl.cv_chunk0 = (int)chunk_lo;
      sl.bad = bad_cols;
      if (sl.col_words % 4 || sl.w_base % 4 || sl.col_words < (((r_hi - r_lo) * F::N + 3) & ~(size_t)3))
        return hipErrorInvalidValue;
      CmEval ev;
      ev.weights = weights;
      ev.partials = partials;
      ev.row0 = r_lo;
      prof::Scope ps("read_segment_chunks", s);
      for (size_t c0 = chunk_lo; c0 < chunk_hi; c0 += 65535) {  // (grid.y is 16 bits)
        const size_t nc = chunk_hi - c0 < 65535 ? chunk_hi - c0 : 65535;
        sl.chunk0 = (int)c0;
        hipLaunchKernelGGL((k_segment_chunks<F>), dim3((unsigned)((n_idx + 255) / 256), (unsigned)nc), dim3(256), 0, s,
                           segs, n_rows, n_idx, cvs, (int)n_chunks, sl, ev);
      }
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  });
}

hipError_t read_segment_groups(const uint32_t *seg_cvs, size_t n_idx, size_t chunk_lo, size_t first,
                               size_t chunk_end, size_t n_groups, uint32_t *group_cvs, hipStream_t s) {
  if (!n_idx || !n_groups) return hipSuccess;
  if (first < chunk_lo || first + (n_groups - 1) * READ_GROUP >= chunk_end || (n_idx + 63) / 64 > 65535)
    return hipErrorInvalidValue;
  prof::Scope ps("read_segment_groups", s);
  hipLaunchKernelGGL(k_segment_groups, dim3((unsigned)n_groups, (unsigned)((n_idx + 63) / 64)), dim3(64), 0, s, seg_cvs,
                     n_idx, chunk_lo, first, chunk_end, group_cvs);
  return hipGetLastError();
}

hipError_t read_segment_leaves(const uint32_t *seg_cvs, const uint32_t *group_cvs, const uint8_t *covers,
                               size_t n_idx, size_t n_cover, size_t n_chunks, const ReadOp *ops, size_t n_ops,
                               uint8_t *leaves, hipStream_t s) {
  if (!n_idx) return hipSuccess;
  if (n_chunks > MAX_CHUNKS || !n_ops) return hipErrorInvalidValue;
  prof::Scope ps("read_segment_leaves", s);
  const dim3 grid((unsigned)((n_idx + 63) / 64));
  if (n_chunks <= 256)
    hipLaunchKernelGGL((k_segment_leaves<8>), grid, dim3(64), 0, s, seg_cvs, group_cvs, covers, n_idx, n_cover, ops,
                       (int)n_ops, leaves);
  else
    hipLaunchKernelGGL((k_segment_leaves<20>), grid, dim3(64), 0, s, seg_cvs, group_cvs, covers, n_idx, n_cover, ops,
                       (int)n_ops, leaves);
  return hipGetLastError();
}

}  // namespace lcpc
