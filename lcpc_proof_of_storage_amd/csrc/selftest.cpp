// selftest.cpp -- on-device check of the stream-ordered pool's fences (pool.hpp, DBuf).
//
// A block released while a slow writer on another stream still owns it must not be overwritten
// by that writer after its next owner's first kernel: each round queues a writer that spins
// ~spin_us before storing X, releases the block (fence on the writer's stream), takes the same
// block on a third stream and stores Y there at once, then reads it back.  With the fence every
// word reads Y; without it (the unfenced control: the buffer is settle()d before release, the
// fast store runs first) the late writer leaves X behind.  This replaces nothing in the
// reference (whose buffers are host Vecs, lcpc-2d/src/lib.rs:659-690); it is the device-side
// evidence for the pool that the commit / prove / shard paths share.
//
// lcpc_selftest_ntt_rows (at the end): the NTT dispatch called directly, for the row lengths and
// pass variants that no commit-sized test can isolate.  lcpc_selftest_spmm (after it): one
// Brakedown level on a caller's matrix, for the kernels and bounds matgen's matrices never reach,
// and lcpc_selftest_reed_solomon, the Reed-Solomon step under the last level.
#include "host_internal.hpp"

#include <vector>

namespace lcpc_host {
namespace {

__global__ __launch_bounds__(256) void k_late_fill(uint32_t *__restrict__ p, size_t n, uint32_t v, uint64_t ticks) {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = v;
}

__global__ __launch_bounds__(256) void k_fill(uint32_t *__restrict__ p, size_t n, uint32_t v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = v;
}

constexpr size_t WORDS = (1 << 18) + 37;
constexpr unsigned BLOCKS = 1024;

// one round: the block is allocated on `a`, the writer runs on `w` (a itself, or a second stream
// marked with use()), the next owner on `b`; adds the words not reading Y to *bad
lcpc_status pool_round(Device *dev, hipStream_t a, hipStream_t w, hipStream_t b, bool fenced, uint64_t ticks,
                       uint32_t x, uint32_t y, uint64_t *bad, uint64_t *reused) {
  struct Restore {
    hipStream_t prev = t_stream;
    ~Restore() { t_stream = prev; }
  } restore;
  void *first = nullptr;
  {
    t_stream = a;
    DBuf buf;
    HIP_TRY(buf.alloc(dev, WORDS * 4));
    first = buf.p;
    buf.use(w);
    hipLaunchKernelGGL(k_late_fill, dim3(BLOCKS), dim3(256), 0, w, (uint32_t *)buf.p, WORDS, x, ticks);
    HIP_TRY(hipGetLastError());
    if (!fenced) buf.settle();  // the control: claim the writer is done while it still spins
  }  // released here, fenced on a and w unless settled
  std::vector<uint32_t> host(WORDS);
  {
    t_stream = b;
    DBuf nxt;
    HIP_TRY(nxt.alloc(dev, WORDS * 4));
    if (nxt.p == first) ++*reused;
    hipLaunchKernelGGL(k_fill, dim3(BLOCKS), dim3(256), 0, b, (uint32_t *)nxt.p, WORDS, y);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b));
    HIP_TRY(hipStreamSynchronize(w));  // the late writer has finished either way
    HIP_TRY(hipStreamSynchronize(a));
    HIP_TRY(hipMemcpy(host.data(), nxt.p, WORDS * 4, hipMemcpyDeviceToHost));
    nxt.settle();
  }
  for (size_t i = 0; i < WORDS; i++) *bad += host[i] != y;
  return LCPC_OK;
}

}  // namespace
}  // namespace lcpc_host

using namespace lcpc_host;

extern "C" lcpc_status lcpc_selftest_pool_ordering(int rounds, uint32_t spin_us, uint64_t *violations,
                                                   uint64_t *control_violations, uint64_t *reused) {
  if (rounds < 1 || !violations || !control_violations || !reused || spin_us > 100000)
    return fail(LCPC_ERR_INVALID_ARG, "rounds / outputs / spin_us");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  *violations = *control_violations = *reused = 0;
  const uint64_t ticks = (uint64_t)spin_us * 100;  // wall_clock64 runs at 100 MHz on gfx950
  // blocks of the test's size that earlier calls left cached are held aside for the run (a
  // host-ordered take), so that every take below can only return the block just released
  const size_t rb = Device::round_bytes(WORDS * 4);
  std::vector<void *> held;
  while (void *q = dev->blocks.take(rb, hipStream_t{})) held.push_back(q);
  Lease la(dev, POOL_BULK);
  const hipStream_t a = la.s;
  hipStream_t w = dev->acquire_stream(POOL_HIGH);
  hipStream_t b = dev->acquire_stream(POOL_PROVER);
  lcpc_status rc = LCPC_OK;
  for (int r = 0; r < rounds && rc == LCPC_OK; r++) {
    const uint32_t x = 0x5a000000u + 2 * r, y = x + 1;
    // fenced: the writer on the allocating stream, then on a use()d second stream
    if ((rc = pool_round(dev, a, a, b, true, ticks, x, y, violations, reused)) != LCPC_OK) break;
    if ((rc = pool_round(dev, a, w, b, true, ticks, x, y, violations, reused)) != LCPC_OK) break;
    rc = pool_round(dev, a, w, b, false, ticks, x, y, control_violations, reused);
  }
  (void)hipStreamSynchronize(w);
  (void)hipStreamSynchronize(b);
  dev->release_stream(w, POOL_HIGH);
  dev->release_stream(b, POOL_PROVER);
  for (void *q : held) dev->blocks.put(q, rb, nullptr, 0);
  return rc;
}

// ntt_rows (ntt.hip) with every argument the commit paths fix chosen by the caller: any row
// length of the four-step dispatch, HALFZ or not, the canonical-output and fused-copy variants of
// pass A, and strides, on one plan that lives for the call.  The device buffers keep the host
// strides and are uploaded whole first, so what the kernels leave in the gap after each row (and
// in copy beyond n_valid) comes back as the caller set it.
extern "C" lcpc_status lcpc_selftest_ntt_rows(lcpc_field f, int log_n, int inverse, const uint64_t *src,
                                              size_t src_stride, size_t n_valid, uint64_t *dst, size_t dst_stride,
                                              size_t n_rows, uint64_t *copy, size_t copy_stride, int canon) {
  if (!valid_field(f)) return fail(LCPC_ERR_INVALID_ARG, "field");
  if (!src || !dst) return fail(LCPC_ERR_INVALID_ARG, "null src or dst");
  if (log_n < 0) return fail(LCPC_ERR_INVALID_ARG, "log_n");
  if (canon && inverse) return fail(LCPC_ERR_INVALID_ARG, "canonical output: forward plans only");
  if (!field_gpu_supported(f) || log_n > ntt_max_log_n(f))
    return fail(LCPC_ERR_UNSUPPORTED, "length beyond the NTT range");
  const size_t n = (size_t)1 << log_n;
  if (n_valid > n) return fail(LCPC_ERR_INVALID_ARG, "n_valid > 2^log_n");
  if (src_stride < n_valid || dst_stride < n || (copy && copy_stride < n_valid))
    return fail(LCPC_ERR_INVALID_ARG, "stride below its row length");
  if (n_rows == 0) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const size_t wb = field_bytes(f);
  NttPlan plan;
  hipError_t he = ntt_plan_init(plan, f, log_n, inverse != 0, lease.s);
  if (he != hipSuccess) {
    ntt_plan_free(plan);
    if (he == hipErrorInvalidValue) return fail(LCPC_ERR_UNSUPPORTED, "length beyond the NTT range");
    HIP_TRY(he);
  }
  struct PlanGuard {
    NttPlan &p;
    hipStream_t s;
    ~PlanGuard() {
      (void)hipStreamSynchronize(s);
      ntt_plan_free(p);
    }
  } guard{plan, lease.s};
  // whole strides, the last row's included: what lies beyond a row's length is part of the check
  const size_t src_b = n_rows * src_stride * wb, dst_b = n_rows * dst_stride * wb;
  const size_t copy_b = copy ? n_rows * copy_stride * wb : 0;
  DBuf ds, dd, dc;
  HIP_TRY(ds.alloc(dev, std::max(src_b, wb)));  // (src_stride = n_valid = 0: nothing to upload or to read)
  HIP_TRY(h2d(ds.p, src, src_b, lease.s));
  if ((st = upload(dev, dd, dst, dst_b))) return st;
  if (copy_b && (st = upload(dev, dc, copy, copy_b))) return st;
  HIP_TRY(ntt_rows(plan, ds.as<uint32_t>(), src_stride, n_valid, dd.as<uint32_t>(), dst_stride, n_rows, lease.s,
                   copy_b ? dc.as<uint32_t>() : nullptr, copy_stride, canon != 0));
  HIP_TRY(hipMemcpyAsync(dst, dd.p, dst_b, hipMemcpyDeviceToHost, lease.s));
  if (copy_b) HIP_TRY(hipMemcpyAsync(copy, dc.p, copy_b, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

// One Brakedown level y = M x (sdig.hip) on a matrix the caller wrote: nonzero counts, indices
// and values that matgen never draws (an empty output, 512 nonzeros, 513, every value p - 1), any
// R and any row range.  The matrix takes the plan's own upload and group padding and the launch
// is the encode's spmm; y is uploaded whole first, so rows outside the range return untouched.
extern "C" lcpc_status lcpc_selftest_spmm(lcpc_field f, size_t m_rows, size_t m_cols, const uint32_t *ptr,
                                          const uint32_t *idx, const uint64_t *val, const uint64_t *x, uint64_t *y,
                                          size_t R, size_t b0, size_t nb, int path, int *used_mfma) {
  if (!valid_field(f)) return fail(LCPC_ERR_INVALID_ARG, "field");
  if (!ptr || !idx || !val || !x || !y || !used_mfma) return fail(LCPC_ERR_INVALID_ARG, "null argument");
  if (path != 0 && path != 1) return fail(LCPC_ERR_INVALID_ARG, "path");
  if (R > UINT32_MAX || m_rows > UINT32_MAX) return fail(LCPC_ERR_INVALID_ARG, "R or m_rows above 2^32 - 1");
  if (b0 > R || nb > R - b0) return fail(LCPC_ERR_INVALID_ARG, "b0 + nb > R");
  if (ptr[0] != 0) return fail(LCPC_ERR_INVALID_ARG, "ptr[0] != 0");
  for (size_t j = 0; j < m_rows; j++)
    if (ptr[j + 1] < ptr[j]) return fail(LCPC_ERR_INVALID_ARG, "ptr decreases");
  const size_t nnz = ptr[m_rows];
  for (size_t k = 0; k < nnz; k++)
    if (idx[k] >= m_cols) return fail(LCPC_ERR_INVALID_ARG, "idx >= m_cols");
  *used_mfma = 0;
  if (nb == 0 || m_rows == 0) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const size_t wb = field_bytes(f);
  CsrHost M;
  M.rows = m_rows;
  M.cols = m_cols;
  M.ptr.assign(ptr, ptr + m_rows + 1);
  M.idx.assign(idx, idx + nnz);
  M.val.assign(val, val + nnz * (wb / 8));
  DBuf dx, dy;
  if ((st = upload(dev, dx, x, m_cols * R * wb))) return st;
  if ((st = upload(dev, dy, y, m_rows * R * wb))) return st;
  bool mfma = false;
  HIP_TRY(sdig_selftest_spmm(f, M, dx.as<uint32_t>(), dy.as<uint32_t>(), R, b0, nb, path == 1, &mfma, lease.s));
  *used_mfma = mfma ? 1 : 0;
  HIP_TRY(hipMemcpyAsync(y, dy.p, m_rows * R * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

// The Reed-Solomon step at the bottom of the Brakedown recursion (k_reed_solomon, sdig.hip) on the
// caller's input: the encode feeds it the last precode's outputs only, never p - 1 in every
// element.  The launch is the encode's; out is uploaded whole first, as y above.
extern "C" lcpc_status lcpc_selftest_reed_solomon(lcpc_field f, const uint64_t *in, size_t m, uint64_t *out,
                                                  size_t n_out, size_t R, size_t b0, size_t nb) {
  if (!valid_field(f)) return fail(LCPC_ERR_INVALID_ARG, "field");
  if (!in || !out) return fail(LCPC_ERR_INVALID_ARG, "null in or out");
  if (R > UINT32_MAX || n_out > UINT32_MAX || m > UINT32_MAX)
    return fail(LCPC_ERR_INVALID_ARG, "R, m or n_out above 2^32 - 1");
  if (b0 > R || nb > R - b0) return fail(LCPC_ERR_INVALID_ARG, "b0 + nb > R");
  if (nb == 0 || n_out == 0) return LCPC_OK;
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  Lease lease(dev);
  HIP_TRY(hipSetDevice(dev->id));
  const size_t wb = field_bytes(f);
  DBuf din, dout;
  if ((st = upload(dev, din, in, m * R * wb))) return st;
  if ((st = upload(dev, dout, out, n_out * R * wb))) return st;
  HIP_TRY(sdig_selftest_reed_solomon(f, din.as<uint32_t>(), m, dout.as<uint32_t>(), n_out, R, b0, nb, lease.s));
  HIP_TRY(hipMemcpyAsync(out, dout.p, n_out * R * wb, hipMemcpyDeviceToHost, lease.s));
  HIP_TRY(hipStreamSynchronize(lease.s));
  return LCPC_OK;
}

// LCPC_POOL_POISON as a caller of Device::alloc sees it: one block of `bytes` (on a leased stream,
// or with none: the fill must then have completed when alloc returns, so the bytes are read back
// by plain copies that wait for nothing but themselves), its first and last byte, and the block
// back to the pool.  No claim when the switch is off: *enabled = 0, *first and *last are what the
// block happened to hold.
extern "C" lcpc_status lcpc_selftest_pool_poison(size_t bytes, int with_stream, int *enabled, uint8_t *first,
                                                 uint8_t *last) {
  if (!bytes || !enabled || !first || !last) return fail(LCPC_ERR_INVALID_ARG, "bytes / outputs");
  lcpc_status st;
  Device *dev = current_device(&st);
  if (!dev) return st;
  *enabled = pool_poison() >= 0 ? 1 : 0;
  Lease lease(dev);
  if (!lease.s) return fail(LCPC_ERR_DEVICE, "no HIP stream");
  const hipStream_t s = with_stream ? lease.s : nullptr;
  const size_t rb = Device::round_bytes(bytes);
  void *p = nullptr;
  HIP_TRY(dev->alloc(&p, bytes, s));
  // (on a second stream when the block was taken with none: nothing orders that stream behind
  // the fill but the fill's own completion)
  hipError_t e = hipMemcpyAsync(first, p, 1, hipMemcpyDeviceToHost, lease.s);
  if (e == hipSuccess) e = hipMemcpyAsync(last, (const uint8_t *)p + rb - 1, 1, hipMemcpyDeviceToHost, lease.s);
  // the block goes back holding the poison's complement: a later call that gets it recycled sees
  // the poison only if it was filled again
  if (e == hipSuccess && *enabled) e = hipMemsetAsync(p, ~pool_poison() & 0xff, rb, lease.s);
  if (e == hipSuccess) e = hipStreamSynchronize(lease.s);
  dev->release(p);  // every use has completed (or the stream is broken)
  HIP_TRY(e);
  return LCPC_OK;
}
