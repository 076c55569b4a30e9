// ntt_ft127.hip -- instantiation of the Ligero encode kernels for Ft127 (see ntt_impl.hpp).
#include "ntt_impl.hpp"

namespace lcpc {
hipError_t ntt_rows_ft127(const NttPlan &p, const uint32_t *src, size_t ss, size_t nv, uint32_t *dst,
                      size_t ds, size_t n_rows, hipStream_t s, uint32_t *cp, size_t cs, bool canon) {
  return ntt_detail::ntt_rows_t<Ft127>(p, src, ss, nv, dst, ds, n_rows, s, cp, cs, canon);
}
hipError_t ntt_tw_table_ft127(uint32_t *tw, int log_n, bool inverse, hipStream_t s) {
  const size_t n = (size_t)1 << log_n;
  hipLaunchKernelGGL((ntt_detail::k_tw_table<Ft127>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     s, tw, log_n, inverse ? 1 : 0);
  return hipGetLastError();
}
hipError_t ntt_tw4_table_ft127(const uint32_t *tw, size_t stride, size_t count, uint32_t *out, hipStream_t s) {
  hipLaunchKernelGGL((ntt_detail::k_tw4_table<Ft127>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, tw,
                     stride, count, out);
  return hipGetLastError();
}
bool ntt_tw4_enabled() { return LCPC_NTT_TW4 != 0; }
// the pass B length the fused leaf pass is built for (0: the build has none, LCPC_NTT_LEAF_FUSE),
// the default tile shape's, which stages its twiddles beside the tile
int ntt_leaf_fuse_l2_ft127() {
  return LCPC_NTT_LEAF_FUSE && ntt_detail::leaf_fuse_l2<Ft127>() <= NTT_TW4_MAX_L
             ? ntt_detail::leaf_fuse_l2<Ft127>()
             : 0;
}
hipError_t ntt_rows_leaf_cvs_ft127(const NttPlan &p, const uint32_t *src, size_t ss, size_t nv, uint32_t *dst, size_t ds,
                                   size_t n_rows, hipStream_t s, uint32_t *cp, size_t cs, uint32_t *cvs) {
  if (!cvs || n_rows == 0) return hipErrorInvalidValue;
  return ntt_detail::ntt_rows_t<Ft127>(p, src, ss, nv, dst, ds, n_rows, s, cp, cs, true, nullptr, cvs);
}
int ntt_persist_blocks_per_cu_ft127(const NttPlan &p) {
  // the rate-1/2 commit's instantiations (HALFZ, canonical output on forward plans)
  int bpc = 1 << 30;
  const hipError_t e = ntt_detail::ntt_rows_t<Ft127>(p, nullptr, 0, ((size_t)1 << p.log_n) / 2, nullptr, 0, 1, nullptr,
                                                     nullptr, 0, !p.inverse, &bpc);
  return e == hipSuccess && bpc != (1 << 30) ? bpc : 0;
}
}  // namespace lcpc
