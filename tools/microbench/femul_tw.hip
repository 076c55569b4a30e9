// femul_tw.hip -- rate of the word-expanded twiddle product (field.hpp fe_mul_tw: two Montgomery
// word-steps, a 64-byte constant) next to the library's lazy product (fe_mul_lazy: four steps, a
// 16-byte constant), Ft127.  Each with the constant in registers (the VALU stream alone) and read
// from an LDS table per product as the NTT passes do (one ds_read_b128 against four, planes
// [i][e] as ntt_v2.hpp's TwWords stages them), lane-varying and wave-uniform index.
// Products are checked against each other first: same residue class, both below 2p.
// Build: hipcc -O3 -std=c++20 --offload-arch=gfx950 femul_tw.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lcpc_proof_of_storage_amd/csrc/field.hpp"

using namespace lcpc;
using F = Ft127;

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e = (x);                                                            \
    if (e != hipSuccess) {                                                         \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

constexpr int ITERS = 4096, HALF = 128;  // HALF: a 256-point pass's table

// V: 0 library / 1 expanded; SRC: 0 registers, 1 LDS lane-varying index, 2 LDS wave-uniform index
template <int V, int SRC>
__global__ __launch_bounds__(256) void k_rate(const uint32_t *__restrict__ tw, uint32_t *out, uint32_t seed) {
  __shared__ __align__(16) uint32_t smem[HALF * F::N * F::N];
  Fe<F> *lds = reinterpret_cast<Fe<F> *>(smem);
  // tw: HALF entries of N elements, element 2 = the Montgomery form; planes [i][e] in LDS
  for (int k = threadIdx.x; k < HALF * F::N; k += 256) lds[(k % F::N) * HALF + k / F::N] = fe_load<F>(tw, k);
  __syncthreads();
  Fe<F> x[4];
  for (int q = 0; q < 4; q++)
    for (int i = 0; i < F::N; i++) x[q].v[i] = (F::ONE[i] ^ (threadIdx.x * 3 + seed + q)) & (i == F::N - 1 ? 0x0fffffffu : ~0u);
  Fe<F> W[F::N];
  for (int i = 0; i < F::N; i++) W[i] = lds[i * HALF + 5];
  int e = SRC == 1 ? threadIdx.x & (HALF - 1) : (int)(seed & (HALF - 1));
  for (int it = 0; it < ITERS / 4; it++) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if constexpr (SRC != 0) {
        e = (e + 37) & (HALF - 1);
        if constexpr (V == 0) {
          W[2] = lds[2 * HALF + e];
        } else {
#pragma unroll
          for (int i = 0; i < F::N; i++) W[i] = lds[i * HALF + e];
        }
      }
      x[q] = V == 0 ? fe_mul_lazy<F>(x[q], W[2]) : fe_mul_tw<F>(x[q], W);
    }
  }
  uint32_t r = 0;
  for (int q = 0; q < 4; q++)
    for (int i = 0; i < F::N; i++) r ^= x[q].v[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

__global__ void k_expand(const uint32_t *__restrict__ w, uint32_t *__restrict__ out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fe<F> W[F::N];
  fe_tw_expand<F>(fe_load<F>(w, t), W);
  for (int i = 0; i < F::N; i++) fe_store<F>(out, (size_t)t * F::N + i, W[i]);
}

// x < 2p, w < p: both products reduced to [0, p) must agree, and fe_mul_tw's raw value is below 2p
__global__ void k_check(const uint32_t *__restrict__ in, uint32_t *bad, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Fe<F> x = fe_load<F>(in, 2 * (size_t)t), w = fe_load<F>(in, 2 * (size_t)t + 1);
  Fe<F> W[F::N];
  fe_tw_expand<F>(w, W);
  const Fe<F> y = fe_mul_tw<F>(x, W);
  const Fe<F> a = fe_reduce_2p<F>(fe_mul_lazy<F>(x, w)), b = fe_reduce_2p<F>(y);
  bool lt2p = false;  // y < 2p
  for (int i = F::N - 1; i >= 0; i--)
    if (y.v[i] != TwoP<F>::limb(i)) {
      lt2p = y.v[i] < TwoP<F>::limb(i);
      break;
    }
  if (!fe_eq<F>(a, b) || !lt2p || !fe_eq<F>(W[F::N - 2], w)) atomicAdd(bad, 1u);
}

template <int V, int SRC>
void rate(const char *name, const uint32_t *tw, uint32_t *buf) {
  const int blocks = 256 * 64, threads = 256;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int rep = 0; rep < 4; rep++) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_rate<V, SRC>), dim3(blocks), dim3(threads), 0, 0, tw, buf, 7u);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (rep && ms < best) best = ms;
  }
  printf("Ft127 %-44s %8.3f ms  %8.2f G mul/s\n", name, best, (double)blocks * threads * ITERS / (best * 1e-3) / 1e9);
}

int main() {
  const int n = 1 << 20;
  std::vector<uint32_t> h((size_t)2 * n * F::N);
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (size_t i = 0; i < h.size(); i++) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    h[i] = (uint32_t)x;
    // x (even elements) below 2p, w (odd) below p, from the top limb
    if (i % F::N == F::N - 1) h[i] = (i / F::N) % 2 ? h[i] % F::P[F::N - 1] : h[i] % (2 * F::P[F::N - 1]);
  }
  uint32_t *din, *bad, *tw, *w, *buf;
  CK(hipMalloc(&din, h.size() * 4));
  CK(hipMalloc(&bad, 4));
  CK(hipMemcpy(din, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(bad, 0, 4));
  hipLaunchKernelGGL(k_check, dim3(n / 256), dim3(256), 0, 0, din, bad, n);
  uint32_t nb = 0;
  CK(hipMemcpy(&nb, bad, 4, hipMemcpyDeviceToHost));
  printf("fe_mul_tw vs fe_mul_lazy on 2^20 random pairs (x < 2p, w < p): %s\n", nb ? "MISMATCH" : "same class, below 2p");
  // a table of HALF constants: the odd elements of the random input
  std::vector<uint32_t> hw((size_t)HALF * F::N);
  for (int e = 0; e < HALF; e++)
    for (int i = 0; i < F::N; i++) hw[(size_t)e * F::N + i] = h[((size_t)2 * e + 1) * F::N + i];
  CK(hipMalloc(&w, hw.size() * 4));
  CK(hipMalloc(&tw, hw.size() * F::N * 4));
  CK(hipMalloc(&buf, (size_t)256 * 64 * 256 * 4));
  CK(hipMemcpy(w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_expand, dim3(1), dim3(HALF), 0, 0, w, tw, HALF);
  CK(hipDeviceSynchronize());
  rate<0, 0>("library lazy product, constant in registers", tw, buf);
  rate<1, 0>("expanded product,     constant in registers", tw, buf);
  rate<0, 1>("library lazy product, LDS, lane-varying", tw, buf);
  rate<1, 1>("expanded product,     LDS, lane-varying", tw, buf);
  rate<0, 2>("library lazy product, LDS, wave-uniform", tw, buf);
  rate<1, 2>("expanded product,     LDS, wave-uniform", tw, buf);
  return nb ? 1 : 0;
}
