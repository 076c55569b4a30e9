// digest.hip -- column leaves, Merkle levels and the path check of an lcpc-2d commitment under a
// digest other than BLAKE3: SHA-256 (FIPS 180-4) and the Keccak-f[1600] sponge at rate 136 with the
// padding byte as a parameter (0x06: SHA3-256, FIPS 202; 0x01: the pre-standard Keccak-256).
//
// The reference's LcCommit<D, E> leaves D: Digest free (lcpc-2d/src/lib.rs:174-191); with D
// substituted, merkleize (:720-734) is
//   leaf[j]  = D(32 zero bytes || to_repr(comm[0][j]) || ... || to_repr(comm[n_rows-1][j]))  hash_columns :736-775
//   node     = D(left || right)                                                               merkle_layer :777-815
//   hashes   = [leaves (next_pow2(n_cols), zero-padded) | level 1 | ... | root]
// and verify_column_path (:985-1012) hashes one column and walks its path.  All digests are 32
// bytes, so every buffer keeps blake3.hip's layout; gather_paths / gather_columns are shared.
//
// Leaves.  Both hashes are serial along a column's message, so BLAKE3's (chunk, column) split is not
// available: one lane owns one column and a wave is 64 adjacent columns, every load of the row-major
// codeword a coalesced row segment.  The message is a stream of 32-bit words (the little-endian words
// of fe_repr_words; SHA-256 byte-swaps them into its big-endian schedule, the sponge pairs them into
// little-endian lanes).  Elements are 2, 4, 6 or 8 words behind an 8-word zero prefix, against a
// 16-word block or a 34-word rate, so elements straddle blocks (Ft191 under SHA-256, every field
// under Keccak).  The absorb position is kept a compile-time quantity by unrolling over the period
// (lcm of element and block size: at most 8 elements for SHA-256, 17 for the sponge): state and
// message buffer are named registers, nothing is indexed dynamically and no kernel uses scratch.
// With one wave per SIMD at 2^16 columns nothing but the kernel's own prefetch hides HBM latency: the
// loads of the next group of elements are issued before the current group is absorbed.
#include <type_traits>
#include <utility>

#include "field.hpp"
#include "kernels.hpp"
#include "prof.hpp"

namespace lcpc {

namespace {

template <int N, class Fn>
__device__ __forceinline__ void static_for(Fn &&f) {
  [&]<int... I>(std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
  }(std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ uint32_t rotr32(uint32_t x, int n) { return __builtin_rotateright32(x, n); }

// ------------------------------------------------------------------ SHA-256
__constant__ uint32_t SHA_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

// 16 rounds on the rotating window w (SCHED: extend the schedule first, rounds 16 and later)
template <bool SCHED>
__device__ __forceinline__ void sha_rounds16(uint32_t v[8], uint32_t w[16], int t0) {
#pragma unroll
  for (int i = 0; i < 16; i++) {
    if constexpr (SCHED) {
      const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
      w[i] += (rotr32(x, 7) ^ rotr32(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] +
              (rotr32(y, 17) ^ rotr32(y, 19) ^ (y >> 10));
    }
    // the working variables rotate by renaming: round i reads a..h at v[(j - i) & 7]
    uint32_t &a = v[(0 - i) & 7], &b = v[(1 - i) & 7], &c = v[(2 - i) & 7], &d = v[(3 - i) & 7];
    uint32_t &e = v[(4 - i) & 7], &f = v[(5 - i) & 7], &g = v[(6 - i) & 7], &h = v[(7 - i) & 7];
    const uint32_t t1 = h + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) + (g ^ (e & (f ^ g))) + SHA_K[t0 + i] + w[i];
    const uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) + ((a & b) | (c & (a | b)));
    d += t1;
    h = t1 + t2;
  }
}

struct Sha256 {
  static constexpr int RATE_W = 16;  // 32-bit words per block
  uint32_t h[8];
  uint32_t m[16];  // the block being filled, big-endian words

  __device__ __forceinline__ void init() {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
  }
  // word POS of the current block; w as read little-endian from the byte stream
  template <int POS>
  __device__ __forceinline__ void absorb(uint32_t w) {
    m[POS] = __builtin_bswap32(w);
  }
  __device__ __forceinline__ void process() {
    uint32_t v[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = h[i];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = m[i];
    sha_rounds16<false>(v, w, 0);
#pragma unroll 1
    for (int t0 = 16; t0 < 64; t0 += 16) sha_rounds16<true>(v, w, t0);
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] += v[i];
  }
  // the message ended at word pos (< 16, wave-uniform) of the current block after `bytes` bytes
  __device__ __forceinline__ void finish(int pos, uint64_t bytes, uint32_t /*pad*/, uint32_t out[8]) {
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = i < pos ? m[i] : (i == pos ? 0x80000000u : 0u);
    if (pos >= 14) {  // no room for the length: it goes to a block of its own
      process();
#pragma unroll
      for (int i = 0; i < 16; i++) m[i] = 0;
    }
    const uint64_t bits = bytes * 8;
    m[14] = (uint32_t)(bits >> 32);
    m[15] = (uint32_t)bits;
    process();
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = __builtin_bswap32(h[i]);
  }
  // D(64-byte message) = a Merkle node: one data block and the padding block
  static __device__ __forceinline__ void hash64(const uint32_t msg[16], uint32_t /*pad*/, uint32_t out[8]) {
    Sha256 s;
    s.init();
#pragma unroll
    for (int i = 0; i < 16; i++) s.m[i] = __builtin_bswap32(msg[i]);
    s.process();
    s.finish(0, 64, 0, out);
  }
};

// ------------------------------------------------------------------ Keccak-f[1600], rate 136
__constant__ uint64_t KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
    0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
    0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// rho offsets of lane x + 5 y
__host__ __device__ constexpr int keccak_rot(int i) {
  constexpr int R[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  return R[i];
}

template <int R>
__device__ __forceinline__ uint64_t rotl64(uint64_t x) {
  if constexpr (R == 0)
    return x;
  else
    return (x << R) | (x >> (64 - R));
}

struct Keccak {
  static constexpr int RATE_W = 34;  // 32-bit words per rate block (17 lanes)
  uint64_t st[25];

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < 25; i++) st[i] = 0;
  }
  template <int POS>
  __device__ __forceinline__ void absorb(uint32_t w) {
    st[POS / 2] ^= (uint64_t)w << (32 * (POS & 1));
  }
  // rounds rolled (only the round constant is indexed by the round); each round's lanes, rotation
  // amounts and permutation are static
  __device__ __forceinline__ void process() {
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
      uint64_t c[5], b[25];
#pragma unroll
      for (int x = 0; x < 5; x++) c[x] = st[x] ^ st[x + 5] ^ st[x + 10] ^ st[x + 15] ^ st[x + 20];
      static_for<5>([&](auto X) {
        constexpr int x = X;
        const uint64_t d = c[(x + 4) % 5] ^ rotl64<1>(c[(x + 1) % 5]);
#pragma unroll
        for (int y = 0; y < 5; y++) st[x + 5 * y] ^= d;
      });
      static_for<25>([&](auto I) {
        constexpr int i = I, x = i % 5, y = i / 5;
        b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64<keccak_rot(i)>(st[i]);
      });
#pragma unroll
      for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) st[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
      st[0] ^= KECCAK_RC[r];
    }
  }
  // the message ended at word pos (even, < 34, wave-uniform); pad: the first padding byte
  __device__ __forceinline__ void finish(int pos, uint64_t /*bytes*/, uint32_t pad, uint32_t out[8]) {
#pragma unroll
    for (int i = 0; i < 17; i++) st[i] ^= (2 * i == pos) ? (uint64_t)pad : 0ull;
    st[16] ^= 0x8000000000000000ull;
    process();
#pragma unroll
    for (int i = 0; i < 4; i++) {
      out[2 * i] = (uint32_t)st[i];
      out[2 * i + 1] = (uint32_t)(st[i] >> 32);
    }
  }
  // D(64-byte message) = a Merkle node: 64 B < rate, one permutation
  static __device__ __forceinline__ void hash64(const uint32_t msg[16], uint32_t pad, uint32_t out[8]) {
    Keccak s;
    s.init();
#pragma unroll
    for (int i = 0; i < 8; i++) s.st[i] = (uint64_t)msg[2 * i] | ((uint64_t)msg[2 * i + 1] << 32);
    s.finish(16, 64, pad, out);
  }
};

__device__ __forceinline__ void load8(const uint32_t *p, uint32_t v[8]) {
  const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(uint32_t *p, const uint32_t v[8]) {
  reinterpret_cast<uint4 *>(p)[0] = make_uint4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<uint4 *>(p)[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

constexpr int cgcd(int a, int b) { return b ? cgcd(b, a % b) : a; }

// ------------------------------------------------------------------ leaves
// One lane per column.  Element row r of column col is at m + (col * col_stride + r * row_stride)
// elements (row-major codeword: col_stride 1, row_stride the row length; [column][row]: col_stride
// n_rows, row_stride 1, each lane walking its own contiguous column).  PER elements fill a whole
// number of blocks, so message word (8 + k N + i) mod RATE_W of element k of a period is the same in
// every period; the period's loads run G elements ahead of its absorbs.
// Four waves per workgroup: a workgroup's waves go one to each SIMD of its CU, so the 1024 waves of
// 2^16 columns land one per SIMD.  As 1024 one-wave workgroups they were placed several to a SIMD
// with other SIMDs idle, and the pass took 1.6-1.8 x as long ("Other digests").
constexpr int LEAF_BLOCK = 256;
template <class H, class F, bool CANON>
__global__ __launch_bounds__(LEAF_BLOCK) void k_leaf_digest(const uint32_t *__restrict__ m, size_t n_rows, size_t n_cols,
                                                    size_t row_stride, size_t col_stride,
                                                    uint8_t *__restrict__ leaves, uint32_t pad) {
  constexpr int N = F::N, RW = H::RATE_W;
  constexpr int PER = RW / cgcd(N, RW);                    // elements per period
  constexpr int G0 = 32 / N, G = G0 < PER ? G0 : PER;      // elements per prefetch group (<= 32 words)
  const size_t col = (size_t)blockIdx.x * LEAF_BLOCK + threadIdx.x;
  if (col >= n_cols) return;
  const uint32_t *colp = m + col * col_stride * N;
  H hs;
  hs.init();
  static_for<8>([&](auto I) { hs.template absorb<I>(0u); });  // the 32 zero bytes (:745-748)
  Fe<F> el[PER], nx[G];
#pragma unroll
  for (int k = 0; k < G; k++) el[k] = (size_t)k < n_rows ? fe_load<F>(colp, k * row_stride) : fe_zero<F>();
  for (size_t row0 = 0; row0 < n_rows; row0 += PER) {
    static_for<PER>([&](auto K) {
      constexpr int k = K;
      if constexpr (k % G == 0) {
        // the next group: later elements of this period, or the first group of the next one
        if constexpr (k + G < PER) {
#pragma unroll
          for (int q = k + G; q < k + 2 * G && q < PER; q++)
            el[q] = row0 + q < n_rows ? fe_load<F>(colp, (row0 + q) * row_stride) : fe_zero<F>();
        } else {
#pragma unroll
          for (int q = 0; q < G; q++)
            nx[q] = row0 + PER + q < n_rows ? fe_load<F>(colp, (row0 + PER + q) * row_stride) : fe_zero<F>();
        }
      }
      if (row0 + k < n_rows) {  // wave-uniform
        uint32_t w[N];
        if constexpr (CANON)
          fe_canon_repr_words<F>(el[k], w);
        else
          fe_repr_words<F>(el[k], w);
        static_for<N>([&](auto I) {
          constexpr int pos = (8 + k * N + I) % RW;
          hs.template absorb<pos>(w[I]);
          if constexpr (pos == RW - 1) hs.process();
        });
      }
    });
#pragma unroll
    for (int q = 0; q < G; q++) el[q] = nx[q];
  }
  const uint64_t bytes = 32 + (uint64_t)n_rows * (4 * N);
  uint32_t out[8];
  hs.finish((int)((8 + n_rows * N) % RW), bytes, pad, out);
  store8(reinterpret_cast<uint32_t *>(leaves + 32 * col), out);
}

// ------------------------------------------------------------------ Merkle levels (k_merkle's structure)
// each workgroup folds 2^levels consecutive nodes of level lvl into one, writing every level
template <class H>
__global__ __launch_bounds__(256) void k_merkle_digest(uint8_t *__restrict__ hashes, size_t np2, int lvl, int levels,
                                                       uint32_t pad) {
  __shared__ __align__(16) uint32_t buf[2][256 * 8];
  const int tid = threadIdx.x;
  size_t n_in = np2 >> lvl;
  size_t base_in = 2 * np2 - 2 * n_in;  // offset of level lvl
  const int width = 1 << levels;         // input nodes per workgroup (<= 512)
  const size_t first = (size_t)blockIdx.x * width;
  int cur = 0;
  for (int i = tid; i < width / 2; i += 256) {
    uint32_t msg[16], o[8];
    load8(reinterpret_cast<const uint32_t *>(hashes + 32 * (base_in + first + 2 * i)), msg);
    load8(reinterpret_cast<const uint32_t *>(hashes + 32 * (base_in + first + 2 * i + 1)), msg + 8);
    H::hash64(msg, pad, o);
#pragma unroll
    for (int k = 0; k < 8; k++) buf[cur][i * 8 + k] = o[k];
    store8(reinterpret_cast<uint32_t *>(hashes + 32 * (base_in + n_in + first / 2 + i)), o);
  }
  base_in += n_in;
  n_in /= 2;
  size_t f = first / 2;
  for (int l = 1; l < levels; l++) {
    __syncthreads();
    const int cnt = width >> (l + 1);
    for (int i = tid; i < cnt; i += 256) {
      uint32_t msg[16], o[8];
#pragma unroll
      for (int k = 0; k < 16; k++) msg[k] = buf[cur][2 * i * 8 + k];
      H::hash64(msg, pad, o);
#pragma unroll
      for (int k = 0; k < 8; k++) buf[cur ^ 1][i * 8 + k] = o[k];
      store8(reinterpret_cast<uint32_t *>(hashes + 32 * (base_in + n_in + f / 2 + i)), o);
    }
    cur ^= 1;
    base_in += n_in;
    n_in /= 2;
    f /= 2;
  }
}

// ------------------------------------------------------------------ path check, one lane per opened column
template <class H>
__global__ __launch_bounds__(64) void k_path_checks_digest(const uint8_t *__restrict__ leaves,
                                                           const uint8_t *__restrict__ paths, size_t n,
                                                           size_t path_len, const uint64_t *__restrict__ idx,
                                                           const uint8_t *__restrict__ root,
                                                           uint32_t *__restrict__ flags, uint32_t pad) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint32_t h[8], msg[16];
  load8(reinterpret_cast<const uint32_t *>(leaves + 32 * k), h);
  size_t col = idx[k];
  for (size_t i = 0; i < path_len; i++) {
    uint32_t p[8];
    load8(reinterpret_cast<const uint32_t *>(paths + 32 * (k * path_len + i)), p);
#pragma unroll
    for (int q = 0; q < 8; q++) {
      msg[q] = (col & 1) ? p[q] : h[q];
      msg[8 + q] = (col & 1) ? h[q] : p[q];
    }
    H::hash64(msg, pad, h);
    col >>= 1;
  }
  uint32_t rt[8];
  load8(reinterpret_cast<const uint32_t *>(root), rt);
  uint32_t diff = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) diff |= h[q] ^ rt[q];
  flags[k] = diff == 0;
}

// the sponge's first padding byte (unused by SHA-256)
uint32_t digest_pad(int digest) { return digest == DIGEST_KECCAK256 ? 0x01u : 0x06u; }

// fn.template operator()<H>() for the hash of a non-BLAKE3 digest
template <class Fn>
hipError_t dispatch_digest(int digest, Fn &&fn) {
  switch (digest) {
    case DIGEST_SHA256: return fn.template operator()<Sha256>();
    case DIGEST_SHA3_256:
    case DIGEST_KECCAK256: return fn.template operator()<Keccak>();
    default: return hipErrorInvalidValue;
  }
}

hipError_t leaf_digest_strided(int digest, int fid, const uint32_t *m, size_t n_rows, size_t n_cols, size_t row_stride,
                               size_t col_stride, uint8_t *leaves, hipStream_t s, bool canon) {
  if (n_cols == 0) return hipSuccess;
  const dim3 grid((unsigned)((n_cols + LEAF_BLOCK - 1) / LEAF_BLOCK));
  const uint32_t pad = digest_pad(digest);
  return dispatch_digest(digest, [&]<class H>() {
    return dispatch_field(fid, [&]<class F>() {
      prof::Scope ps("leaf_digest", s);
      if (canon)
        hipLaunchKernelGGL((k_leaf_digest<H, F, true>), grid, dim3(LEAF_BLOCK), 0, s, m, n_rows, n_cols, row_stride, col_stride,
                           leaves, pad);
      else
        hipLaunchKernelGGL((k_leaf_digest<H, F, false>), grid, dim3(LEAF_BLOCK), 0, s, m, n_rows, n_cols, row_stride, col_stride,
                           leaves, pad);
      return hipGetLastError();
    });
  });
}

}  // namespace

bool digest_valid(int digest) { return digest >= DIGEST_BLAKE3 && digest <= DIGEST_KECCAK256; }

hipError_t leaf_hashes_d(int digest, int fid, const uint32_t *m, size_t n_rows, size_t n_cols, size_t stride,
                         uint8_t *leaves, void *scratch, hipStream_t s, bool canon) {
  if (digest == DIGEST_BLAKE3) return leaf_hashes(fid, m, n_rows, n_cols, stride, leaves, scratch, s, canon);
  return leaf_digest_strided(digest, fid, m, n_rows, n_cols, stride, 1, leaves, s, canon);
}

hipError_t leaf_hashes_cols_d(int digest, int fid, const uint32_t *cols, size_t n_rows, size_t n_cols, uint8_t *leaves,
                              void *scratch, hipStream_t s, bool canon) {
  if (digest == DIGEST_BLAKE3) return leaf_hashes_cols(fid, cols, n_rows, n_cols, leaves, scratch, s, canon);
  return leaf_digest_strided(digest, fid, cols, n_rows, n_cols, 1, n_rows, leaves, s, canon);
}

hipError_t merkle_tree_d(int digest, uint8_t *hashes, size_t np2, hipStream_t s) {
  if (digest == DIGEST_BLAKE3) return merkle_tree(hashes, np2, s);
  const uint32_t pad = digest_pad(digest);
  return dispatch_digest(digest, [&]<class H>() {
    int lvl = 0;
    size_t n = np2;
    while (n > 1) {
      int levels = 0;
      while (levels < 9 && ((size_t)1 << (levels + 1)) <= n) levels++;
      const size_t blocks = n >> levels;
      prof::Scope ps("merkle", s);
      hipLaunchKernelGGL((k_merkle_digest<H>), dim3((unsigned)blocks), dim3(256), 0, s, hashes, np2, lvl, levels, pad);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      lvl += levels;
      n >>= levels;
    }
    return hipSuccess;
  });
}

hipError_t path_checks_d(int digest, const uint8_t *leaves, const uint8_t *paths, size_t n, size_t path_len,
                         const uint64_t *idx, const uint8_t *root, uint32_t *flags, hipStream_t s) {
  if (digest == DIGEST_BLAKE3) return path_checks(leaves, paths, n, path_len, idx, root, flags, s);
  if (!n) return hipSuccess;
  const uint32_t pad = digest_pad(digest);
  return dispatch_digest(digest, [&]<class H>() {
    hipLaunchKernelGGL((k_path_checks_digest<H>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, leaves, paths, n,
                       path_len, idx, root, flags, pad);
    return hipGetLastError();
  });
}

}  // namespace lcpc
