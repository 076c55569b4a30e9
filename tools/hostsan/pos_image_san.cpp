// pos_image_san.cpp -- the stored-file image stager (csrc/pos_image.hpp) under ASan + UBSan:
// gather from a mapping against gather by pread against a naive double loop, skip sets, a file one
// byte short, scatter / gather round trips, the chunk-aligned row batches and the column-block
// partition.  Every buffer is allocated to its exact size, so a slice one byte too long is caught.
#include <fcntl.h>

#include <cstdio>
#include <random>
#include <string>

#include "pos_image.hpp"

using namespace lcpc_host;

static int bad = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      bad++;                            \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fputc('\n', stderr);         \
    }                                   \
  } while (0)

struct TempFile {
  std::string path;
  int fd = -1;
  TempFile(const uint8_t *data, size_t n) {
    const char *dir = std::getenv("TMPDIR");
    path = std::string(dir ? dir : "/tmp") + "/pos_image_san.XXXXXX";
    fd = mkstemp(path.data());
    for (size_t off = 0; fd >= 0 && off < n;) {
      const ssize_t w = write(fd, data + off, n - off);
      if (w <= 0) break;
      off += (size_t)w;
    }
  }
  ~TempFile() {
    if (fd >= 0) close(fd);
    unlink(path.c_str());
  }
};

// one image, one slice: every way of reading it against the double loop
static void check_slices(std::mt19937_64 &rng, size_t enc, size_t cap, size_t r0, size_t R, size_t c0, size_t nc,
                         bool with_skip) {
  std::vector<uint8_t> image(enc * cap * POS_WB);
  for (auto &b : image) b = (uint8_t)rng();
  std::vector<uint8_t> skip(enc, 0);
  if (with_skip)
    for (auto &x : skip) x = rng() % 3 == 0;
  const size_t stride = (R + (rng() & 1)) * POS_WB;  // packed, or with the cache's one-element pad
  const size_t n = nc * stride;
  std::vector<uint8_t> want(n, 0xA5), from_map(n, 0xA5), from_fd(n, 0xA5), zeroed(n, 0xA5);
  for (size_t c = 0; c < nc; c++)
    for (size_t b = 0; b < R * POS_WB; b++)
      if (!skip[c0 + c]) want[c * stride + b] = image[((c0 + c) * cap + r0) * POS_WB + b];
  TempFile f(image.data(), image.size());
  CHECK(f.fd >= 0, "no temp file");
  ImageSrc img{image.data(), -1, cap, with_skip ? skip.data() : nullptr, false};
  CHECK(gather_slices(img, c0, nc, r0, R, stride, from_map.data()), "mapping: short read?");
  ImageSrc by_fd{nullptr, f.fd, cap, with_skip ? skip.data() : nullptr, false};
  CHECK(gather_slices(by_fd, c0, nc, r0, R, stride, from_fd.data()), "pread: short read on a whole file");
  CHECK(from_map == want, "mapping differs from the double loop (enc %zu cap %zu r0 %zu R %zu c0 %zu nc %zu)", enc, cap,
        r0, R, c0, nc);
  CHECK(from_fd == want, "pread differs from the double loop (enc %zu cap %zu r0 %zu R %zu c0 %zu nc %zu)", enc, cap, r0,
        R, c0, nc);
  // skipped columns zero-filled: the slice is zeros, its pad and every other byte as before
  img.zero_skipped = true;
  CHECK(gather_slices(img, c0, nc, r0, R, stride, zeroed.data()), "mapping: short read?");
  for (size_t c = 0; c < nc; c++)
    for (size_t b = 0; b < stride; b++) {
      const uint8_t w = skip[c0 + c] && b < R * POS_WB ? 0 : want[c * stride + b];
      if (zeroed[c * stride + b] != w) {
        CHECK(false, "zero-filled skip: column %zu byte %zu", c0 + c, b);
        return;
      }
    }
  // a file one byte short: only a slice that reaches its last element can notice, and must
  if (image.size()) {
    CHECK(ftruncate(f.fd, (off_t)image.size() - 1) == 0, "ftruncate");
    std::vector<uint8_t> again(n, 0xA5);
    const bool reaches_end = R && c0 + nc == enc && r0 + R == cap && !(with_skip && skip[enc - 1]);
    CHECK(gather_slices(by_fd, c0, nc, r0, R, stride, again.data()) == !reaches_end, "short file: %s",
          reaches_end ? "not reported" : "reported for a slice that does not reach the end");
  }
  // scatter, then gather: the same bytes come back and nothing else of the image changed
  std::vector<uint8_t> target(image.size(), 0x3C), back(n, 0xA5), packed(nc * R * POS_WB);
  for (auto &b : packed) b = (uint8_t)rng();
  scatter_slices(target.data(), cap, c0, nc, r0, R, R * POS_WB, packed.data());
  ImageSrc timg{target.data(), -1, cap};
  gather_slices(timg, c0, nc, r0, R, R * POS_WB, back.data());
  back.resize(packed.size());
  CHECK(back == packed, "scatter then gather");
  size_t untouched = 0;
  for (uint8_t b : target) untouched += b == 0x3C;
  CHECK(untouched >= target.size() - packed.size(), "scatter wrote outside its slices");
}

// the first row of the column message at or after byte 1024 * chunk, the slow way
static size_t first_row_naive(size_t chunk) {
  size_t r = 0;
  while (32 + r * POS_WB < 1024 * chunk) r++;
  return r;
}

static void check_batches(size_t rows, size_t cpb) {
  const size_t n_chunks = std::max<size_t>(1, (32 + rows * POS_WB + 1023) / 1024);
  const ChunkBatches cb{n_chunks, cpb, rows, n_chunks};
  size_t next_row = 0, c_lo = 0;
  while (c_lo < cb.n_chunks) {
    const ChunkBatches::Batch b = cb.at(c_lo);
    CHECK(b.r0 == next_row, "rows %zu cpb %zu: batch at chunk %zu starts at row %zu, not %zu", rows, cpb, c_lo, b.r0,
          next_row);
    CHECK(b.B <= cb.max_rows(), "rows %zu cpb %zu: batch of %zu rows > max_rows", rows, cpb, b.B);
    CHECK(b.c_hi > c_lo && b.c_hi <= cb.n_chunks, "rows %zu cpb %zu: chunk range", rows, cpb);
    if (b.c_hi < cb.n_chunks)
      CHECK(b.r0 + b.B == first_row_naive(b.c_hi), "rows %zu cpb %zu: batch ends at row %zu, chunk %zu starts at %zu",
            rows, cpb, b.r0 + b.B, b.c_hi, first_row_naive(b.c_hi));
    next_row = b.r0 + b.B;
    c_lo = b.c_hi;
  }
  CHECK(next_row == rows, "rows %zu cpb %zu: %zu rows covered", rows, cpb, next_row);
  for (size_t c = 0; c <= cb.n_chunks; c++)
    CHECK(leaf_chunk_first_row(POS_WB, c) == first_row_naive(c), "first row of chunk %zu", c);
}

static void check_column_blocks(size_t enc, size_t col_bytes, size_t stage_bytes) {
  const size_t cpb = column_block_cols(enc, col_bytes, stage_bytes);
  CHECK(cpb >= 1 && cpb <= enc, "enc %zu col_bytes %zu: %zu columns per block", enc, col_bytes, cpb);
  CHECK(!col_bytes || cpb == 1 || cpb * col_bytes <= stage_bytes, "enc %zu col_bytes %zu: block over the budget", enc,
        col_bytes);
  std::vector<int> seen(enc, 0);
  int blocks = 0;
  for_blocks(enc, cpb, [&](size_t c0, size_t nc, int k) {  // the iteration of for_column_blocks
    CHECK(k == blocks++ && nc >= 1 && nc <= cpb && c0 + nc <= enc, "enc %zu: block %d = [%zu, +%zu)", enc, k, c0, nc);
    for (size_t c = c0; c < c0 + nc; c++) seen[c]++;
    return 0;
  });
  for (size_t c = 0; c < enc; c++) CHECK(seen[c] == 1, "enc %zu col_bytes %zu: column %zu in %d blocks", enc, col_bytes, c, seen[c]);
}

int main() {
  std::mt19937_64 rng(20240521);
  // the seam shapes: (enc, rows) with capacity 2 * rows, whole columns in blocks of two and row
  // batches of 28, the last of either partial
  for (size_t enc : {32, 4})
    for (size_t rows : {125, 301}) {
      const size_t cap = 2 * rows;
      for (size_t c0 = 0; c0 < enc; c0 += 2) check_slices(rng, enc, cap, 0, rows, c0, std::min<size_t>(2, enc - c0), false);
      for (size_t r0 = 0; r0 < rows; r0 += 28) check_slices(rng, enc, cap, r0, std::min<size_t>(28, rows - r0), 0, enc, true);
      check_slices(rng, enc, rows, 0, rows, 0, enc, false);  // to the image's last byte
    }
  for (int it = 0; it < 300; it++) {
    const size_t enc = (size_t)1 << (1 + rng() % 6), cap = 1 + rng() % 70;
    const size_t r0 = rng() % cap, R = rng() % (cap - r0 + 1);
    const size_t c0 = rng() % enc, nc = 1 + rng() % (enc - c0);
    check_slices(rng, enc, cap, r0, R, c0, nc, rng() & 1);
  }
  for (size_t rows : {1, 124, 125, 300, 301, 1000})
    for (size_t cpb : {1, 2, 7}) check_batches(rows, cpb);
  for (size_t enc : {2, 4, 32, 1024})
    for (size_t col_bytes : {0, 8, 2408, 2416, 7200, 7201})
      for (size_t stage : {1, 7200, 1 << 20}) check_column_blocks(enc, col_bytes, stage);
  std::printf("pos_image bad %d\n", bad);
  return bad != 0;
}
