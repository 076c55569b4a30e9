// pos_image.hpp -- host side of a stored file's column-major image (`.porenc`: column c is
// row_capacity 8-byte elements from byte c * row_capacity * 8): slices gathered into and scattered
// from contiguous staging, and row batches that end on BLAKE3 chunk boundaries of the column
// messages.  No HIP types: it builds alone under the sanitizers (tools/hostsan/pos_image_san.cpp).
#pragma once
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace lcpc_host {

constexpr size_t POS_DB = 7;  // F::DATA_BYTE_CAPACITY (data_field.rs:22)
constexpr size_t POS_WB = 8;  // F::WRITTEN_BYTES_WIDTH = size_of::<F>() (data_field.rs:24)

template <class Fn>
void parallel_for(size_t n, Fn fn) {
  const size_t hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t T = std::min<size_t>(n, std::min<size_t>(16, hw));
  if (T <= 1) {
    for (size_t i = 0; i < n; i++) fn(i);
    return;
  }
  std::atomic<size_t> next{0};
  const size_t grain = std::max<size_t>(1, n / (T * 8));
  std::vector<std::thread> th;
  for (size_t t = 0; t < T; t++)
    th.emplace_back([&] {
      for (;;) {
        const size_t i0 = next.fetch_add(grain);
        if (i0 >= n) break;
        const size_t i1 = std::min(n, i0 + grain);
        for (size_t i = i0; i < i1; i++) fn(i);
      }
    });
  for (auto &t : th) t.join();
}

// large memcpy split over host threads
inline void par_memcpy(uint8_t *dst, const uint8_t *src, size_t n) {
  constexpr size_t BLK = (size_t)8 << 20;
  if (n <= BLK) {
    if (n) std::memcpy(dst, src, n);
    return;
  }
  parallel_for((n + BLK - 1) / BLK, [&](size_t i) {
    const size_t o = i * BLK;
    std::memcpy(dst + o, src + o, std::min(BLK, n - o));
  });
}

// An image to read: the mapping `map` or, with fd >= 0, the open file read with pread (mapping a
// multi-GB file costs more than an update's 1 KiB per column).  skip[c] != 0: column c is never
// read, its slice of the destination left as it is or zero-filled.
struct ImageSrc {
  const uint8_t *map = nullptr;
  int fd = -1;
  size_t row_capacity = 0;
  const uint8_t *skip = nullptr;
  bool zero_skipped = false;
};

// Rows [r0, r0 + R) of the columns [c0, c0 + nc) into dst, column c0 + c at dst + c * stride_bytes
// (a row batch is c0 = 0, nc = the image's width).  false: the file ended before a slice did.
inline bool gather_slices(const ImageSrc &img, size_t c0, size_t nc, size_t r0, size_t R, size_t stride_bytes,
                          uint8_t *dst) {
  const size_t want = R * POS_WB;
  if (!want) return true;
  std::atomic<bool> short_read{false};
  parallel_for(nc, [&](size_t c) {
    uint8_t *to = dst + c * stride_bytes;
    if (img.skip && img.skip[c0 + c]) {
      if (img.zero_skipped) std::memset(to, 0, want);
      return;
    }
    const size_t at = ((c0 + c) * img.row_capacity + r0) * POS_WB;
    if (img.fd < 0) {
      std::memcpy(to, img.map + at, want);
      return;
    }
    for (size_t got = 0; got < want;) {
      const ssize_t n = pread(img.fd, to + got, want - got, (off_t)(at + got));
      if (n <= 0) {
        if (n < 0 && errno == EINTR) continue;
        short_read = true;
        return;
      }
      got += (size_t)n;
    }
  });
  return !short_read;
}

// The mirror image: src + c * stride_bytes into rows [r0, r0 + R) of column c0 + c of the image.
inline void scatter_slices(uint8_t *image, size_t row_capacity, size_t c0, size_t nc, size_t r0, size_t R,
                           size_t stride_bytes, const uint8_t *src) {
  if (!R) return;
  parallel_for(nc, [&](size_t c) {
    std::memcpy(image + ((c0 + c) * row_capacity + r0) * POS_WB, src + c * stride_bytes, R * POS_WB);
  });
}

// A column message is 32 zero bytes and then the column's elements of wb bytes, hashed in 1-KiB
// BLAKE3 chunks: the first row at or after byte 1024 * chunk (lcpc_leaf_chunk_first_row).
inline size_t leaf_chunk_first_row(size_t wb, size_t chunk) { return chunk ? (1024 * chunk - 32 + wb - 1) / wb : 0; }
constexpr size_t POS_ROWS_PER_CHUNK = 1024 / POS_WB;

// Row batches of whole chunks: the batch at chunk c_lo covers the chunks [c_lo, c_hi) and the rows
// [r0, r0 + B).  n_chunks = the chunks of the whole column message (the last ends with the last of
// `rows`), c_end = where the batches stop, cpb = chunks per batch.
struct ChunkBatches {
  size_t n_chunks = 1, cpb = 1, rows = 0, c_end = 1;
  struct Batch { size_t r0, B, c_hi; };
  Batch at(size_t c_lo) const {
    const size_t c_hi = std::min(c_end, c_lo + cpb);
    const size_t r0 = std::min(rows, leaf_chunk_first_row(POS_WB, c_lo));
    const size_t r1 = c_hi == n_chunks ? rows : std::min(rows, leaf_chunk_first_row(POS_WB, c_hi));
    return {r0, r1 - r0, c_hi};
  }
  size_t max_rows() const { return std::max<size_t>(1, std::min(rows, cpb * POS_ROWS_PER_CHUNK)); }
};

// The batches of scrub-side passes over an image of `rows` rows (n_chunks chunks) and `enc` columns:
// a staging buffer's worth of rows or LCPC_POS_REPAIR_BATCH_ROWS, whichever is less (tests of the
// batch seams on small files, A/B runs), rounded down to whole chunks, at least one.
inline ChunkBatches repair_batches(size_t rows, size_t n_chunks, size_t enc, size_t stage_bytes) {
  size_t want_rows = std::max<size_t>(POS_ROWS_PER_CHUNK, stage_bytes / (enc * POS_WB));
  if (const char *env = std::getenv("LCPC_POS_REPAIR_BATCH_ROWS")) {
    const unsigned long long v = std::strtoull(env, nullptr, 10);
    if (v) want_rows = std::min<size_t>(want_rows, (size_t)v);
  }
  return {n_chunks, std::max<size_t>(1, want_rows / POS_ROWS_PER_CHUNK), rows, n_chunks};
}

// How many of `enc` columns of col_bytes each go through one staging block of stage_bytes, and the
// blocks themselves: fn(c0, nc, k) for block k = columns [c0, c0 + nc), until one returns non-zero.
inline size_t column_block_cols(size_t enc, size_t col_bytes, size_t stage_bytes) {
  return col_bytes ? std::max<size_t>(1, std::min(enc, stage_bytes / col_bytes)) : enc;
}
template <class Fn>
int for_blocks(size_t enc, size_t cpb, Fn fn) {
  int k = 0;
  for (size_t c0 = 0; c0 < enc; c0 += cpb, k++)
    if (int r = fn(c0, std::min(enc, c0 + cpb) - c0, k)) return r;
  return 0;
}

}  // namespace lcpc_host
