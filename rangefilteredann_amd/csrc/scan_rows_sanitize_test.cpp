// scan_rows_sanitize_test.cpp -- the staged row fetch of k_brute_staged (wann_set_scan_rows) under address + undefined-behaviour
// sanitizers (make sanitize, fifth program): scan_fetch and the LDS sizes of wann_device.h, the text the kernel itself loads
// and stores by.  The program plays the 64 lanes of a wave over a copy of EXACTLY n x pitch bytes and a staging area of
// exactly scan_stage_bytes_per_wave bytes: every byte of a window is fetched once, none outside it, every row arrives whole at
// its padded place.  CPU only; no HIP.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/wann.h"
#include "wann_device.h"

using namespace wann;

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      failures++;                                                      \
    }                                                                  \
  } while (0)

static uint8_t byte_of(int64_t at) { return (uint8_t)((at * 131 + (at >> 9) * 7 + 5) & 0xff); }

// One scan of rows [a, b) the way brute_body walks it: passes of `step` rows, each pass one span.
static void play(int64_t n, int pitch, int64_t qwords, int k, int64_t a, int64_t b) {
  const int pad = kScanStagePad;
  const int step = scan_stage_rows(pitch, pad, qwords, k);
  const int64_t stage_bytes = scan_stage_bytes_per_wave(pitch, pad, qwords, k);
  CHECK(step >= 1 && step <= 64 && (int64_t)step * (pitch + pad) <= stage_bytes && stage_bytes % 16 == 0);
  std::vector<uint8_t> copy((size_t)(n * pitch));  // (exactly the copy: a read past row n - 1 is the sanitizer's to find)
  for (int64_t i = 0; i < n * pitch; i++) copy[(size_t)i] = byte_of(i);
  std::vector<uint8_t> stage((size_t)stage_bytes);
  std::vector<int> fetched((size_t)(n * pitch), 0);
  for (int64_t r0 = a; r0 < b; r0 += step) {
    const int cnt = (int)std::min<int64_t>(b - r0, step);
    std::fill(stage.begin(), stage.end(), (uint8_t)0xee);
    std::vector<int> written((size_t)stage_bytes, 0);
    const uint8_t *src = copy.data() + r0 * pitch;
    const int nsteps = scan_fetch_steps(cnt, pitch);
    // (the kernel walks the steps eight at a time: the steps beyond nsteps of the last group must all be invalid)
    for (int s = 0; s < ((nsteps + 7) & ~7); s++)
      for (int lane = 0; lane < 64; lane++) {
        const ScanFetch f = scan_fetch(lane, s, cnt, pitch, pad);
        if (s >= nsteps) CHECK(!f.valid);
        if (!f.valid) continue;
        CHECK(f.src % 16 == 0 && f.dst % 8 == 0);
        CHECK(f.src >= 0 && f.src + 16 <= cnt * pitch);
        CHECK(f.dst >= 0 && f.dst + 16 <= stage_bytes);
        memcpy(stage.data() + f.dst, src + f.src, 16);
        for (int x = 0; x < 16; x++) {
          fetched[(size_t)(r0 * pitch + f.src + x)]++;
          written[(size_t)(f.dst + x)]++;
        }
      }
    bool whole = true, once = true;
    for (int r = 0; r < cnt; r++)
      for (int x = 0; x < pitch; x++) whole = whole && stage[(size_t)(r * (pitch + pad) + x)] == byte_of((r0 + r) * pitch + x);
    for (int64_t x = 0; x < stage_bytes; x++) once = once && written[(size_t)x] <= 1;
    CHECK(whole);
    CHECK(once);
  }
  bool exact = true;
  for (int64_t i = 0; i < n * pitch; i++) exact = exact && fetched[(size_t)i] == ((i >= a * pitch && i < b * pitch) ? 1 : 0);
  if (!exact) {
    fprintf(stderr, "FAILED: window [%lld, %lld) of %lld rows, pitch %d: not every byte exactly once\n", (long long)a, (long long)b,
            (long long)n, pitch);
    failures++;
  }
}

// the 16 pairs of one ds_read_b32 group (banks modulo 32) start on different banks: lane h of pair p reads block h of row p
static void check_banks(int pitch) {
  std::vector<int> hits(32, 0);
  for (int lane = 0; lane < 32; lane++) hits[(size_t)((((lane >> 1) * (pitch + kScanStagePad) + (lane & 1) * 4) / 4) % 32)]++;
  for (int h : hits) CHECK(h == 1);
}

int main() {
  const int pitches[] = {64, 128, 256, 448};
  const int64_t widths[] = {1, 63, 64, 65, 127, 129};
  for (int pitch : pitches) {
    check_banks(pitch);
    const int64_t d = pitch, qwords = (d + 15) & ~(int64_t)15;
    CHECK(u8_widened_stride_words(d) * 4 == pitch);
    for (int64_t n : {(int64_t)333, (int64_t)6037}) {  // (neither a multiple of 64)
      for (int64_t w : widths) {
        play(n, pitch, qwords, 10, 0, w);          // at the start of the set
        play(n, pitch, qwords, 10, 101, 101 + w);  // in the middle, at an odd first row
        play(n, pitch, qwords, 10, n - w, n);      // ending on the last row
      }
      play(n, pitch, qwords, 10, 0, n);  // the whole set: its last pass is n % 64 rows
    }
    // a wide k leaves less than 64 rows' room: fewer rows per pass, the same bytes
    play(333, pitch, qwords, 1024, 7, 7 + 129);
    play(333, pitch, qwords, 1024, 333 - 65, 333);
  }
  // the sizes: 64 rows where they fit, fewer where they do not, never none; the workgroup stays within its 160 KiB whenever one row fits
  static_assert(scan_stage_rows(128, kScanStagePad, 128, 10) == 64 && scan_stage_rows(256, kScanStagePad, 256, 10) == 64, "d = 128 / 256: a wave stages its 64 rows");
  static_assert(scan_stage_bytes_per_wave(128, kScanStagePad, 128, 10) == 64 * 136, "");
  static_assert(brute_staged_lds_bytes(32, 128, 10) == 4 * (1616 + 8704), "one-byte rows, d = 128, k = 10");
  static_assert(scan_stage_rows(448, kScanStagePad, 448, 10) == 37, "16896 / 456");
  static_assert(scan_stage_rows(4096, kScanStagePad, 4096, 1024) == 3, "a long row at a wide k: what is left of 40 KiB a wave");
  for (int k : {1, 10, 100, 1024})
    for (int64_t d : {1, 20, 100, 128, 200, 960, 2048, 4096}) {
      const int64_t qwords = (d + 15) & ~(int64_t)15;
      const int stride = (int)u8_widened_stride_words(d);
      const int64_t plain = brute_lds_bytes(qwords, k), staged = brute_staged_lds_bytes(stride, qwords, k);
      CHECK(staged > plain && staged % 16 == 0);
      const int64_t one_row = plain + (int64_t)kWavesPerBlock * (stride * 4 + kScanStagePad + 15);
      if (one_row <= kLdsPerWorkgroup) CHECK(staged <= kLdsPerWorkgroup);
    }
  if (failures) {
    fprintf(stderr, "scan_rows_sanitize_test: %d failures\n", failures);
    return 1;
  }
  printf("scan_rows_sanitize_test ok\n");
  return 0;
}
