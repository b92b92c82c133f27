// host_sanitize_test.cpp -- driver of the `make sanitize` target: the CPU-side C++ of the engine (index layout,
// label sort, window-search-tree / super-tree shapes, the host Vamana builder, graph cache I/O, the
// insertion permutation, the reference's printed words of wann_refdump.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer.  CPU build only: GPU sanitizers are not available on the pool, and nothing here touches HIP.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../include/wann.h"
#include "wann_build.h"
#include "wann_gemm_device.h"
#include "wann_refdump.h"
#include "wann_stdsort.h"
#include <algorithm>

using namespace wann;

static int fails = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #c);  \
      fails++;                                                         \
    }                                                                  \
  } while (0)

static void check_graph(const HostGraph &g, int64_t n, int64_t R) {
  CHECK(g.n == n && g.maxdeg == R);
  for (int64_t i = 0; i < g.n; i++) {
    const int32_t *r = g.row(i);
    CHECK(r[0] >= 0 && r[0] <= g.maxdeg);
    for (int j = 0; j < r[0]; j++) CHECK(r[1 + j] >= 0 && r[1 + j] < n);
  }
}

// The reference's words (wann_refdump.cpp) from hand-made records, against strings written out from the formats of
// tests/golden/verbose_golden.json.  Every array is exactly as long as the dump may read.
static unsigned long long vrec(long long beam, long long unfiltered, long long frontier) {
  return ((unsigned long long)beam << 42) | ((unsigned long long)unfiltered << 21) | (unsigned long long)frontier;
}
static std::string printed(const wann_host::VerboseDump &d) {
  char *buf = nullptr;
  size_t len = 0;
  FILE *f = open_memstream(&buf, &len);
  wann_host::print_verbose_dump(f, d);
  fclose(f);
  std::string s(buf, len);
  free(buf);
  return s;
}
static std::string printed_outside(const std::vector<float> &ranges, float first, float last, int digits) {
  char *buf = nullptr;
  size_t len = 0;
  FILE *f = open_memstream(&buf, &len);
  wann_host::print_outside_range(f, ranges.data(), (int64_t)ranges.size() / 2, first, last, digits);
  fclose(f);
  std::string s(buf, len);
  free(buf);
  return s;
}
static Task task(int query, int mode, int part, int flags) {
  Task t{};
  t.query = query;
  t.mode = mode;
  t.part = part;
  t.flags = flags;
  return t;
}

static void check_refdump() {
  std::vector<PartDesc> parts(3);
  parts[0].n = 2500;
  parts[1].n = 312;
  parts[2].n = 156;
  {  // four queries of three task slots, six records per task, six route entries per query; beam 10 x2, no beam limit in reach
    const int maxt = 3, cap = 6, rw = 1 + 7 * 6;
    const std::vector<Task> tasks = {
        task(0, T_GRAPH, 1, 0), Task{}, Task{},                                        // the super tree's one search
        task(1, T_GRAPH, 1, 2), task(1, T_BRUTE, 0, 0), task(1, T_GRAPH, 2, 2),        // fenwick: a scan between two searches
        task(2, T_GRAPH, 0, 0), Task{}, Task{},                                        // the final search's record is missing
        task(3, T_GRAPH, 0, 0), Task{}, Task{}};                                       // more searches than records fit
    const std::vector<int32_t> qtask_cnt = {1, 3, 1, 1};
    std::vector<int32_t> vlog_n = {4, 0, 0, 1, 0, 2, 1, 0, 0, 9, 0, 0};
    std::vector<unsigned long long> vlog((size_t)4 * maxt * cap, 0);
    auto put = [&](int ti, std::vector<unsigned long long> r) { std::copy(r.begin(), r.end(), vlog.begin() + (size_t)ti * cap); };
    put(0, {vrec(10, 10, 3), vrec(20, 20, 7), vrec(40, 40, 12), vrec(80, 80, 25)});  // doubles twice, re-searched at 40 x 2
    put(3, {vrec(10, 10, 10)});                                                       // flags & 2: multiply 1
    put(5, {vrec(10, 10, 6), vrec(20, 20, 11)});
    put(6, {vrec(10, 10, 10)});
    put(9, {vrec(10, 10, 0), vrec(20, 20, 0), vrec(40, 40, 1), vrec(80, 80, 2), vrec(160, 160, 4), vrec(320, 320, 8)});
    std::vector<int64_t> vroute((size_t)4 * rw, 0);
    auto route = [&](int q, std::vector<std::vector<int64_t>> entries) {
      int64_t *w = vroute.data() + (size_t)q * rw;
      w[0] = 7 * (int64_t)entries.size();
      for (size_t i = 0; i < entries.size(); i++) std::copy(entries[i].begin(), entries[i].end(), w + 1 + 7 * i);
    };
    // (kind, index of the query's next task, five arguments)
    route(0, {{1, 0, 28, 0, 0, 0, 0}, {1, 0, 14, 0, 0, 0, 0}, {2, 0, 2239, 2395, 2198, 2500, 313}, {3, 0, 0, 0, 0, 0, 0}});
    route(1, {{4, 0, 1790, 2415, 0, 0, 0}, {5, 0, 1875, 2188, 0, 0, 0}, {5, 2, 2188, 2344, 0, 0, 0}, {4, 3, 1846, 1875, 0, 0, 0}, {9, 1, 1, 1, 1, 1, 1}});
    const wann_host::VerboseDump d{4, maxt, tasks.data(), qtask_cnt.data(), vlog_n.data(), vlog.data(), cap, vroute.data(), rw, parts.data(), 1234, 10, 10, 2, 10000};
    const std::string want =
        "Testing bucket 28\n"
        "Testing bucket 14\n"
        "Query range = (2239,2395), smallest containing range (size 313) = (2198,2500)\n"
        "Time to find bucket: 0ns\n"
        "Starting optimized postfiltering, beam size = 10, k = 10, final multiply = 2, n = 312\n"
        "Unfiltered return = 10\n"
        "Finished a double, frontier size = 3, beam size = 10\n"
        "Unfiltered return = 20\n"
        "Finished a double, frontier size = 7, beam size = 20\n"
        "Unfiltered return = 40\n"
        "Finished a double, frontier size = 12, beam size = 40\n"
        "Unfiltered return = 80\n"
        "Final frontier size = 25, final beam size 80\n"
        "Time to do searcht: 1234ns\n"
        "Query range: 1790 2415\n"
        "Searching bucket: 1875 2188\n"
        "Starting optimized postfiltering, beam size = 10, k = 10, final multiply = 1, n = 312\n"
        "Unfiltered return = 10\n"
        "Finished a double, frontier size = 10, beam size = 10\n"
        "Final frontier size = 10, final beam size 10\n"
        "Searching bucket: 2188 2344\n"
        "Starting optimized postfiltering, beam size = 10, k = 10, final multiply = 1, n = 156\n"
        "Unfiltered return = 10\n"
        "Finished a double, frontier size = 6, beam size = 10\n"
        "Unfiltered return = 20\n"
        "Finished a double, frontier size = 11, beam size = 20\n"
        "Final frontier size = 11, final beam size 20\n"
        "Query range: 1846 1875\n"  // (belongs to index qtask_cnt: after the last task)
        "Starting optimized postfiltering, beam size = 10, k = 10, final multiply = 2, n = 2500\n"
        "Unfiltered return = 10\n"
        "Finished a double, frontier size = 10, beam size = 10\n"
        "Final frontier size = 10, final beam size 20\n"  // (no record of the final search: the beam is named all the same)
        "Starting optimized postfiltering, beam size = 10, k = 10, final multiply = 2, n = 2500\n"
        "Unfiltered return = 10\n"
        "Finished a double, frontier size = 0, beam size = 10\n"
        "Unfiltered return = 20\n"
        "Finished a double, frontier size = 0, beam size = 20\n"
        "Unfiltered return = 40\n"
        "Finished a double, frontier size = 1, beam size = 40\n"
        "Unfiltered return = 80\n"
        "Finished a double, frontier size = 2, beam size = 80\n"
        "Unfiltered return = 160\n"
        "Finished a double, frontier size = 4, beam size = 160\n"
        "Unfiltered return = 320\n"
        "Finished a double, frontier size = 8, beam size = 320\n"
        "Final frontier size = 8, final beam size 1280\n";
    CHECK(printed(d) == want);
  }
  {  // the beam reaches postfiltering_max_beam: no final search (the golden's postfilter_maxbeam case: beam 8 x3, limit 40)
    const std::vector<Task> tasks = {task(0, T_GRAPH, 0, 0)};
    const std::vector<int32_t> qtask_cnt = {1}, vlog_n = {3};
    const std::vector<unsigned long long> vlog = {vrec(8, 8, 0), vrec(16, 16, 0), vrec(32, 32, 1)};
    const wann_host::VerboseDump d{1, 1, tasks.data(), qtask_cnt.data(), vlog_n.data(), vlog.data(), 3, nullptr, 0, parts.data(), 0, 10, 8, 3, 40};
    CHECK(printed(d) ==
          "Starting optimized postfiltering, beam size = 8, k = 10, final multiply = 3, n = 2500\n"
          "Unfiltered return = 8\n"
          "Finished a double, frontier size = 0, beam size = 8\n"
          "Unfiltered return = 16\n"
          "Finished a double, frontier size = 0, beam size = 16\n"
          "Unfiltered return = 32\n"
          "Finished a double, frontier size = 1, beam size = 32\n"
          "Final frontier size = 1, final beam size 64\n");
  }
  {  // a tree with scan leaves: no records at all, the descent's lines only
    const int rw = 1 + 7;
    const std::vector<Task> tasks = {task(0, T_GRAPH, 0, 0), task(1, T_BRUTE, 0, 0)};
    const std::vector<int32_t> qtask_cnt = {1, 1};
    const std::vector<int64_t> vroute = {7, 2, 0, 2090, 2402, 1875, 2500, 625, 7, 2, 0, 2155, 2467, 1875, 2500, 625};
    const wann_host::VerboseDump d{2, 1, tasks.data(), qtask_cnt.data(), nullptr, nullptr, 24, vroute.data(), rw, parts.data(), 77, 10, 10, 1, 10000};
    CHECK(printed(d) ==
          "Query range = (2090,2402), smallest containing range (size 625) = (1875,2500)\n"
          "Query range = (2155,2467), smallest containing range (size 625) = (1875,2500)\n");
  }
  // the window outside the index's label range: above, inside, below, straddling the upper end
  const std::vector<float> ranges = {2.f, 3.5f, 0.3f, 0.4f, -5.f, -0.9998f, 0.9f, 2.f};
  CHECK(printed_outside(ranges, 0.0002f, 0.9998f, 4) ==
        "Query range is entirely outside the index range (0.0002, 0.9998) index range vs. (2, 3.5) This shouldn't happen but does not directly impact correctness\n"
        "Query range is entirely outside the index range (0.0002, 0.9998) index range vs. (-5, -0.9998) This shouldn't happen but does not directly impact correctness\n");
  const std::vector<float> ranges2 = {0.5f, 0.75f, 1.23456789f, 2.5f};
  CHECK(printed_outside(ranges2, 0.123456789f, 0.987654321f, 6) ==
        "Query range is entirely outside the index range (0.123457, 0.987654) index range vs. (1.23457, 2.5) This shouldn't happen but does not directly impact correctness\n");
  CHECK(printed_outside(ranges2, 0.123456789f, 0.987654321f, 4) ==
        "Query range is entirely outside the index range (0.1235, 0.9877) index range vs. (1.235, 2.5) This shouldn't happen but does not directly impact correctness\n");
  CHECK(printed_outside({}, 0.f, 1.f, 4).empty());
}

// The exact scan's LDS need (brute_lds_bytes_per_wave, wann_device.h: what k_brute carves, launch_brute asks for and run_batch
// checks) against byte counts worked out by hand, on the strides an uploaded index has; and k_finalize_multi's.
static IndexView view_of(int dtype, int d) {
  IndexView v{};
  v.dtype = dtype;
  v.d = d;
  v.stride = dtype == WANN_DTYPE_F32 ? (d + 15) / 16 * 16 : dtype == WANN_DTYPE_F16 ? (2 * d + 63) / 64 * 16 : (d + 63) / 64 * 64 / 4;
  return v;
}
static int64_t scan_lds(int dtype, int d, int k) { return brute_lds_bytes(query_words(view_of(dtype, d)), k); }

static void check_scan_lds() {
  static_assert(kWavesPerBlock == 4 && kLdsPerWorkgroup == 163840 && kLdsNoAttribute == 49152 && kMaxK == 1024, "the figures below assume these");
  // query row + 64 keys + 64 ids + 64 distances + the list: 512 + 512 + 256 + 256 + 80
  CHECK(brute_lds_bytes_per_wave(128, 10) == 1616);
  CHECK(scan_lds(WANN_DTYPE_F32, 128, 10) == 4 * 1616);
  CHECK(scan_lds(WANN_DTYPE_F32, 1024, 1024) == 53248);   // 4 x (4096 + 1024 + 8192): the attribute is needed
  CHECK(scan_lds(WANN_DTYPE_F32, 3072, 10) == 53568);     // 4 x (12288 + 1024 + 80)
  CHECK(scan_lds(WANN_DTYPE_F16, 4096, 1024) == 102400);  // the staged query is the float32 upcast: 4 x (16384 + 1024 + 8192)
  CHECK(scan_lds(WANN_DTYPE_U8, 8192, 1024) == 69632);    // a byte per element: 4 x (8192 + 1024 + 8192)
  CHECK(scan_lds(WANN_DTYPE_I8, 8192, 65) == 38976);      // the list holds an even number of keys: 4 x (8192 + 1024 + 66 x 8)
  CHECK(scan_lds(WANN_DTYPE_F32, 2049, 10) == 37440);     // (the longest row of the suite before result widths were tested)
  // an odd k takes the next even one's list; every count is a multiple of 16
  for (int k = 1; k <= kMaxK; k++) {
    CHECK(brute_lds_bytes_per_wave(16, k) == brute_lds_bytes_per_wave(16, (k + 1) & ~1));
    CHECK(brute_lds_bytes_per_wave(16, k) % 16 == 0 && finalize_lds_bytes_per_wave(k) % 16 == 0);
    CHECK(brute_lds_bytes_per_wave(16, k) == 64 + 1024 + ((k + 1) / 2) * 16);
    CHECK(finalize_lds_bytes_per_wave(k) == 512 + ((k + 1) / 2) * 16);
  }
  CHECK(finalize_lds_bytes_per_wave(kMaxK) * kWavesPerBlock == 34816);
  // the first row length past a CU's 160 KiB (40 960 B a wave) for every element type, at a narrow and at the widest k:
  // 40 960 - 1024 - 80 = 39 856 B of query at k = 10, 40 960 - 1024 - 8192 = 31 744 B at k = 1024, in whole 64-byte rows
  struct { int dtype, k, last_ok; } edges[] = {{WANN_DTYPE_F32, 10, 9952},  {WANN_DTYPE_F32, 1024, 7936}, {WANN_DTYPE_F16, 10, 9952}, {WANN_DTYPE_F16, 1024, 7936},
                                               {WANN_DTYPE_U8, 10, 39808},  {WANN_DTYPE_U8, 1024, 31744}, {WANN_DTYPE_I8, 10, 39808},  {WANN_DTYPE_I8, 1024, 31744}};
  for (auto &e : edges) {
    CHECK(scan_lds(e.dtype, e.last_ok, e.k) <= kLdsPerWorkgroup);
    CHECK(scan_lds(e.dtype, e.last_ok + 1, e.k) > kLdsPerWorkgroup);
    int first_over = 0;  // (and by walking up: the need never decreases with the row length)
    for (int d = 1; d <= 40000 && !first_over; d++)
      if (scan_lds(e.dtype, d, e.k) > kLdsPerWorkgroup) first_over = d;
    CHECK(first_over == e.last_ok + 1);
  }
  // no overflow at row lengths far beyond any index: the count stays positive and above the limit
  CHECK(brute_lds_bytes((int64_t)1 << 31, kMaxK) > kLdsPerWorkgroup);
}

// The dense path's window gate as a function of k (dense_min_window) and the LDS of its re-rank kernels (rerank_lds_bytes): k <= 16
// keeps the two constants and k_rerank's bytes, beyond it 96 k positions and the list of kSelectLarge candidates.
static void check_dense_large_k() {
  static_assert(kSelectLarge == 256 && kDenseMaxK == 128 && kGroupMinWindow == 1024 && kCoverMinWindow == 1024, "the figures below assume these");
  for (int floor : {kGroupMinWindow, kCoverMinWindow}) {
    CHECK(dense_min_window(1, floor) == floor && dense_min_window(16, floor) == floor);
    CHECK(dense_min_window(17, floor) == 1632 && dense_min_window(128, floor) == 12288);
    for (int k = 1; k < kDenseMaxK; k++) CHECK(dense_min_window(k, floor) >= floor && dense_min_window(k, floor) <= dense_min_window(k + 1, floor));
  }
  CHECK(dense_min_window(104, kGroupMinWindow) <= 10000 && dense_min_window(105, kGroupMinWindow) > 10000);  // (the adversarial shape's windows)
  // query row + 64 keys + 64 ids + 64 distances + the list: k <= 16 as it was, beyond it 2 KiB a wave whatever k is
  CHECK(rerank_lds_bytes(view_of(WANN_DTYPE_F32, 128), 10) == 4 * (512 + 1024 + 80));
  CHECK(rerank_lds_bytes(view_of(WANN_DTYPE_F32, 128), 16) == 4 * (512 + 1024 + 128));
  CHECK(rerank_lds_bytes(view_of(WANN_DTYPE_F32, 128), 17) == 4 * (512 + 1024 + 2048));
  CHECK(rerank_lds_bytes(view_of(WANN_DTYPE_F32, 128), 128) == 4 * (512 + 1024 + 2048));
  CHECK(rerank_lds_bytes(view_of(WANN_DTYPE_F32, 2048), 128) == 45056 && 45056 < 48 * 1024);  // 4 x (8192 + 1024 + 2048)
  CHECK(rerank_lds_bytes(view_of(WANN_DTYPE_F16, 2048), 128) == 45056);                       // (the staged query is the float32 upcast)
}

// wann_set_dense_centred without a device: which indexes the switch takes (dense_centred_type), which batches the centred route
// (dense_centred_route), the layout of the centred buffer, the room k_row_centre's partial sums need inside it, and the error
// term against its derivation evaluated in double precision.
static void check_dense_centred() {
  for (int dt = -1; dt <= 9; dt++)
    for (int metric = 0; metric < 2; metric++)
      CHECK(dense_centred_type(dt, metric) == ((dt == WANN_DTYPE_F32 || dt == WANN_DTYPE_F16) && metric == 0));
  for (int dt : {WANN_DTYPE_F32, WANN_DTYPE_F16})
    for (int d : {1, 16, 100, 128, 129, 200, 2048}) {
      IndexView v = view_of(dt, d);
      CHECK(dense_centred_route(v, true, false) == (d <= 128));  // (the narrow class alone)
      CHECK(!dense_centred_route(v, false, false));              // (switch off)
      CHECK(!dense_centred_route(v, true, true));                // (wann_set_dense_rows keeps precedence)
      v.metric = 1;
      CHECK(!dense_centred_route(v, true, false));
    }
  CHECK(!dense_centred_route(view_of(WANN_DTYPE_BF16, 64), true, false) && !dense_centred_route(view_of(WANN_DTYPE_F8, 64), true, false) &&
        !dense_centred_route(view_of(WANN_DTYPE_U8, 64), true, false));
  // norms | c | maximum: n + words + 1 floats; the partial sums are at most 256 rows of `words` floats and lie inside the norms'
  // floats, or are the single row c
  for (int64_t n : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)127, (int64_t)128, (int64_t)1000, (int64_t)32767, (int64_t)32768, (int64_t)100000000})
    for (int words : {16, 112, 128}) {
      const int parts = centred_parts(n, words);
      CHECK(centred_buf_floats(n, words) == (size_t)n + words + 1);
      CHECK(parts >= 1 && parts <= 256 && (n >= words ? (int64_t)parts * words <= n : parts == 1));
      const int64_t per = (n + parts - 1) / parts;  // (k_row_centre's slices cover every row)
      CHECK(per * parts >= n);
    }
  const double u = std::ldexp(1.0, -24), u1 = u / (1.0 - u);
  CHECK((double)kCentredErr > 2.0 * u1 + u1 * u1 && (double)kCentredErr <= 2.5 * u);
}

// wann_set_dense_window_norms without a device: the sparse table's shape.  Level j holds runs of 2^j blocks; the lookup of a window
// that spans m blocks reads level floor(log2 m), so the last level must reach a run of at least nblocks / 2 + 1 blocks, and the
// levels of the launcher's loop (1 .. levels - 1, half = 2^(j-1)) must be exactly the ones the table has room for.
static void check_dense_window_norms() {
  CHECK(norm_table_words(0) == 0 && norm_table_words(1) == 1 && norm_table_words(64) == 1 && norm_table_words(65) == 4);
  CHECK(norm_table_blocks(1000000) == 15625 && norm_table_levels(15625) == 15 && norm_table_words(1000000) * 4 < (1u << 20));
  for (int64_t nb : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)33554432}) {
    const int levels = norm_table_levels(nb);
    int j = 0;  // floor(log2 nb): the level a window over every block reads
    while (((int64_t)2 << j) <= nb) j++;
    CHECK(levels >= 1 && j < levels && ((int64_t)1 << (levels - 1)) >= nb && (levels == 1 || ((int64_t)1 << (levels - 2)) < nb));
  }
  // The index arithmetic the kernels run (norm_level_half / norm_level_partner: k_norm_levels and its launcher; norm_lookup:
  // window_norm_max), over whole small tables -- levels 0 .. 3 and most clamps are out of reach of any dense batch, whose
  // windows hold at least 1 024 positions.  Level 0 is filled with three patterns at once (random values; rising: the maximum is
  // the LAST block of the cover; falling: the first), the levels are built as the launcher builds them, and for every window
  // 0 <= lo < hi <= 64 nblocks the two entries read must lie inside the table and their maximum must be the maximum of level 0
  // over the blocks lo >> 6 .. (hi - 1) >> 6, no more and no less: at least the window's own maximum, and nothing of a block
  // beyond that cover.  The vectors are exactly the table's words: a read outside them is AddressSanitizer's.
  constexpr int kPat = 3;
  std::mt19937 rng(12345);
  std::vector<int> sizes;
  for (int nb = 1; nb <= 70; nb++) sizes.push_back(nb);
  for (int nb : {127, 128, 129, 641}) sizes.push_back(nb);
  long long windows = 0;
  for (int nb : sizes) {
    const int levels = norm_table_levels(nb), stride = nb > 70 ? 7 : 1;
    std::vector<unsigned int> table[kPat], cover[kPat];  // cover[b0 * nb + b1]: level 0's maximum over b0 .. b1, by brute force
    for (int p = 0; p < kPat; p++) {
      std::vector<unsigned int> &t = table[p];
      t.assign((size_t)nb * levels, 0u);
      for (int b = 0; b < nb; b++) t[b] = p == 0 ? (unsigned int)(rng() >> 1) : p == 1 ? 1000u + b : 1000000u - b;
      for (int j = 1; j < levels; j++)
        for (int b = 0; b < nb; b++) {
          const int b2 = norm_level_partner(b, norm_level_half(j), nb);
          CHECK(b2 >= 0 && b2 < nb);
          t[(size_t)j * nb + b] = std::max(t[(size_t)(j - 1) * nb + b], t[(size_t)(j - 1) * nb + b2]);
        }
      cover[p].assign((size_t)nb * nb, 0u);
      for (int b0 = 0; b0 < nb; b0++) {
        unsigned int m = 0;
        for (int b1 = b0; b1 < nb; b1++) cover[p][(size_t)b0 * nb + b1] = m = std::max(m, t[b1]);
      }
    }
    int bad = 0;
    for (int64_t lo = 0; lo < (int64_t)kNormBlock * nb; lo += stride)
      for (int64_t hi = lo + 1; hi <= (int64_t)kNormBlock * nb; hi += stride) {
        const NormLookup at = norm_lookup(lo, hi, nb);
        windows++;
        if (at.j < 0 || at.j >= levels || at.x < 0 || at.x >= nb || at.y < 0 || at.y >= nb) {
          bad++;
          continue;
        }
        const size_t row = (size_t)at.j * nb, want = (size_t)(lo >> 6) * nb + (size_t)((hi - 1) >> 6);
        for (int p = 0; p < kPat; p++) bad += std::max(table[p][row + at.x], table[p][row + at.y]) != cover[p][want];
      }
    if (bad) fprintf(stderr, "norm table of %d blocks: %d windows whose lookup is not the maximum of their covering blocks\n", nb, bad);
    CHECK(bad == 0);
    // degenerate arguments: the clamps keep both entries inside the table (empty and reversed windows, positions before the
    // first and beyond the last block)
    for (int64_t lo : {(int64_t)-100000, (int64_t)-65, (int64_t)-64, (int64_t)-1, (int64_t)0, (int64_t)63, (int64_t)64, (int64_t)kNormBlock * nb - 1,
                       (int64_t)kNormBlock * nb, (int64_t)kNormBlock * nb + 1, (int64_t)kNormBlock * nb + 100000, ((int64_t)1 << 30) * kNormBlock - 1})
      for (int64_t hi : {(int64_t)-100000, (int64_t)-64, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)64, (int64_t)65, (int64_t)kNormBlock * nb - 1,
                         (int64_t)kNormBlock * nb, (int64_t)kNormBlock * nb + 1, (int64_t)kNormBlock * nb + 64, (int64_t)kNormBlock * nb + 100000,
                         ((int64_t)1 << 30) * kNormBlock}) {
        const NormLookup at = norm_lookup(lo, hi, nb);
        CHECK(at.j >= 0 && at.j < levels && at.x >= 0 && at.x < nb && at.y >= 0 && at.y < nb && at.y + (1 << at.j) <= nb);
        unsigned int sink = std::max(table[0][(size_t)at.j * nb + at.x], table[0][(size_t)at.j * nb + at.y]);
        CHECK(sink >= table[0][at.x]);  // (the first run starts at block x: its maximum holds that block)
      }
  }
  CHECK(windows > 200000000);  // (every window of the 70 small tables alone: sum of (64 nb)(64 nb + 1) / 2)
}

// The row-type table (wann_row_types.h) against the values written out here: every class, the caller's bytes, the device
// pitch, the staged query's length and the kinds of unit of every id from -1 to 9.  (That the two layout rules are
// permutations: byte_layout_sanitize_test.cpp and half_layout_sanitize_test.cpp.)
static void check_row_types() {
  struct Want {
    int id, known, caller_bytes, byte_dot, two_byte, quad, upcast, pitch /* 0 the spec's, 1 two-byte, 2 one-byte */, search, dense, build;
  };
  const Want want[] = {{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 4, 0, 0, 0, 0, 0, 1, 1, 1}, {1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1},
                       {2, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1},  {3, 1, 2, 0, 1, 0, 1, 1, 1, 1, 0}, {4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                       {5, 1, 2, 0, 1, 0, 1, 1, 1, 1, 0},  {6, 0, 0, 0, 0, 1, 0, 2, 1, 1, 0}, {7, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0},
                       {8, 1, 1, 0, 0, 1, 1, 2, 1, 1, 0},  {9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
  const int ds[10] = {1, 31, 32, 33, 63, 64, 65, 100, 128, 2048};
  const int two_byte_words[10] = {16, 16, 16, 32, 32, 32, 48, 64, 64, 1024};  // ((2 d + 63) / 64) * 16
  const int one_byte_words[10] = {16, 16, 16, 16, 16, 16, 32, 32, 32, 512};   // ((d + 63) / 64) * 16
  const int f32_words[10] = {16, 32, 32, 48, 64, 64, 80, 112, 128, 2048};     // d rounded up to 16: the float32 row, the widened types' query
  const int spec = 12345;  // (a stride no rule gives: the types that keep the spec's hand it through)
  static_assert(kRowsU8Widened == 6 && kRowsF16Paired == 7 && kRowsF8 == 8, "the ids that code names");
  int seen = 0;
  for (const Want &w : want) {
    CHECK(w.id == seen - 1);
    seen++;
    CHECK(known_dtype(w.id) == (w.known != 0));
    CHECK(element_bytes(w.id) == w.caller_bytes);
    CHECK(byte_rows(w.id) == (w.byte_dot != 0));
    CHECK(two_byte_rows(w.id) == (w.two_byte != 0));
    CHECK(one_byte_widened_rows(w.id) == (w.quad != 0));
    CHECK(widened_rows(w.id) == (w.two_byte != 0 || w.quad != 0));
    CHECK(upcast_built(w.id) == (w.upcast != 0));
    CHECK(row_type(w.id).search == (w.search != 0) && row_type(w.id).dense == (w.dense != 0) && row_type(w.id).build == (w.build != 0));
    CHECK(row_type(w.id).id == (w.search ? w.id : -1));  // (every listed type has a search unit; an unlisted id is no entry at all)
    for (int i = 0; i < 10; i++) {
      const int d = ds[i], words = w.pitch == 1 ? two_byte_words[i] : w.pitch == 2 ? one_byte_words[i] : spec;
      CHECK(row_stride_words(w.id, d, spec) == words);
      CHECK(query_words(w.id, d, words) == ((w.two_byte || w.quad) ? f32_words[i] : words));
      IndexView v{};
      v.dtype = w.id, v.d = d, v.stride = words;
      CHECK(query_words(v) == query_words(w.id, d, words));
    }
  }
  CHECK(seen == 11);
  for (int i = 0; i < 10; i++) {  // the build spec's stride: the stored rows -- the float32 upcast where the type is built from it
    CHECK(spec_stride_words(0, ds[i]) == f32_words[i] && spec_stride_words(3, ds[i]) == f32_words[i] && spec_stride_words(5, ds[i]) == f32_words[i] &&
          spec_stride_words(8, ds[i]) == f32_words[i]);
    CHECK(spec_stride_words(1, ds[i]) == one_byte_words[i] && spec_stride_words(2, ds[i]) == one_byte_words[i]);
  }
}

int main(int argc, char **argv) {
  const std::string tmp = argc > 1 ? argv[1] : "/tmp/wann_sanitize";
  (void)system(("mkdir -p " + tmp).c_str());
  std::mt19937 rng(7);
  std::normal_distribution<float> nd;
  for (int metric = 0; metric < 2; metric++)
    for (int kind : {WANN_KIND_PREFILTER, WANN_KIND_POSTFILTER, WANN_KIND_TREE_PREFILTER, WANN_KIND_TREE_VAMANA, WANN_KIND_SUPER}) {
      const int64_t n = kind == WANN_KIND_SUPER ? 1500 : 2300, d = metric ? 20 : 13;  // d not a multiple of 4 / 8 / 16
      std::vector<float> pts((size_t)n * d), labels((size_t)n);
      for (auto &x : pts) x = metric ? nd(rng) : std::rint(nd(rng) * 20.f);  // integer-valued rows: distance ties
      for (int64_t i = 0; i < n; i++) labels[(size_t)i] = (float)((i * 7919) % n) + 0.5f;
      for (int pass = 0; pass < 2; pass++) {  // pass 0 builds and saves the cache, pass 1 loads it
        HostIndex H;
        H.spec.kind = kind;
        H.spec.metric = metric;
        H.spec.n = n;
        H.spec.d = d;
        H.spec.cutoff = 300;
        H.spec.split_factor = kind == WANN_KIND_SUPER ? 2.5 : 3;
        H.spec.shift_factor = 0.3;
        H.spec.R = 12;
        H.spec.L = 24;
        H.spec.alpha = 1.1;
        H.spec.threads = 3;
        H.spec.cache = tmp + "/k" + std::to_string(kind) + "m" + std::to_string(metric) + "_";
        std::vector<HostPart *> pending;
        build_host_index(H, pts.data(), labels.data(), -1, 0, &pending);
        CHECK(pass == 0 || pending.empty());
        if (!pending.empty()) {
          build_pending_on_host(H, pending);
          save_built_graphs(H, pending, true);
        }
        CHECK((int64_t)H.labels.size() == n && (int64_t)H.pts.size() == n * H.spec.stride);
        for (auto &lv : H.levels)
          for (auto &P : lv) {
            CHECK(P.start >= 0 && P.start + P.n <= n);
            if (H.vamana_leaves) check_graph(P.g, P.n, H.spec.R);
          }
      }
      // the sharded cache build (wann_build_cache_shard's body) writes the same files
      for (int shard = 0; shard < 2; shard++) {
        HostIndex H;
        H.spec.kind = kind;
        H.spec.metric = metric;
        H.spec.n = n;
        H.spec.d = d;
        H.spec.cutoff = 300;
        H.spec.split_factor = kind == WANN_KIND_SUPER ? 2.5 : 3;
        H.spec.shift_factor = 0.3;
        H.spec.R = 12;
        H.spec.L = 24;
        H.spec.alpha = 1.1;
        H.spec.threads = 2;
        H.spec.cache = tmp + "/shard_k" + std::to_string(kind) + "m" + std::to_string(metric) + "_";
        build_host_index(H, pts.data(), labels.data(), shard, 2);
      }
    }
  // graph file round trip, truncated / corrupt files must be rejected without reading out of bounds
  {
    HostGraph g;
    std::vector<float> pts(400 * 16);
    for (auto &x : pts) x = nd(rng);
    vamana_build(pts.data(), 16, 9, 0, 0, 400, 8, 16, 1.2, g, 2);
    check_graph(g, 400, 8);
    const std::string path = tmp + "/roundtrip.bin";
    CHECK(graph_file_save(path, g));
    HostGraph h;
    CHECK(graph_file_load(path, h) && h.n == g.n && h.maxdeg == g.maxdeg);
    for (int64_t i = 0; i < g.n && h.n == g.n; i++) {  // (slots past the degree are unspecified in a built row)
      CHECK(h.row(i)[0] == g.row(i)[0]);
      for (int j = 1; j <= g.row(i)[0]; j++) CHECK(h.row(i)[j] == g.row(i)[j]);
    }
    CHECK(truncate(path.c_str(), 100) == 0);
    HostGraph t;
    CHECK(!graph_file_load(path, t));
    CHECK(!graph_file_load(tmp + "/does_not_exist.bin", t));
  }
  for (int64_t n : {1, 2, 3, 100, 8191, 8192, 8193, 20000}) {
    std::vector<int32_t> p = insertion_order(n);
    std::vector<char> seen((size_t)n, 0);
    CHECK((int64_t)p.size() == n);
    for (int32_t x : p) {
      CHECK(x >= 0 && x < n && !seen[(size_t)x]);
      if (x >= 0 && x < n) seen[(size_t)x] = 1;
    }
  }
  // the restated std::sort (wann_stdsort.h) against libstdc++'s own, distance-only comparator, sequences full of ties
  {
    auto check = [&](std::vector<uint64_t> v) {
      std::vector<uint64_t> want = v, got = v;
      std::sort(want.begin(), want.end(), DistOnlyLess());
      int32_t stack[128];
      std_sort_emulated(got.data(), (int)got.size(), stack, DistOnlyLess());
      CHECK(got == want);
      want = v;
      got = v;
      std::sort(want.begin(), want.end(), FullKeyLess());
      std_sort_emulated(got.data(), (int)got.size(), stack, FullKeyLess());
      CHECK(got == want);
    };
    for (int n = 0; n <= 2600; n += (n < 70 ? 1 : 37)) {
      for (int levels : {1, 2, 5, 40, 1 << 20}) {  // number of distinct distances
        std::vector<uint64_t> v((size_t)n);
        for (int i = 0; i < n; i++) v[(size_t)i] = ((uint64_t)(rng() % (uint32_t)levels) << 32) | ((uint64_t)(uint32_t)i << 1);
        check(v);
        std::sort(v.begin(), v.end());
        check(v);  // already sorted
        std::reverse(v.begin(), v.end());
        check(v);
      }
    }
    // a median-of-three killer (exhausts the depth limit: the heapsort branch) and an organ pipe
    for (int n : {64, 512, 2048, 4096}) {
      std::vector<uint64_t> v((size_t)n);
      const int k = n / 2;
      for (int i = 1; i <= k; i++) {
        if (i & 1) {
          v[(size_t)i - 1] = (uint64_t)i << 32;
          v[(size_t)i] = (uint64_t)(k + i) << 32;
        }
        v[(size_t)(k + i - 1)] = (uint64_t)(2 * i) << 32;
      }
      for (int i = 0; i < n; i++) v[(size_t)i] |= (uint64_t)(uint32_t)i << 1;
      check(v);
      for (int i = 0; i < n; i++) v[(size_t)i] = ((uint64_t)(i < n / 2 ? i : n - i) << 32) | ((uint64_t)(uint32_t)i << 1);
      check(v);
    }
  }
  // the dense path's row classes (dense_row_class, wann_gemm_device.h) against the table written out as literal boundaries, on the
  // strides an uploaded index has: float32 d rounded up to 16 words, bytes d rounded up to 64 bytes, float16 2 d bytes likewise
  for (int dtype : {WANN_DTYPE_F32, WANN_DTYPE_U8, WANN_DTYPE_I8, WANN_DTYPE_F16})
    for (int d = 1; d <= 2200; d++)
      for (int dense_long = 0; dense_long < 2; dense_long++) {
        IndexView v{};
        v.dtype = dtype;
        v.d = d;
        v.stride = dtype == WANN_DTYPE_F32 ? (d + 15) / 16 * 16 : dtype == WANN_DTYPE_F16 ? (2 * d + 63) / 64 * 16 : (d + 63) / 64 * 64 / 4;
        // elements a row holds after padding: floats and halves to 16, bytes to 64
        const int len = dtype == WANN_DTYPE_U8 || dtype == WANN_DTYPE_I8 ? (d + 63) / 64 * 64 : (d + 15) / 16 * 16;
        DenseRows want;
        if (dtype == WANN_DTYPE_F32) want = len <= 128 ? kRowsNarrow : len <= 512 ? kRowsWide : len <= 2048 ? kRowsLong : kRowsNone;
        else if (dtype == WANN_DTYPE_F16) want = len <= 128 ? kRowsNarrow : len <= 2048 ? kRowsLong : kRowsNone;
        else want = len <= 512 ? kRowsNarrow : len <= 2048 ? kRowsLong : kRowsNone;
        const DenseRows got = dense_row_class(v);
        CHECK(got == want);
        // what the host admits (dense_rows_ok): the long class only where the process has opted in
        const bool admitted = got != kRowsNone && (got != kRowsLong || dense_long);
        const int limit = dense_long ? 2048 : dtype == WANN_DTYPE_F16 ? 128 : 512;  // elements: floats, halves, bytes
        CHECK(admitted == (len <= limit));
        v.stride += 8;  // not a multiple of 16 words: no kernel takes it
        CHECK(dense_row_class(v) == kRowsNone);
      }
  check_scan_lds();
  check_dense_large_k();
  check_dense_centred();
  check_dense_window_norms();
  check_row_types();
  check_refdump();
  // the C ABI's argument validation (no device needed for these paths) lives in wann_abi.cpp and is covered by tests/test_abi.py
  if (fails) {
    fprintf(stderr, "host sanitize test: %d check(s) failed\n", fails);
    return 1;
  }
  printf("HOST_SANITIZE_OK\n");
  return 0;
}
