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
