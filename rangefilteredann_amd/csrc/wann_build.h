// wann_build.h -- host side of index construction: label sort, tree shapes, graph cache files and
// the multi-threaded Vamana builder.  Reference behaviour being reproduced (not its code):
//   label sort / id mapping      src/tree_utils.h:39-98
//   B-ary window search tree     src/range_filter_tree.h:129-189
//   overlapping "super" tree     src/super_optimized_postfilter_tree.h:118-171
//   graph cache name + format    src/postfilter_vamana.h:126-132, ParlayANN/algorithms/utils/graph.h:126-196
//   Vamana batch build           ParlayANN/algorithms/vamana/index.h:61-135,211-313
#pragma once
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

namespace wann {

struct HostGraph {
  int64_t n = 0;
  int32_t maxdeg = 0;
  std::vector<int32_t> rows;  // n x (maxdeg+1), slot 0 = degree (the reference's in-memory layout)
  int32_t *row(int64_t i) { return rows.data() + i * (maxdeg + 1); }
  const int32_t *row(int64_t i) const { return rows.data() + i * (maxdeg + 1); }
};

struct HostPart {
  int64_t start = 0, n = 0;  // slice [start, start+n) of the sorted order
  float lo = 0, hi = 0;      // min / max label of the slice
  HostGraph g;               // Vamana leaves only
};

struct BuildSpec {
  int kind = 0, metric = 0;
  int dtype = 0;  // element type of the caller's rows (wann.h WANN_DTYPE_*): float32, uint8 / int8 bytes, float16, bfloat16 or float8
  int64_t n = 0, d = 0, stride = 0;  // stride: 32-bit words per row of HostIndex::pts
  int32_t cutoff = 1000;
  double split_factor = 2, shift_factor = 0.5;
  int64_t R = 64, L = 500;
  double alpha = 1.0;
  std::string cache;
  int threads = 0;
};

struct HostIndex {
  BuildSpec spec;
  bool vamana_leaves = false, sorted = false;
  std::vector<float> pts;          // n x stride 32-bit words: zero padded rows (label-sorted for tree kinds); float32 values, or the
                                   // d bytes of a uint8 / int8 row (float16 points: their exact float32 upcast -- the host builder
                                   // and the GPU builder score float32 rows; upload_index stores the device rows as halves)
  std::vector<float> labels;       // same order as pts
  std::vector<uint32_t> decoding;  // row -> original id
  std::vector<std::vector<int64_t>> offsets;  // WST bucket offsets per level
  std::vector<int64_t> sup_size, sup_shift;   // super tree per level
  std::vector<std::vector<HostPart>> levels;
  std::vector<float> fv_sorted;    // stand-alone prefilter
  std::vector<int32_t> fi_sorted;
};

// parallel-for over [0,n) on a persistent pool (dynamic chunks); nested calls run inline
void parallel_for(int64_t n, int threads, const std::function<void(int64_t)> &f);
int default_threads();

// true if every one of the n x d values (rows `stride` floats apart) is exactly representable in IEEE binary16 and finite:
// what a float32 index needs to be searched from half rows (wann.h wann_rows_fp16_exact).  threads <= 0: default_threads().
bool rows_fp16_exact(const float *rows, int64_t n, int64_t d, int64_t stride, int threads);
// true if every one of the n x d values is an integer 0 .. 255 with the bits of (float)(uint8_t)x (no -0.0): what a float32
// index needs to be searched from one-byte rows (wann.h wann_rows_u8_exact).  threads <= 0: default_threads().
bool rows_u8_exact(const float *rows, int64_t n, int64_t d, int64_t stride, int threads);
// such a point set as one-byte rows: the d values of row r as bytes, natural order, at word r * out_words of the ZEROED buffer
// `out` (n * out_words 32-bit words; out_words * 4 >= d -- u8_widened_stride_words(d) in wann_row_types.h)
void pack_u8_rows(const float *rows, int64_t n, int64_t d, int64_t stride, int64_t out_words, int threads, float *out);
// the rows of a float8 index (`rows`: the exact float32 upcast of its E4M3 patterns) as those patterns again, the same way
void pack_f8_rows(const float *rows, int64_t n, int64_t d, int64_t stride, int64_t out_words, int threads, float *out);
// packed rows (natural order) into the device copy's layout, in place: the byte at position e of a row moves to position
// u8_row_position(e) (wann_row_types.h: a permutation inside every aligned 32 bytes).  `words` 32-bit words per row, a multiple of 8.
void interleave_u8_rows(float *rows, int64_t n, int64_t words, int threads);
// half rows (natural order, zero padded) into the half shadow rows' device layout, in place: the half at position e of a row
// moves to position h16_row_position(e) (wann_row_types.h: a permutation inside every aligned 16 halves).  `words` 32-bit words
// per row, a multiple of 8.
void interleave_h16_rows(float *rows, int64_t n, int64_t words, int threads);

// metric: bit 0 = inner product, bits 4-5 = element type of the rows behind p / q (0 float32, 1 uint8, 2 int8; float16 point
// sets are built from their float32 upcast and pass 0)
float host_distance(int metric, const float *p, const float *q, int d);

bool graph_file_load(const std::string &path, HostGraph &g);
bool graph_file_save(const std::string &path, const HostGraph &g);
std::string graph_file_name(const BuildSpec &s, float lo, float hi, int64_t n);

// Build the graph of one partition (rows [start, start+n) of pts).
// parlay::random_permutation<int>(n): the reference's insertion order (vamana/index.h:233, parlay/random.h:79-159)
std::vector<int32_t> insertion_order(int64_t n);

void vamana_build(const float *pts, int64_t stride, int64_t d, int metric, int64_t start, int64_t n,
                  int64_t R, int64_t L, double alpha, HostGraph &g, int threads);

// Sort, lay out the tree and obtain every partition's graph (cache or build).
// shard/nshards >= 0: only materialise (build + save) partitions p with p % nshards == shard.
// pending != nullptr: graphs missing from the cache are NOT built here but returned in *pending
// (the caller builds them, on the GPU or with build_pending_on_host, then calls save_built_graphs).
void build_host_index(HostIndex &H, const void *points, const float *labels, int shard = -1,
                      int nshards = 0, std::vector<HostPart *> *pending = nullptr);
void build_pending_on_host(HostIndex &H, std::vector<HostPart *> &pending);
void save_built_graphs(HostIndex &H, std::vector<HostPart *> &built, bool keep);

}  // namespace wann
