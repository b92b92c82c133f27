// wann_gemm_launch.inc -- the launchers of the dense prefilter path, included at the end of wann_gemm_kernels_body.inc: one text,
// compiled in every unit (float32, uint8, int8, float16, bfloat16, one-byte shadow rows, float8) against that unit's kernels.  A unit picks its kernels by the row class
// (dense_row_class, wann_gemm_device.h: the only place that knows a row length) and exposes its launchers as one constant table,
// gemm_unit(); the float32 unit also holds the entry points of wann_gemm_device.h, which look the table up by ix.dtype (gemm_unit_of).
// Every launcher returns null when it has launched, otherwise the error text.

static const char *gerr_of(hipError_t e) { return e == hipSuccess ? nullptr : hipGetErrorString(e); }

struct ScoreKernel {
  void (*kern)(GemmArgs);  // null: the unit has no kernel for the row class
  size_t lds;              // dynamic LDS bytes
  int per_cu;              // workgroups per CU the grid is sized for
  bool needs_qsplit;       // takes the queries pre-split / pre-packed (GemmArgs::qsplit)
};

WANN_GNS_BEGIN
// (the launchers stand in the order in which they first name their kernels -- cover re-rank, score kernels, re-rank: the order the
// compiler lays the template instances out in, so a unit's code object stays byte for byte what it was)
// the selection / re-rank kernels: a wave per query, four waves x (staged query row, candidate arrays, the k-entry merge list) of LDS
static dim3 rerank_grid(const GemmArgs &a) { return dim3((unsigned)std::min<int64_t>(4096, (a.nq + 3) / 4)); }
static size_t rerank_lds_bytes(const IndexView &ix, int k) {
  return (size_t)4 * (((query_words(ix) * 4 + 15) & ~15) + 64 * 8 + 64 * 4 + 64 * 4 + ((k + 1) & ~1) * 8);
}

#if WANN_DT != 6  // (the unit of the one-byte shadow rows holds score kernels only)
static const char *unit_rerank_cover(const CoverArgs &c, void *stream) {
  void (*kern)(CoverArgs) = nullptr;
#if WANN_BYTE_ROWS
  if (dense_row_class(c.g.ix) == kRowsLong) kern = c.g.ix.metric == 1 ? k_rerank_cover_bslab<1> : k_rerank_cover_bslab<0>;  // (quantised keys)
#endif
  if (!kern) kern = c.g.ix.metric == 1 ? k_rerank_cover<1> : k_rerank_cover<0>;
  hipLaunchKernelGGL(kern, rerank_grid(c.g), dim3(256), rerank_lds_bytes(c.g.ix, c.g.k), (hipStream_t)stream, c);
  return gerr_of(hipGetLastError());
}
#endif

static ScoreKernel pick_score_kernel(const IndexView &ix) {
  const DenseRows rows = dense_row_class(ix);
  const int words = query_words(ix);
  void (*kern)(GemmArgs) = nullptr;
#if WANN_BYTE_ROWS
  // long: run-time slab count, both operands staged per 256-byte slab (queries pre-packed)
  if (rows == kRowsLong) return {k_gemm_scores_bslab, (size_t)2 * 128 * (256 + 16) + 3 * 128 * 4, 2, true};
  if (rows != kRowsNarrow) return {};
  const int nch = words / 16;  // 64-byte chunks of a row
  int per_cu = 2;
  switch (nch) {
    case 1: kern = k_gemm_scores_b<1>; break;
    case 2: kern = k_gemm_scores_b<2>; break;
    case 3: kern = k_gemm_scores_b<3>; break;
    case 4: kern = k_gemm_scores_b<4>; break;
    case 5: kern = k_gemm_scores_b<5>, per_cu = 1; break;
    case 6: kern = k_gemm_scores_b<6>, per_cu = 1; break;
    case 7: kern = k_gemm_scores_b<7>, per_cu = 1; break;
    default: kern = k_gemm_scores_b<8>, per_cu = 1; break;
  }
  return {kern, (size_t)128 * (64 * nch + 16) + 3 * 128 * 4, per_cu, false};
#else
  // long: run-time slab count, both operands staged per slab (queries pre-split, `words` words a row), one workgroup per CU
#if WANN_DT == 3
  if (rows == kRowsLong) return {k_gemm_scores_hslab, (size_t)2 * 128 * (4 * 128 + 16) + 2 * 128 * 4, 1, true};
#elif WANN_DT == 5 || WANN_QUAD_ROWS
  // (bfloat16 and float8 rows, and the one-byte shadow rows of a float32 index: narrow only; dense_row_class names no other class for them)
#else
  if (rows == kRowsLong) return {k_gemm_scores_long, (size_t)2 * 128 * (4 * 128 + 16) + 2 * 128 * 4, 1, true};
  if (rows == kRowsWide) {  // slabs of 128, A operand in registers, one workgroup per CU
    const int slabs = (words + 127) / 128;
    // (four slabs: + the low halves of the last slab's A operand; the overlapped kernel: + its parity arrays and the raw half slab)
    const bool four = slabs == 4;
    kern = slabs == 2 ? k_gemm_scores_wide<2> : slabs == 3 ? k_gemm_scores_wide<3> : k_gemm_scores_wide4;
    return {kern, (size_t)128 * (4 * 128 + 16) + (four ? 4 : 3) * 128 * 4 + (four ? (size_t)4 * 8 * 64 * 16 + (size_t)32 * 1024 : 0), 1, false};
  }
#endif
  if (rows != kRowsNarrow) return {};
  switch (words) {
    case 16: kern = k_gemm_scores<16>; break;
    case 32: kern = k_gemm_scores<32>; break;
    case 48: kern = k_gemm_scores<48>; break;
    case 64: kern = k_gemm_scores<64>; break;
    case 80: kern = k_gemm_scores<80>; break;
    case 96: kern = k_gemm_scores<96>; break;
    case 112: kern = k_gemm_scores<112>; break;
    default: kern = k_gemm_scores<128>; break;
  }
  // two workgroups per CU (the LDS allows it): one stores its scores while the other runs its MFMAs
  // (bfloat16 rows and one-byte shadow rows: the same bytes -- the float32 query tile passes through the staging area, see
  // wann_gemm_kernels_bf16.inc)
  return {kern, (size_t)128 * (4 * words + 16) + 3 * 128 * 4, 2, false};
#endif
}

static const char *unit_gemm_scores(const GemmArgs &a, int num_cus, void *stream) {
  const ScoreKernel s = pick_score_kernel(a.ix);
  if (!s.kern) return "row too long for the dense prefilter tile";
  if (s.needs_qsplit && !a.qsplit) return "the long-row score kernel needs the split / packed queries";
  if (s.lds > 48 * 1024)
    if (const char *e = gerr_of(hipFuncSetAttribute((const void *)s.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds))) return e;
  hipLaunchKernelGGL(s.kern, dim3(s.per_cu * (num_cus > 0 ? num_cus : 256)), dim3(256), s.lds, (hipStream_t)stream, a);
  return gerr_of(hipGetLastError());
}

#if WANN_DT != 6
static const char *unit_point_sums(const IndexView &ix, float *norm2, unsigned int *max_bits, int32_t *term, void *stream) {
  if (ix.n <= 0) return nullptr;
  const int wpb = 4;  // a wave per row
  const dim3 grid((unsigned)((ix.n + wpb - 1) / wpb)), block(64 * wpb);
#if WANN_BYTE_ROWS
  hipLaunchKernelGGL(k_point_terms_b, grid, block, 0, (hipStream_t)stream, ix, term);
#else
  hipLaunchKernelGGL(k_point_norms, grid, block, 0, (hipStream_t)stream, ix, norm2, max_bits);
#endif
  return gerr_of(hipGetLastError());
}

#if !WANN_HALF_ROWS && WANN_DT != 8  // (float16 rows: the float32 unit's k_split_queries; bfloat16 / float8 rows have no long class)
static const char *unit_prep_queries(const float *queries, int64_t nq, int d, int words, uint32_t *out, void *stream) {
#if WANN_BYTE_ROWS
  const int64_t items = nq * words;  // a thread per packed word
#else
  const int64_t items = nq * (words >> 1);  // a thread per bf16 pair
#endif
  if (items <= 0) return nullptr;
  const dim3 grid((unsigned)((items + 255) / 256)), block(256);
#if WANN_BYTE_ROWS
  hipLaunchKernelGGL(k_pack_queries_b, grid, block, 0, (hipStream_t)stream, queries, nq, d, words, out);
#else
  hipLaunchKernelGGL(k_split_queries, grid, block, 0, (hipStream_t)stream, queries, nq, d, words, out);
#endif
  return gerr_of(hipGetLastError());
}
#endif

static const char *unit_select_rerank(const GemmArgs &a, Counters *ctr, void *stream) {
  void (*kern)(GemmArgs, Counters *) = nullptr;
#if WANN_BYTE_ROWS
  if (dense_row_class(a.ix) == kRowsLong) kern = a.ix.metric == 1 ? k_rerank_bslab<1> : k_rerank_bslab<0>;  // (quantised keys)
#endif
  if (!kern) kern = a.ix.metric == 1 ? k_rerank<1> : k_rerank<0>;
  hipLaunchKernelGGL(kern, rerank_grid(a), dim3(256), rerank_lds_bytes(a.ix, a.k), (hipStream_t)stream, a, ctr);
  return gerr_of(hipGetLastError());
}
#endif  // WANN_DT != 6

// (reached through a function: host code only, and no order of initialisation to depend on)
const GemmUnit &gemm_unit() {
#if WANN_DT == 6
  static constexpr GemmUnit unit = {nullptr, nullptr, unit_gemm_scores, nullptr, nullptr};  // (only ever asked for gemm_scores: dense_prefilter)
#elif WANN_HALF_ROWS || WANN_DT == 8
  static constexpr GemmUnit unit = {unit_point_sums, nullptr, unit_gemm_scores, unit_select_rerank, unit_rerank_cover};
#else
  static constexpr GemmUnit unit = {unit_point_sums, unit_prep_queries, unit_gemm_scores, unit_select_rerank, unit_rerank_cover};
#endif
  return unit;
}
WANN_GNS_END

#if WANN_DT == 0
// ------------------------------------------------------------------------------------------------
// entry points (wann_gemm_device.h) and the launchers of the grouping / cover kernels, which only this unit has
// (the float32 unit's kernels and launchers keep their names outside any dt_* namespace; this is its unit for the lookup)
namespace dt_f32 {
const GemmUnit &gemm_unit() { return wann::gemm_unit(); }
}

static thread_local const char *g_gerr = "";
const char *gemm_launch_last_error() { return g_gerr; }
static int record(const char *err) {
  if (err) g_gerr = err;
  return err ? 1 : 0;
}
// calls the launcher `fn` of the row type's unit and records its error; a type without a dense unit, or whose unit lacks that
// launcher, is an error that names the type -- no other type's kernels stand in
template <typename... P, typename... A>
static int unit_launch(int dtype, const char *(*GemmUnit::*fn)(P...), const char *what, const A &...args) {
  const GemmUnit *u = gemm_unit_of(dtype);
  if (u && u->*fn) return record((u->*fn)(args...));
  static thread_local char text[80];
  snprintf(text, sizeof text, "row type %d has no dense %s launcher", dtype, what);
  return record(text);
}

int launch_point_norms(const IndexView &ix, float *norm2, unsigned int *max_bits, void *stream) { return unit_launch(ix.dtype, &GemmUnit::point_sums, "point_sums", ix, norm2, max_bits, nullptr, stream); }
int launch_point_terms(const IndexView &ix, int32_t *term, void *stream) { return unit_launch(ix.dtype, &GemmUnit::point_sums, "point_sums", ix, nullptr, nullptr, term, stream); }
int launch_split_queries(const float *queries, int64_t nq, int d, int stride, uint32_t *out, void *stream) { return record(gemm_unit().prep_queries(queries, nq, d, stride, out, stream)); }
int launch_pack_queries(const IndexView &ix, const float *queries, int64_t nq, uint32_t *out, void *stream) { return unit_launch(ix.dtype, &GemmUnit::prep_queries, "prep_queries", queries, nq, ix.d, ix.stride, out, stream); }
int launch_gemm_scores(const GemmArgs &a, int num_cus, void *stream) { return unit_launch(a.ix.dtype, &GemmUnit::gemm_scores, "gemm_scores", a, num_cus, stream); }
int launch_select_rerank(const GemmArgs &a, Counters *ctr, void *stream) { return unit_launch(a.ix.dtype, &GemmUnit::select_rerank, "select_rerank", a, ctr, stream); }

int launch_group_windows(const GemmArgs &a, Counters *ctr, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const int cap = a.cap_mask + 1;
  hipLaunchKernelGGL(k_group_clear, dim3((cap + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_group_insert, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_group_plan, dim3(1), dim3(1024), 0, s, a, ctr);
  hipLaunchKernelGGL(k_group_scatter, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, s, a);
  return record(gerr_of(hipGetLastError()));
}

int launch_cover_plan(const CoverArgs &c, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const unsigned qb = (unsigned)((c.g.nq + 255) / 256);
  hipLaunchKernelGGL(k_cover_count, dim3(qb), dim3(256), 0, s, c);
  hipLaunchKernelGGL(k_cover_blocks, dim3(1), dim3(1024), 0, s, c);
  hipLaunchKernelGGL(k_cover_assign, dim3(1), dim3(1024), 0, s, c);
  hipLaunchKernelGGL(k_cover_plan, dim3((unsigned)c.max_passes), dim3(1024), 0, s, c);
  hipLaunchKernelGGL(k_cover_scatter, dim3((unsigned)std::min<int64_t>(2048, (c.g.nq + 3) / 4)), dim3(256), 0, s, c);
  return record(gerr_of(hipGetLastError()));
}

int launch_cover_pass(const CoverArgs &c, int pass, int num_cus, void *stream, const IndexView *score_ix) {
  // the pass's plan, groups, tiles and query lists stand where the score kernels look for a batch's
  GemmArgs a = c.g;
  if (score_ix) a.ix = *score_ix;  // (wann_set_dense_rows: the score kernel reads the one-byte copy, the re-rank the float32 rows)
  a.plan = c.pplan + pass * P_INTS;
  a.groups = c.groups + (int64_t)pass * c.nblocks;
  a.tile_group = c.tile_group + (int64_t)pass * c.tile_stride;
  a.gq = c.gq + (int64_t)pass * c.pair_stride;
  if (launch_gemm_scores(a, num_cus, stream)) return 1;
  CoverArgs cp = c;
  cp.pass = pass;
  return unit_launch(c.g.ix.dtype, &GemmUnit::rerank_cover, "rerank_cover", cp, stream);
}
#endif  // WANN_DT == 0
