/*
 * include/wann.h -- C ABI of the MI355X-native window-filtered ANN engine (libwann.so).
 *
 * This is the drop-in boundary for the ONE hot path of JoshEngels/RangeFilteredANN that this
 * repository accelerates: `batch_search` on the reference's window-search index classes.
 * Plain pointers and sizes only (no torch / pybind11 / STL types); the pybind11 module
 * `window_ann` (rangefilteredann_amd/csrc/window_ann_pybind.cpp) is a thin shim over it and
 * re-exports the reference's Python names.  All file:line citations are into the reference.
 *
 *   wann_index_create        replaces the constructors of
 *       PrefilterIndex<T,Point>                              python_bindings.cpp:111-117, src/prefiltering.h:76-122
 *       PostfilterVamanaIndex<T,Point>                       python_bindings.cpp:129-134, src/postfilter_vamana.h:91-124
 *       RangeFilterTreeIndex<T,Point>                        python_bindings.cpp:119-127, src/range_filter_tree.h:50-59
 *       RangeFilterTreeIndex<T,Point,PostfilterVamanaIndex>  python_bindings.cpp:136-145, src/range_filter_tree.h:50-59,129-189
 *       SuperOptimizedPostfilterTree<..,PostfilterVamanaIndex> python_bindings.cpp:147-157, src/super_optimized_postfilter_tree.h:45-58,118-171
 *   wann_batch_search        replaces <Index>::batch_search
 *       src/range_filter_tree.h:62-96, src/super_optimized_postfilter_tree.h:60-87,
 *       src/postfilter_vamana.h:191-219, src/prefiltering.h:124-146
 *   wann_batch_search_device the same call with queries / ranges / outputs already resident in HBM
 *   wann_batch_search_device_async / wann_wait   that call without blocking: two batches in flight (src/range_filter_tree.h:62-96)
 *   wann_batch_search_device_ids   that call for queries that are not a contiguous range of their batch: per-query own ids
 *       (ParlayANN/algorithms/utils/beamSearch.h:128, src/range_filter_tree.h:71-72; src/postfilter_vamana.h:161-181 for what it is for)
 *   wann_set_refine_rows / wann_batch_search_device_refined / wann_batch_search_refined   (not calls of the reference) a float16 /
 *       bfloat16 / float8 index searched for refine_k >= k candidates that are re-ranked against the caller's float32 rows
 *   wann_batch_search_device_wide / wann_batch_search_wide   (not calls of the reference) rows of `width` columns from the search
 *       that stops as at k: the tail of the frontier that src/postfilter_vamana.h:141-188 returns and batch_search drops
 *   wann_query_params        QueryParams   ParlayANN/algorithms/utils/types.h:115-140, python_bindings.cpp:204-209
 *   wann_build_params        BuildParams   ParlayANN/algorithms/utils/types.h:77-112,  python_bindings.cpp:211-213
 *
 * Error model: functions return 0 on success, non-zero on failure; wann_last_error() gives the
 * message (thread local).  There is NO CPU fallback: every entry point that computes fails with
 * WANN_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef WANN_H
#define WANN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WANN_ABI_VERSION 5
#define WANN_MAX_DEGREE 128

enum { WANN_OK = 0, WANN_ERR_INVALID = 1, WANN_ERR_NO_DEVICE = 2, WANN_ERR_HIP = 3, WANN_ERR_IO = 4,
       WANN_ERR_UNSUPPORTED = 5 };

/* distance: Euclidian_Point (squared L2, euclidian_point.h:62-75) / Mips_Point (-<q,p>, mips_point.h:60-76) */
enum { WANN_METRIC_L2 = 0, WANN_METRIC_MIPS = 1 };
/* element type of points/queries (python_bindings.cpp:232-237): float32 rows, or uint8 / int8 BYTE rows scored with
 * v_dot4 into exact int32 sums (euclidian_point.h:44-60, mips_point.h:44-58), any dimension.
 * WANN_DTYPE_F16 (not a type of the reference): IEEE binary16 points, stored on the device as half rows (half the vector bytes
 * of float32).  Every binary16 value converts to float32 exactly, and the kernels score each row in the float32 path's own
 * arithmetic and order, so a float16 index returns -- ids, distance bits and the reference's operation counters -- what the
 * float32 index of the same kind / metric / parameters returns for the points and queries upcast to float32 (ids of
 * equidistant points in an exact scan may permute, as between the GPU and the reference).  Its graphs are the float32 index's
 * graphs on the upcast points, byte for byte, under the same cache file names: the two share a graph cache.  (A float32 index
 * on the UNROUNDED points gets the same file names but other graphs: keep such caches apart.)  Host-buffer calls take
 * float16 queries; device-buffer calls take fp32 queries (not rounded).  Labels stay float32.  The unfiltered wann_vamana_*
 * API refuses float16.
 * The MFMA prefilter path (PrefilterIndex batches in which queries share windows, counted in gemm_queries) serves every
 * element type and returns the exact scan's rows: float32 rows of up to 512 elements; float16 rows of up to 128 elements (the
 * float32 kernels on the exact upcast, half loads) -- float16 rows of up to 2048 elements in a process started with
 * WANN_DENSE_LONG_ROWS=1 (129 .. 2048: the slab kernel, opt-in), longer float16 rows take the exact scan; uint8 / int8 rows of up to 512
 * bytes on the int8 MFMA with exact int32 scores -- up to 2048 bytes in a process started with WANN_DENSE_LONG_ROWS=1 (a kernel
 * that walks the row in slabs; opt-in until it is timed against the scan) -- longer byte rows take the exact scan.  Queries of
 * a byte index become bytes by the exact scan's rule, (int)q & 0xff, on both paths.
 * HALF-PRECISION SHADOW ROWS of a float32 index.  A WANN_DTYPE_F32 index that has graphs (the post filter, the graph-backed tree,
 * the super tree) and whose n x d values are ALL finite binary16 values -- wann_rows_fp16_exact: half(x) converts back to the bits
 * of x, which keeps -0.0 and the binary16 subnormals and drops NaN, the infinities and |x| > 65504; SIFT / BIGANN vectors, integers
 * in [0, 255], qualify -- keeps a second copy of its points as half rows (64-byte padded, elements paired inside groups of 16 --
 * wann_half_row_position: wann_half_rows_bytes) and its BEAM
 * SEARCHES read that copy through the float16 kernels' arithmetic (a kernel unit of its own for the paired rows): the same rows, distance bits and operation counters (see above), half the
 * vector bytes per scored row.  Everything else -- routing, the exact scans (unless wann_set_scan_rows is on, below), the dense
 * path, the GPU builder, the raw-search hooks, the unfiltered wann_vamana_* API -- reads the float32 rows, which stay where they were.  The property is tested once,
 * when the index is created; an index that is not eligible (or found no memory for the copy) has no shadow and behaves as before.
 * wann_set_half_rows switches the use of the copy off and on between batches (on by default where the copy exists).
 * wann_device_bytes does NOT count the copy (it reports what it always has: a float32 index and the float16 index of the same
 * points differ there by the bytes of their rows); wann_half_rows_bytes does.
 * ONE-BYTE SHADOW ROWS of a float32 index (opt-in).  Where ALL n x d values of such an index are moreover integers 0 .. 255 --
 * wann_rows_u8_exact: (float)(uint8_t)x has the bits of x, so +0.0 only; -0.0, negatives, fractions, 256 and above, NaN and the
 * infinities are refused; SIFT / BIGANN vectors qualify, signed [-128, 127] sets do not -- the index keeps a THIRD copy of its
 * points as uint8 rows (zero padded to a multiple of 64 bytes, elements interleaved inside groups of 32 -- wann_byte_row_position: wann_byte_rows_bytes, a quarter of the float32
 * bytes) beside the float32 rows and the half rows.  After wann_set_byte_rows(index, 1) the BEAM SEARCHES read that copy: each
 * byte is widened to the float32 it was made from and scored against the caller's float32 query in the float32 kernels'
 * arithmetic and order -- the same rows, distance bits and operation counters, queries of any float32 value.  (This is not the
 * WANN_DTYPE_U8 path, whose queries become bytes.)  OFF by default: a batch reads the one-byte rows if that switch is on, else
 * the half rows if theirs is on, else the float32 rows; everything the half rows leave to the float32 rows stays there.
 * wann_device_bytes does not count this copy either.  6, the type of that internal view, is not a WANN_DTYPE_* value and is
 * refused like any unknown dtype.
 * EXACT SCANS FROM THE SHADOW ROWS (opt-in).  After wann_set_scan_rows(index, 1) the exact scans of a batch (k_brute: the tiny
 * windows, the end scans of fenwick / three_split, the scanned queries of wann_set_exact_windows, what the dense path could not
 * prove) read the copy that the same batch's beam searches read -- the one-byte rows if wann_set_byte_rows is on, else the half
 * rows if wann_set_half_rows is on, else the index's own rows -- widened exactly and scored in the float32 scan's arithmetic and
 * order: the same ids, distance bits and operation counters (brute_rows included) with a quarter or half of the row bytes.  OFF
 * by default.  The dense path (exact-window batches included), routing, the finalisation, the GPU builder and the raw hooks keep
 * the float32 rows.
 * DENSE SCORES FROM ONE-BYTE ROWS (opt-in).  After wann_set_dense_rows(index, 1) the SCORE launches of the MFMA prefilter path
 * (k_gemm_scores: shared windows, the cover groups of wann_set_dense_windows, the exact windows of wann_set_exact_windows) read
 * a one-byte copy of the rows instead of the float32 rows: a quarter of the bytes fetched.  An integer 0 .. 255 is exactly one
 * bfloat16 value, so the kernel is the bfloat16 index's (one staged row per point, two products per step) behind a fetch that
 * widens each byte, and its scores are the float32 kernel's.  Only those launches change their source: the point norms, the
 * selection, the proof bound, the exact re-rank and the finalisation read the float32 rows as before -- the same ids, distance
 * bits and dense counters (gemm_queries / gemm_unproven / gemm_rescued, wann_dense_window_counters, wann_exact_window_counters).
 * Which indexes have such a copy: the graph-backed tree and the super tree read their one-byte shadow rows (nothing more is
 * allocated); a WANN_DTYPE_F32 PrefilterIndex whose points pass wann_rows_u8_exact keeps a copy of its own in the same layout
 * (wann_byte_row_position) and the row order of its points -- not a shadow of the kind above: wann_byte_rows_bytes stays 0 and
 * wann_set_byte_rows / wann_set_scan_rows stay refused there.  Rows of up to 128 elements only (the score kernel's narrow
 * class): longer rows have no copy for this path.  The post filter, the prefilter-leaf tree, byte / float16 / bfloat16 indexes
 * and points that are not eligible have none either.  wann_device_bytes does not count the copy.  OFF by default, and
 * independent of wann_set_byte_rows / wann_set_scan_rows.  The contract is for FINITE queries: the float32 score kernels
 * already assume finite scores, and so does this one.
 * WANN_DTYPE_BF16 (not a type of the reference): bfloat16 points, rows of uint16_t bit patterns (the top 16 bits of a float32:
 * float32's exponent range, 8 significant bits).  Everything said of WANN_DTYPE_F16 holds with "bfloat16" for "binary16": the
 * same row pitch and layout (natural order, zero padded to 32 elements), the widening -- one shift, exact for every pattern,
 * subnormals, signed zeros, inf and NaN included, integer instructions only -- followed by the float32 path's own arithmetic, so
 * the float32 index's ids, distance bits and operation counters on the upcast points; the float32 build's graphs and cache
 * file names on the upcast points; bfloat16 bit patterns as host-buffer queries, fp32 device queries (not rounded), float32
 * labels; no wann_vamana_* variant.  Its MFMA prefilter path covers rows of up to 128 elements with a kernel of its own (a
 * bfloat16 row is its own high bf16 term: one staged row per point, two products per step instead of three, the float32
 * kernel's scores on the upcast row); longer rows take the exact scan, with or without WANN_DENSE_LONG_ROWS.  A bfloat16 index
 * has no shadow rows (wann_half_rows: 0).
 * The value is 5: 4 is UNASSIGNED and refused as an unknown dtype, like every other value not listed here.
 * WANN_DTYPE_F8 (not a type of the reference): float8 points, rows of uint8_t bit patterns of OCP E4M3 ("e4m3fn": 1 sign bit, 4
 * exponent bits with bias 7, 3 mantissa bits; no infinities, 0x7f / 0xff are NaN, the largest finite value is 448, subnormals
 * are M * 2^-9) -- a quarter of the float32 vector bytes for REAL-VALUED sets.  Everything said of WANN_DTYPE_BF16 holds with
 * "float8" for "bfloat16", except: (1) the device rows are d bytes zero padded to a multiple of 64, and inside every aligned
 * group of 32 elements the bytes sit in wann_byte_row_position order, the layout of the one-byte shadow rows (host arrays and
 * cache inputs stay in natural order; wann_device_bytes counts n * 64 * ceil(d / 64) for them); (2) the widening is the
 * hardware's two-at-a-time E4M3 -> float32 conversion, exact for all 254 finite patterns whatever the FP mode (every one is a
 * normal float32 value; -0.0 and the subnormals are ordinary values); (3) NaN patterns are REFUSED, not scored:
 * wann_index_create, wann_build_cache_shard and a host-buffer wann_batch_search fail with WANN_ERR_INVALID, the message naming
 * the first offending row, if any point (or host query) element is 0x7f or 0xff, and nothing is written to the cache before
 * that check.  Rounding to float8 (the Python classes, window_ann.float8_bits) is to nearest, ties to even, on the value; a
 * magnitude that rounds above 448 (464 ties down to 448, anything larger does not), an infinity or a NaN becomes the NaN pattern of
 * its sign -- so out-of-range data is an error when the index is created, never silently saturated.  A caller may scale points
 * and queries by a power of two without changing any ordering.  Host-buffer calls take float8 bit patterns as queries,
 * device-buffer calls fp32 queries (not rounded); labels stay float32; no wann_vamana_* variant; wann_raw_beam_search_typed
 * accepts the type.  The MFMA prefilter path covers rows of up to 128 elements (each byte is also exactly one bfloat16 value: the
 * bfloat16 kernel behind a byte fetch, norms and re-rank on the float8 rows); longer rows take the exact scan, with or without
 * WANN_DENSE_LONG_ROWS.  A float8 index has no shadow copies: wann_half_rows, wann_byte_rows and wann_dense_rows are 0 and the
 * four setters return 0 as on any index without a copy.
 * The value is 8: 6 and 7 are INTERNAL view types (the shadow rows above) and stay refused, like 4. */
enum { WANN_DTYPE_F32 = 0, WANN_DTYPE_U8 = 1, WANN_DTYPE_I8 = 2, WANN_DTYPE_F16 = 3, WANN_DTYPE_BF16 = 5, WANN_DTYPE_F8 = 8 };
/* index classes */
enum {
  WANN_KIND_PREFILTER = 0,      /* PrefilterIndex                                   */
  WANN_KIND_POSTFILTER = 1,     /* PostfilterVamanaIndex (one graph, raw point ids)  */
  WANN_KIND_TREE_PREFILTER = 2, /* RangeFilterTreeIndex with PrefilterIndex leaves   */
  WANN_KIND_TREE_VAMANA = 3,    /* VamanaRangeFilterTreeIndex (B-ary window search tree) */
  WANN_KIND_SUPER = 4           /* SuperOptimizedPostfilterTreeIndex                 */
};

typedef struct {
  int64_t k;                      /* QueryParams::k                      */
  int64_t beam_width;             /* QueryParams::beamSize               */
  double cut;                     /* QueryParams::cut (inactive on the post-filter path) */
  int64_t limit;                  /* visit limit                         */
  int64_t degree_limit;
  int64_t final_beam_multiply;
  int64_t postfiltering_max_beam;
  int32_t has_min_query_to_bucket_ratio; /* std::optional<float>::has_value() */
  float min_query_to_bucket_ratio;
  int32_t verbose;                /* the doubling loop of every search is dumped to stdout in the reference's words
                                     (postfilter_vamana.h:155-185,230); such a call runs in the one-wave legacy kernel */
} wann_query_params;

typedef struct {
  int64_t max_degree;     /* R; at most 128 (WANN_MAX_DEGREE).  Up to 64 an adjacency row is one 64-lane load and one pass of the seen
                           * filter per hop (every kernel).  64 < R <= 128 (the reference accepts any R: types.h:77-112,
                           * graph.h:115-124,198): rows of up to 128 ids are worked in two halves per hop by the general core of the
                           * one-wave kernel -- same rows as the reference, lower throughput -- and such graphs are built by the host
                           * builder.  A larger R is refused with WANN_ERR_UNSUPPORTED, never truncated.  Every shipped configuration of
                           * the reference's driver uses R = 64 (run_our_method.py:28). */
  int64_t limit;          /* L (build beam) */
  double alpha;
  const char *cache_path; /* graph cache prefix, "" / NULL = none (postfilter_vamana.h:54-78,126-132) */
} wann_build_params;

/* Work counters of the last batch_search (exact, produced by the kernels). */
typedef struct {
  int64_t beam_searches; /* raw beam searches (all doubling rounds + final re-searches) */
  int64_t hops;          /* adjacency rows expanded (= visited nodes)                   */
  int64_t dist_cmps;     /* vectors scored by graph search                              */
  int64_t brute_rows;    /* vectors scored by brute-force scans                         */
  int64_t label_reads;   /* labels read by the post filter                              */
  int64_t rounds;        /* kernel launches of the beam-search kernel                   */
  int64_t spec_searches; /* searches run speculatively beyond the beam the loop stops at */
  int64_t spec_hops;     /*   (extra work of the concurrent doubling levels; not part of  */
  int64_t spec_dist_cmps;/*   the reference's operation count)                            */
  int64_t gemm_queries;  /* PrefilterIndex queries scored through the MFMA GEMM path        */
  double device_ms;      /* HIP-event time of the whole call on its stream              */
  double search_kernel_ms; /* HIP-event time summed over beam-search kernel launches    */
  int64_t recovered_continuations; /* searches a follow-up launch ran because the companion launch's pollers did not
                                      serve them (launches serialised by the runtime / a profiler); 0 normally     */
  int64_t gemm_unproven; /* of gemm_queries: sent on to the exact scan because the MFMA scores could not prove the top k */
  int64_t gemm_rescued;  /* of gemm_queries: proven after an exact scan of a few 64-position blocks of the window        */
  int64_t deep_handoffs; /* search chains that an idle poller of the companion launch (a CU to itself) took over       */
  int64_t lookaheads_used; /* levels of a chain that a poller had searched ahead by the time the chain needed them   */
  /* ABI 3: the one-wave kernel (long searches: a search wave fed by three scoring helper waves) */
  int64_t big_searches;    /* beam searches that ran there (speculated ones included)                                  */
  int64_t big_hops;        /* their hops                                                                               */
  int64_t packet_hops;     /* of big_hops: adjacency row and distances came from a helper wave's packet                */
  int64_t own_scorings;    /* of big_hops: the search wave had to score at least one neighbour itself                  */
  int64_t prefetched_hops; /* of big_hops: packet and filter probes were fetched during the previous hop               */
  int64_t poll_timeouts;   /* pollers of the companion launch that gave up waiting (serialised launches)               */
  int64_t lookaheads_issued; /* look-ahead searches handed to waiting pollers (lookaheads_used of them were needed)    */
} wann_counters;

typedef struct wann_index wann_index;

int wann_abi_version(void);
const char *wann_last_error(void);
/* number of usable gfx950 devices (0 when none); never initialises a context */
int wann_device_count(void);

/* Build (or load from the graph cache) an index and make it resident in the HBM of `device`.
 * points: (n,d) row-major of `dtype` (uint8 / int8 sets stay bytes on the device); labels: (n) float32.  cutoff / split_factor /
 * shift_factor as in the reference constructors (ignored by kinds that have none).
 * build_threads <= 0: PARLAY_NUM_THREADS if set, else all host cores. */
wann_index *wann_index_create(int kind, int metric, int dtype, const void *points, int64_t n,
                              int64_t d, const float *labels, int32_t cutoff, double split_factor,
                              double shift_factor, const wann_build_params *bp, int device,
                              int build_threads);
void wann_index_destroy(wann_index *index);

/* Host-buffer call (the reference's boundary: numpy in, numpy out).  queries: (nq,d) of the index's dtype.  ranges = nq x 2 float32
 * (lo, hi), bounds inclusive (range_filter_tree.h:61).  method: "optimized_postfilter",
 * "three_split", anything else = fenwick (range_filter_tree.h:76-82); ignored by non-tree kinds.
 * ids: nq x k uint32, dists: nq x k float32, caller allocated. */
int wann_batch_search(wann_index *index, const void *queries, const float *ranges, int64_t nq,
                      const char *method, const wann_query_params *qp, uint32_t *ids, float *dists);

/* Device-buffer call: same semantics, every pointer is device memory on the index's device (queries are fp32
 * rows also for uint8 / int8 indexes);
 * `query_id_base` is the global row number of queries[0] (the reference uses the query's row
 * number as its "own id", beamSearch.h:128 + range_filter_tree.h:71-72, so a query shard must
 * keep its global numbering).  Runs on `hip_stream` (a hipStream_t; NULL = the HIP default stream,
 * i.e. ordered after the work the caller queued there) and returns after the stream work is
 * complete.  With a non-blocking stream the caller must make sure that the inputs are complete and
 * that no work still pending on another stream uses the output buffers' memory. */
int wann_batch_search_device(wann_index *index, const void *d_queries, const float *d_ranges,
                             int64_t nq, int64_t query_id_base, const char *method,
                             const wann_query_params *qp, uint32_t *d_ids, float *d_dists,
                             void *hip_stream);

/* wann_batch_search_device for queries that do NOT form a contiguous range of their batch (ABI 5): `d_query_ids[i]` (device array of
 * nq int64) is the global row number of queries[i] -- its "own id" (beamSearch.h:128 + range_filter_tree.h:71-72: the reference never
 * scores the neighbour whose number equals the query's row number).  What a scheduler needs that deals single doubling LEVELS of a
 * query's chain to different GPUs (rangefilteredann_amd/distributed.py level_dealt_batch_search; postfilter_vamana.h:161-172: every
 * level restarts from scratch).  Otherwise as wann_batch_search_device. */
int wann_batch_search_device_ids(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq,
                                 const int64_t *d_query_ids, const char *method, const wann_query_params *qp,
                                 uint32_t *d_ids, float *d_dists, void *hip_stream);

/* Asynchronous form of wann_batch_search_device (ABI 4).  The reference's call is blocking (src/range_filter_tree.h:62-96: it
 * returns when every query is answered) and so are the two calls above; a serving loop that answers batch after batch leaves
 * the GPU to the tail of one batch and the ramp-up of the next about a fifth of the time at 10 000 queries per batch.  This call
 * returns at once with a ticket: the batch runs on one of the LANES of the index (two; the environment variable WANN_ASYNC_LANES,
 * 1 .. 4, read when the first asynchronous call creates them, sets another depth; a lane = its own per-batch workspace, streams
 * and host worker thread), ordered after the work the caller has queued on `after_stream` so far (its inputs; NULL = the HIP
 * default stream), and concurrently with the other lane's batch.  Same rows as the blocking call.  The output buffers belong
 * to the call until wann_wait(ticket) has returned; wait for ticket t before submitting ticket t + <lanes> (its lane is reused).
 * wann_wait returns the batch's status (message in wann_last_error) and, if `counters` is not NULL, its work counters. */
int wann_batch_search_device_async(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq,
                                   int64_t query_id_base, const char *method, const wann_query_params *qp, uint32_t *d_ids,
                                   float *d_dists, void *after_stream, int64_t *ticket);
int wann_wait(wann_index *index, int64_t ticket, wann_counters *counters);

/* Predicted work of every query of a batch, in beam-search hops (cost[nq], host; ranges: nq x 2 float32, host): the batch is
 * routed like wann_batch_search routes it (src/range_filter_tree.h:403-471) and every query's tasks are priced with the doubling
 * loop of src/postfilter_vamana.h:161-181 under "a beam finds k entries once it is expected to hold k in-window points".  What a
 * strong-scaling shard cut balances: contiguous shards of equal predicted work instead of equal query counts. */
int wann_predict_costs(wann_index *index, const float *ranges, int64_t nq, const char *method, const wann_query_params *qp,
                       float *cost);

int wann_get_counters(const wann_index *index, wann_counters *out);

/* Distinct wide windows of a PrefilterIndex batch on the matrix cores (opt-in; off when an index is created).  The dense
 * prefilter path takes a batch's queries that SHARE a window (gemm_queries).  With this option on, the queries it left over whose
 * window holds at least 1 024 points are grouped by 2 048-position block of the label order instead -- a COVER GROUP is one block
 * and the queries whose window touches it, provided at least 32 such queries touch every block of a query's window and the batch's
 * eligible windows hold at least 2 GiB of rows in all (smaller batches are faster on the scan) -- and scored
 * by the same kernels; candidates outside a query's own window are dropped before the exact re-rank.  Rows are those of the
 * exact scan (same ids, same distance bits: both order by (distance, id)); only the work counters differ: brute_rows no longer
 * counts the rows of the queries taken.  Row lengths the dense path does not take (float16 above 128 elements, bytes above 512 --
 * above 2048 elements or bytes where WANN_DENSE_LONG_ROWS=1 opts in to the long-row kernels) and k > 16 stay on the exact scan.  Applies to every replica of WANN_DEVICES and to every call form.
 * Returns the previous setting (0 / 1) or a NEGATIVE error: -WANN_ERR_UNSUPPORTED for on = 1 on any kind but
 * WANN_KIND_PREFILTER, -WANN_ERR_INVALID for a null index. */
int wann_set_dense_windows(wann_index *index, int on);
/* Cover-path counters of the last batch (all zero with the option off; gemm_queries / gemm_unproven / gemm_rescued of
 * wann_counters keep counting shared-window groups only). */
typedef struct {
  int64_t queries;        /* queries taken by the cover path                                                     */
  int64_t unproven;       /* of those: sent on to the exact scan because the scores could not prove the top k    */
  int64_t rescued;        /* of those: proven after an exact scan of a few 64-position blocks                    */
  int64_t groups;         /* cover groups (position block x its query list), summed over the passes              */
  int64_t tiles;          /* tiles (cover group x 128 queries)                                                   */
  int64_t passes;         /* passes over query ranges (the hand-over of one pass fits the 256-MiB score buffer)  */
  int64_t handover_bytes; /* bytes reserved for the score kernels' hand-over to the selection, summed over the passes */
} wann_dense_window_counters;
int wann_get_dense_window_counters(const wann_index *index, wann_dense_window_counters *out);

/* Exact answers for small windows of the graph-backed tree indexes (opt-in; 0 = off, the state of a new index).  With a limit
 * L > 0 a query whose window [istart, eend) of the label order holds 0 < w <= L points is ONE exact task over those positions,
 * whatever the query method: its row is what the reference's brute-force branch returns for that window -- the k nearest
 * in-window points, distances in the exact scan's fp32 order, ordered by (distance, sorted position), ids through `decoding`,
 * the class's own padding when w < k -- instead of the rows of the doubling graph search (so the reference's rows are no longer
 * what such a query returns).  The rule is tested once, on the query's whole window, before three_split / fenwick decompose it
 * and before the super tree scans its levels.  Queries with w > L, empty windows and windows outside the label span take the
 * ordinary path and return the ordinary rows bit for bit.  In a batch of at least 32 queries the flagged queries take the dense
 * prefilter path (shared-window groups and cover groups on the matrix cores, under its usual gates: windows of >= 1 024
 * points, >= 32 queries per block, 2 GiB of eligible rows per batch, k <= 16, the row-length limits per element type); what it
 * does not take or cannot prove goes to the exact scan, and both return the same rows bit for bit.  The scans and the dense
 * launches run beside the graph searches of the same batch.  While the limit is non-zero a batch holds the index's dense
 * buffers: the asynchronous lanes then run one batch at a time.  A call with wann_query_params::verbose set ignores the option
 * (its purpose is the reference's trace), and so does wann_predict_costs.  Applies to every replica of WANN_DEVICES and to every
 * call form.  Returns the previous limit or a NEGATIVE error: -WANN_ERR_INVALID for a null index or a negative limit,
 * -WANN_ERR_UNSUPPORTED for any kind but WANN_KIND_TREE_VAMANA and WANN_KIND_SUPER (the stand-alone post filter has no sorted
 * labels; PrefilterIndex and the prefilter-leaf tree are exact already). */
int64_t wann_set_exact_windows(wann_index *index, int64_t max_points);
/* Exact-window counters of the last batch (all zero with the option off). */
typedef struct {
  int64_t queries;       /* queries answered exactly because of the option                                   */
  int64_t dense_queries; /* of those: taken by the matrix-core path (shared-window groups + cover groups)    */
  int64_t unproven;      /* of dense_queries: sent on to the exact scan because the scores could not prove the top k */
  int64_t rescued;       /* of dense_queries: proven after an exact scan of a few 64-position blocks         */
  int64_t passes;        /* cover passes over query ranges                                                   */
  int64_t rows_scanned;  /* rows the exact scan scored for `queries`                                         */
} wann_exact_window_counters;
int wann_get_exact_window_counters(const wann_index *index, wann_exact_window_counters *out);

/* Introspection (tests, tools). */
int64_t wann_num_points(const wann_index *index);
int64_t wann_dim(const wann_index *index);
int64_t wann_num_levels(const wann_index *index);
int64_t wann_level_size(const wann_index *index, int64_t level);
int wann_partition_range(const wann_index *index, int64_t level, int64_t idx, int64_t *start, int64_t *end);
/* copy partition graph out in the reference's in-memory layout: n x (R+1) int32, slot 0 = degree.  `rows` holds
 * cap_rows x (max_degree+1) ints; max_degree must equal the index's R (wann_max_degree), cap_rows >= partition size. */
int wann_partition_graph(const wann_index *index, int64_t level, int64_t idx, int32_t *rows, int64_t cap_rows,
                         int64_t max_degree);
int64_t wann_max_degree(const wann_index *index);
int64_t wann_device_bytes(const wann_index *index);  /* (without the shadow rows: wann_half_rows_bytes, wann_byte_rows_bytes) */

/* Half-precision shadow rows (see WANN_DTYPE_*).
 * wann_rows_fp16_exact: 1 if every one of the n x d float32 values (row-major, contiguous) is a finite IEEE binary16 value, else 0;
 * 1 for an empty set.  Pure host code: needs no device.
 * wann_set_half_rows: whether the beam searches of the NEXT batches read the shadow rows (a batch submitted earlier keeps what it
 * was submitted with).  Returns the setting now in force, 0 / 1: asking for 1 on an index without a shadow leaves it at 0 and
 * returns 0.  Allocates and frees nothing; applies to every replica of WANN_DEVICES; a NEGATIVE error for a null index.
 * wann_half_rows: that setting.  wann_half_rows_bytes: device bytes of the shadow rows, n * 64 * ceil(2 d / 64), or 0 without one.
 * wann_last_half_rows: 1 if the beam searches of the last finished batch -- the last blocking call, or the ticket last waited
 * for -- read the shadow rows (wann_counters keeps its ABI 5 layout, so this is a call of its own).
 * wann_half_row_position: the LAYOUT of the device copy, as a pure function (no device, no index): the position, counted in
 * halves, inside a half shadow row at which element `element` of the row is stored,
 *     16 (e >> 4) + 8 ((e >> 2) & 1) + 4 ((e >> 3) & 1) + (e & 3)
 * -- a permutation inside every aligned group of 16 elements that lets a lane of the search kernels fetch two of its 4-element
 * blocks with one 16-byte load; -1 for a negative argument.  The row pitch and wann_half_rows_bytes do not depend on it, and
 * float16 / bfloat16 indexes keep the natural order. */
int wann_rows_fp16_exact(const float *rows, int64_t n, int64_t d);
int64_t wann_half_row_position(int64_t element);
int wann_set_half_rows(wann_index *index, int on);
int wann_half_rows(const wann_index *index);
int64_t wann_half_rows_bytes(const wann_index *index);
int wann_last_half_rows(const wann_index *index);
/* One-byte shadow rows (see WANN_DTYPE_*), the same five calls.
 * wann_rows_u8_exact: 1 if every one of the n x d float32 values (row-major, contiguous) is an integer 0 .. 255 with the bits of
 * (float)(uint8_t)x, else 0; 1 for an empty set.  Pure host code: needs no device.
 * wann_set_byte_rows: whether the beam searches of the NEXT batches read the one-byte rows (a batch submitted earlier keeps what
 * it was submitted with).  Returns the setting now in force, 0 / 1: asking for 1 on an index without the copy leaves it at 0 and
 * returns 0.  Allocates and frees nothing; applies to every replica of WANN_DEVICES; a NEGATIVE error for a null index.  The
 * setting of wann_set_half_rows is kept and counts again once this one is off.
 * wann_byte_rows: that setting (0 after wann_index_create).  wann_byte_rows_bytes: device bytes of the copy,
 * n * 64 * ceil(d / 64), or 0 without one.
 * wann_last_byte_rows: 1 if the beam searches of the last finished batch read the one-byte rows; wann_last_half_rows is then 0
 * (it keeps its meaning: 1 only when the half rows were read).
 * wann_byte_row_position: the LAYOUT of the device copy, as a pure function (no device, no index): the byte position inside a
 * one-byte shadow row at which element `element` of the row is stored,
 *     32 (e >> 5) + 16 ((e >> 2) & 1) + 4 ((e >> 3) & 3) + (e & 3)
 * -- a permutation inside every aligned group of 32 elements that lets a lane of the search kernels fetch four of its 4-element
 * blocks with one 16-byte load; -1 for a negative argument.  The row pitch and wann_byte_rows_bytes do not depend on it. */
int wann_rows_u8_exact(const float *rows, int64_t n, int64_t d);
int64_t wann_byte_row_position(int64_t element);
int wann_set_byte_rows(wann_index *index, int on);
int wann_byte_rows(const wann_index *index);
int64_t wann_byte_rows_bytes(const wann_index *index);
int wann_last_byte_rows(const wann_index *index);
/* Exact scans from the shadow rows (see WANN_DTYPE_*).
 * wann_set_scan_rows: whether the exact scans of the NEXT batches read the shadow copy that the same batch's beam searches read
 * (a batch submitted earlier keeps what it was submitted with, the asynchronous lanes included).  Returns the setting now in
 * force, 0 / 1: asking for 1 on an index that has no shadow copy at all (a PrefilterIndex, the prefilter-leaf tree, points that
 * are not eligible, byte / float16 / bfloat16 indexes) leaves it at 0 and returns 0.  Allocates and frees nothing; applies to
 * every replica of WANN_DEVICES; a NEGATIVE error for a null index.
 * wann_scan_rows: that setting (0 after wann_index_create).
 * wann_last_scan_rows: which rows the exact-scan launch of the last finished batch read -- 0 the index's own rows, 1 the half
 * rows, 2 the one-byte rows; 0 when the batch launched no scan. */
int wann_set_scan_rows(wann_index *index, int on);
int wann_scan_rows(const wann_index *index);
int wann_last_scan_rows(const wann_index *index);
/* Dense scores from one-byte rows (see WANN_DTYPE_*).
 * wann_set_dense_rows: whether the score launches of the dense path of the NEXT batches read the one-byte copy of the rows (a
 * batch submitted earlier keeps what it was submitted with, the asynchronous lanes included).  Returns the setting now in
 * force, 0 / 1: asking for 1 on an index without a copy this path can read (see above) leaves it at 0 and returns 0.  Allocates
 * and frees nothing; applies to every replica of WANN_DEVICES; a NEGATIVE error for a null index.  Independent of
 * wann_set_byte_rows and wann_set_scan_rows.
 * wann_dense_rows: that setting (0 after wann_index_create).
 * wann_dense_rows_bytes: device bytes of the copy the dense path would read, n * 64 * ceil(d / 64) -- on a tree index the bytes
 * wann_byte_rows_bytes reports, the same buffer -- or 0 without one; -1 for a null index.
 * wann_last_dense_rows: 1 if a score launch of the last finished batch read the copy; 0 for a batch whose dense path scored no
 * query (or launched nothing). */
int wann_set_dense_rows(wann_index *index, int on);
int wann_dense_rows(const wann_index *index);
int64_t wann_dense_rows_bytes(const wann_index *index);
int wann_last_dense_rows(const wann_index *index);

/* WIDE ROWS: stop as at k, keep up to `width` entries (not calls of the reference; it computes this and drops the tail).
 * The reference's query() (src/postfilter_vamana.h:141-188) returns the whole filtered frontier of the last beam it searched;
 * knn appears in its stop test `frontier.size() < knn` and in batch_search's copy of the first knn entries, nowhere else.  An
 * ordinary call uses one number, qp->k, for three things; a wide call separates them:
 *   k       what the caller gets back,
 *   stop_k  the doubling loop ends at the first level with >= stop_k in-window entries,
 *   width   the columns of the search's row.
 * wann_batch_search_device_wide has k = width and stop_k = qp->k; every other entry point has k == stop_k == width.  Semantics:
 *   - Every graph search of the call runs the reference's loop with knn = stop_k: the doubling, the speculated levels, the final
 *     re-search by final_beam_multiply and the postfiltering_max_beam end.
 *   - The call keeps the first `width` in-window entries of the frontier that loop returns.  Pads follow, as today.
 *   - Exact scans keep the best `width`: tiny windows, PrefilterIndex, prefilter leaves, the ends of fenwick / three_split and
 *     wann_set_exact_windows scans.
 *   - Merges (k_finalize_multi) keep `width`.
 *   - Consequently the first stop_k columns are the ordinary call's row at k = stop_k.
 *   - beam_searches, hops and dist_cmps equal that call's counters.  (They count the graph searches.  What goes by the row's
 *     columns follows `width`: label_reads -- a level's beam is filtered until `width` entries are kept -- and the dense path,
 *     which takes rows of at most 16 columns: exact windows (wann_set_exact_windows) and PrefilterIndex windows that the call at
 *     k = stop_k scores on the matrix cores may be scanned by a wide call, as by the ordinary call at k = width -- the same
 *     rows either way, gemm_* counters as that call's.  Which windows are exact does not depend on any k.)
 * wann_batch_search_device_wide: wann_batch_search_device's arguments and `width`; d_ids / d_dists are nq x width.  It requires
 * 1 <= qp->k <= width <= 1024 (WANN_ERR_INVALID otherwise) and refuses qp->verbose with WANN_ERR_UNSUPPORTED when width != qp->k:
 * the printed words name one k.  Nothing is launched by a refused call.  Any element type and any index kind; on kinds with no
 * graph search it equals the ordinary call at k = width.  width == qp->k is the ordinary call.
 * wann_batch_search_wide: the host-buffer form, queries as wann_batch_search takes them (the index dtype's bit patterns); ids /
 * dists: nq x width, host.
 * Primary device only and blocking only: no asynchronous, all-gather or WANN_DEVICES-replica form.  A NULL index is answered
 * with the NEGATIVE code -WANN_ERR_INVALID. */
int wann_batch_search_device_wide(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq, int64_t query_id_base,
                                  const char *method, const wann_query_params *qp, int64_t width, uint32_t *d_ids, float *d_dists,
                                  void *hip_stream);
int wann_batch_search_wide(wann_index *index, const void *queries, const float *ranges, int64_t nq, const char *method,
                           const wann_query_params *qp, int64_t width, uint32_t *ids, float *dists);

/* REFINED SEARCH: re-rank a compact index's candidates against full-precision rows.  A WANN_DTYPE_F16 / BF16 / F8 index answers
 * for the ROUNDED points.  A caller who still has the float32 points gives them to the index as a ROW STORE; a refined call then
 * searches the compact rows for refine_k >= k candidates (a half or a quarter of the float32 bytes per scored row), scores
 * those candidates against the store's rows and returns the best k.  This saves bandwidth, NOT capacity: the float32 rows sit
 * in HBM beside the compact index.
 *
 * wann_set_refine_rows: `points` is the host array of full-precision points, (n, d) row-major float32, IN THE CALLER'S POINT
 * ORDER -- the order of the array the index was created from, which is the order of the ids every kind returns (decoded ids of
 * the sorted kinds, raw ids of the post filter): the store is indexed by returned id and knows nothing of the label sort.  The
 * device copy has its rows zero padded to a multiple of 16 floats, the float32 index's row pitch.  points == NULL drops the store
 * (n and d are then ignored).  A second call replaces the store.  WANN_ERR_INVALID, with a message: a null index, n or d not
 * the index's, or a non-finite element (the message names the first offending row; the store in place is kept).
 * WANN_ERR_UNSUPPORTED: an index of any other element type -- float32 has nothing to refine, and a uint8 / int8 search turns
 * the query into bytes, so one fp32 query cannot serve both spaces.  The rows are NOT compared with the index's rounded points:
 * a caller who scaled points and queries by a power of two to fit float8 passes the scaled originals, and distances are
 * reported in the space of the queries.  With WANN_DEVICES the store lives on the primary, which the refined calls serve.
 * wann_refine_rows_bytes: device bytes of the store, n * 4 * 16 * ceil(d / 16); 0 without one, -1 for a null index.
 * wann_device_bytes does not count the store (as it does not count the shadow copies).
 *
 * wann_batch_search_device_refined: wann_batch_search_device's semantics -- fp32 device queries (not rounded), device ranges,
 * d_ids / d_dists of nq x qp->k, `hip_stream`, blocking -- with this result.  Let C(q) be the row the ordinary call returns for
 * query q with k = refine_k and everything else of `qp` unchanged.
 *   - The candidates are the entries of C(q) before its first pad; a pad is an entry with dist == FLT_MAX and id == the kind's
 *     padding id (0 for the sorted kinds, 2^32-1 for the post filter and the PrefilterIndex), and pads are always a suffix.
 *   - Each candidate id gets the distance of (store row id, q) in the FLOAT32 INDEX'S arithmetic and evaluation order: the bits a
 *     WANN_DTYPE_F32 index of those rows returns for that pair (the kernel calls the float32 row-distance routines themselves).
 *   - The result is the first qp->k candidates under the key (refined distance, id), the exact scan's order, followed by pads
 *     (padding id, FLT_MAX).
 *   - An id the search returned twice (fenwick and three_split can) is a candidate twice and may be returned twice: duplicates
 *     are kept, as everywhere else.
 *   - No address is ever made from a pad's id.
 * It needs a store and qp->k <= refine_k <= 1024, and whatever the ordinary call demands of k holds for refine_k; otherwise
 * WANN_ERR_INVALID.  If the re-rank kernel's LDS need for this (d, k) -- the staged query row and the k-entry list, per wave --
 * exceeds a workgroup's 160 KiB the call returns WANN_ERR_UNSUPPORTED before anything is launched; it never truncates.  The
 * search itself is the ordinary call's at k = refine_k, untouched: afterwards wann_get_counters reports that search (every
 * operation counter equals the ordinary call's at k = refine_k).
 * wann_batch_search_refined: the host-buffer form.  `queries` is (nq, d) FLOAT32 -- unlike wann_batch_search, which takes the
 * index dtype's bit patterns and so searches with rounded queries; here the fp32 queries are uploaded as they are and go
 * through the device path.  ids / dists: nq x qp->k, host.  Serves the primary.
 * wann_batch_search_device_refined_stop / wann_batch_search_refined_stop: the refined calls with one more argument, stop_k,
 * qp->k <= stop_k <= refine_k (WANN_ERR_INVALID otherwise).  C(q) is then the WIDE row (above) at (stop_k, width = refine_k): the
 * search stops as the ordinary call at k = stop_k does and the re-rank sees up to refine_k entries of that same frontier, so the
 * candidates cost the search at stop_k, not the one at refine_k.  Afterwards wann_get_counters reports that search:
 * beam_searches, hops and dist_cmps equal the ordinary call's at k = stop_k.  The functions without the argument are the case
 * stop_k = refine_k.  qp->verbose with stop_k != refine_k: WANN_ERR_UNSUPPORTED, nothing launched.
 * wann_get_refine_counters: the last refined call's re-rank -- queries, candidates scored (pads excluded) and the HIP-event
 * time of the re-rank launch alone (wann_counters::device_ms stays the search's).
 * There is no asynchronous form and no all-gather form, and no environment switch: refinement happens where it is called.
 * Return values: 0, or a WANN_ERR_* code as above; a NULL index is answered with the NEGATIVE code -WANN_ERR_INVALID by the
 * setter, both searches and the counters' getter (as by the setters of the shadow rows), and with -1 by wann_refine_rows_bytes. */
typedef struct {
  int64_t refined_queries; /* queries of the last refined call                              */
  int64_t refined_rows;    /* candidates scored against the store (pads excluded)           */
  double refine_ms;        /* HIP-event time of the re-rank launch alone                    */
} wann_refine_counters;
int wann_set_refine_rows(wann_index *index, const float *points, int64_t n, int64_t d);
int64_t wann_refine_rows_bytes(const wann_index *index);
int wann_batch_search_device_refined(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq,
                                     int64_t query_id_base, const char *method, const wann_query_params *qp, int64_t refine_k,
                                     uint32_t *d_ids, float *d_dists, void *hip_stream);
int wann_batch_search_refined(wann_index *index, const float *queries, const float *ranges, int64_t nq, const char *method,
                              const wann_query_params *qp, int64_t refine_k, uint32_t *ids, float *dists);
int wann_batch_search_device_refined_stop(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq,
                                          int64_t query_id_base, const char *method, const wann_query_params *qp, int64_t refine_k,
                                          int64_t stop_k, uint32_t *d_ids, float *d_dists, void *hip_stream);
int wann_batch_search_refined_stop(wann_index *index, const float *queries, const float *ranges, int64_t nq, const char *method,
                                   const wann_query_params *qp, int64_t refine_k, int64_t stop_k, uint32_t *ids, float *dists);
int wann_get_refine_counters(const wann_index *index, wann_refine_counters *out);

/* In-process multi-device mode: with WANN_DEVICES=a,b,... in the environment wann_index_create makes the index resident on
 * every listed device (a device may be listed twice) and wann_batch_search -- the host-buffer call, the reference's boundary
 * (src/range_filter_tree.h:62-96: one call parallelises over all queries) -- cuts its batch into contiguous shards, one host
 * thread + stream per replica; queries keep their global row numbers.  wann_batch_search_device serves the primary only.
 * Returns the number of replicas (1 without WANN_DEVICES). */
int wann_num_replicas(const wann_index *index);

/* The multi-device call with DEVICE-RESIDENT gathered rows (ABI 4), for a host that keeps working on the GPUs: every replica of
 * WANN_DEVICES (distinct devices: one RCCL rank each) searches its contiguous shard -- wann_gather_layout gives shard s's first
 * row, row count and the common capacity cap = ceil(nq / replicas) -- and ONE ncclAllGather over RCCL / xGMI leaves, on EVERY
 * replica's device, the planes of all shards:   d_planes[r] -> int32 [replicas][2][cap][k]   (device memory of replica r, owned
 * by the index, valid until its next call): plane [s][0] = ids (uint32) of shard s's rows, plane [s][1] = their distances
 * (float32 bits); rows beyond a shard's count are the reference's padding (id 0, FLT_MAX).  Global query q of shard s sits at
 * row q - lo_s.  queries / ranges: host buffers like wann_batch_search.  librccl.so is opened at the first call (dlopen). */
int wann_gather_layout(int64_t nq, int world, int shard, int64_t *lo, int64_t *count, int64_t *cap);
int wann_batch_search_allgather(wann_index *index, const void *queries, const float *ranges, int64_t nq, const char *method,
                                const wann_query_params *qp, int32_t **d_planes, int64_t *cap);

/* Graph-cache tool: build (host, multi-threaded) and save only the cache files of the
 * partitions p with p % nshards == shard, without creating a device index.  Used to split the
 * build of one index over the ranks of a multi-GPU job that share a cache directory. */
int wann_build_cache_shard(int kind, int metric, int dtype, const void *points, int64_t n, int64_t d,
                           const float *labels, int32_t cutoff, double split_factor,
                           double shift_factor, const wann_build_params *bp, int shard, int nshards,
                           int build_threads);

/* Raw kernels, exported for parity tests and micro-benchmarks (device pointers). */
/* one beam search per query over ONE graph given in the reference's layout (host pointers;
 * the call uploads, runs the production kernel and downloads). */
int wann_raw_beam_search(int metric, const float *points, int64_t n, int64_t d,
                         const int32_t *graph_rows /* n x (maxdeg+1) */, int64_t maxdeg,
                         int64_t subset_start, int64_t subset_n, const float *queries, int64_t nq,
                         const int64_t *query_ids, int64_t beam, int64_t limit,
                         int64_t degree_limit, int32_t *out_ids /* nq x beam */,
                         float *out_dists /* nq x beam */, int32_t *out_sizes /* nq */,
                         int64_t *out_hops /* nq */, int64_t *out_dist_cmps /* nq */, int device);
/* the same over points of any element type (`dtype`: WANN_DTYPE_*, rows as wann_index_create takes them); queries stay fp32 */
int wann_raw_beam_search_typed(int metric, int dtype, const void *points, int64_t n, int64_t d,
                               const int32_t *graph_rows /* n x (maxdeg+1) */, int64_t maxdeg,
                               int64_t subset_start, int64_t subset_n, const float *queries, int64_t nq,
                               const int64_t *query_ids, int64_t beam, int64_t limit,
                               int64_t degree_limit, int32_t *out_ids /* nq x beam */,
                               float *out_dists /* nq x beam */, int32_t *out_sizes /* nq */,
                               int64_t *out_hops /* nq */, int64_t *out_dist_cmps /* nq */, int device);

/* Unfiltered VamanaIndex<T,Point> (ParlayANN/python/vamana_index.cpp:42-76, bound at python_bindings.cpp:92-109): a graph
 * index opened from a point file (uint32 n, uint32 d, n*d elements of dtype: point_range.h:63-93) and a graph file
 * (graph.h:126-196: the format of the graph cache).  batch_search = beam_search from node 0 with
 * QueryParams(knn, beam_width, 1.35, n, max_degree) -- including the k / cut step of beamSearch.h:159-167, which only this
 * path takes (it lives in the first-generation core of the one-wave legacy kernel, k_search<., 2>: same rows as the reference, a
 * fraction of the filtered path's throughput) -- and the first knn entries of the final beam (a shorter beam is padded with id
 * 2^32-1, FLT_MAX; the reference reads past it).  queries: host (nq,d) of the index's dtype. */
typedef struct wann_vamana wann_vamana;
wann_vamana *wann_vamana_open(int metric, int dtype, const char *data_path, const char *graph_path, int device);
void wann_vamana_close(wann_vamana *index);
int64_t wann_vamana_num_points(const wann_vamana *index);
int64_t wann_vamana_dim(const wann_vamana *index);
int wann_vamana_batch_search(wann_vamana *index, const void *queries, int64_t nq, int64_t knn, int64_t beam_width,
                             uint32_t *ids, float *dists);
/* build_vamana_index (ParlayANN/python/builder.cpp:33-59, bound at python_bindings.cpp:93-95): point file -> graph file,
 * built on the GPU with the reference's insertion order */
int wann_vamana_build_file(int metric, int dtype, const char *data_path, const char *graph_out_path, int64_t max_degree,
                           int64_t limit, double alpha, int device);

#ifdef __cplusplus
}
#endif
#endif /* WANN_H */
