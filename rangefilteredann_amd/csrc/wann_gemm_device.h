// wann_gemm_device.h -- argument block of the dense prefilter path (wann_gemm_kernels_body.inc).
#pragma once
#include <stdint.h>

#include "wann_device.h"

namespace wann {

constexpr int kSelect = 32;      // candidates kept per query by MFMA score before the exact re-rank
constexpr int kGemmPointChunk = 2048;  // window positions per tile (multiple of 128)
constexpr int kGemmMaxFloats = 2048;   // longest float32 / float16 row, in 32-bit words of the float32 row (dense_row_class only)
constexpr int kGemmMaxBytes = 2048;    // longest padded uint8 / int8 row, in bytes (dense_row_class only)
// (a window hands over three candidates per 64 positions: too short a window could never prove a top 10)
constexpr int kGroupMinQueries = 16, kGroupMinWindow = 1024;
// cover groups (distinct windows, wann_set_dense_windows): a query is eligible if its window has at least kCoverMinWindow
// positions and every kGemmPointChunk-position block it touches is touched by at least kCoverMinQueries such queries
// (measured crossover, tools/bench_windows.py --sweep, DESIGN.md 3.5: at 16 queries per block the eighth-filled tiles and the
// queries left ineligible lose against the scan at every batch size below 10 000; the window width itself does not decide --
// the batch's total scan work does, CoverArgs::min_rows)
constexpr int kCoverMinQueries = 32, kCoverMinWindow = 1024;
constexpr long long kCoverMinScanBytes = 1ll << 31;  // eligible windows' rows x bytes per row below which the scan is faster than the cover path's ~0.2 ms of launches
constexpr int kCoverPairFloats = (kGemmPointChunk / 128) * 8;  // hand-over of one (query, block) pair: 16 steps x 2 half waves x 4 floats

struct GemmGroup {   // queries sharing the window [a, b) of the label argsort
  int64_t a, b;
  int64_t soff;      // offset (floats) of the group's block entries [qcount][steps of 128 positions][2][4] in `scores`
  int32_t qoff;      // the group's query rows are gq[qoff .. qoff + qcount)
  int32_t qcount;
  int32_t tile0;     // the group's tiles are tile0 .. tile0 + nqt * nch - 1: tile = tile0 + ch * nqt + qt
  int32_t nqt, nch;  // 128-query tiles x kGemmPointChunk-position slices
  int32_t pad;
};

// device-side plan of one batch (k_group_*): counts written by the device, read by the kernels that follow
enum { P_NGROUPS = 0, P_NTQ = 1, P_NTILES = 2, P_NSLOTS = 3, P_ANY = 4 /* some slot has enough queries and a long enough window */, P_INTS = 5 };

struct GemmArgs {
  IndexView ix;
  const float *queries;
  const Task *tasks;
  int64_t nq;
  // Query q's task is tasks[q * tstride] (its slot 0): 1 for a PrefilterIndex.  The sorted kinds (wann_set_exact_windows) run
  // with the index's task stride; only slots that hold an exact-window task are taken (dense_task).
  int32_t tstride;
  // Sorted kinds: the exact scan's list also holds tasks that are none of the dense path's business (end scans of fenwick /
  // three_split, the reference's tiny windows), so the list is APPENDED to, never rebuilt (list_keep), and the queries the
  // window grouping leaves over are listed by exactly one stage: k_group_scatter (scatter_lists) or the cover stage.
  int32_t list_keep, scatter_lists;
  // grouping (open-addressing table over (a, b), `cap` slots, cleared per batch)
  unsigned long long *slot_key;
  int32_t *slot_count, *slot_group;
  int32_t *slot_list;        // the occupied slots, in arrival order
  int32_t cap_mask;
  int32_t *q_slot, *q_rank;  // per query: its slot and its arrival number inside the slot
  int32_t *plan;             // P_*
  unsigned long long *score_used;  // floats of `scores` handed out so far
  GemmGroup *groups;
  int32_t *tile_group;  // per tile: its group (score_cap / 1024 + 1 entries: the smallest group takes 1024 floats of scores per tile)
  int32_t *gq;        // grouped query rows
  int32_t *tq_group;  // per grouped query: its group and its row inside the group
  int32_t *tq_local;
  const float *pnorm2;   // float32 / float16 rows: |p|^2 per point and the bits of its maximum
  const unsigned int *pnorm2_max_bits;
  const int32_t *pterm;  // uint8 / int8 rows: the per-point integer term of the score (wann_gemm_kernels_bytes.inc)
  // float32 rows of more than 512 floats (k_gemm_scores_long): the batch's queries split into their two bf16 terms, per query
  // `stride` words -- stride / 2 pairs of high terms, then the pairs of low terms; columns d .. stride are zero.
  // uint8 / int8 rows of more than 512 bytes (k_gemm_scores_bslab): the batch's queries packed to bytes by pack_query_word's
  // rule and biased like the rows, per query `stride` words = the padded row.  Null otherwise.
  const uint32_t *qsplit;
  float *scores;      // what k_gemm_scores hands to k_rerank's selection: per query, step and half wave the four smallest scores
  int64_t score_cap;  // floats; groups that do not fit any more are left to the exact scan
  int32_t k;
  float acc_factor;  // safety factor on the fp32-accumulation term of the proof's error bound (k_rerank)
  unsigned long long *out_key;
  int32_t *out_cnt;
  int32_t *brute_list, *brute_count;  // exact scan: ungrouped queries + queries whose top-k could not be proven
  unsigned long long *prof;           // dev tool (make PROFILE=1): phase-cycle sums of k_gemm_scores
};

// Cover groups: the queries the window grouping left over, grouped by position block of the label argsort instead of by window.
// A cover group is a GemmGroup (a, b = the block's bounds clipped to n, nch = 1), so the score kernels run on it as they are; a
// batch whose hand-over outgrows the score buffer runs in PASSES over query ranges, all planned at once (k_cover_*).
enum { CP_NPASS = 0, CP_QUERIES = 1, CP_INTS = 4 };
struct CoverArgs {
  GemmArgs g;           // the shared-window path's arguments (tasks, queries, q_slot / slot_group, scores, out_*, brute_*)
  int32_t nblocks;      // position blocks of the index: ceil(n / kGemmPointChunk)
  int32_t max_passes;   // passes the host enqueues (the device uses cplan[CP_NPASS] <= max_passes of them)
  int32_t pass;         // k_rerank_cover: the pass this launch serves
  int32_t pass_pairs;   // (query, block) pairs a pass starts queries for; a pass holds < pass_pairs + nblocks pairs
  int32_t pair_stride;  // pairs of gq reserved per pass (>= pass_pairs + nblocks)
  int32_t tile_stride;  // tile_group entries reserved per pass
  int64_t min_rows;     // the batch takes the cover path only if its eligible windows hold at least this many rows in all (0: always)
  int32_t *cplan;       // CP_*
  int32_t *diff;        // [nblocks + 1] difference array -> wide queries per block
  int32_t *badp;        // [nblocks + 1] exclusive prefix of 'block has too few wide queries'
  int32_t *pdiff;       // [max_passes][nblocks + 1] difference arrays of the passes' queries
  int32_t *pfill;       // [max_passes][nblocks] rows of a block's query list handed out so far
  int32_t *blk_group;   // [max_passes][nblocks] the block's cover group in its pass (-1: none)
  int32_t *pplan;       // [max_passes][P_INTS] what GemmArgs::plan is to a pass's score kernel
  GemmGroup *groups;    // [max_passes][nblocks]
  int32_t *tile_group;  // [max_passes][tile_stride]
  int32_t *gq;          // [max_passes][pair_stride] the blocks' query lists
  int32_t *q_pass;      // [nq] the query's pass, -1 = not on the cover path
  int32_t *q_off;       // [nq] first of the query's pairs inside its pass
  int32_t *qb_base;     // [max_passes][pair_stride] per pair: index (in 16-byte entries) of the query's row in the block's hand-over
  CoverCounters *cctr;  // of the batch
};

// Which rows the dense path takes, and on which kind of score kernel: THE table -- the host (dense_rows_ok, dense_prefilter) and
// the launchers (wann_gemm_launch.inc) ask here and hold no row length of their own.  Lengths in 32-bit words: `stride` for
// float32 and byte rows, query_words (the row of the float32 upcast; the stride counts two-byte rows) for float16 / bfloat16.
//
//                  narrow              wide                      long (opt-in: WANN_DENSE_LONG_ROWS=1; queries pre-split / packed)
//   float32        16 .. 128           129 .. 512                513 .. 2048 (kGemmMaxFloats)
//                  k_gemm_scores<W>    k_gemm_scores_wide<2|3>   k_gemm_scores_long
//                                      / k_gemm_scores_wide4
//   float16        16 .. 128           -                         129 .. 2048 (kGemmMaxFloats)
//                  k_gemm_scores<W>                              k_gemm_scores_hslab
//   bfloat16       16 .. 128           -                         -
//                  k_gemm_scores<W>, two products (the row is its own high bf16 term)
//   one-byte shadow rows of a float32 index (internal view type 6, wann_set_dense_rows)
//                  16 .. 128           -                         -
//                  k_gemm_scores<W> of wann_gemm_kernels_w8.inc: the bfloat16 kernel, a quarter of the float32 bytes fetched
//   float8         16 .. 128           -                         -
//                  k_gemm_scores<W> of the one-byte rows (each E4M3 byte is one bf16: the bfloat16 kernel behind a byte fetch)
//   uint8 / int8   16 .. 128 (512 B)   -                         129 .. 512 (kGemmMaxBytes / 4)
//                  k_gemm_scores_b<N>                            k_gemm_scores_bslab, quantised keys: k_rerank_bslab
//
// Anything longer, and a stride that is not a multiple of 16 words, is kRowsNone: the exact scan.
enum DenseRows { kRowsNone, kRowsNarrow, kRowsWide, kRowsLong };
inline DenseRows dense_row_class(const IndexView &ix) {
  const bool bytes = byte_rows(ix.dtype);
  const int words = query_words(ix);
  if ((ix.stride & 15) || words < 16 || words > (bytes ? kGemmMaxBytes / 4 : kGemmMaxFloats)) return kRowsNone;
  if (words <= 128) return kRowsNarrow;
  if (ix.dtype == kRowsBF16 || ix.dtype == kRowsF8) return kRowsNone;  // bfloat16 / float8 rows beyond 128 elements: the exact scan, with or without WANN_DENSE_LONG_ROWS
  // (the view of a float32 index's one-byte shadow rows, wann_set_dense_rows: its score kernel is the bfloat16 one with a byte
  // fetch and covers the narrow class alone -- longer rows are scored from the float32 rows)
  if (ix.dtype == kRowsU8Widened) return kRowsNone;
  return ix.dtype == kRowsF32 && words <= 512 ? kRowsWide : kRowsLong;
}

// One unit's launchers (wann_gemm_launch.inc, compiled once per element type): a null return = launched, otherwise the error
// text.  Each unit's table is a constant reached through its gemm_unit(): nothing depends on an order of initialisation.
struct GemmUnit {
  const char *(*point_sums)(const IndexView &ix, float *norm2, unsigned int *max_bits, int32_t *term, void *stream);  // norms (float types) / terms (bytes)
  // long rows: the batch's queries split into bf16 terms (the float32 unit's; it serves float16 rows too) / packed to bytes
  const char *(*prep_queries)(const float *queries, int64_t nq, int d, int words, uint32_t *out, void *stream);
  const char *(*gemm_scores)(const GemmArgs &a, int num_cus, void *stream);
  const char *(*select_rerank)(const GemmArgs &a, Counters *ctr, void *stream);
  const char *(*rerank_cover)(const CoverArgs &c, void *stream);
};

WANN_UNIT_LOOKUP(dense, GemmUnit, gemm_unit, gemm_unit_of)  // (null: the row type has no dense unit)

// entry points (the float32 unit): each looks up ix.dtype's unit, calls it and records the error; 0 = launched
int launch_point_norms(const IndexView &ix, float *norm2, unsigned int *max_bits, void *stream);  // float32 / float16 / bfloat16 rows
int launch_point_terms(const IndexView &ix, int32_t *term, void *stream);                         // uint8 / int8 rows
int launch_split_queries(const float *queries, int64_t nq, int d, int stride, uint32_t *out, void *stream);  // long float32 / float16 rows
int launch_pack_queries(const IndexView &ix, const float *queries, int64_t nq, uint32_t *out, void *stream);  // long uint8 / int8 rows
int launch_group_windows(const GemmArgs &a, Counters *ctr, void *stream);
int launch_gemm_scores(const GemmArgs &a, int num_cus, void *stream);
int launch_select_rerank(const GemmArgs &a, Counters *ctr, void *stream);
int launch_cover_plan(const CoverArgs &c, void *stream);     // after launch_group_windows, before launch_select_rerank
// score kernel + selection / re-rank of one pass; score_ix: the view the score kernel reads instead of c.g.ix (null: c.g.ix)
int launch_cover_pass(const CoverArgs &c, int pass, int num_cus, void *stream, const IndexView *score_ix = nullptr);
const char *gemm_launch_last_error();

}  // namespace wann
