// wann_host_internal.h -- what the host side's translation units share (round 5: wann_host.cpp was one 2 100-line file):
//   wann_host.cpp  device residency of the index, launch geometry, GPU build
//   wann_batch.cpp the batch driver (run_batch, as a list of stages) and the dense prefilter path
//   wann_refdump.cpp the text printed in the reference's name (outside-range message, QueryParams::verbose dump): no HIP, own header
//   wann_abi.cpp   the C ABI of include/wann.h: index life cycle, blocking / asynchronous / multi-device search calls, RCCL all-gather
//   wann_raw.cpp   one graph over one slice of a point set: wann_raw_beam_search and the unfiltered VamanaIndex API
// Internal: nothing here is part of the boundary (include/wann.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <unistd.h>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/wann.h"
#include "wann_build.h"
#include "wann_device.h"
#include "wann_gemm_device.h"
#include "wann_gpu_build.h"
#include "wann_refine_device.h"
#include "wann_hip_util.h"
#include "wann_tuning.h"

#include <rccl/rccl.h>  // types only: librccl.so is opened at first use (wann_batch_search_allgather), never linked

using namespace wann;

namespace wann_host {

extern thread_local std::string g_err;
int fail(int code, const std::string &msg);
int usable_devices();
int hash_bits(int64_t beam);  // beamSearch.h:66
void convert_rows(const HostGraph &g, int rs, int32_t *out);  // reference in-memory rows -> device rows: rs ints per row, neighbours packed, -1 padded

constexpr int kInts = 160;
enum { I_GRAPH_COUNT = 0, I_BRUTE_COUNT = 1, I_BRUTE_CURSOR = 2, I_HEAVY_COUNT = 3, I_SUB_COUNT = 4, I_BIG_COUNT = 5 /* two ints */, I_BIG_CURSOR = 7, I_DYN_COUNT = 140, I_DYN_CURSOR = 141, I_DONE = 142, I_MID_COUNT = 143, I_RISK = 144, I_BIG_RESIDENT = 145, I_POLL_WAITING = 146, I_PRIO_COUNT = 147, I_SCAN_COUNT = 148, I_CURSOR0 = 8, I_NEXT0 = 72, I_FINAL0 = 104 };
constexpr int kMaxRounds = 30;
// follow-up launches (beams beyond the in-kernel cap): a postfiltering_max_beam up to this runs in one launch whose scratch is
// sized for the limit; a larger limit is reached in stages of doubling caps, sized for what tasks really need (SearchRounds::follow_up)
constexpr int64_t kFollowUpStageBeam = 16384;
// the largest beam a search can run: its seen-filter has 2^hash_bits(beam) entries, hash_bits = ceil(log2(beam^2)) - 2, and the
// kernels index a filter with 32-bit arithmetic (1u << bits): 92 681^2 < 2^33 <= 92 682^2, so 31 bits up to here and 32 beyond
constexpr int64_t kLargestBeam = 92681;
static_assert(kLargestBeam * kLargestBeam < ((int64_t)1 << 33) && (kLargestBeam + 1) * (kLargestBeam + 1) >= ((int64_t)1 << 33), "hash_bits(kLargestBeam) == 31");
constexpr int kVlogCap = 24;  // QueryParams::verbose: records per task (a doubling loop from beam 1 to 2^20 is 21 searches + the final one)

struct Workspace {
  DevBuf<Task> tasks;
  DevBuf<int32_t> list_a, list_b, list_final, list_heavy, list_heavy_ordered, list_mid, list_big, list_brute, ints, out_cnt, g_table, g_table_big, qtask_cnt, next_beam, part_cnt, part_done;
  DevBuf<unsigned long long> part_key;
  DevBuf<unsigned long long> out_key, g_beam;
  // wave_beam_search_big: per-slot exact seen bitmaps and filter epochs for the ordinary / follow-up launches
  // (g_table) and for the companion launch (g_table_big); a table and its epochs are zeroed together
  DevBuf<uint32_t> g_seen, g_seen_big, g_seen_f;
  DevBuf<int32_t> g_epoch, g_epoch_big, g_epoch_f, g_table_f;  // (_f: follow-up launches, whose slot layout varies)
  int64_t g_table_layout = -1, g_table_big_layout = -1, g_table_f_layout = -1;  // (slots << 8 | bits) of the last use
  DevBuf<long long> sub_hops, sub_cmps;
  DevBuf<int32_t> par_done;
  DevBuf<Counters> ctr;
  DevBuf<float> q_stage, r_stage, dist_stage;
  DevBuf<uint32_t> id_stage;
  DevBuf<unsigned long long> vlog;  // QueryParams::verbose: per-task records of the doubling loop (SearchArgs::vlog)
  DevBuf<int32_t> vlog_n;
  DevBuf<int64_t> vroute;            // QueryParams::verbose on a tree class: the descent's dump (RouteArgs::vroute)
  // wann_batch_search_device_refined: the search's rows at k = refine_k (nq x refine_k ids and distances, 8 bytes an entry),
  // what k_refine reads; the candidates it scored
  DevBuf<uint32_t> refine_ids;
  DevBuf<float> refine_dists;
  DevBuf<unsigned long long> refine_ctr;
  DevBuf<int32_t> gat_send, gat_recv;  // wann_batch_search_allgather: this replica's [2][cap][k] planes / everybody's [world][2][cap][k]
  int32_t big_stride = 0;
  int32_t *h_ints = nullptr;  // pinned
  Counters *h_ctr = nullptr;  // pinned
  std::vector<hipEvent_t> ev;
  hipEvent_t ev_side = nullptr;   // end of the companion (big) launch on the index's side stream
  hipEvent_t ev_route = nullptr;  // list sizes of k_route are on the host
  // fenwick / three_split: the end scans (k_brute) run BESIDE the graph searches of the same batch on a stream of the lane's own
  hipStream_t scan_stream = nullptr;
  hipEvent_t ev_scan = nullptr;
  ~Workspace() {
    if (h_ints) (void)hipHostFree(h_ints);
    if (h_ctr) (void)hipHostFree(h_ctr);
    for (auto e : ev) (void)hipEventDestroy(e);
    if (ev_side) (void)hipEventDestroy(ev_side);
    if (ev_route) (void)hipEventDestroy(ev_route);
    if (ev_scan) (void)hipEventDestroy(ev_scan);
    if (scan_stream) (void)hipStreamDestroy(scan_stream);
  }
  void ensure(int64_t nq, int k, int maxt, int64_t sub_slots) {
    const size_t nt = (size_t)nq * maxt + (size_t)sub_slots;
    par_done.ensure(nt);
    sub_hops.ensure(nt);
    sub_cmps.ensure(nt);
    tasks.ensure(nt);
    qtask_cnt.ensure(nq);
    list_a.ensure(nt);
    list_b.ensure(nt);
    list_final.ensure(nt);
    list_heavy.ensure(nt);
    list_heavy_ordered.ensure(nt);
    list_mid.ensure(nt);
    list_big.ensure(4 * nt);
    next_beam.ensure(nt);
    big_stride = (int32_t)nt;
    list_brute.ensure(nt);
    ints.ensure(kInts);
    out_cnt.ensure(nt);
    out_key.ensure(nt * k);
    ctr.ensure(1);
    if (!h_ints) HIP_CHECK(hipHostMalloc((void **)&h_ints, kInts * sizeof(int32_t)));
    if (!h_ctr) HIP_CHECK(hipHostMalloc((void **)&h_ctr, sizeof(Counters)));
    if (!ev_side) HIP_CHECK(hipEventCreateWithFlags(&ev_side, hipEventDisableTiming));
    if (!ev_route) HIP_CHECK(hipEventCreateWithFlags(&ev_route, hipEventDisableTiming));
    while (ev.size() < 2 + 4 * kMaxRounds) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreate(&e));
      ev.push_back(e);
    }
  }
};


// the row store a batch's beam searches read: the index's own rows, the half-precision shadow rows, the one-byte shadow rows
enum { kStoreRows = 0, kStoreHalf = 1, kStoreBytes = 2 };

}  // namespace wann_host

struct wann_index {
  HostIndex H;
  // WANN_DEVICES (in-process multi-device mode): further replicas of the device index, one per extra device listed; a replica
  // shares the primary's host index
  HostIndex *Hp = nullptr;
  HostIndex &host() { return Hp ? *Hp : H; }
  const HostIndex &host() const { return Hp ? *Hp : H; }
  std::vector<std::unique_ptr<wann_index>> replicas;
  int device = 0;
  int dtype = WANN_DTYPE_F32;  // element type of the caller's points / host queries (device queries are fp32)
  int num_cus = 256;
  DevBuf<float> d_points, d_labels, d_fv;
  // Shadow rows of a float32 index whose every value is a finite binary16 value (rows_fp16_exact) and that has graphs: the same
  // points as halves, 64-byte padded -- what a float16 index of these points keeps in d_points.  Only the beam-search launches
  // (k_search) read them, through search_view; everything else reads d_points.  Empty: no shadow (not eligible, or no memory).
  DevBuf<float> d_half;
  IndexView search_view{};     // `view` with points = d_half (paired: h16_row_position), the half stride and dtype = kRowsF16Paired (valid when d_half.p)
  bool half_rows_on = false;   // wann_set_half_rows (under tune_mu; on when a shadow exists): the next batch searches the shadow
  std::atomic<int> last_half_rows{0};  // the last finished batch (blocking call / ticket waited for) searched the shadow
  // One-byte shadow rows of a float32 index whose every value is an integer 0 .. 255 (rows_u8_exact) and that has graphs: the
  // same points as uint8, 64-byte padded, read by the beam-search launches through byte_view (dtype kRowsU8Widened: the
  // kernels of wann_kernels_w8.hip).  Beside d_half, not instead of it; off until wann_set_byte_rows asks for it, and then it
  // goes before the half rows.  Empty: no copy (not eligible, or no memory).
  DevBuf<float> d_bytes;
  IndexView byte_view{};       // `view` with points = d_bytes, the byte stride and dtype = kRowsU8Widened (valid when d_bytes.p)
  bool byte_rows_on = false;   // wann_set_byte_rows (under tune_mu; off by default): the next batch searches the one-byte rows
  std::atomic<int> last_byte_rows{0};  // the last finished batch searched the one-byte rows
  // wann_set_scan_rows (under tune_mu; off by default, only ever on where a shadow copy exists): the exact scans of the next
  // batch read the copy its beam searches read
  bool scan_rows_on = false;
  std::atomic<int> last_scan_rows{0};  // the store (kStore*) the k_brute launch of the last finished batch read
  // wann_set_dense_rows (under tune_mu; off by default, only ever on where dense_view is a one-byte view): the score launches of
  // the dense path (k_gemm_scores; float32 rows of the narrow class, d <= 128) read the one-byte copy of the rows through
  // dense_view.  Norms, selection, re-rank and finalisation keep the float32 rows.  The copy is d_bytes for the kinds whose
  // exact windows take the dense path (tree-of-graphs, super tree) and d_dense, a buffer of its own with the same layout and
  // the row order of d_points, for a float32 PrefilterIndex of byte-exact points -- which has no d_bytes: its
  // wann_byte_rows_bytes stays 0.  Neither is counted in device_bytes.
  DevBuf<float> d_dense;
  IndexView dense_view{};      // `view` with points = the copy, the byte stride and dtype = kRowsU8Widened (dtype as `view`'s: no copy)
  bool dense_rows_on = false;
  std::atomic<int> last_dense_rows{0};  // a score launch of the last finished batch read the copy
  bool has_dense_copy() const { return dense_view.dtype == kRowsU8Widened && dense_view.points != nullptr; }
  bool has_half_copy() const { return d_half.p != nullptr; }
  bool has_byte_copy() const { return d_bytes.p != nullptr; }
  bool has_scan_copy() const { return has_half_copy() || has_byte_copy(); }
  int64_t dense_copy_bytes() const { return !has_dense_copy() ? 0 : (int64_t)(d_dense.p ? d_dense.bytes() : d_bytes.bytes()); }
  // which row stores a finished batch read (run_batch's result: the beam searches' store, the scan's in the next byte, whether
  // a dense score launch read the one-byte copy in the byte after that)
  void note_row_store(int stores) {
    const int store = stores & 0xff;
    last_half_rows = store == wann_host::kStoreHalf ? 1 : 0;
    last_byte_rows = store == wann_host::kStoreBytes ? 1 : 0;
    last_scan_rows = (stores >> 8) & 0xff;
    last_dense_rows = (stores >> 16) & 1;
  }
  // wann_set_refine_rows (float16 / bfloat16 / float8 indexes; under mu): the caller's full-precision points as float32 rows in
  // the CALLER'S point order -- the order of returned ids -- zero padded to refine_row_words(d) words, the float32 index's row
  // pitch.  Only k_refine reads it (wann_batch_search_device_refined).  Empty: no store.  The primary's only: the refined calls
  // serve the primary, like wann_batch_search_device.  Not in device_bytes (wann_refine_rows_bytes reports it).
  DevBuf<float> d_refine;
  wann_refine_counters last_refine{};  // of the last refined call (under mu)
  hipEvent_t ev_refine[2] = {nullptr, nullptr};  // round the k_refine launch (created at the first refined call)
  DevBuf<uint32_t> d_decoding;
  DevBuf<int32_t> d_graph, d_fi;
  DevBuf<PartDesc> d_parts;
  DevBuf<int64_t> d_wst_off, d_wst_ptr, d_level_part0, d_level_nb, d_sup_size, d_sup_shift;
  std::vector<PartDesc> parts;
  std::vector<int64_t> level_part0;
  IndexView view{};
  int64_t device_bytes = 0;
  wann_host::Workspace ws;
  // dense prefilter path (wann_gemm_kernels_body.inc): |p|^2 per point, computed at first use
  // (float32 / float16 rows; uint8 / int8 rows keep one exact integer term per point instead, counted in device_bytes)
  DevBuf<float> d_pnorm2;
  DevBuf<unsigned int> d_pnorm2_max;
  DevBuf<int32_t> d_pterm;
  bool have_norms = false;
  // (touched by the blocking calls and by both asynchronous lanes, outside dense_mu for every class but PrefilterIndex)
  std::atomic<int> dense_idle{0};  // batches in a row on which the dense path found no window group (run_batch)
  std::atomic<uint32_t> dense_batches{0};
  DevBuf<GemmGroup> g_groups;
  DevBuf<int32_t> g_gq, g_tile_group, g_tq_group, g_tq_local, g_slot_count, g_slot_group, g_slot_list, g_q_slot, g_q_rank, g_plan;
  DevBuf<unsigned long long> g_slot_key, g_score_used;
  DevBuf<float> g_scores;
  DevBuf<uint32_t> g_qsplit;    // rows of more than 512 elements (float16: 128): the batch's queries as bf16 pairs (float32, float16) / packed biased bytes (uint8, int8) (GemmArgs::qsplit)
  int64_t qsplit_counted = 0;   // bytes of it that device_bytes holds (sorted kinds only, as with the norms)
  DevBuf<unsigned long long> g_prof;
  // cover groups (wann_set_dense_windows): distinct wide windows of a PrefilterIndex batch on the matrix cores, grouped by
  // position block.  c_ints is what a batch clears: cplan | diff | pdiff | pfill | pplan
  std::atomic<int> dense_windows{0};
  DevBuf<int32_t> c_ints, c_badp, c_blk_group, c_tile_group, c_gq, c_q_pass, c_q_off, c_qb_base;
  DevBuf<GemmGroup> c_groups;
  wann_dense_window_counters last_cover{};  // of the last batch (under dense_mu)
  // wann_set_exact_windows (tree / super indexes): a query whose window holds at most this many points is answered exactly
  // (0 = off).  A batch that runs with a non-zero limit holds dense_mu: the dense buffers above belong to the index.
  std::atomic<int64_t> exact_windows{0};
  wann_exact_window_counters last_exact{};  // of the last batch (under dense_mu)
  hipStream_t own_stream = nullptr;
  hipStream_t side_stream = nullptr;  // companion (big) k_search launches, concurrent with the caller's stream
  wann_counters last{};
  // every WANN_* switch, read when the index is created (wann_tuning.h); run_batch never reads the environment
  // (a call works on a COPY taken under tune_mu -- snapshot_tuning: with WANN_TEST_HOOKS=1 the entry points re-read the record
  // while a lane's worker may still be inside a batch)
  Tuning tune;
  std::mutex tune_mu;
  std::mutex mu;
  std::mutex dense_mu;  // the dense prefilter path's buffers and counters belong to the index: one batch at a time uses them
  // wann_batch_search_device_async: further LANES -- a lane is everything one batch in flight needs (workspace, streams, a
  // worker thread); the blocking calls use the members above
  struct Rccl;                 // librccl.so + one communicator per replica (wann_batch_search_allgather)
  std::unique_ptr<Rccl> rccl;
  struct AsyncLane;
  std::vector<std::unique_ptr<AsyncLane>> lanes;
  std::mutex lanes_mu;   // lanes, next_ticket (held briefly)
  std::mutex gather_mu;  // wann_batch_search_allgather: RCCL set-up, the replicas' send / receive planes and the collective, one call at a time
  std::mutex submit_mu;  // one submission at a time (held while a submitter waits for its lane to fall idle)
  int64_t next_ticket = 0;
  wann_index();   // (both out of line, wann_abi.cpp: AsyncLane / Rccl are complete types only there)
  ~wann_index();
};

namespace wann_host {

// A row switch of an index (wann_set_half_rows / _byte_rows / _scan_rows / _dense_rows): the flag the setter writes under
// tune_mu, the "a copy exists" predicate that bounds it, and what the last finished batch did.  The setters and getters of the
// C ABI and snapshot_tuning go through these four records.
struct RowSwitch {
  bool wann_index::*on;
  bool (wann_index::*has_copy)() const;
  std::atomic<int> wann_index::*last;
};
constexpr RowSwitch kHalfRowsSwitch = {&wann_index::half_rows_on, &wann_index::has_half_copy, &wann_index::last_half_rows};
constexpr RowSwitch kByteRowsSwitch = {&wann_index::byte_rows_on, &wann_index::has_byte_copy, &wann_index::last_byte_rows};
constexpr RowSwitch kScanRowsSwitch = {&wann_index::scan_rows_on, &wann_index::has_scan_copy, &wann_index::last_scan_rows};
constexpr RowSwitch kDenseRowsSwitch = {&wann_index::dense_rows_on, &wann_index::has_dense_copy, &wann_index::last_dense_rows};
// (under I.tune_mu)
inline bool row_switch_in_force(const wann_index &I, const RowSwitch &s) { return I.*s.on && (I.*s.has_copy)(); }

Tuning snapshot_tuning(wann_index &I);  // the index's switches for one call (WANN_TEST_HOOKS=1: re-read from the environment first)
void upload_index(wann_index &I);
// wann_set_refine_rows: (n, d) float32 points in the caller's order -> I.d_refine (checked by the caller; throws HipError)
void upload_refine_rows(wann_index &I, const float *points);
int ensure_filter_scratch(DevBuf<int32_t> &table, DevBuf<int32_t> &epoch, DevBuf<uint32_t> &seen, int64_t &layout, int slots,
                          int table_bits, int64_t seen_words, hipStream_t st, bool any_slots = false);
struct RoundCfg {
  LaunchCfg lc;
  bool big_lds;      // the one-wave-per-workgroup kernel
  int slots;
  int pool_bytes;    // per-wave LDS pool of this launch
  int table_bits;    // per-slot global seen-filter of 4 << table_bits bytes (0 = none needed)
  int64_t beam_cap;  // per-slot global beam entries (0 = none needed)
};
// V: the view the launch's kernel reads (I.view, or I.search_view / I.byte_view for a batch that searches a shadow copy of the rows)
RoundCfg config_for(const wann_index &I, const IndexView &V, const Tuning &T, int64_t first_beam, int64_t cap, int64_t work_items, bool big_lds = false, bool force_table = false,
                    bool legacy = false, int base_pool = kSearchPoolBytes);
int lean_pool_bytes(const IndexView &V);
int method_code(const char *m);
// W / side / last: the lane of this batch (the index's own members for the blocking calls, an AsyncLane's for the asynchronous one)
// Returns the row store the batch's beam searches read (kStore*): the one-byte rows if T.byte_rows, else the half rows if
// T.half_rows, else the index's own rows -- and, shifted left by 8, the store its k_brute launch read (the same one if
// T.scan_rows, else kStoreRows; kStoreRows too for a batch that launched no scan) -- and, shifted left by 16, 1 if a score launch
// of its dense path read the one-byte copy (T.dense_rows) for at least one query.
// stop_k: the rows have qp.k columns, and every graph search's doubling loop ends at the first level with >= stop_k in-window
// entries (wann.h WIDE ROWS); 0 = qp.k, the ordinary call.  1 <= stop_k <= qp.k otherwise, and not with qp.verbose.
int run_batch(wann_index &I, Workspace &W, hipStream_t side, wann_counters &last, const float *d_queries, const float *d_ranges, int64_t nq,
               int64_t qid_base, const char *method, const wann_query_params &qp, uint32_t *d_ids, float *d_dists, hipStream_t st, const Tuning &T,
               const int64_t *d_qids = nullptr, int64_t stop_k = 0);
void build_pending(wann_index &I, std::vector<HostPart *> &pending);
// host queries of the index's element type (uint8 / int8 / float16 / bfloat16 / float8) -> the fp32 rows every kernel stages (exact)
std::vector<float> bytes_to_float(int dtype, const void *src, int64_t count);
// (element_bytes, known_dtype and the row-type predicates: wann_row_types.h)
static_assert(WANN_DTYPE_F32 == kRowsF32 && WANN_DTYPE_U8 == kRowsU8 && WANN_DTYPE_I8 == kRowsI8 && WANN_DTYPE_F16 == kRowsF16 &&
                  WANN_DTYPE_BF16 == kRowsBF16,
              "the C ABI's element types are row types of the table");
static_assert(WANN_DTYPE_F8 == kRowsF8, "the float8 element type is its own view type");
// uint8 / int8 rows: scored with v_dot4 by kernels built for more waves per SIMD
inline bool byte_rows(const IndexView &v) { return wann::byte_rows(v.dtype); }
// this view's four-wave k_search is built for THREE waves per SIMD (at most 168 registers): the inner-product and byte-row
// kernels.  The squared-L2 kernels keep two whole rows per lane pair in flight and are built for two: float32 needs 256
// registers, float16 (k_search<0, 0, 3>) 215, the paired half shadow rows (k_search<0, 0, 7>) 189 -- see DESIGN.md 3.10.
inline bool three_waves_per_simd(const IndexView &v) { return v.metric == 1 || byte_rows(v); }
BuildSpec make_spec(int kind, int metric, int dtype, int64_t n, int64_t d, int32_t cutoff, double split_factor, double shift_factor,
                    const wann_build_params *bp, int threads);

}  // namespace wann_host
using namespace wann_host;

