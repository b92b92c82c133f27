// wann_host.cpp -- host side of the MI355X window-filtered ANN engine: device residency of the index, the launch geometry of
// the beam-search launches, the GPU build of missing graphs.  The batch_search driver (run_batch) and the dense prefilter
// path's launches are wann_batch.cpp.  The C ABI (include/wann.h) that calls into this is wann_abi.cpp; the raw-graph entry
// points are wann_raw.cpp.
//
// There is no CPU search path in this library: every compute entry point needs a gfx950 device
// and fails loudly otherwise.
#include "wann_host_internal.h"
#include "wann_bf16.h"
#include "wann_f8.h"
#include "wann_half.h"

namespace wann_host {


thread_local std::string g_err;
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

int usable_devices() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int hash_bits(int64_t beam) {  // beamSearch.h:66
  return std::max<int>(10, (int)std::ceil(std::log2((double)(beam * beam))) - 2);
}

// reference in-memory rows -> device rows: rs ints per row, neighbours packed, -1 padded
void convert_rows(const HostGraph &g, int rs, int32_t *out) {
  for (int64_t i = 0; i < g.n; i++) {
    const int32_t *r = g.row(i);
    int32_t *o = out + i * rs;
    const int deg = r[0];
    if (deg < 0 || deg > g.maxdeg || deg > rs) throw std::runtime_error("graph row degree out of range");
    for (int j = 0; j < deg; j++) {
      if (r[1 + j] < 0 || r[1 + j] >= g.n) throw std::runtime_error("graph edge out of range");
      o[j] = r[1 + j];  // a row may list a node twice (reference-built graphs do); the kernel copes
    }
    for (int j = deg; j < rs; j++) o[j] = -1;
  }
}


// the index's switches for one call (WANN_TEST_HOOKS=1: re-read from the environment first)
Tuning snapshot_tuning(wann_index &I) {
  std::lock_guard<std::mutex> lk(I.tune_mu);
  if (I.tune.hooks_live) I.tune = Tuning::from_env();
  Tuning t = I.tune;
  t.half_rows = row_switch_in_force(I, kHalfRowsSwitch);
  t.byte_rows = row_switch_in_force(I, kByteRowsSwitch);
  t.scan_rows = row_switch_in_force(I, kScanRowsSwitch);
  t.dense_rows = row_switch_in_force(I, kDenseRowsSwitch);
  return t;
}

// A shadow copy of a float32 index's rows in `buf`: n rows of `words` 32-bit words, zeroed, filled by fill(rows) -- packed and
// laid out -- and uploaded.  An index that cannot have the copy (no host or device memory) simply has none: `buf` stays empty.
template <typename Fill>
static void upload_shadow_rows(DevBuf<float> &buf, int64_t n, int64_t words, Fill fill) {
  std::vector<float> rows;
  try {
    rows.assign((size_t)n * words, 0.f);
    buf.ensure(rows.size());
  } catch (std::bad_alloc &) {
    buf.release();
  } catch (HipError &) {
    (void)hipGetLastError();  // (the allocation that failed is not left behind as the next call's error)
    buf.release();
  }
  if (!buf.p) return;
  fill(rows.data());
  buf.upload(rows);
}

void upload_index(wann_index &I) {
  HostIndex &H = I.host();
  const BuildSpec &s = H.spec;
  HIP_CHECK(hipSetDevice(I.device));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, I.device));
  I.num_cus = prop.multiProcessorCount;
  std::string arch = prop.gcnArchName;
  if (arch.rfind("gfx950", 0) != 0)
    throw HipError("device " + std::to_string(I.device) + " is " + arch + ", this library holds gfx950 code only");
  HIP_CHECK(hipStreamCreateWithFlags(&I.own_stream, hipStreamNonBlocking));
  {  // highest priority: when both launches become ready the companion's few workgroups are dispatched first
    int prio_low = 0, prio_high = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    HIP_CHECK(hipStreamCreateWithPriority(&I.side_stream, hipStreamNonBlocking, prio_high));
  }

  IndexView &v = I.view;
  v.n = s.n;
  v.d = (int32_t)s.d;
  // float16 / bfloat16 points: the host rows are their float32 upcast; the device rows are two-byte elements again (exact), 64-byte padded
  // float8 points: likewise one-byte patterns again, d bytes zero padded to a multiple of 64, in the one-byte shadow rows' layout
  v.stride = (int32_t)row_stride_words(s.dtype, s.d, s.stride);
  v.metric = s.metric;
  v.dtype = s.dtype;
  v.kind = s.kind;
  v.cutoff = s.cutoff;
  v.split = (int32_t)s.split_factor;
  v.vamana_leaves = H.vamana_leaves ? 1 : 0;
  v.maxdeg = (int32_t)s.R;
  v.rs = (int32_t)(((s.R + 15) / 16) * 16);
  v.nlevels = (int32_t)H.levels.size();

  if (two_byte_rows(s.dtype)) {
    std::vector<float> rows((size_t)s.n * v.stride, 0.f);
    parallel_for(s.n, s.threads > 0 ? s.threads : default_threads(), [&](int64_t r) {
      const float *src = H.pts.data() + r * s.stride;
      uint16_t *dst = reinterpret_cast<uint16_t *>(rows.data() + r * v.stride);
      for (int64_t j = 0; j < s.d; j++) dst[j] = float_to_two_byte(s.dtype, src[j]);
    });
    I.d_points.upload(rows);
  } else if (s.dtype == WANN_DTYPE_F8) {
    std::vector<float> rows((size_t)s.n * v.stride, 0.f);
    pack_f8_rows(H.pts.data(), s.n, s.d, s.stride, v.stride, s.threads, rows.data());
    interleave_u8_rows(rows.data(), s.n, v.stride, s.threads);  // (the device layout: u8_row_position, wann_row_types.h)
    I.d_points.upload(rows);
  } else {
    I.d_points.upload(H.pts);
  }
  // float32 points that are all binary16 values, on an index with graphs: a second copy as half rows (the float16 branch's
  // conversion and padding) for the beam searches, which are bound by the bytes of the rows they score.  Every shape the
  // float16 k_search serves qualifies -- that is every shape: a float16 index of any kind / metric / R / d runs these kernels.
  if (s.dtype == WANN_DTYPE_F32 && H.vamana_leaves && rows_fp16_exact(H.pts.data(), s.n, s.d, s.stride, s.threads)) {
    const int64_t hstride = row_stride_words(kRowsF16Paired, s.d, s.stride);
    upload_shadow_rows(I.d_half, s.n, hstride, [&](float *rows) {
      parallel_for(s.n, s.threads > 0 ? s.threads : default_threads(), [&](int64_t r) {
        const float *src = H.pts.data() + r * s.stride;
        uint16_t *dst = reinterpret_cast<uint16_t *>(rows + r * hstride);
        for (int64_t j = 0; j < s.d; j++) dst[j] = float_to_half(src[j]);
      });
      interleave_h16_rows(rows, s.n, hstride, s.threads);  // (the copy's layout: h16_row_position, wann_row_types.h)
    });
  }
  // ... and where they are all integers 0 .. 255 (SIFT / BIGANN are), a third copy as one-byte rows: a quarter of the float32
  // bytes, scored by the kernels of wann_kernels_w8.hip.  Beside the half copy, not instead of it: wann_set_byte_rows chooses
  // between batches without allocating anything, and the copy is off until it is asked for.
  const int64_t bstride = row_stride_words(kRowsU8Widened, s.d, s.stride);
  const auto fill_u8_rows = [&](float *rows) {
    pack_u8_rows(H.pts.data(), s.n, s.d, s.stride, bstride, s.threads, rows);
    interleave_u8_rows(rows, s.n, bstride, s.threads);  // (the copy's layout: u8_row_position, wann_row_types.h)
  };
  if (s.dtype == WANN_DTYPE_F32 && H.vamana_leaves && rows_u8_exact(H.pts.data(), s.n, s.d, s.stride, s.threads))
    upload_shadow_rows(I.d_bytes, s.n, bstride, fill_u8_rows);
  // A float32 PrefilterIndex of such points keeps the same one-byte rows for the score kernel of its dense path
  // (wann_set_dense_rows, off by default), where that kernel takes them: rows of the narrow class.  The layout of d_bytes, the
  // row order of d_points, a buffer of its own: the index has no beam searches and no byte rows to switch on.
  if (s.dtype == WANN_DTYPE_F32 && s.kind == WANN_KIND_PREFILTER && dense_row_class(v) == kRowsNarrow &&
      rows_u8_exact(H.pts.data(), s.n, s.d, s.stride, s.threads))
    upload_shadow_rows(I.d_dense, s.n, bstride, fill_u8_rows);
  I.d_labels.upload(H.labels);
  I.d_decoding.upload(H.decoding);
  v.points = I.d_points.p;
  v.labels = I.d_labels.p;
  v.decoding = I.d_decoding.p;
  if (s.kind == WANN_KIND_PREFILTER) {
    I.d_fv.upload(H.fv_sorted);
    I.d_fi.upload(H.fi_sorted);
    v.fv_sorted = I.d_fv.p;
    v.fi_sorted = I.d_fi.p;
  }
  // partitions + adjacency pool
  int64_t rows = 0;
  std::vector<int64_t> level_nb;
  for (auto &lv : H.levels) {
    I.level_part0.push_back((int64_t)I.parts.size());
    level_nb.push_back((int64_t)lv.size());
    for (auto &P : lv) {
      PartDesc pd;
      pd.row_base = rows;
      pd.start = (int32_t)P.start;
      pd.n = (int32_t)P.n;
      I.parts.push_back(pd);
      if (H.vamana_leaves) rows += P.n;
    }
  }
  I.d_parts.upload(I.parts);
  v.parts = I.d_parts.p;
  I.d_level_part0.upload(I.level_part0);
  I.d_level_nb.upload(level_nb);
  v.level_part0 = I.d_level_part0.p;
  v.level_nb = I.d_level_nb.p;
  if (H.vamana_leaves) {
    I.d_graph.ensure((size_t)rows * v.rs);
    // convert + upload partition by partition through a bounded pinned staging buffer
    const size_t stage_rows = 1 << 20;
    std::vector<int32_t> stage;
    size_t pi = 0;
    for (auto &lv : H.levels)
      for (auto &P : lv) {
        const PartDesc &pd = I.parts[pi++];
        if (P.g.n != P.n) {  // not in the cache: built on the device afterwards, rows start empty
          HIP_CHECK(hipMemset(I.d_graph.p + pd.row_base * v.rs, 0xFF, (size_t)pd.n * v.rs * 4));
          continue;
        }
        for (int64_t r0 = 0; r0 < P.n; r0 += (int64_t)stage_rows) {
          int64_t cnt = std::min<int64_t>((int64_t)stage_rows, P.n - r0);
          stage.resize((size_t)cnt * v.rs);
          for (int64_t i = 0; i < cnt; i++) {
            const int32_t *r = P.g.row(r0 + i);
            int32_t *o = stage.data() + i * v.rs;
            const int deg = r[0];
            if (deg < 0 || deg > P.g.maxdeg || deg > v.rs) throw std::runtime_error("graph row degree out of range");
            for (int j = 0; j < deg; j++) {
              if (r[1 + j] < 0 || r[1 + j] >= P.n) throw std::runtime_error("graph edge out of range");
              o[j] = r[1 + j];
            }
            for (int j = deg; j < v.rs; j++) o[j] = -1;
          }
          HIP_CHECK(hipMemcpy(I.d_graph.p + (pd.row_base + r0) * v.rs, stage.data(), stage.size() * 4, hipMemcpyHostToDevice));
        }
      }
    v.graph = I.d_graph.p;
  }
  if (!H.offsets.empty()) {
    std::vector<int64_t> flat, ptr;
    for (auto &o : H.offsets) {
      ptr.push_back((int64_t)flat.size());
      flat.insert(flat.end(), o.begin(), o.end());
    }
    ptr.push_back((int64_t)flat.size());
    I.d_wst_off.upload(flat);
    I.d_wst_ptr.upload(ptr);
    v.wst_off = I.d_wst_off.p;
    v.wst_ptr = I.d_wst_ptr.p;
  }
  if (!H.sup_size.empty()) {
    I.d_sup_size.upload(H.sup_size);
    I.d_sup_shift.upload(H.sup_shift);
    v.sup_size = I.d_sup_size.p;
    v.sup_shift = I.d_sup_shift.p;
  }
  I.search_view = v;
  if (I.d_half.p) {
    I.search_view.points = I.d_half.p;
    I.search_view.stride = (int32_t)row_stride_words(kRowsF16Paired, s.d, s.stride);
    I.search_view.dtype = kRowsF16Paired;
    I.half_rows_on = true;
  }
  I.byte_view = v;
  if (I.d_bytes.p) {  // (byte_rows_on stays false: the one-byte rows are opt-in, wann_set_byte_rows)
    I.byte_view.points = I.d_bytes.p;
    I.byte_view.stride = (int32_t)bstride;
    I.byte_view.dtype = kRowsU8Widened;
  }
  // the copy the dense path's score launches read under wann_set_dense_rows: the PrefilterIndex's own, or the one-byte shadow
  // rows of the kinds whose exact windows take the dense path -- where the float32 rows are in the score kernel's narrow class
  I.dense_view = v;
  {
    const bool exact_kind = s.kind == WANN_KIND_TREE_VAMANA || s.kind == WANN_KIND_SUPER;
    const float *copy = I.d_dense.p ? I.d_dense.p : (exact_kind && dense_row_class(v) == kRowsNarrow) ? I.d_bytes.p : nullptr;
    if (copy) {
      I.dense_view.points = copy;
      I.dense_view.stride = (int32_t)bstride;
      I.dense_view.dtype = kRowsU8Widened;
    }
  }
  // (neither shadow copy is in device_bytes, which keeps counting what it always has: wann_half_rows_bytes / wann_byte_rows_bytes report them)
  I.device_bytes = (int64_t)(I.d_points.bytes() + I.d_labels.bytes() + I.d_decoding.bytes() + I.d_graph.bytes() +
                             I.d_parts.bytes() + I.d_fv.bytes() + I.d_fi.bytes() + I.d_wst_off.bytes());
}

// The full-precision row store of a compact index (wann_set_refine_rows): the caller's float32 points, row r = point r of the
// array the index was made from (the order of returned ids: nothing here knows the label sort), zero padded to the float32
// index's row pitch so that the float32 row-distance routines read it as they read a float32 index.
void upload_refine_rows(wann_index &I, const float *points) {
  const BuildSpec &s = I.host().spec;
  const int64_t words = refine_row_words(s.d);
  HIP_CHECK(hipSetDevice(I.device));
  std::vector<float> rows((size_t)s.n * words, 0.f);
  parallel_for(s.n, s.threads > 0 ? s.threads : default_threads(), [&](int64_t r) {
    memcpy(rows.data() + r * words, points + r * s.d, (size_t)s.d * sizeof(float));
  });
  I.d_refine.release();  // (exactly n rows: wann_refine_rows_bytes is the store's size)
  I.d_refine.upload(rows);
}

// Global scratch of a launch whose searches keep their seen-filter in global memory: the per-slot filter tables
// (entries tagged with the slot's search epoch), the epochs, and the per-slot exact seen bitmaps.  A table whose
// slot layout changes (or that was reallocated) is zeroed together with its epochs.
int ensure_filter_scratch(DevBuf<int32_t> &table, DevBuf<int32_t> &epoch, DevBuf<uint32_t> &seen, int64_t &layout, int slots,
                          int table_bits, int64_t seen_words, hipStream_t st, bool any_slots) {
  // any_slots: a slot's region depends on the region stride only (slot << stride bits), so launches with different slot counts
  // share one zeroed table -- and the stride never SHRINKS: a launch whose filters are smaller than the largest seen so
  // far uses a prefix of every region (the search masks with its own `bits`), instead of a 2^bits-word re-layout that zeroes the
  // whole table and every epoch each time two launch shapes alternate.  The stride in use is returned (SearchArgs::g_table_bits).
  if (any_slots && layout > table_bits && layout < 32 && ((size_t)slots << layout) * sizeof(int32_t) <= ((size_t)20 << 30)) table_bits = (int)layout;
  const size_t need = (size_t)slots << table_bits;
  const int64_t want = any_slots ? (int64_t)table_bits : (((int64_t)slots << 8) | table_bits);
  const bool fresh = need > table.cap || (size_t)slots > epoch.cap;
  table.ensure(need);
  epoch.ensure((size_t)slots);
  seen.ensure((size_t)slots * (size_t)seen_words);
  if (fresh || layout != want) {
    HIP_CHECK(hipMemsetAsync(table.p, 0, table.cap * sizeof(int32_t), st));
    HIP_CHECK(hipMemsetAsync(epoch.p, 0, epoch.cap * sizeof(int32_t), st));
    layout = want;
  }
  return table_bits;
}

// Launch geometry for a k_search launch whose searches run beams in [first_beam, cap].
// big_lds: the rare follow-up launch for beams beyond the in-kernel cap -- one wave per workgroup with a
// pool large enough to keep even a 10 000-entry beam in the LDS (only its seen-filter lives in global memory).
// The four-wave kernel holds the register-resident cores and the second-generation general core only (256 registers per
// wave); everything else -- beams whose LDS beam exceeds the four-wave pool, the first-generation cores behind the test
// switches -- runs in the one-wave-per-workgroup kernel (big_lds).  force_table: a global seen-filter even if the LDS would do.
// legacy: the one-wave kernel that holds the first-generation cores (k_search<., 2>: dev switches, the cut step); it is also
// what a beam that does not fit the LDS next to the helper waves' mailbox gets.  The production one-wave kernel
// (k_search<., 1>) always keeps its seen-filter in global memory.
// base_pool: the four-wave kernel's per-wave pool (kSearchPoolBytes, or lean_pool_bytes() for three workgroups per CU).
// A workgroup's LDS is handed out in granules: 1 280 bytes fits what round 4 measured (three workgroups of 53 KiB = 43 granules each
// are not co-resident in a CU's 128 granules, three of 52.5 KiB = 42 are; two of 77.5 KiB = 62 are) -- whatever
// hipOccupancyMaxActiveBlocksPerMultiprocessor says.
constexpr int kLdsGranule = 1280;  // (of a CU's kLdsPerWorkgroup bytes: wann_device.h)
inline int lds_blocks_per_cu(int per_block) { return kLdsPerWorkgroup / (((per_block + kLdsGranule - 1) / kLdsGranule) * kLdsGranule); }

RoundCfg config_for(const wann_index &I, const IndexView &V, const Tuning &T, int64_t first_beam, int64_t cap, int64_t work_items, bool big_lds, bool force_table,
                    bool legacy, int base_pool) {
  RoundCfg rc{};
  const int64_t cap_bytes = ((cap + 1) & ~(int64_t)1) * 8;
  if (cap_bytes > base_pool) big_lds = true;
  // Rows of more than 64 neighbours (64 < R <= 128) are worked in two halves by the first-generation general core only: every
  // search of such an index runs in the one-wave kernel that holds it (k_search<., 2>), eight workgroups per CU.
  if (V.rs > 64) big_lds = legacy = true;
  const int wpb = big_lds ? 1 : kWavesPerBlock;
  const int common = search_lds_bytes_per_wave(query_words(V), 0);
  if (big_lds && !legacy && cap_bytes + 4096 + kScoreBoxBytes > 150 * 1024 - common) legacy = true;
  const int box_bytes = (big_lds && !legacy) ? kScoreBoxBytes : 0;
  if (big_lds && !legacy) force_table = true;
  int pool = base_pool;
  // (one-wave kernels: + the clash-detection scratch beside the largest beam; production kernel: + the helper waves' mailbox
  // at the end of the pool -- the kernel takes kScoreBoxBytes off whenever it runs with helpers, so the decisions below use
  // what is left)
  if (big_lds) pool = (int)std::min<int64_t>(std::max<int64_t>(cap_bytes + 4096, kSearchPoolBytes) + box_bytes, 150 * 1024 - common);
  rc.pool_bytes = pool;
  const int usable = pool - box_bytes;
  const int per_block = (common + pool) * wpb;
  if (per_block > kLdsPerWorkgroup) throw std::runtime_error("beam-search LDS footprint exceeds 160 KiB");
  // register budget: the L2 kernel holds two whole 512-B rows per lane pair in flight (2 waves/SIMD)
  // (four-wave kernel: the squared-L2 float kernel needs 232 registers: two waves per SIMD; the inner-product and byte-row
  // kernels are built for three)
  const int waves_per_cu = three_waves_per_simd(V) ? 12 : 8;
  int blocks_per_cu = std::min((big_lds ? 8 : waves_per_cu) / wpb, lds_blocks_per_cu(per_block));
  blocks_per_cu = std::max(1, blocks_per_cu);
  int64_t blocks = (int64_t)I.num_cus * blocks_per_cu;
  const int cap_bits = hash_bits(cap);
  if (force_table || cap_bytes + ((int64_t)4 << cap_bits) > usable) {  // some beam of the range keeps its filter in global memory
    rc.table_bits = cap_bits;
    int64_t per_slot = (int64_t)4 << cap_bits;
    int64_t max_slots = std::max<int64_t>(wpb, ((int64_t)16 << 30) / per_slot);
    blocks = std::min(blocks, max_slots / wpb);
  }
  if (cap_bytes > usable) rc.beam_cap = (cap + 1) & ~(int64_t)1;
  (void)first_beam;
  blocks = std::min<int64_t>(blocks, (work_items + wpb - 1) / wpb);
  rc.lc.blocks = (int)std::max<int64_t>(blocks, 1);
  rc.lc.waves_per_block = wpb;
  rc.lc.big = big_lds ? (legacy ? 2 : 1) : 0;
  rc.big_lds = big_lds;
  rc.slots = rc.lc.blocks * wpb;
  return rc;
}

// Per-wave pool with which THREE four-wave workgroups share a CU's 160 KiB of LDS (inner-product / byte-row kernels, which
// fit three waves per SIMD): the in-kernel cap's beam (10 KiB) still fits, the seen-filter of beams up to 90 too.  0: this
// index can not use it (rows too long).
int lean_pool_bytes(const IndexView &V) {
  if (!three_waves_per_simd(V)) return 0;
  const int common = search_lds_bytes_per_wave(query_words(V), 0);
  // 52 KiB per workgroup.  Three workgroups of 53 KiB (159 of the CU's 160 KiB) are NOT co-resident on gfx950, whatever
  // hipOccupancyMaxActiveBlocksPerMultiprocessor says (3): a launch of 768 such workgroups ran at the speed of 512 until round 4
  // measured it (stand-alone inner-product graph, 30 000 searches at beam 80: 6.65 ms at 53 KiB, 5.22 ms at 52.5 KiB and below).
  int pool = (52 * 1024) / kWavesPerBlock - common;
  return pool >= kInKernelBeamCap * 8 + 1536 ? pool : 0;
}

int method_code(const char *m) {
  if (m && !strcmp(m, "optimized_postfilter")) return M_OPTIMIZED;
  if (m && !strcmp(m, "three_split")) return M_THREE_SPLIT;
  return M_FENWICK;  // range_filter_tree.h:76-82: everything else falls through to fenwick
}

// Graphs missing from the cache: built on the GPU straight into the adjacency pool (with WANN_HOST_BUILD=1:
// by the host builder and then uploaded -- a test hook, never a fallback).
void upload_part_rows(wann_index &I, const HostPart &P, const PartDesc &pd) {
  const int rs = I.view.rs;
  std::vector<int32_t> stage((size_t)P.n * rs);
  convert_rows(P.g, rs, stage.data());
  HIP_CHECK(hipMemcpy(I.d_graph.p + pd.row_base * rs, stage.data(), stage.size() * 4, hipMemcpyHostToDevice));
}

void build_pending(wann_index &I, std::vector<HostPart *> &pending) {
  HostIndex &H = I.H;
  const BuildSpec &s = H.spec;
  std::vector<GpuBuildTarget> targets;
  size_t pi = 0;
  for (auto &lv : H.levels)
    for (auto &P : lv) {
      if (std::find(pending.begin(), pending.end(), &P) != pending.end()) targets.push_back(GpuBuildTarget{(int32_t)pi, &P});
      pi++;
    }
  // WANN_HOST_BUILD=1 (tests: the host builder as a cross-check) is the only way onto the host builder; a
  // visited list that outgrows its LDS buffer restarts the build ON THE GPU with a larger buffer.
  // (R > 64: the GPU builder's rows are one wave wide -- such graphs are built by the host builder, byte-identical to the
  // reference's like the GPU builder's)
  if (getenv("WANN_HOST_BUILD") != nullptr || s.R > 64) {
    build_pending_on_host(H, pending);
    for (auto &t : targets) upload_part_rows(I, *t.part, I.parts[t.part_index]);
  } else {
    // float16 / bfloat16 / float8 points are built from their float32 upcast (the host rows) by the float32 build kernels: the graphs are those of
    // the float32 index on the upcast points, byte for byte.  The float32 rows live on the device for the build only.
    IndexView bv = I.view;
    DevBuf<float> rows32;
    if (upcast_built(s.dtype)) {
      rows32.upload(H.pts);
      bv.points = rows32.p;
      bv.stride = (int32_t)s.stride;
      bv.dtype = WANN_DTYPE_F32;
    }
    for (int vis_scale = 1;; vis_scale *= 2) {
      try {
        gpu_build_graphs(bv, I.d_graph.p, I.parts, targets, s.R, s.L, s.alpha, I.num_cus, s.threads, I.own_stream, vis_scale);
        break;
      } catch (std::runtime_error &e) {
        if (std::string(e.what()).find("gpu build overflow: a visited list") == std::string::npos || vis_scale >= 8) throw;
        if (I.tune.verbose) fprintf(stderr, "[wann] %s; restarting the GPU build with a %dx buffer\n", e.what(), 2 * vis_scale);
      }
    }
  }
  save_built_graphs(H, pending, true);
}

std::vector<float> bytes_to_float(int dtype, const void *src, int64_t count) {
  std::vector<float> out((size_t)count);
  if (element_bytes(dtype) == 2) {
    const uint16_t *p = (const uint16_t *)src;
    for (int64_t i = 0; i < count; i++) out[(size_t)i] = two_byte_to_float(dtype, p[i]);
  } else if (dtype == WANN_DTYPE_F8) {
    const uint8_t *p = (const uint8_t *)src;
    for (int64_t i = 0; i < count; i++) out[(size_t)i] = f8_to_float(p[i]);
  } else if (dtype == WANN_DTYPE_U8) {
    const uint8_t *p = (const uint8_t *)src;
    for (int64_t i = 0; i < count; i++) out[(size_t)i] = (float)p[i];
  } else {
    const int8_t *p = (const int8_t *)src;
    for (int64_t i = 0; i < count; i++) out[(size_t)i] = (float)p[i];
  }
  return out;
}

BuildSpec make_spec(int kind, int metric, int dtype, int64_t n, int64_t d, int32_t cutoff, double split_factor,
                    double shift_factor, const wann_build_params *bp, int threads) {
  BuildSpec s;
  s.kind = kind;
  s.metric = metric;
  s.dtype = dtype;
  s.n = n;
  s.d = d;
  s.cutoff = cutoff;
  s.split_factor = split_factor;
  s.shift_factor = shift_factor;
  s.R = bp ? bp->max_degree : 64;
  s.L = bp ? bp->limit : 500;
  s.alpha = bp ? bp->alpha : 1.175;
  s.cache = (bp && bp->cache_path) ? bp->cache_path : "";
  s.threads = threads;
  return s;
}


}  // namespace wann_host
