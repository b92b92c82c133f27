// wann_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the window-filtered ANN engine.
//
// One wavefront owns one unit of work (a beam search of one query in one partition, or a
// brute-force scan); a 256-thread workgroup holds four independent waves that never synchronise
// with each other.  All cross-lane traffic is ballots / readlane / per-wave LDS.  Kernels are
// persistent over a device-side work list (atomic cursor), so no launch depends on a host count.
//
//   k_route     window -> work item (window search tree descent)          reference: src/range_filter_tree.h:403-471,
//                                                                          src/super_optimized_postfilter_tree.h:187-270
//   k_search    batched beam search + post filter of the final beam       reference: ParlayANN/algorithms/utils/beamSearch.h:51-184,
//                                                                          src/postfilter_vamana.h:141-188,223-254
//   k_brute     exact scan of a contiguous (or gathered) window            reference: src/range_filter_tree.h:393-397, src/prefiltering.h:154-204
//   k_finalize  top-k rows -> (ids, dists) with id decoding and padding    reference: src/range_filter_tree.h:84-93
//
// fp32 evaluation order is the reference's as compiled (SURVEY.md A.3); this file is built with
// -ffp-contract=off and every fused multiply-add below is an explicit fmaf().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdio.h>

#include <algorithm>

#include "wann_device.h"
#include "wann_wave.h"

namespace wann {

// One translation unit per element type (WANN_DT, set by wann_kernels.hip / _u8.hip / _i8.hip / _f16.hip / _bf16.hip / _w8.hip / _h16.hip / _f8.hip before this body is
// included): the search and scan kernels and their launchers live in a per-type namespace; the type-independent
// kernels (routing, finalisation) and the dispatchers are compiled with the float32 unit only.
// (the unit's namespace WANN_DT_NS, the template parameter WANN_DT_TPARAM of the widened types' kernels and the class flags come
// from the row type's entry in wann_row_types.h)
#ifndef WANN_MIPS_WAVES
#define WANN_MIPS_WAVES 3  // waves per SIMD the four-wave kernel of inner-product / byte rows is built for (dev: 4 = 128 registers)
#endif
namespace WANN_DT_NS {


// --------------------------------------------------------------------------------------------
// k_search: one wavefront takes a task (query, partition) through the WHOLE post-filter loop of
// PostfilterVamanaIndex::query (postfilter_vamana.h:141-188): search at beam b, count the in-window
// beam entries, double b and search again from scratch while fewer than k were found, then the
// optional final re-search at min(b * final_beam_multiply, max_beam).  Doing the loop inside the
// wave (instead of one launch per doubling round) keeps the GPU busy while the few queries that
// need large beams run their long, strictly sequential searches.
//
// Per-wave LDS: common scratch + a pool of A.pool_bytes that holds, per search,
//   small: beam + seen-filter          (4 << bits) + 8 B <= pool
//   big  : beam only, filter in global (8 B <= pool)
//   huge : nothing (beam and filter in per-slot global scratch)
// Beams above A.cap_inkernel leave the kernel: speculative levels were routed to the companion launch
// (BIG = true) from the start, continuations go to its pollers, the rest (next_list / final_list) to
// follow-up launches of this same kernel.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ int hash_bits_dev(long long beam) {  // beamSearch.h:66
  long long sq = beam * beam;
  int e = (sq <= 1) ? 0 : (64 - __builtin_clzll((unsigned long long)(sq - 1)));  // ceil(log2(beam^2))
  e -= 2;
  return e < 10 ? 10 : e;
}

// BIG = false: the ordinary kernel (four independent waves per workgroup, each with its own LDS slice).
// BIG = true : the companion launch for speculative levels beyond cap_inkernel: ONE wave per workgroup that
// owns a large LDS pool (beams up to big_cap), runs concurrently with the ordinary kernel on a second stream,
// serves the static big list (longest class first) and then -- in its first npollers workgroups -- waits for
// continuations handed over by ordinary waves until every ordinary ticket is done.  Two kernels rather than
// two modes of one: the mode logic cost the ordinary kernel 20 VGPRs (it needs all 256 of two waves per SIMD).
// a look-ahead search (k_search) that its chain does not need: if it has finished, its work was speculation; if it still
// waits in the pollers' queue, nobody need pick it up (lane 0 only)
__device__ __forceinline__ void la_withdraw(const SearchArgs &A, int la) {
  if (atomicExch(&A.par_done[la], 2) == 1) {
    atomicAdd(&A.ctr->spec_searches, 1ull);
    atomicAdd(&A.ctr->spec_hops, (unsigned long long)__hip_atomic_load(&A.sub_hops[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    atomicAdd(&A.ctr->spec_dist_cmps, (unsigned long long)__hip_atomic_load(&A.sub_cmps[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  atomicCAS(A.dyn_list + A.next_beam[la], la, -2 - la);
}

// KIND 0: the four-wave kernel.  KIND 1: the one-wave kernel of production (BIG): the second-generation core fed by its
// helper waves, nothing else -- its beams always fit the LDS and its filter is always global (the host sees to both).
// KIND 2: the one-wave kernel with every other core (first-generation general cores incl. the unfiltered VamanaIndex
// API's cut step, beams beyond the LDS, the register-resident cores for raw searches): tests, dev switches, rare follow-ups.
// the look-ahead slot recorded for task t (-1: none); -2 = an idle poller's scan is publishing one right now: wait it out (lane 0 only)
__device__ __forceinline__ int la_slot_of(const SearchArgs &A, int t) {
  long long v = __hip_atomic_load(&A.sub_cmps[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int spin = 0; v == -2 && spin < 4096; spin++) {
    __builtin_amdgcn_s_sleep(2);
    v = __hip_atomic_load(&A.sub_cmps[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return v < 0 ? -1 : (int)v;
}

// Tagged filter entries (wave_beam_search_big / _mid): a search takes its slot's next epoch (1 .. 254) and returns the tag of
// its entries (epoch << 24); on wrap-around, or after a search that stored plain ids (epoch 254), the slot's whole region is
// zeroed.  Partitions of more than 2^24 nodes use plain ids (tag 0) and clear what they use to -1.
__device__ __forceinline__ uint32_t next_filter_epoch(const SearchArgs &A, int slot, int32_t *gtable, int bits, int part_n) {
  const int lane = lane_id();
  int e = 0;
  if (lane == 0) e = A.g_epoch[slot];
  e = uni(e);
  uint32_t tag = 0;
  if (part_n <= (1 << 24)) {
    if (e >= 254) {
      int4 *gt = reinterpret_cast<int4 *>(gtable);
      for (int i = lane; i < (1 << (A.g_table_bits - 2)); i += 64) gt[i] = make_int4(0, 0, 0, 0);
      e = 0;
    }
    e++;
    tag = (uint32_t)e << 24;
  } else {
    int4 *gt = reinterpret_cast<int4 *>(gtable);
    for (int i = lane; i < (1 << (bits - 2)); i += 64) gt[i] = make_int4(-1, -1, -1, -1);
    e = 254;
  }
  if (lane == 0) A.g_epoch[slot] = e;
  return tag;
}

template <int METRIC, int KIND WANN_DT_TPARAM>
__global__ __launch_bounds__(KIND == 1 ? 64 * (1 + kHelpers) : (KIND == 2 ? 64 : 64 * kWavesPerBlock),
                             KIND == 1 ? 2 : (KIND == 0 ? ((METRIC == 1 || WANN_BYTE_ROWS) ? WANN_MIPS_WAVES : 2) : 1)) void k_search(SearchArgs A) {
  // (four-wave kernel, inner product / byte rows: three waves per SIMD -- these searches wait for memory two thirds of their
  // time, and a third workgroup per CU is 50 % more loads in flight; the squared-L2 float kernel keeps two 512-B rows per
  // lane pair in flight and stays at two)  // (KIND 0 must stay within 256 VGPRs: two waves per SIMD; an explicit occupancy hint made the schedule 5 % slower)
  constexpr bool BIG = KIND != 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView &ix = A.ix;
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  // four searching waves per workgroup; the one-wave kernel has ONE searching wave (plus, with A.helper, its prefetch helper)
  const int slot = BIG ? (int)blockIdx.x : (int)(blockIdx.x * (blockDim.x >> 6) + wib);
  const int per_wave = wave_lds_common_bytes(qv_words(ix)) + A.pool_bytes;
  unsigned char *base = smem + (BIG ? 0 : (size_t)wib * per_wave);
  // the helper waves' mailbox takes the last bytes of the pool
  ScoreBox *const box = (KIND == 1 && A.helper) ? reinterpret_cast<ScoreBox *>(base + per_wave - kScoreBoxBytes) : nullptr;
  if (KIND == 1 && A.helper) {
    if (wib == 0) {
      int32_t *vb = reinterpret_cast<int32_t *>(box);
      for (int j = lane; j < (int)(sizeof(ScoreBox) / 4); j += 64) vb[j] = 0;
    }
    __syncthreads();  // (the only workgroup barrier of the kernel: the mailbox is initialised before the helpers poll it)
  }
  u64 *gbeam = (KIND == 2 && A.g_beam) ? A.g_beam + (size_t)slot * A.g_beam_cap : nullptr;  // (beams outside the LDS: one-wave kernel only)
  int32_t *const gtable = A.g_table ? A.g_table + ((size_t)slot << A.g_table_bits) : nullptr;
  const int prio = A.prio_count ? *A.prio_count : 0;
  const int heavy = prio + (A.heavy_count ? *A.heavy_count : 0);
  const int mid_end = heavy + (A.mid_count ? *A.mid_count : 0);
  const int total = mid_end + *A.list_count;  // ordinary tickets
  const int pool_bytes = A.pool_bytes - ((KIND == 1 && A.helper) ? kScoreBoxBytes : 0), cap = A.cap_inkernel;
  // BIG: the first npollers workgroups only serve continuations, so that one starts as soon as it is handed over
  bool polling = BIG && A.big_list && (int)blockIdx.x < A.npollers;

  // ordinary launch with a companion: as many ordinary workgroups as there are big items (+ pollers) leave at once, so that
  // the companion's workgroups (launched first, but the LDS of every CU is fully booked by this launch) find room
  // (a companion workgroup and an ordinary one share a CU -- 80 KB of LDS and <= 256 registers each -- so only as many
  // ordinary workgroups leave as companion workgroups have not found their place yet)
  if (BIG && A.big_resident && threadIdx.x == 0) atomicAdd(A.big_resident, 1);
  if (!BIG && A.yield_for_big) {
    // one decision per WORKGROUP (a workgroup whose waves disagree frees nothing: its LDS and registers stay booked): thread 0
    // reads the counter, the others take its word through the LDS
    int *const word = reinterpret_cast<int *>(smem);
    if (threadIdx.x == 0) {
      const int items = A.big_count[0] + A.big_count[1];
      const int need = min(items + A.npollers, (int)gridDim.x / 2);
      *word = ((int)blockIdx.x < need && (int)blockIdx.x >= __hip_atomic_load(A.big_resident, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 1 : 0;
    }
    __syncthreads();
    const int leave = *word;
    __syncthreads();  // (the word is wave 0's query staging area afterwards)
    if (leave) return;
  }

  if (KIND == 1 && A.helper && wib >= 1) {  // a scoring helper wave of this workgroup's search wave
    score_helper<METRIC>(ix, A.g_table ? A.g_table + ((size_t)slot << A.g_table_bits) : nullptr,
                         A.g_seen ? A.g_seen + (size_t)slot * A.g_seen_words : nullptr, A.degree_limit, box,
                         reinterpret_cast<const float *>(base), wib - 1);
    return;
  }
  for (;;) {
    int ti;
    bool dyn = false;
    if (BIG && !polling && A.big_list) {
      const int big_first = A.big_count[0], big_total = big_first + A.big_count[1];
      const int t = wave_ticket(A.big_cursor);
      if (t >= big_total) {
        // the static list is done: this workgroup joins the pollers (continuations, look-aheads) instead of leaving --
        // the chains that outgrow their levels show up in the second half of a batch, when most of the list is done
        // (only where there was a list: the pollers of a launch without one -- the deep chains' -- book whole CUs)
        if (big_total > 0 && A.npollers > 0 && A.dyn_list && !A.force_poll_timeout) {
          polling = true;
          continue;
        }
        break;
      }
      ti = (t < big_first) ? A.big_list[t] : A.big_list[A.big_stride + t - big_first];
    } else if (BIG && polling) {
      // wait for continuation number d, or for the end of all ordinary work (a producer publishes its item
      // before it reports its ticket done, so the item count is final once done_count == total)
      const int d = wave_ticket(A.dyn_cursor);
      int item = -1;
      bool settled = false;
      // Bounded wait.  The producers are waves of a DIFFERENT launch; HIP does not promise that the two launches are
      // resident together (a shared hardware queue, HIP_LAUNCH_BLOCKING / AMD_SERIALIZE_KERNEL, rocprofv3 --pmc all
      // serialise them).  A poller gives up soon when no ordinary wave has ever taken a ticket (the other launch has
      // not started: it may be queued BEHIND this one) and after a long bound otherwise; whatever it leaves unserved
      // stays in dyn_list (entries >= 0) and the host hands it to a follow-up launch (run_batch).
      const int spins = A.force_poll_timeout ? 0 : (1 << 22);
      // (producers hand chains and look-aheads over only while a poller is known to wait: a ticket of dyn_cursor that its
      // poller has abandoned -- end of the ordinary work, serialised launches, a timeout -- would look idle for ever)
      if (lane == 0 && spins) __hip_atomic_fetch_add(A.poll_waiting, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int spin = 0; spin < spins; spin++) {
        int have = 0, fin = 0, idle = 0;
        if (lane == 0) {
          // relaxed device-scope atomics: served by the memory side, no cache invalidation per poll
          fin = __hip_atomic_load(A.done_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= total;
          have = __hip_atomic_load(A.dyn_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > d;
          if (have) item = __hip_atomic_load(A.dyn_list + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (spin >= (1 << 12) && (spin & 255) == 0)
            idle = total > 0 && __hip_atomic_load(A.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
        }
        item = uni(item);
        if (item >= 0 || item <= -2 || (uni(fin) && !uni(have))) {
          settled = true;
          break;
        }
        if (uni(idle)) break;  // serialised dispatch: nobody will produce while this launch occupies the queue
        // An idle poller looks for chains that will outgrow their speculated levels: a speculating task whose level at half
        // (a quarter) of its highest beam has finished with at most k/2 (k/5) in-window entries while the highest level has
        // not succeeded gets the level AFTER the highest one searched now, as a look-ahead (see below), instead of when its
        // last level has failed -- by then the launch is all but over and that search runs alone for as long again.  If the
        // highest level succeeds after all, the wave that resolves the task calls the look-ahead off (it stops within 32
        // hops).  The four-wave kernel, where the small levels finish, has no registers to spare; here a wave waits anyway.
        if (A.scan_list && (spin & 63) == 32) {
          // (every waiting poller goes over the whole list -- k_route keeps it to the tasks with levels in the companion
          // launch -- from a place of its own: a task waits for no particular poller to be idle)
          const int nscan = *A.scan_count;
          const int first = (int)(((long long)((int)blockIdx.x % A.npollers) * nscan / A.npollers) & ~63ll);
          for (int i0 = 0; i0 < nscan; i0 += 64) {
            int i = first + i0 + lane;
            if (i >= ((nscan + 63) & ~63)) i -= (nscan + 63) & ~63;
            if (i >= nscan) continue;
            const int p = A.scan_list[i];
            const int nsub = (int)A.tasks[p].a, sbase = (int)A.tasks[p].b;
            const long long top = (long long)A.B << (nsub - 1);
            if (nsub < 3 || top < A.scan_min_top || 2 * top > A.big_cap || 2 * top >= A.max_beam) continue;
            if (__hip_atomic_load(&A.sub_cmps[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != -1) continue;
            const int ft = __hip_atomic_load(&A.out_cnt[sbase + nsub - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ft >= A.stop_k) continue;  // (out_cnt of a sub-task slot is -1 until its search has finished)
            // the highest level has failed -- or the largest lower level that has finished (down to an eighth of the highest
            // beam) found so little that the highest one is expected to find at most k: in-window entries scale with the beam
            bool deeper = ft >= 0;
            for (int r = nsub - 2; !deeper && r >= 0 && r >= nsub - 4; r--) {
              const int f = __hip_atomic_load(&A.out_cnt[sbase + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (f >= 0) {
                deeper = ((long long)f << (nsub - 1 - r)) * 8 <= (long long)A.stop_k * A.scan_num;
                break;
              }
            }
            if (!deeper) continue;
            if (atomicCAS((unsigned long long *)&A.sub_cmps[p], ~0ull, ~1ull) != ~0ull) continue;  // one per task
            const int at = atomicAdd(A.la_count, 1);
            if (A.la_base0 + at >= A.la_cap) {  // out of look-ahead slots: -2 must only ever mean "publishing right now" (la_slot_of waits it out)
              A.sub_cmps[p] = -3;
              continue;
            }
            atomicAdd(&A.ctr->lookaheads_issued, 1ull);
            const int sl = A.la_base0 + at;
            Task t = A.tasks[sbase];
            t.flags = (t.flags & ~1) | 4 | 16;
            t.a = 2 * top;
            t.b = p;
            A.tasks[sl] = t;
            A.par_done[sl] = 0;
            __threadfence();
            const int dd = atomicAdd(A.dyn_count, 1);
            A.next_beam[sl] = dd;
            A.sub_cmps[p] = sl;
            __hip_atomic_store(A.dyn_list + dd, sl, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        __builtin_amdgcn_s_sleep(32);
      }
      if (lane == 0 && spins) __hip_atomic_fetch_add(A.poll_waiting, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!settled && lane == 0) atomicAdd(&A.ctr->poll_timeouts, 1ull);
      if (item <= -2) continue;  // a look-ahead its producer has withdrawn: next ticket
      if (item < 0) break;  // nothing more can arrive (or given up)
      if (lane == 0) __hip_atomic_store(A.dyn_list + d, -2 - item, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // served
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the producer's writes (next_beam) before its publication
      ti = item;
      dyn = true;
    } else {
      const int t = wave_ticket(A.cursor);
      if (t >= total) break;
      ti = (t < prio) ? A.prio_list[A.heavy_cap - 1 - t]
           : (t < heavy) ? A.heavy_list[t - prio] : (t < mid_end) ? A.mid_list[t - heavy] : A.list[t - mid_end];  // evidence, then long searches, first
    }
    // (the task's fields are read where they are used, not kept in scalar registers across the searches)
    // (wave-uniform values that come from vector / atomic loads are moved to scalar registers explicitly: left to itself the
    // compiler keeps everything derived from them -- beam sizes, list lengths, the whole bookkeeping of a hop -- in vector
    // registers under exec masks)
    PartDesc part = ix.parts[uni(A.tasks[ti].part)];
    part.row_base = uni64(part.row_base);
    part.start = uni(part.start);
    part.n = uni(part.n);
    const int64_t qrow = uni(A.tasks[ti].query);
    const int64_t qid = uni64(A.raw_qids ? A.raw_qids[qrow] : (A.qid_base + qrow));  // (per-query ids: raw searches, wann_batch_search_device_ids)
    const int64_t row_off = part.start;

    long long b = A.B;
    bool final_pass = A.is_final != 0;
    bool sub = (A.tasks[ti].flags & 4) != 0;  // speculative sub-task: ONE search at beam B << level
    if (A.tasks[ti].flags & 16) {  // a look-ahead: ONE search for a chain that runs elsewhere (see below)
      sub = true;
      b = A.tasks[ti].a;  // (the beam itself)
      if (__hip_atomic_load(&A.par_done[ti], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 2) continue;  // withdrawn already
    } else if (BIG && dyn) {  // a continuation: a plain task or a resolved parent, at the beam its producer recorded
      sub = false;
      b = __hip_atomic_load(A.next_beam + ti, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (sub) b = (long long)A.B << (int)A.tasks[ti].a;
    else if (A.start_beam) b = A.start_beam[ti];
    // A speculated level is MOOT once a lower level of its task has found stop_k entries (the sequential loop stops at the first
    // such level, postfilter_vamana.h:161-172): it is not searched (here) or stops at its next check (one-wave core).  The
    // lowest successful level of a task is kept in sub_hops[parent] (the host presets it to a huge value per batch).
    const bool spec_level = sub && !(A.tasks[ti].flags & 16);
    const int my_level = spec_level ? (int)A.tasks[ti].a : 0;
    long long *moot_word = spec_level ? &A.sub_hops[A.tasks[ti].b] : nullptr;  // (cleared when this wave carries on as the resolved parent)
    bool moot = false;
    if (spec_level) {
      int mt = 0;
      if (lane == 0) mt = __hip_atomic_load(moot_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < my_level;
      moot = uni(mt) != 0;
    }
    for (;;) {  // postfilter_vamana.h:161-181
      // Look-ahead: a chain that has just failed a level badly (it found less than 0.4 k entries: the next level will most
      // likely fail too) has its level AFTER the next searched by an idle poller while this wave searches the next one --
      // every level restarts from scratch anyway (postfilter_vamana.h:161-172).  The sequential rule is applied afterwards:
      // if the next level fails, the level after it is taken from the look-ahead instead of being searched -- by a poller
      // (one-wave kernel: a four-wave chain with a look-ahead out moves to a poller when its level fails).
      // (what the chain's previous level found is still in out_cnt; the look-ahead's slot is kept in sub_cmps[ti], its queue
      // position in next_beam[slot]: scalar registers are scarce in the four-wave kernel)
      bool took = false;
      int took_found = 0;
      if (BIG && A.la_count && !sub) {
        int la = -1;
        if (lane == 0) la = la_slot_of(A, ti);
        la = uni(la);
        if (la >= 0) {
          int st = 0;
          if (A.tasks[la].a == b && !final_pass)
            for (int spin = 0; spin < (1 << 18); spin++) {
              if (lane == 0) {
                st = __hip_atomic_load(&A.par_done[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // still in the queue after a few milliseconds: no poller is coming (serialised launches, a profiler)
                if (st != 1 && spin >= 4096 && (spin & 255) == 0 &&
                    __hip_atomic_load(A.dyn_list + A.next_beam[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == la)
                  st = 3;
              }
              st = uni(st);
              if (st == 1 || st == 3) break;
              __builtin_amdgcn_s_sleep(32);
            }
          if (st == 1) {  // this level has been searched already: take its result
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            took = true;
            took_found = __hip_atomic_load(&A.out_cnt[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int j = lane; j < took_found; j += 64)
              A.out_key[(size_t)ti * A.k + j] = __hip_atomic_load(&A.out_key[(size_t)la * A.k + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lane == 0) {
              A.out_cnt[ti] = took_found;
              atomicAdd(&A.ctr->beam_searches, 1ull);
              atomicAdd(&A.ctr->hops, (unsigned long long)__hip_atomic_load(&A.sub_hops[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
              atomicAdd(&A.ctr->dist_cmps, (unsigned long long)__hip_atomic_load(&A.sub_cmps[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
              atomicAdd(&A.ctr->lookaheads_used, 1ull);
            }
          } else if (lane == 0)
            la_withdraw(A, la);
        }
      }
      if (A.la_count && !sub && lane == 0) A.sub_cmps[ti] = -1;
      if (A.la_count && !sub && !took && !final_pass && !A.raw && A.npollers > 0 && b >= A.la_min_beam && b > A.B &&
          2 * b <= A.big_cap && 2 * b < A.max_beam) {
        if (lane == 0 && __hip_atomic_load(&A.out_cnt[ti], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < A.la_found_max &&
            __hip_atomic_load(A.poll_waiting, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) {
          const int at = atomicAdd(A.la_count, 1);
          if (A.la_base0 + at < A.la_cap) {
            atomicAdd(&A.ctr->lookaheads_issued, 1ull);
            const int sl = A.la_base0 + at;
            Task t = A.tasks[ti];
            t.flags = (t.flags & ~1) | 4 | 16;
            t.a = 2 * b;
            t.b = ti;
            A.tasks[sl] = t;
            A.par_done[sl] = 0;
            A.sub_cmps[ti] = sl;
            __threadfence();
            const int dd = atomicAdd(A.dyn_count, 1);
            A.next_beam[sl] = dd;
            __hip_atomic_store(A.dyn_list + dd, sl, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
      b = uni64(b);
      const int B = (int)b;
      const int bits = hash_bits_dev(b);
      const int beam_bytes = ((B + 1) & ~1) * 8;
      const bool beam_lds = beam_bytes <= pool_bytes;
      const bool table_lds = beam_lds && (beam_bytes + (4 << bits) <= pool_bytes);
      WaveLds L = carve_wave_lds(base, qv_words(ix), B, beam_lds);
      // stage the query (zero padded); every search restarts from scratch
      for (int i = lane; i < qv_words(ix); i += 64) L.qv[i] = stage_query_word(A.queries, qrow, i, ix.d);
      WAVE_SYNC();
      int m;
      long long nvis, ncmp;
#ifdef WANN_TASK_TRACE
      const long long trace_t0 = A.trace ? (long long)wall_clock64() : 0;
#endif
      // the part of the pool that the beam leaves free serves as the clash-detection scratch of the general cores
      int32_t *mini = nullptr;
      uint32_t mini_mask = 0;
      const int free_words = beam_lds ? (pool_bytes - beam_bytes) >> 2 : 0;
      if (free_words >= 1024 && !A.force_general) {
        mini = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(L.lbeam) + beam_bytes);
        mini_mask = (1u << (31 - __builtin_clz((unsigned)free_words))) - 1u;
      }
      const bool small_ok = table_lds && !A.force_general;
      if (took || moot) {  // (searched ahead by a poller / a lower level has settled the task)
        m = 0;
        nvis = ncmp = 0;
      } else if (KIND != 1 && small_ok && B <= 64)
        wave_beam_search_small<METRIC, 1>(ix, part, L, B, bits, qid, A.limit, A.degree_limit, m, nvis, ncmp, A.prof);
      else if (KIND != 1 && small_ok && B <= 128)
        wave_beam_search_small<METRIC, 2>(ix, part, L, B, bits, qid, A.limit, A.degree_limit, m, nvis, ncmp, A.prof);
      else if (KIND == 0 && beam_lds && gtable && A.g_epoch) {
        // Four-wave kernel, beams 129 .. cap_inkernel: the third-generation general core (round 5) -- rows, filter probes and
        // vectors in flight across hops, the next hop committed before this hop's union.  (Rounds 2 - 4 ran the first-generation
        // core here: three dependent round trips + union per hop, 5.5 us a hop, 10 under load; the second-generation core without
        // its helper waves lost 10-15 % against it.)
        const uint32_t tag = next_filter_epoch(A, slot, gtable, bits, part.n);
        // behind the beam: the "slot written" bitmap of the filter (a bit per slot if the pool allows, else per 2 / 4 / ... slots),
        // then the slot-sharing test's scratch
        uint32_t *wbits = nullptr;
        int wwords = 0, wshift = 0;
        {
          const int avail = (pool_bytes - beam_bytes) >> 2;  // 32-bit words
          const int want_log = bits > 5 ? bits - 5 : 0;
          int bm_log = want_log;
          while (bm_log > 0 && (1 << bm_log) > avail - (A.force_general ? 0 : 256)) bm_log--;
          if ((1 << bm_log) <= avail - (A.force_general ? 0 : 256)) {
            wbits = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(L.lbeam) + beam_bytes);
            wwords = 1 << bm_log;
            wshift = want_log - bm_log;
            const int rest = avail - wwords;
            if (rest >= 256 && !A.force_general) {
              mini = reinterpret_cast<int32_t *>(wbits + wwords);
              mini_mask = (1u << (31 - __builtin_clz((unsigned)rest))) - 1u;
            } else
              mini = nullptr;
          }
        }
        if (!mini) {  // no room beside the beam: the merge scratch (unused during the filter step) serves
          mini = reinterpret_cast<int32_t *>(L.cand_key);
          mini_mask = 127u;
        }
        // (rows of 128 floats under squared L2 -- the SIFT shape -- get the core with its block count compiled in: no branch per
        // 16-byte block of a row, twice per hop)
        if (METRIC == 0 && !WANN_BYTE_ROWS && RowRegsFor<METRIC>::NR >= 16 && uni(row_regs_blocks<METRIC>(ix)) == 16)
          wave_beam_search_mid<METRIC, (METRIC == 0 && !WANN_BYTE_ROWS) ? 16 : 0>(ix, part, L, gtable, tag, B, bits, qid, A.limit, A.degree_limit, mini, mini_mask, m, nvis, ncmp, A.prof, wbits, wwords, wshift);
        else
          wave_beam_search_mid<METRIC>(ix, part, L, gtable, tag, B, bits, qid, A.limit, A.degree_limit, mini, mini_mask, m, nvis, ncmp, A.prof, wbits, wwords, wshift);
      } else if (KIND == 1 && beam_lds && A.g_seen && gtable) {
        // Second-generation general core.  Tagged filter entries: this search takes the slot's next epoch; on
        // wrap-around (or after a search that stored plain ids) the slot's whole region is zeroed.  Partitions of
        // more than 2^24 nodes use plain ids and clear what they use.
        const uint32_t tag = next_filter_epoch(A, slot, gtable, bits, part.n);
        if (!mini) {  // no room beside the beam: the merge scratch (unused during the filter step) serves
          mini = reinterpret_cast<int32_t *>(L.cand_key);
          mini_mask = 127u;
        }
        wave_beam_search_big<METRIC>(ix, part, L, gtable, tag, A.g_seen + (size_t)slot * A.g_seen_words, B, bits, qid, A.limit,
                                     A.degree_limit, mini, mini_mask, m, nvis, ncmp, A.prof, box, A.tasks[ti].part,
                                     (sub && (A.tasks[ti].flags & 16)) ? &A.par_done[ti] : nullptr, A.ctr, moot_word, my_level);
      } else if (KIND == 2) {
        // First-generation general cores: only in the second one-wave-per-workgroup kernel (512 registers per wave), which
        // serves the test / dev switches, the cut step and beams beyond the LDS.
        if (A.g_epoch && lane == 0) A.g_epoch[slot] = 254;  // plain ids go into the table: the next tagged search clears it
        uint32_t *const vset = (A.cut_k > 0 && A.g_seen) ? A.g_seen + (size_t)slot * A.g_seen_words : nullptr;
        if (A.cut_k > 0 && beam_lds)  // unfiltered VamanaIndex queries: the k / cut step (global filter: the host forces one)
          wave_beam_search<METRIC, false, true, false, true>(ix, part, L, nullptr, gtable, B, bits, qid, A.limit, A.degree_limit,
                                                             nullptr, 0, m, nvis, ncmp, A.prof, mini, mini_mask, A.cut_k, A.cut, vset);
        else if (table_lds)
          wave_beam_search<METRIC, true, true, false>(ix, part, L, nullptr, nullptr, B, bits, qid, A.limit, A.degree_limit,
                                                      nullptr, 0, m, nvis, ncmp, A.prof);
        else if (beam_lds)
          wave_beam_search<METRIC, false, true, false>(ix, part, L, nullptr, gtable, B, bits, qid, A.limit, A.degree_limit,
                                                       nullptr, 0, m, nvis, ncmp, A.prof, mini, mini_mask);
        else
          wave_beam_search<METRIC, false, false, false>(ix, part, L, gbeam, gtable, B, bits, qid, A.limit, A.degree_limit,
                                                        nullptr, 0, m, nvis, ncmp, A.prof);
      } else {
        // (the host never gives the four-wave kernel a beam that needs one of those: see config_for)
        m = 0;
        nvis = ncmp = 0;
        if (lane == 0) atomicAdd(&A.ctr->unsupported, 1ull);
      }
      auto beam_ld = [&](int i) -> u64 { return (KIND != 2 || beam_lds) ? L.lbeam[i] : gbeam[i]; };
#ifdef WANN_TASK_TRACE
      const long long trace_t1 = A.trace ? (long long)wall_clock64() : 0;
#endif
      if (lane == 0 && !took) {
        if (sub) {  // attributed when the parent is resolved
          A.sub_hops[ti] = nvis;
          A.sub_cmps[ti] = ncmp;
        } else {
          atomicAdd(&A.ctr->beam_searches, 1ull);
          atomicAdd(&A.ctr->hops, (unsigned long long)nvis);
          atomicAdd(&A.ctr->dist_cmps, (unsigned long long)ncmp);
        }
      }
      if (A.raw) {  // dump the whole beam (ids local to the partition)
        for (int x = lane; x < m; x += 64) {
          u64 e = beam_ld(x);
          A.raw_ids[qrow * B + x] = (int)((uint32_t)e >> 1);
          A.raw_dists[qrow * B + x] = funkey((uint32_t)(e >> 32));
        }
        if (lane == 0) {
          A.raw_sizes[qrow] = m;
          A.raw_hops[qrow] = nvis;
          A.raw_cmps[qrow] = ncmp;
        }
        break;
      }
      // ---- post filter: keep beam entries whose label lies in [lo,hi], first k of them (k: the row's columns; whether the
      //      level has ENOUGH is decided on stop_k <= k below -- wann.h WIDE ROWS: equal but for the wide calls)
      //      (postfilter_vamana.h:234-251); ids become sorted-order indices (subset[local])
      int found = 0;
      long long labs = 0;
      const float win_lo = A.tasks[ti].lo, win_hi = A.tasks[ti].hi;
      const bool vfull = KIND == 2 && A.vlog != nullptr;  // verbose: the reference prints the size of the whole filtered frontier
      for (int bx = 0; bx < m && (found < A.k || vfull); bx += 64) {
        int x = bx + lane;
        bool act = x < m;
        u64 e = act ? beam_ld(x) : 0ull;
        int lid = (int)((uint32_t)e >> 1);
        float lab = act ? ix.labels[row_off + lid] : 0.f;
        bool inw = act && (lab >= win_lo) && (lab <= win_hi);
        u64 im = ballot64(inw);
        int idx = found + popc64(im & lanemask_lt());
        if (inw && idx < A.k)
          A.out_key[(size_t)ti * A.k + idx] = (e & 0xffffffff00000000ull) | (uint32_t)(row_off + lid);
        found += popc64(im);
        labs += (m - bx) < 64 ? (m - bx) : 64;
      }
      if (vfull && lane == 0 && !took && !sub) {
        const int vn = atomicAdd(&A.vlog_n[ti], 1);
        if (vn < A.vlog_cap) A.vlog[(size_t)ti * A.vlog_cap + vn] = ((u64)(uint32_t)B << 42) | ((u64)(uint32_t)m << 21) | (u64)(uint32_t)found;
      }
      if (found > A.k) found = A.k;
      if (lane == 0 && !took) {
        A.out_cnt[ti] = found;
        atomicAdd(&A.ctr->label_reads, (unsigned long long)labs);
      }
      if (took) found = took_found;
#ifdef WANN_TASK_TRACE
      if (A.trace && lane == 0 && !took) {  // task | what it found | sub / big flags, beam | parent of a sub-task, start, end
        long long *rec = A.trace + 1 + 4 * atomicAdd((unsigned long long *)A.trace, 1ull);
        rec[0] = ti | ((long long)(found < 255 ? found : 255) << 32) | (sub ? 1ll << 40 : 0) | (BIG ? 1ll << 41 : 0);
        rec[1] = B | (sub ? (long long)A.tasks[ti].b << 32 : 0);
        rec[2] = trace_t0;
        rec[3] = trace_t1;
      }
#endif
      WAVE_SYNC();
      if (sub && (A.tasks[ti].flags & 16)) {
        // a look-ahead is done: the chain's wave takes the result (or has withdrawn: then this was speculation)
        __threadfence();
        int old_state = 0;
        if (lane == 0) {
          old_state = atomicExch(&A.par_done[ti], 1);
          if (old_state == 2) {
            atomicAdd(&A.ctr->spec_searches, 1ull);
            atomicAdd(&A.ctr->spec_hops, (unsigned long long)nvis);
            atomicAdd(&A.ctr->spec_dist_cmps, (unsigned long long)ncmp);
          }
        }
        break;
      }
      if (A.la_count && !sub && (found >= A.stop_k || final_pass)) {  // the chain ends here: a look-ahead of its next level is not needed
        if (lane == 0) {
          const int la = la_slot_of(A, ti);
          if (la >= 0) {
            la_withdraw(A, la);
            A.sub_cmps[ti] = -1;
          }
        }
      }
      if (sub) {
        // Publish this level, then the LAST sub-task to finish replays the sequential rule over the
        // levels: the result is that of the first level with >= stop_k in-window entries (or of the last
        // level), exactly what the doubling loop returns; it then continues as the parent.
        const int parent = (int)A.tasks[ti].b;
        // a level that has found stop_k entries makes every higher level of its task moot (see above)
        if (found >= A.stop_k && !moot && lane == 0) atomicMin((unsigned long long *)&A.sub_hops[parent], (unsigned long long)my_level);
        // ... and settles that the chain will not go beyond its speculated levels: a look-ahead an
        // idle poller is running for it (the pollers' scan) is called off NOW, not when the slowest level has finished --
        // the poller is free for the next chain that needs one; the scan leaves the task alone from now on (a moot top level
        // reports nothing found: that must not look like a failed one)
        if (A.la_count && found >= A.stop_k && lane == 0) {
          const int la = la_slot_of(A, parent);
          if (la >= 0) {
            la_withdraw(A, la);
            A.sub_cmps[parent] = -3;  // (withdrawn: neither the scan nor the resolver touches it again)
          } else {
            // (the operands are formed HERE: as plain constants the compiler set the pair up at kernel entry and held four vector
            // registers for it through every core -- in the float32 unit's k_search<0, 0>, which sits at the 256-register limit,
            // the first thing to go to scratch)
            unsigned long long none = ~0ull;
            asm volatile("" : "+v"(none));
            atomicCAS((unsigned long long *)&A.sub_cmps[parent], none, none - 2);  // -1 (none) -> -3
          }
        }
        __threadfence();
        int old_done = 0;
        if (lane == 0) old_done = atomicAdd(&A.par_done[parent], 1);
        old_done = uni(old_done);
        const int nsub = (int)A.tasks[parent].a, sbase = (int)A.tasks[parent].b;
        if (old_done + 1 != nsub) break;  // not the last one: take the next ticket
        __threadfence();
        int succ = -1;
        for (int r = 0; r < nsub; r++)
          if (__hip_atomic_load(&A.out_cnt[sbase + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= A.stop_k) {
            succ = r;
            break;
          }
        const int upto = succ >= 0 ? succ : nsub - 1;
        if (A.la_count && succ >= 0 && lane == 0) {  // a look-ahead beyond the speculated levels is not needed after all
          const int la = la_slot_of(A, parent);
          if (la >= 0) {
            la_withdraw(A, la);
            A.sub_cmps[parent] = -1;
          }
        }
        if (lane == 0) {
          unsigned long long h0 = 0, c0 = 0, h1 = 0, c1 = 0;
          for (int r = 0; r < nsub; r++) {
            const unsigned long long hh = (unsigned long long)__hip_atomic_load(&A.sub_hops[sbase + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long cc = (unsigned long long)__hip_atomic_load(&A.sub_cmps[sbase + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (r <= upto) {
              h0 += hh;
              c0 += cc;
            } else {
              h1 += hh;
              c1 += cc;
            }
          }
          atomicAdd(&A.ctr->beam_searches, (unsigned long long)(upto + 1));
          atomicAdd(&A.ctr->hops, h0);
          atomicAdd(&A.ctr->dist_cmps, c0);
          atomicAdd(&A.ctr->spec_searches, (unsigned long long)(nsub - 1 - upto));
          atomicAdd(&A.ctr->spec_hops, h1);
          atomicAdd(&A.ctr->spec_dist_cmps, c1);
        }
        found = __hip_atomic_load(&A.out_cnt[sbase + upto], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int j = lane; j < found; j += 64)
          A.out_key[(size_t)parent * A.k + j] =
              __hip_atomic_load(&A.out_key[(size_t)(sbase + upto) * A.k + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) A.out_cnt[parent] = found;
        WAVE_SYNC();
        ti = parent;
        sub = false;
        moot_word = nullptr;  // (what follows -- the final re-search, further doublings -- is the parent's own chain, never moot)
        moot = false;
        b = (long long)A.B << upto;
      }
      if (final_pass) break;
      if (found >= A.stop_k) {  // doubling loop ends here (postfilter_vamana.h:161-172); final re-search?
        long long fb = b * ((A.tasks[ti].flags & 2) ? 1 : A.mult);
        if (fb > A.max_beam) fb = A.max_beam;
        if (fb <= b) break;
        if (fb <= cap) {
          b = fb;
          final_pass = true;
          continue;
        }
        if (lane == 0) {
          int at = atomicAdd(A.final_count, 1);
          A.final_list[at] = ti;
          A.next_beam[ti] = (int32_t)fb;
        }
        break;
      }
      const long long nb = 2 * b;
      if (nb >= A.max_beam) break;  // cannot double any more: the short result stands
      if (nb > cap) {
        if (lane == 0) {
          if (A.next_beam) A.next_beam[ti] = (int32_t)nb;
          if (!BIG && A.npollers > 0 && nb <= A.big_cap) {  // to a poller of the companion launch
            __threadfence();
            const int d = atomicAdd(A.dyn_count, 1);
            __hip_atomic_store(A.dyn_list + d, ti, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          } else {
            A.next_list[atomicAdd(A.next_count, 1)] = ti;
          }
        }
        break;
      }
      if (!BIG && A.npollers > 0 && nb <= A.big_cap && ((A.handoff_beam > 0 && nb >= A.handoff_beam) || A.la_count)) {
        int go = 0;
        if (lane == 0) {
          // a look-ahead of level nb is out: a poller takes it over with the chain.  Otherwise (deep chains): a poller is waiting
          go = A.la_count && A.sub_cmps[ti] >= 0;
          if (!go && A.handoff_beam > 0 && nb >= A.handoff_beam)
            go = __hip_atomic_load(A.poll_waiting, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0;
          if (go) {
            A.next_beam[ti] = (int32_t)nb;
            __threadfence();
            const int d = atomicAdd(A.dyn_count, 1);
            __hip_atomic_store(A.dyn_list + d, ti, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(&A.ctr->deep_handoffs, 1ull);
          }
        }
        if (uni(go)) break;
      }
      b = nb;
    }
    if (!BIG && A.done_count) {
      WAVE_SYNC();
      // relaxed: a continuation is published by an atomic whose result this wave has already waited for, so it
      // is counted in dyn_count before this ticket is counted as done; no cache write-back per ticket
      if (lane == 0) __hip_atomic_fetch_add(A.done_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (KIND == 1 && box && lane == 0) lds_box(box)->gen = -1;  // the helper waves leave too
}

// --------------------------------------------------------------------------------------------
// k_brute: exact top-k over rows [a,b) of the sorted order (T_BRUTE) or over the label-argsort
// positions [a,b) of an unsorted point set (T_BRUTE_GATHER, prefiltering.h:189-194)
// The unit of the one-byte shadow rows and the float16 unit serve the shadow views of a float32 index under wann_set_scan_rows:
// the half view takes the plain k_brute of its own unit (wann_kernels_h16.hip: the float16 unit's, on paired rows).
// k_brute_staged (the one-byte unit): the rows of a pass -- contiguous in a T_BRUTE task -- reach the lane pairs through the
// LDS: scan_fetch (wann_device.h) copies the span with 16-byte loads, and wave_distances scores a view of the staging area, the
// same routines on the same blocks in the same order.  (On the half view the same fetch lost to the plain one: DESIGN.md 3.4.)
// --------------------------------------------------------------------------------------------
// The float8 unit holds both: the staged kernel for the sorted kinds, whose T_BRUTE rows are contiguous, and the plain one for
// the PrefilterIndex, whose T_BRUTE_GATHER rows are not (scan_staged, wann_device.h, chooses) -- the same routines on the
// same blocks either way.
#define WANN_SCAN_STAGED WANN_QUAD_ROWS
#define WANN_SCAN_PLAIN (WANN_DT != 6)
#if WANN_SCAN_PLAIN
template <int METRIC>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_brute(BruteArgs A) {
#define WANN_BRUTE_STAGED 0
#include "wann_brute_body.inc"
#undef WANN_BRUTE_STAGED
}
#endif
#if WANN_SCAN_STAGED
template <int METRIC>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_brute_staged(BruteArgs A) {
#define WANN_BRUTE_STAGED 1
#include "wann_brute_body.inc"
#undef WANN_BRUTE_STAGED
}
#endif

}  // namespace WANN_DT_NS

#if WANN_DT == 0
// --------------------------------------------------------------------------------------------
// k_route: one thread per query
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t first_ge(const float *fv, int64_t n, float v) {  // tree_utils.h:19-37
  if (fv[0] >= v) return 0;
  int64_t s = 0, e = n;
  while (s + 1 < e) {
    int64_t mid = (s + e) / 2;
    if (fv[mid] >= v) e = mid;
    else s = mid;
  }
  return e;
}

// the two lower bounds of a window with their probes issued together: two independent chains of ~log2(n)
// dependent loads cost the latency of one
__device__ __forceinline__ void first_ge2(const float *fv, int64_t n, float v1, float v2, uint64_t &r1, uint64_t &r2) {
  const float f0 = fv[0];
  int64_t s1 = 0, e1 = n, s2 = 0, e2 = n;
  if (f0 >= v1) e1 = 0;  // (tree_utils.h:20-22: index 0 is special-cased)
  if (f0 >= v2) e2 = 0;
  while (s1 + 1 < e1 || s2 + 1 < e2) {
    const bool g1 = s1 + 1 < e1, g2 = s2 + 1 < e2;
    const int64_t m1 = (s1 + e1) / 2, m2 = (s2 + e2) / 2;
    const float x1 = g1 ? fv[m1] : 0.f, x2 = g2 ? fv[m2] : 0.f;
    if (g1) {
      if (x1 >= v1) e1 = m1;
      else s1 = m1;
    }
    if (g2) {
      if (x2 >= v2) e2 = m2;
      else s2 = m2;
    }
  }
  r1 = (uint64_t)e1;
  r2 = (uint64_t)e2;
}

// prefiltering.h:159-184 (r = n-1: the last point can never be selected), both ends of a window at once: the two searches'
// loads are in flight together.  (A sixteen-way search -- five dependent round trips instead of twenty -- was no faster: what
// the route of a PrefilterIndex batch waits for is the last few levels' cold lines, 17 us either way.)
__device__ __forceinline__ void prefilter_bounds(const float *fv, int64_t n, float lo, float hi, int64_t &a, int64_t &b) {
  int64_t l1 = 0, r1 = n - 1, l2 = 0, r2 = n - 1;
  while (l1 < r1 || l2 < r2) {
    const int64_t m1 = (l1 + r1) / 2, m2 = (l2 + r2) / 2;
    float f1 = 0.f, f2 = 0.f;
    if (l1 < r1) f1 = fv[m1];
    if (l2 < r2) f2 = fv[m2];
    if (l1 < r1) {
      if (f1 < lo) l1 = m1 + 1;
      else r1 = m1;
    }
    if (l2 < r2) {
      if (f2 < hi) l2 = m2 + 1;
      else r2 = m2;
    }
  }
  a = l1;
  b = l2;
}

// ---- task emission: a query owns the slots tasks[q*maxt .. q*maxt+maxt) ---------------------------
struct Emitter {
  const RouteArgs &A;
  int64_t q;
  int n;
  bool exact;  // the query is one exact-window task (wann_set_exact_windows)
  __device__ Emitter(const RouteArgs &a, int64_t qq) : A(a), q(qq), n(0), exact(false) {}
  // QueryParams::verbose: one entry of the descent's dump (RouteArgs::vroute)
  __device__ __forceinline__ void note(int64_t kind, int64_t a = 0, int64_t b = 0, int64_t c = 0, int64_t d = 0, int64_t size = 0) {
    if (!A.vroute) return;
    int64_t *base = A.vroute + q * kVRouteWords;
    const int64_t used = base[0];
    if (used + 7 > kVRouteWords - 1) return;
    int64_t *e = base + 1 + used;
    e[0] = kind;
    e[1] = n;
    e[2] = a;
    e[3] = b;
    e[4] = c;
    e[5] = d;
    e[6] = size;
    base[0] = used + 7;
  }
  __device__ __forceinline__ void push(const Task &t) {
    if (t.mode == T_EMPTY) return;
    if (n >= A.maxt) {  // the host raises an error for the batch
      atomicAdd(&A.ctr->unsupported, 1ull);
      return;
    }
    const int32_t ti = (int32_t)(q * A.maxt + n);
    n++;
    A.tasks[ti] = t;
    if (t.mode == T_GRAPH) {
      if (t.flags & 1) A.heavy_list[atomicAdd(A.heavy_count, 1)] = ti;
      else if (t.flags & 8) A.mid_list[atomicAdd(A.mid_count, 1)] = ti;
      else A.graph_list[atomicAdd(A.graph_count, 1)] = ti;
    } else if (!((t.flags & kTaskExactWindow) && A.exact_unlisted)) {  // (the dense path lists the exact windows it leaves to the scan)
      A.brute_list[atomicAdd(A.brute_count, 1)] = ti;
    }
  }
  // SpatialIndex::query on partition pidx for window [lo,hi]: the post-filter loop on a Vamana
  // leaf (postfilter_vamana.h:141-188), brute force on a PrefilterIndex leaf (prefiltering.h:154-204)
  __device__ __forceinline__ void leaf(int32_t pidx, float lo, float hi, uint64_t w, bool mult_one) {
    const IndexView &ix = A.ix;
    Task t;
    t.query = (int32_t)q;
    t.part = pidx;
    t.flags = 0;
    t.a = (int64_t)w;  // (a plain graph task keeps its window's size here: k_task_cost; sub-tasks and parents overwrite it)
    t.b = 0;
    t.lo = lo;
    t.hi = hi;
    const PartDesc pd = ix.parts[pidx];
    if (ix.vamana_leaves) {
      t.mode = (A.beam < A.max_beam) ? T_GRAPH : T_EMPTY;  // postfilter_vamana.h:161: no search otherwise
      if (mult_one) t.flags |= 2;  // three_split centre: final_beam_multiply forced to 1
      // A window that is a small fraction of its partition needs several doublings, i.e. a long chain of
      // strictly sequential searches.  Such a task is started first and its doubling levels are searched
      // CONCURRENTLY by different waves (each level restarts from scratch anyway, postfilter_vamana.h:
      // 161-172); the sequential rule "first level with >= k in-window results" is applied afterwards.
      // a first beam that expects fewer than 4k in-window entries fails now and then: such a task starts before the
      // bulk, so that its second, longer search is not what the launch ends with
      if (t.mode == T_GRAPH && (uint64_t)A.beam * w < 4ull * (uint64_t)A.stop_k * (uint64_t)pd.n) t.flags |= 8;
      if (t.mode == T_GRAPH && w > 0 && 2ull * (uint64_t)A.stop_k * (uint64_t)pd.n >= (uint64_t)A.cap_inkernel * w) atomicAdd(A.risk_count, 1);
      // (partition / window >= heavy_ratio, with an eighth of slack: a window one point wider than a power-of-two share of
      // its partition is as heavy as one that is not)
      if (t.mode == T_GRAPH && w > 0 && 8ull * (uint64_t)pd.n >= (8ull * (uint64_t)A.heavy_ratio - 1ull) * w) {
        t.flags |= 1;
        if (A.spec && n < A.maxt) {
          // expected in-window share of a beam ~ w / partition size: levels up to the first beam with
          // beam * w / n_p >= k, plus one
          int nsub = 0;
          long long bb = A.beam;
          const unsigned long long need = (unsigned long long)A.stop_k * (uint64_t)pd.n;
          bool reached = false;  // the loop ended at the first level predicted to hold k entries (bb = its beam)
          while (bb < A.max_beam && (bb <= A.cap_inkernel || bb <= A.big_cap) && nsub < 12) {
            nsub++;
            if ((unsigned long long)bb * w >= need * (unsigned long long)A.spec_num / 8ull) {
              reached = true;
              break;
            }
            bb *= 2;
          }
          // A last level that expects k .. 2 k entries fails about every second time, and its successor then runs AFTER it -- the
          // longest search of the chain, alone (2^-5 / 2^-6 of SIFT-1M: 145 beam-640 / 70 beam-1 280 searches started at 2.5 - 4 ms
          // of a 6.7 / 8.2 ms batch).  Long chains get that successor speculated too where the four-wave kernel runs it (a level
          // in the companion launch costs four wave slots); a level that turns out moot stops when the lower one has succeeded.
          // ... where the window is wide enough that even the root partition's chain is expected to end at a beam of 4 x the first
          // one (k n <= 4 beam w): there the extra level is a search of a few hundred hops; for narrower windows it is the chip's
          // most expensive level (beam 1 280 in the four-wave kernel, everything above in the companion launch) on a launch that is
          // bound by throughput -- measured on SIFT-1M at (80, x1): 2^-4 4.6 -> 4.3 ms, 2^-5 6.7 -> 5.6 ms with it, 2^-6 ... 2^-11
          // 10 - 40 % SLOWER with blanket extra levels (profiles/r06_extra_level_speculation.txt).
          if (A.spec_extra > 0 && reached && nsub >= A.spec_extra && nsub < 12 && (unsigned long long)bb * w < 2ull * need && 2 * bb < A.max_beam &&
              2 * bb <= A.cap_inkernel && 8ull * (unsigned long long)A.stop_k * (unsigned long long)ix.n <= 36ull * (unsigned long long)A.beam * w)  // (an eighth of slack, like the heavy rule)
            nsub++;
          if (nsub >= 2) {
            const int base = atomicAdd(A.sub_count, nsub);
            if (A.sub_base0 + base + nsub <= A.sub_cap) {
              const int32_t pti = (int32_t)(q * A.maxt + n);
              Task parent = t;
              parent.mode = T_PARENT;
              parent.a = nsub;
              parent.b = A.sub_base0 + base;
              A.tasks[pti] = parent;
              n++;
              if (A.scan_list && nsub >= 3 && ((long long)A.beam << (nsub - 1)) > A.cap_inkernel) A.scan_list[atomicAdd(A.scan_count, 1)] = pti;
              // tasks with levels in the companion launch may outgrow them: their small levels run first of all (evidence)
              const bool evidence = A.prio_count && (((long long)A.beam << (nsub - 1)) > A.cap_inkernel) && nsub >= 4;
              for (int r = nsub - 1; r >= 0; r--) {  // longest search first
                Task st = t;
                st.flags |= 4;
                st.a = r;
                st.b = pti;
                const int32_t sti = A.sub_base0 + base + r;
                A.tasks[sti] = st;
                if (((long long)A.beam << r) > A.cap_inkernel) {
                  const int cls = (((long long)A.beam << r) >= 4096) ? 0 : 1;
                  A.big_list[cls * A.big_stride + atomicAdd(A.big_count + cls, 1)] = sti;
                }
                else if (evidence && r <= nsub - 3 && r >= nsub - 5) A.heavy_list[A.heavy_cap - 1 - atomicAdd(A.prio_count, 1)] = sti;
                else A.heavy_list[atomicAdd(A.heavy_count, 1)] = sti;
              }
              return;
            }
          }
        }
      }
    } else {
      int64_t s, e;
      prefilter_bounds(ix.labels + pd.start, pd.n, lo, hi, s, e);
      t.a = pd.start + s;
      t.b = pd.start + e;
      t.mode = (e > s) ? T_BRUTE : T_EMPTY;
    }
    push(t);
  }
  __device__ __forceinline__ void brute(uint64_t a, uint64_t b, int32_t flags = 0) {  // rows [a,b) of the sorted order, no label test
    if (b <= a) return;
    Task t;
    t.query = (int32_t)q;
    t.mode = T_BRUTE;
    t.part = 0;
    t.flags = flags;
    t.a = (int64_t)a;
    t.b = (int64_t)b;
    t.lo = t.hi = 0.f;
    push(t);
  }
};

struct Centre {
  int64_t row, first, last;
  uint64_t cover_start, cover_end;
};

__device__ __forceinline__ int64_t bucket_containing(const int64_t *off, int64_t nb, uint64_t index) {
  int64_t lo = 0, hi = nb;  // largest b with off[b] <= index   (range_filter_tree.h:213-232)
  while (lo + 1 < hi) {
    const int64_t mid = (lo + hi) / 2;
    if ((uint64_t)off[mid] <= index) lo = mid;
    else hi = mid;
  }
  return lo;
}

// find_largest_ranges_within_query_range (range_filter_tree.h:234-295)
__device__ __forceinline__ bool find_centre(const IndexView &ix, uint64_t istart, uint64_t eend, Centre &c) {
  const uint64_t range_size = eend - istart;
  int64_t row = -1;
  for (int r = 0; r < ix.nlevels; r++) {
    const int64_t *off = ix.wst_off + ix.wst_ptr[r];
    if ((uint64_t)(off[1] - off[0] - 1) <= range_size) {
      row = r;
      break;
    }
  }
  if (row < 0) return false;
  const int64_t *off = ix.wst_off + ix.wst_ptr[row];
  int64_t nb = ix.level_nb[row];
  int64_t first = (istart == 0) ? 0 : bucket_containing(off, nb, istart - 1) + 1;
  if (first >= nb) return false;  // the reference indexes past the row here (out_of_range)
  uint64_t start = (uint64_t)off[first], end = (uint64_t)off[first + 1];
  if (end > eend) {
    row += 1;
    if (row >= ix.nlevels) return false;
    off = ix.wst_off + ix.wst_ptr[row];
    nb = ix.level_nb[row];
    first = (istart == 0) ? 0 : bucket_containing(off, nb, istart - 1) + 1;
    if (first >= nb) return false;
    start = (uint64_t)off[first];
    end = (uint64_t)off[first + 1];
  }
  int64_t last = first + 1;
  while (last < nb) {
    const uint64_t next_end = (uint64_t)off[last + 1];
    if (next_end > eend) break;
    last++;
    end = next_end;
  }
  c.row = row;
  c.first = first;
  c.last = last;
  c.cover_start = start;
  c.cover_end = end;
  return true;
}

// Tree query methods (range_filter_tree.h:62-96).  The reference's three entry points call each other:
// three_split_search (:473-540) covers its two remainders with optimized_postfiltering_search (:403-471),
// which falls back to fenwick_tree_search (:297-401) for tiny windows / a large bucket-to-window ratio.
// Here one loop walks the (at most three) label windows a query decomposes into and each body exists
// once, fully inlined: k_route must not need a scratch segment (no calls, no stack objects).
enum { W_FENWICK = 0, W_OPTIMIZED = 1, W_THREE_SPLIT = 2 };

__device__ __forceinline__ void emit_tree(Emitter &E, float lo0, float hi0, int mode0) {
  const IndexView &ix = E.A.ix;
  float lo1 = 0.f, hi1 = 0.f, lo2 = 0.f, hi2 = 0.f;  // remainders of three_split (always W_OPTIMIZED)
  int nwin = 1;
  for (int it = 0; it < nwin; it++) {
    const float lo = it == 0 ? lo0 : (it == 1 ? lo1 : lo2);
    const float hi = it == 0 ? hi0 : (it == 1 ? hi1 : hi2);
    int mode = it == 0 ? mode0 : W_OPTIMIZED;
    bool mult_one = false;
    if (hi < ix.labels[0] || lo > ix.labels[ix.n - 1]) {  // check_empty (:191-203)
      if (it == 0) atomicAdd(&E.A.ctr->empty_windows, 1ull);
      continue;
    }
    uint64_t istart, eend;
    first_ge2(ix.labels, ix.n, lo, hi, istart, eend);
    const uint64_t w = eend - istart;
    // wann_set_exact_windows: tested once, on the query's whole window, before three_split decomposes it and before find_centre
    if (it == 0 && w > 0 && w <= (uint64_t)E.A.exact_limit) {
      E.exact = true;
      E.brute(istart, eend, kTaskExactWindow);
      return;
    }
    Centre c;
    bool have_centre = false;
    if (mode != W_OPTIMIZED) have_centre = find_centre(ix, istart, eend, c);

    if (mode == W_THREE_SPLIT) {  // three_split_search (:473-540)
      if (have_centre) {
        for (int64_t b = c.first; b < c.last; b++) E.leaf((int32_t)(ix.level_part0[c.row] + b), lo, hi, w, true);
        if (c.cover_start - istart > 0) {
          lo1 = lo;
          hi1 = ix.labels[c.cover_start];
          nwin = 2;
        }
        if (eend - c.cover_end > 0) {
          if (nwin == 2) {
            lo2 = ix.labels[c.cover_end];
            hi2 = hi;
          } else {
            lo1 = ix.labels[c.cover_end];
            hi1 = hi;
          }
          nwin++;
        }
        continue;
      }
      mode = W_FENWICK;  // qp_fenwick: final_beam_multiply = 1 (:490-498)
      mult_one = true;
    }

    if (mode == W_OPTIMIZED) {  // optimized_postfiltering_search (:403-471)
      bool fallback = 4 * w < (uint64_t)(int64_t)ix.cutoff;  // :419-421
      if (!fallback) {
        int64_t row = 0, idx = 0;
        while (row + 1 < ix.nlevels) {  // :426-451
          const int64_t nrow = row + 1;
          const int64_t *off = ix.wst_off + ix.wst_ptr[nrow];
          int64_t nidx = -1;
          for (int64_t ch = idx * ix.split; ch < idx * ix.split + ix.split; ch++) {
            if (ch >= ix.level_nb[nrow]) break;
            if (istart >= (uint64_t)off[ch] && eend <= (uint64_t)off[ch + 1]) nidx = ch;
          }
          if (nidx < 0) break;
          idx = nidx;
          row = nrow;
        }
        {  // :452-457
          const int64_t *off = ix.wst_off + ix.wst_ptr[row];
          E.note(2, (int64_t)istart, (int64_t)eend, off[idx], off[idx + 1], off[idx + 1] - off[idx]);
        }
        if (E.A.has_ratio) {  // :460-466
          const int64_t *off = ix.wst_off + ix.wst_ptr[row];
          const float ratio = (float)(uint64_t)(off[idx + 1] - off[idx]) / (float)w;
          fallback = ratio > E.A.ratio;
        }
        if (!fallback) {
          E.leaf((int32_t)(ix.level_part0[row] + idx), lo, hi, w, false);
          continue;
        }
      }
      mode = W_FENWICK;
      have_centre = find_centre(ix, istart, eend, c);
    }

    // fenwick_tree_search (:297-401)
    E.note(4, (int64_t)istart, (int64_t)eend);
    if (!have_centre) {
      E.brute(istart, eend);
      continue;
    }
    for (int64_t b = c.first; b < c.last; b++) {
      const int64_t *off = ix.wst_off + ix.wst_ptr[c.row];
      E.note(5, off[b], off[b + 1]);
      E.leaf((int32_t)(ix.level_part0[c.row] + b), lo, hi, w, mult_one);
    }
    uint64_t cov_s = c.cover_start, cov_e = c.cover_end;
    int64_t left = c.first, right = c.last - 1;
    const int64_t B = ix.split;
    for (int64_t row = c.row + 1; row < ix.nlevels; row++) {
      const int64_t *off = ix.wst_off + ix.wst_ptr[row];
      const int64_t nb = ix.level_nb[row];
      left *= B;
      right = right * B + B - 1;
      while (left > 0) {
        const uint64_t nls = (uint64_t)off[left - 1];
        if (nls < istart) break;
        cov_s = nls;
        left -= 1;
        E.note(5, off[left], off[left + 1]);
        E.leaf((int32_t)(ix.level_part0[row] + left), lo, hi, w, mult_one);
      }
      while (right < nb - 1) {
        const uint64_t nre = (uint64_t)off[right + 2];
        if (nre > eend) break;
        cov_e = nre;
        right += 1;
        E.note(5, off[right], off[right + 1]);
        E.leaf((int32_t)(ix.level_part0[row] + right), lo, hi, w, mult_one);
      }
    }
    E.brute(istart, cov_s);
    E.brute(cov_e, eend);
  }
}

// super_optimized_postfiltering_search (super_optimized_postfilter_tree.h:187-270)
__device__ __forceinline__ void emit_super(Emitter &E, float lo, float hi) {
  const IndexView &ix = E.A.ix;
  if (hi < ix.labels[0] || lo > ix.labels[ix.n - 1]) {
    atomicAdd(&E.A.ctr->empty_windows, 1ull);
    return;
  }
  uint64_t istart, eend;
  first_ge2(ix.labels, ix.n, lo, hi, istart, eend);
  const uint64_t w = eend - istart;
  if (w > 0 && w <= (uint64_t)E.A.exact_limit) {  // wann_set_exact_windows: before the level scan
    E.exact = true;
    E.brute(istart, eend, kTaskExactWindow);
    return;
  }
  int level;
  int64_t idx = 0;
  for (level = ix.nlevels - 1; level >= 0; level--) {
    if (level == 0) {
      idx = 0;
      break;
    }
    const uint64_t bsz = (uint64_t)ix.sup_size[level];
    if (bsz < w) continue;
    const uint64_t shift = (uint64_t)ix.sup_shift[level];
    const uint64_t nb = (uint64_t)ix.level_nb[level];
    uint64_t fp = istart / shift, lp = (eend - 1) / shift;
    if (fp > nb - 1) fp = nb - 1;
    if (lp > nb - 1) lp = nb - 1;
    bool found = false;
    for (uint64_t tb = fp; tb <= lp; tb++) {
      E.note(1, (int64_t)tb);  // :226-228
      uint64_t bs = tb * shift, be = bs + bsz;
      if (be > (uint64_t)ix.n) be = (uint64_t)ix.n;
      if (istart >= bs && eend <= be) {
        E.note(2, (int64_t)istart, (int64_t)eend, (int64_t)bs, (int64_t)be, (int64_t)bsz);  // :233-238 (the size printed is the level's nominal bucket size)
        idx = (int64_t)tb;
        found = true;
        break;
      }
    }
    if (found) break;
  }
  E.note(3);  // :248-254, :260-267: the two timing lines around the leaf's search
  E.leaf((int32_t)(ix.level_part0[level] + idx), lo, hi, w, false);
}

// KIND is the index class (wann.h WANN_KIND_*; 2 stands for both tree kinds): one small kernel per class.
template <int KIND>
__global__ void k_route(RouteArgs A) {
  const IndexView &ix = A.ix;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= A.nq) return;
  const float lo = A.ranges[2 * q], hi = A.ranges[2 * q + 1];
  Emitter E(A, q);
  if (KIND == 0) {  // PrefilterIndex: [lb(lo), lb(hi)) over the label argsort (prefiltering.h:159-184)
    Task t;
    t.query = (int32_t)q;
    t.part = 0;
    t.flags = 0;
    t.lo = lo;
    t.hi = hi;
    prefilter_bounds(ix.fv_sorted, ix.n, lo, hi, t.a, t.b);
    t.mode = (t.b > t.a) ? T_BRUTE_GATHER : T_EMPTY;
    // (an empty window emits no task, but the dense path's k_group_insert reads EVERY query's task slot: it must say T_EMPTY,
    // not hold an earlier batch's window -- that one would be scanned again, or even join a group)
    if (t.mode == T_EMPTY) A.tasks[q * A.maxt] = t;
    E.push(t);
  } else if (KIND == 1) {  // stand-alone PostfilterVamanaIndex: always the one graph, no window lookup
    Task t;
    t.query = (int32_t)q;
    t.part = 0;
    t.flags = 0;
    t.a = t.b = 0;
    t.lo = lo;
    t.hi = hi;
    t.mode = (A.beam < A.max_beam) ? T_GRAPH : T_EMPTY;
    E.push(t);
  } else if (KIND == 4) {
    emit_super(E, lo, hi);
  } else {
    emit_tree(E, lo, hi, A.method == M_OPTIMIZED ? W_OPTIMIZED : (A.method == M_THREE_SPLIT ? W_THREE_SPLIT : W_FENWICK));
  }
  A.qtask_cnt[q] = E.n;
  if ((KIND == 4 || KIND == 2) && A.exact_limit > 0) {
    // (a query without a task: the dense grouping reads EVERY query's slot 0 -- it must not hold an earlier batch's window)
    if (E.n == 0) {
      Task t;
      t.query = (int32_t)q;
      t.mode = T_EMPTY;
      t.part = 0;
      t.flags = 0;
      t.a = t.b = 0;
      t.lo = lo;
      t.hi = hi;
      A.tasks[q * A.maxt] = t;
    }
    const unsigned long long em = __ballot(E.exact);  // one counter update per wave
    if (em && (threadIdx.x & 63) == __builtin_ctzll(em)) atomicAdd(&A.ctr->exact_queries, (unsigned long long)__builtin_popcountll(em));
  }
}

// wann_set_exact_windows: the rows k_brute scores for exact-window tasks = the widths of the flagged tasks on its list (the
// slices of a split scan add up to the task).  A kernel of its own, launched with the option on only, keeps the count out of
// k_brute's loop: a second running sum there cost the float32 instance 29 registers.  One counter update per wave.
__global__ void k_exact_rows(const Task *tasks, const int32_t *list, const int32_t *list_count, Counters *ctr) {
  const int total = *list_count;
  unsigned long long rows = 0;
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
    const Task t = tasks[list[i]];
    if (t.mode == T_BRUTE && (t.flags & kTaskExactWindow) && t.b > t.a) rows += (unsigned long long)(t.b - t.a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rows += __shfl_down(rows, o);
  if ((threadIdx.x & 63) == 0 && rows) atomicAdd(&ctr->exact_rows, rows);
}

// Longest first: the heavy list comes out of k_route in query order; one workgroup reorders it by speculated level,
// highest (= longest search) first, plain heavy tasks (whole chains) before all -- a long search that starts late is what
// a launch ends with, and a level that fails late starts its continuation late.  (Counting sort; the order within a level is
// whatever the atomics give: results do not depend on it.)
__global__ __launch_bounds__(1024) void k_order_heavy(OrderArgs A) {
  // key = (number of levels of the sub-task's PARENT, the sub-task's own level), highest first: the levels of the tasks with
  // the longest chains come first and, within such a class, the longest searches first.  A parent is resolved when its LAST
  // level has finished; ordered by level alone (round 3) the cheap beam-80 levels of every speculating task ran at the very end
  // of the heavy list -- at 8.4 ms of a 13.5 ms batch at 2^-9 -- and a task whose levels had all failed started its
  // continuation (4.7 ms at beam 1 280) only then.
  __shared__ int hist[256], place[256];
  const int n = *A.count;
  if (threadIdx.x < 256) hist[threadIdx.x] = 0;
  __syncthreads();
  auto key_of = [&](const Task &t) -> int {
    if (!(t.flags & 4)) return 255;  // plain heavy tasks (whole chains) before all
    const int cls = (int)A.tasks[t.b].a, lvl = (int)t.a;
    return (cls < 15 ? cls : 14) * 16 + (lvl < 16 ? lvl : 15);
  };
  for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[key_of(A.tasks[A.in[i]])], 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int off = 0;
    for (int key = 255; key >= 0; key--) {
      place[key] = off;
      off += hist[key];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ti = A.in[i];
    A.out[atomicAdd(&place[key_of(A.tasks[ti])], 1)] = ti;
  }
}

// One thread per query when every query has at most one task; the multi-task form (fenwick,
// three_split) merges the per-task top-k lists: concatenate, sort by (dist, id), truncate
// (range_filter_tree.h:542-549; duplicates are kept like the reference keeps them).
__global__ void k_finalize(FinalizeArgs A) {
  // one thread per OUTPUT ENTRY (query, j): three dependent round trips (counts -> key -> decoding) whatever k is.  One thread per
  // query walked its k entries one after the other -- the stores to ids / dists may alias the loads for all the compiler knows --
  // i.e. 2 k dependent round trips: 14 us per 10 000 queries (21 us on the GloVe-like index) for what is 3 - 4 us of work.
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= A.nq * (int64_t)A.k) return;
  const int64_t q = t / A.k;
  const int j = (int)(t - q * A.k);
  const int nt = A.qtask_cnt[q];
  const int64_t ti = q * A.maxt;
  const int cnt = nt > 0 ? A.out_cnt[ti] : 0;
  uint32_t id = A.pad_id;
  float dist = 3.402823466e+38f;  // std::numeric_limits<float>::max()
  if (j < cnt) {
    const bool decode = A.decode && A.tasks[ti].mode != T_BRUTE_GATHER;
    const u64 e = A.out_key[(size_t)ti * A.k + j];
    id = (uint32_t)e;
    if (decode) id = A.ix.decoding[id];
    dist = funkey((uint32_t)(e >> 32));
  }
  A.ids[t] = id;
  A.dists[t] = dist;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_finalize_multi(FinalizeArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  const int K = A.k;
  const int per_wave = finalize_lds_bytes_per_wave(K);
  u64 *cand_key = reinterpret_cast<u64 *>(smem + (size_t)wib * per_wave);
  u64 *top = cand_key + 64;
  for (int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + wib; q < A.nq; q += (int64_t)gridDim.x * kWavesPerBlock) {
    const int nt = A.qtask_cnt[q];
    int m = 0;
    for (int t = 0; t < nt; t++) {
      const int64_t ti = q * A.maxt + t;
      const int cnt = A.out_cnt[ti];
      for (int c0 = 0; c0 < cnt; c0 += 64) {
        const bool have = (c0 + lane) < cnt;
        u64 e = have ? A.out_key[(size_t)ti * K + c0 + lane] : 0ull;
        // out_key = fkey(dist) << 32 | sorted id  ->  merge key with the id shifted (bit 0 = flag)
        u64 key = (e & 0xffffffff00000000ull) | ((u64)(uint32_t)e << 1);
        bool pass = have;
        if (pass && m >= K) pass = (key | 1ull) < (top[K - 1] | 1ull);
        int p0;
        m = wave_merge<u64 *, false>(top, m, K, pass, key, cand_key, &p0);
      }
    }
    for (int j = lane; j < K; j += 64) {
      uint32_t id = A.pad_id;
      float dist = 3.402823466e+38f;
      if (j < m) {
        const u64 e = top[j];
        id = (uint32_t)e >> 1;
        if (A.decode) id = A.ix.decoding[id];
        dist = funkey((uint32_t)(e >> 32));
      }
      A.ids[q * K + j] = id;
      A.dists[q * K + j] = dist;
    }
    WAVE_SYNC();
  }
}

// --------------------------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------------------------
thread_local const char *g_launch_err = "";
const char *launch_last_error() { return g_launch_err; }
#else
extern thread_local const char *g_launch_err;
#endif  // WANN_DT == 0

static int check(hipError_t e) {
  if (e != hipSuccess) {
    g_launch_err = hipGetErrorString(e);
    return 1;
  }
  return 0;
}

#if WANN_DT == 0

int search_lds_bytes_per_wave(int qwords, int pool_bytes) {
  return ((qwords * 4 + 15) & ~15) + 64 * 8 + 64 * 4 + 64 * 4 + pool_bytes;
}

int launch_route(const RouteArgs &a, void *stream) {
  if (a.nq == 0) return 0;
  int threads = 128;
  int blocks = (int)((a.nq + threads - 1) / threads);
  hipStream_t s = (hipStream_t)stream;
  switch (a.ix.kind) {
    case 0: hipLaunchKernelGGL(k_route<0>, dim3(blocks), dim3(threads), 0, s, a); break;
    case 1: hipLaunchKernelGGL(k_route<1>, dim3(blocks), dim3(threads), 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_route<4>, dim3(blocks), dim3(threads), 0, s, a); break;
    default: hipLaunchKernelGGL(k_route<2>, dim3(blocks), dim3(threads), 0, s, a); break;
  }
  return check(hipGetLastError());
}

int launch_exact_rows(const BruteArgs &a, int64_t nq, void *stream) {
  const int threads = 256, blocks = (int)std::min<int64_t>(64, (nq + threads - 1) / threads);
  if (blocks <= 0) return 0;
  hipLaunchKernelGGL(k_exact_rows, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, a.tasks, a.list, a.list_count, a.ctr);
  return check(hipGetLastError());
}

// Predicted work per query of a routed batch (routed WITHOUT speculative levels: every graph task is a plain one that carries
// its window's size): the doubling loop of postfilter_vamana.h:161-181 with "a level finds k entries once its beam is expected
// to hold k in-window points" (beam * window / partition >= k), a hop per beam entry; an exact scan's rows count 1/36 of a hop
// (a hop scores about 36 vectors).  What a strong-scaling shard cut balances (rangefilteredann_amd/distributed.py).
__global__ void k_task_cost(CostArgs A) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= A.nq) return;
  float cost = 0.f;
  const int nt = A.qtask_cnt[q];
  for (int i = 0; i < nt; i++) {
    const Task &t = A.tasks[q * A.maxt + i];
    if (t.mode == T_GRAPH) {
      const unsigned long long np = (unsigned long long)A.parts[t.part].n, w = (unsigned long long)(t.a > 0 ? t.a : 1);
      long long b = A.beam, c = 0;
      for (;;) {
        c += b;
        if ((unsigned long long)b * w >= (unsigned long long)A.k * np || 2 * b >= A.max_beam) break;
        b *= 2;
      }
      long long fb = b * ((t.flags & 2) ? 1 : A.mult);
      if (fb > A.max_beam) fb = A.max_beam;
      if (fb > b) c += fb;
      cost += (float)c;
    } else if (t.mode == T_BRUTE || t.mode == T_BRUTE_GATHER)
      cost += 1.f + (float)(t.b - t.a) / 36.f;
  }
  A.cost[q] = cost;
}

int launch_task_cost(const CostArgs &a, void *stream) {
  if (a.nq <= 0) return 0;
  hipLaunchKernelGGL(k_task_cost, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check(hipGetLastError());
}

// Holds the stream until `need` workgroups of the companion launch (queued first, on the side stream) have started -- or a bound
// of about 0.25 ms has passed (launches that the runtime serialises: the companion cannot start before this kernel ends).
// The deep-chain pollers book whole CUs; an ordinary launch that reaches the CUs first books them all for the length of the
// batch, and the chains the pollers were meant for stay in the four-wave kernel (run_batch).
__global__ void k_gate(const int32_t *resident, int need) {
  for (int i = 0; i < 256; i++) {  // (a poll is a memory-side atomic, about a microsecond)
    if (__hip_atomic_load(resident, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need) break;
    __builtin_amdgcn_s_sleep(8);
  }
}

int launch_gate(const int32_t *resident, int need, void *stream) {
  hipLaunchKernelGGL(k_gate, dim3(1), dim3(1), 0, (hipStream_t)stream, resident, need);
  return check(hipGetLastError());
}

int launch_order_heavy(const OrderArgs &a, void *stream) {
  hipLaunchKernelGGL(k_order_heavy, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  return check(hipGetLastError());
}

#endif  // WANN_DT == 0

namespace WANN_DT_NS {
template <int METRIC, int KIND>
static int launch_search_t(const SearchArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
  auto kern = k_search<METRIC, KIND>;
  if (lds > 48 * 1024)
    if (check(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))) return 1;
  hipLaunchKernelGGL(kern, grid, block, lds, s, a);
  return check(hipGetLastError());
}

// what the runtime says about co-residency: workgroups of this launch shape per CU (registers, LDS and its allocation granule)
template <int METRIC, int KIND>
static int search_occupancy_t(int threads, size_t lds) {
  auto kern = k_search<METRIC, KIND>;
  if (lds > 48 * 1024)
    if (check(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))) return -1;
  int n = 0;
  if (check(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)kern, threads, lds))) return -1;
  return n;
}

static int search_occupancy(const SearchArgs &a, const LaunchCfg &cfg) {
  const int wpb = cfg.waves_per_block > 0 ? cfg.waves_per_block : kWavesPerBlock;
  const size_t lds = (size_t)search_lds_bytes_per_wave(query_words(a.ix), a.pool_bytes) * wpb;
  const int threads = 64 * wpb + ((cfg.big == 1 && a.helper) ? 64 * a.helper : 0);
  if (cfg.big == 1) return a.ix.metric == 1 ? search_occupancy_t<1, 1>(threads, lds) : search_occupancy_t<0, 1>(threads, lds);
  if (cfg.big == 2) return a.ix.metric == 1 ? search_occupancy_t<1, 2>(threads, lds) : search_occupancy_t<0, 2>(threads, lds);
  return a.ix.metric == 1 ? search_occupancy_t<1, 0>(threads, lds) : search_occupancy_t<0, 0>(threads, lds);
}

static int launch_search(const SearchArgs &a, const LaunchCfg &cfg, void *stream) {
  if (cfg.blocks <= 0) return 0;
  const int wpb = cfg.waves_per_block > 0 ? cfg.waves_per_block : kWavesPerBlock;
  size_t lds = (size_t)search_lds_bytes_per_wave(query_words(a.ix), a.pool_bytes) * wpb;
  dim3 grid(cfg.blocks), block(64 * wpb + ((cfg.big == 1 && a.helper) ? 64 * a.helper : 0));  // (+ the scoring helper waves)
  hipStream_t s = (hipStream_t)stream;
  if (cfg.big == 1) return a.ix.metric == 1 ? launch_search_t<1, 1>(a, grid, block, lds, s) : launch_search_t<0, 1>(a, grid, block, lds, s);
  if (cfg.big == 2) return a.ix.metric == 1 ? launch_search_t<1, 2>(a, grid, block, lds, s) : launch_search_t<0, 2>(a, grid, block, lds, s);
  return a.ix.metric == 1 ? launch_search_t<1, 0>(a, grid, block, lds, s) : launch_search_t<0, 0>(a, grid, block, lds, s);
}

template <int METRIC>
static int launch_brute_t(const BruteArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t s, bool staged) {
#if WANN_SCAN_STAGED && WANN_SCAN_PLAIN
  auto kern = staged ? k_brute_staged<METRIC> : k_brute<METRIC>;
#elif WANN_SCAN_STAGED
  auto kern = k_brute_staged<METRIC>;  // (the one scan kernel of this unit)
#else
  auto kern = k_brute<METRIC>;
#endif
  (void)staged;
  if (lds > (size_t)kLdsNoAttribute)
    if (check(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))) return 1;
  hipLaunchKernelGGL(kern, grid, block, lds, s, a);
  return check(hipGetLastError());
}

static int launch_brute(const BruteArgs &a, int blocks, void *stream) {
  if (blocks <= 0) return 0;
  // (long rows or a wide k: more than a launch gets unasked -- run_batch has refused what exceeds kLdsPerWorkgroup)
  const bool staged = scan_staged(a.ix, a.k);  // (wann_device.h: by the view's type and kind -- this unit's kernel for it)
  const size_t lds = (size_t)scan_lds_bytes(a.ix, a.k);
  dim3 grid(blocks), block(64 * kWavesPerBlock);
  return a.ix.metric == 1 ? launch_brute_t<1>(a, grid, block, lds, (hipStream_t)stream, staged)
                          : launch_brute_t<0>(a, grid, block, lds, (hipStream_t)stream, staged);
}

// (reached through a function: host code only, and no order of initialisation to depend on)
const SearchUnit &search_unit() {
  static constexpr SearchUnit unit = {search_occupancy, launch_search, launch_brute};
  return unit;
}

}  // namespace WANN_DT_NS

#if WANN_DT == 0
// the entry points: the view's row type picks the unit (a type without a search unit is an error, never another type's kernels)
static const SearchUnit *unit_or_error(const IndexView &ix) {
  const SearchUnit *u = search_unit_of(ix.dtype);
  if (!u) {
    static thread_local char text[48];
    snprintf(text, sizeof text, "row type %d has no search unit", ix.dtype);
    g_launch_err = text;
  }
  return u;
}
int search_occupancy(const SearchArgs &a, const LaunchCfg &cfg) { const SearchUnit *u = unit_or_error(a.ix); return u ? u->search_occupancy(a, cfg) : -1; }
int launch_search(const SearchArgs &a, const LaunchCfg &cfg, void *stream) { const SearchUnit *u = unit_or_error(a.ix); return u ? u->launch_search(a, cfg, stream) : 1; }
int launch_brute(const BruteArgs &a, int blocks, void *stream) { const SearchUnit *u = unit_or_error(a.ix); return u ? u->launch_brute(a, blocks, stream) : 1; }

int launch_finalize(const FinalizeArgs &a, void *stream) {
  if (a.nq == 0) return 0;
  if (a.maxt > 1) {
    const int per_wave = finalize_lds_bytes_per_wave(a.k);  // (never beyond kLdsNoAttribute: asserted in wann_device.h)
    int blocks = (int)std::min<int64_t>(2048, (a.nq + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(k_finalize_multi, dim3(blocks), dim3(64 * kWavesPerBlock), (size_t)per_wave * kWavesPerBlock,
                       (hipStream_t)stream, a);
  } else {
    int threads = 256;
    int blocks = (int)((a.nq * (int64_t)a.k + threads - 1) / threads);
    hipLaunchKernelGGL(k_finalize, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, a);
  }
  return check(hipGetLastError());
}

#endif  // WANN_DT == 0

}  // namespace wann
