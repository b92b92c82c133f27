// wann_brute_body.inc -- the body of k_brute and k_brute_staged (wann_kernels_body.inc includes it once for each, with
// WANN_BRUTE_STAGED 0 / 1): one text for both, and with 0 exactly the text k_brute has always compiled.
// Parameters of the enclosing kernel: template <int METRIC>, BruteArgs A.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView &ix = A.ix;
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  const int K = A.k;
#if WANN_BRUTE_STAGED
  const int pitch = ix.stride * 4, pad = kScanStagePad;
  const int per_wave = (int)brute_lds_bytes_per_wave(qv_words(ix), K) + (int)scan_stage_bytes_per_wave(pitch, pad, qv_words(ix), K);
#else
  const int per_wave = (int)brute_lds_bytes_per_wave(qv_words(ix), K);
#endif
  unsigned char *base = smem + (size_t)wib * per_wave;
  float *qv = reinterpret_cast<float *>(base);
  int off = (qv_words(ix) * 4 + 15) & ~15;
  u64 *cand_key = reinterpret_cast<u64 *>(base + off);
  off += 64 * 8;
  int32_t *cand_id = reinterpret_cast<int32_t *>(base + off);
  off += 64 * 4;
  float *cand_dist = reinterpret_cast<float *>(base + off);
  off += 64 * 4;
  u64 *top = reinterpret_cast<u64 *>(base + off);
#if WANN_BRUTE_STAGED
  unsigned char *stage = base + brute_lds_bytes_per_wave(qv_words(ix), K);
#endif
  const int total = *A.list_count;
  if (total == 0) return;  // (the list is sized on the device; an empty one must not cost a ticket per wave)
#if WANN_BRUTE_STAGED
  // (the top-k of a window does not depend on how many rows a pass takes: keys are distinct, wave_merge keeps the k smallest)
  const int step = scan_stage_rows(pitch, pad, qv_words(ix), K);
#else
  const int step = (METRIC == 1) ? 64 : 64;
#endif
  // scans are short and uniform: a wave takes four tickets at a time and reports its row count once (ten thousand
  // same-address atomics per batch were most of a tiny-window batch)
  // A short list (a few queries, or the handful the dense path could not prove) would leave the chip to `total` waves,
  // each walking its whole window alone: such scans are cut into S slices, one wave per slice; the slice that finishes
  // last merges the others' partial results (they are in memory; a counter per task tells who is last).
  int S = 1, lgS = 0;
  if (A.part_key) {
    const int64_t waves = (int64_t)gridDim.x * kWavesPerBlock, kpad = (K + 1) & ~1;
    while (S < 64 && (int64_t)total * S * 4 <= waves && (int64_t)total * S * 2 * kpad <= A.part_cap && (int64_t)total * S * 2 <= A.part_slots) {
      S <<= 1;
      lgS++;
    }
  }
  const int ntickets = total << lgS;
  // Tickets are dealt, not drawn: wave w takes tickets w, w + W, w + 2 W, ... (W = the waves of the launch, sized to what the
  // chip holds at once).  Scans of one batch are about equally long, and a few long ones are cut into slices above; drawing
  // tickets from a counter cost ten thousand same-address atomics per tiny-window batch, and drawing four at a time (round 1)
  // left a 10 000-query batch to 2 500 waves of four scans in a row.
  const int nwaves = (int)gridDim.x * kWavesPerBlock;
  unsigned long long rows_done = 0;

  for (int t = (int)blockIdx.x * kWavesPerBlock + wib; t < ntickets; t += nwaves) {
    const int li = t >> lgS, part = t & (S - 1);
    const int ti = A.list[li];
    const Task task = A.tasks[ti];
    const int64_t qrow = task.query;
    for (int i = lane; i < qv_words(ix); i += 64) qv[i] = stage_query_word(A.queries, qrow, i, ix.d);
    WAVE_SYNC();
    int64_t ra = task.a, rb = task.b;
    if (S > 1) {
      const int64_t len = (((task.b - task.a + S - 1) >> lgS) + 63) & ~(int64_t)63;
      ra = task.a + part * len;
      rb = (ra + len < task.b) ? ra + len : task.b;
    }
    int m = 0;
    for (int64_t r0 = ra; r0 < rb; r0 += step) {
      int cnt = (int)((rb - r0) < step ? (rb - r0) : step);
      int64_t row = r0 + lane;
      int rid = 0;
      if (lane < cnt) rid = (task.mode == T_BRUTE_GATHER) ? ix.fi_sorted[row] : (int)row;
#if WANN_BRUTE_STAGED
      float dist;
      {
        // Every task of a staged launch is T_BRUTE: only an index with graphs owns a shadow copy, k_route emits T_BRUTE_GATHER for
        // the PrefilterIndex alone (KIND 0), and the dense path hands tasks back as it got them.  So rid is the row number, and
        // rows r0 .. r0 + cnt are bytes [r0 pitch, (r0 + cnt) pitch) of the copy: nothing outside them is loaded -- the copy
        // ends with row n - 1.
        const unsigned char *src = reinterpret_cast<const unsigned char *>(ix.points) + r0 * (int64_t)pitch;
        const int nsteps = scan_fetch_steps(cnt, pitch);
        for (int s0 = 0; s0 < nsteps; s0 += 8) {
          uint4 v[8];
#pragma unroll
          for (int j = 0; j < 8; j++) {
            const ScanFetch f = scan_fetch(lane, s0 + j, cnt, pitch, pad);
            if (f.valid) v[j] = *reinterpret_cast<const uint4 *>(src + f.src);
          }
#pragma unroll
          for (int j = 0; j < 8; j++) {
            const ScanFetch f = scan_fetch(lane, s0 + j, cnt, pitch, pad);
            if (f.valid) {  // (two 8-byte stores: a staged row starts on a multiple of 8, not always of 16)
              uint2 *dst = reinterpret_cast<uint2 *>(stage + f.dst);
              dst[0] = make_uint2(v[j].x, v[j].y);
              dst[1] = make_uint2(v[j].z, v[j].w);
            }
          }
        }
        cand_id[lane] = lane < cnt ? lane : 0;  // row numbers within the staging area
        WAVE_SYNC();
        IndexView sv = ix;
        sv.points = reinterpret_cast<const float *>(stage);
        sv.stride = (pitch + pad) >> 2;
        dist = wave_distances<METRIC, true, true>(sv, cand_id, cand_dist, qv, cnt, 0);
      }
#else
      cand_id[lane] = rid;
      WAVE_SYNC();
      float dist = wave_distances<METRIC, true, true>(ix, cand_id, cand_dist, qv, cnt, 0);
#endif
      u64 key = ((u64)fkey(dist) << 32) | ((u64)(uint32_t)rid << 1);
      bool pass = lane < cnt;
      if (m >= K) pass = pass && ((key | 1ull) < (top[K - 1] | 1ull));
      int p0;
      m = wave_merge(top, m, K, pass, key, cand_key, &p0);
    }
    rows_done += (unsigned long long)(rb > ra ? rb - ra : 0);
    bool last = true;
    if (S > 1) {
      const size_t kpad = (size_t)((K + 1) & ~1);
      u64 *mine = A.part_key + ((size_t)li * S + part) * kpad;
      for (int x = lane; x < m; x += 64) mine[x] = top[x];
      if (lane == 0) A.part_cnt[li * S + part] = m;
      __threadfence();
      int old = 0;
      if (lane == 0) old = atomicAdd(&A.part_done[li], 1);
      last = __builtin_amdgcn_readfirstlane(old) == S - 1;
      if (last) {
        __threadfence();
        // the other slices' lists, 64 slots at a time (a slot = (slice, place); most lists are short)
        const u64 *all = A.part_key + (size_t)li * S * kpad;
        for (int x0 = 0; x0 < S * (int)kpad; x0 += 64) {
          const int x = x0 + lane, p = x / (int)kpad, off = x - p * (int)kpad;
          bool pass = p < S && p != part;
          if (pass) pass = off < __hip_atomic_load(&A.part_cnt[li * S + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          u64 key = 0;
          if (pass) key = __hip_atomic_load(&all[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (m >= K) pass = pass && ((key | 1ull) < (top[K - 1] | 1ull));
          if (ballot64(pass)) {
            int p0;
            m = wave_merge(top, m, K, pass, key, cand_key, &p0);
          }
        }
        if (lane == 0) A.part_done[li] = 0;  // ready for the next batch
      }
    }
    if (last) {
      for (int x = lane; x < m; x += 64) {
        u64 e = top[x];
        A.out_key[(size_t)ti * K + x] = (e & 0xffffffff00000000ull) | (uint32_t)((uint32_t)e >> 1);
      }
      if (lane == 0) A.out_cnt[ti] = m;
    }
    WAVE_SYNC();
  }
  if (lane == 0 && rows_done) atomicAdd(&A.ctr->brute_rows, rows_done);
