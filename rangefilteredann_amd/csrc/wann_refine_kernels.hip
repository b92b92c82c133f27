// wann_refine_kernels.hip -- re-ranking of a compact index's candidates against full-precision rows (wann.h
// wann_batch_search_device_refined).  A float16 / bfloat16 / float8 index answers for the ROUNDED points; the
// refined call searches it for refine_k >= k candidates and this unit scores those candidates against the caller's float32
// rows (wann_set_refine_rows) and keeps the best k.
//
// The unit is a float32 one (WANN_DT 0): the store has the float32 index's row pitch, and the distances come from
// wave_distances of wann_wave.h -- l2_pair_ct / l2_pair2_ct / l2_pair, mips_pair_ct / mips_pair2_ct / mips_pair, the routines of
// the float32 index's exact scan, in their order.  There is no distance code here: a refined distance is, bit for bit, what a
// float32 index of the store's rows returns for that (row, query) pair.
#include "wann_wave.h"
#include "wann_refine_device.h"

#include <algorithm>

namespace wann {

// One wave per query, kWavesPerBlock waves per workgroup, grid-stride over the queries.  LDS per wave: k_brute's carve
// (refine_lds_bytes_per_wave).  Per query: stage the query row; walk the candidates 64 at a time -- a chunk's candidates are
// its entries before the first pad, and since pads are a suffix the walk ends with the first chunk that is not full -- gather
// and score their rows (two rows per lane pair in flight where the routines have that form), and merge the keys
// fkey(dist) << 32 | id << 1 into the k-entry list (bit 0 is wave_merge's flag; ids are below 2^31).  Equal keys -- a row the
// search returned twice: fenwick and three_split can -- are kept, as k_finalize_multi keeps them.
template <int METRIC>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_refine(RefineArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView &ix = A.ix;
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  const int K = A.k, RK = A.refine_k;
  const int per_wave = (int)refine_lds_bytes_per_wave(qv_words(ix), K);
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
  unsigned long long scored = 0;

  for (int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + wib; q < A.nq; q += (int64_t)gridDim.x * kWavesPerBlock) {
    for (int i = lane; i < qv_words(ix); i += 64) qv[i] = stage_query_word(A.queries, q, i, ix.d);
    WAVE_SYNC();
    const uint32_t *cid = A.cand_ids + q * RK;
    const float *cdist = A.cand_dists + q * RK;
    int m = 0;
    for (int c0 = 0; c0 < RK; c0 += 64) {
      const bool have = c0 + lane < RK;
      const uint32_t id = have ? cid[c0 + lane] : A.pad_id;
      const float was = have ? cdist[c0 + lane] : 3.402823466e+38f;
      // a candidate: not a pad -- and a row of the store (the search returns nothing else; no address is ever made from an id that is not)
      const bool cand = have && !(id == A.pad_id && was == 3.402823466e+38f) && (int64_t)id < ix.n;
      const u64 stop = ~ballot64(cand);
      const int cnt = stop ? ctz64(stop) : 64;  // the entries before the first pad
      if (cnt > 0) {
        cand_id[lane] = lane < cnt ? (int32_t)id : 0;
        WAVE_SYNC();
        const float dist = wave_distances<METRIC, true, true>(ix, cand_id, cand_dist, qv, cnt, 0);
        const u64 key = ((u64)fkey(dist) << 32) | ((u64)id << 1);
        bool pass = lane < cnt;
        if (m >= K) pass = pass && ((key | 1ull) < (top[K - 1] | 1ull));
        int p0;
        m = wave_merge<u64 *, false>(top, m, K, pass, key, cand_key, &p0);
        scored += (unsigned long long)cnt;
      }
      if (cnt < 64) break;
    }
    for (int j = lane; j < K; j += 64) {
      uint32_t id = A.pad_id;
      float dist = 3.402823466e+38f;  // std::numeric_limits<float>::max(), as k_finalize pads
      if (j < m) {
        const u64 e = top[j];
        id = (uint32_t)e >> 1;
        dist = funkey((uint32_t)(e >> 32));
      }
      A.ids[q * K + j] = id;
      A.dists[q * K + j] = dist;
    }
    WAVE_SYNC();
  }
  if (lane == 0 && scored) atomicAdd(A.rows_scored, scored);
}

static thread_local const char *g_refine_err = "";
const char *refine_launch_last_error() { return g_refine_err; }

static int refine_check(hipError_t e) {
  if (e != hipSuccess) {
    g_refine_err = hipGetErrorString(e);
    return 1;
  }
  return 0;
}

template <int METRIC>
static int launch_refine_t(const RefineArgs &a, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
  auto kern = k_refine<METRIC>;
  if (lds > (size_t)kLdsNoAttribute)
    if (refine_check(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))) return 1;
  hipLaunchKernelGGL(kern, grid, block, lds, s, a);
  return refine_check(hipGetLastError());
}

int launch_refine(const RefineArgs &a, int num_cus, void *stream) {
  if (a.nq <= 0) return 0;
  const size_t lds = (size_t)refine_lds_bytes(query_words(a.ix), a.k);
  // as many workgroups as the chip holds at once (by LDS, at most eight four-wave workgroups a CU), no more than the queries need
  const int per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(8, kLdsPerWorkgroup / (int64_t)lds));
  const int64_t blocks = std::min<int64_t>((a.nq + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)std::max(num_cus, 1) * per_cu);
  dim3 grid((unsigned)blocks), block(64 * kWavesPerBlock);
  return a.ix.metric == 1 ? launch_refine_t<1>(a, grid, block, lds, (hipStream_t)stream) : launch_refine_t<0>(a, grid, block, lds, (hipStream_t)stream);
}

}  // namespace wann
