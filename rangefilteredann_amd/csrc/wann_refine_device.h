// wann_refine_device.h -- what the refine kernel (wann_refine_kernels.hip) shares with the host side (wann_abi.cpp): the
// launch arguments, the launcher and the ONE formula of its LDS footprint.  See include/wann.h (wann_set_refine_rows,
// wann_batch_search_device_refined) and DESIGN.md 3.12.
#pragma once
#include "wann_device.h"

namespace wann {

// k_refine<METRIC>: one wave per query.  The candidates of query q are the entries of cand_ids / cand_dists[q][0 .. refine_k)
// before the first pad (id == pad_id and dist == FLT_MAX; pads are a suffix); each is scored against rows[id] -- the
// full-precision row store, float32 rows of `ix.stride` words, indexed by RETURNED id -- and the k smallest under
// (distance, id) go to ids / dists[q][0 .. k), followed by pads.
struct RefineArgs {
  IndexView ix;  // points = the row store, n, d, stride, metric; dtype 0 (float32 rows): nothing else is read
  const float *queries;  // (nq, d) row-major fp32, unpadded
  const uint32_t *cand_ids;  // [nq][refine_k]
  const float *cand_dists;   // [nq][refine_k]
  int64_t nq;
  int32_t refine_k, k;
  uint32_t pad_id;
  uint32_t *ids;  // [nq][k]
  float *dists;   // [nq][k]
  unsigned long long *rows_scored;  // += candidates scored (pads excluded)
};

// Bytes of LDS one wave of k_refine needs, and a workgroup of kWavesPerBlock waves: the carve of k_brute -- the staged query
// (`row_words` 32-bit words: the store's row pitch, d rounded up to 16), 64 candidate keys, ids and distances, and the list of
// k keys.  The kernel carves by it, launch_refine sizes the launch by it and the C ABI refuses with WANN_ERR_UNSUPPORTED what
// exceeds kLdsPerWorkgroup before anything is launched.
constexpr int64_t refine_lds_bytes_per_wave(int64_t row_words, int k) { return brute_lds_bytes_per_wave(row_words, k); }
constexpr int64_t refine_lds_bytes(int64_t row_words, int k) { return refine_lds_bytes_per_wave(row_words, k) * kWavesPerBlock; }
// the row pitch of the store in 32-bit words: the float32 index's, d rounded up to 16 floats (64 bytes)
constexpr int64_t refine_row_words(int64_t d) { return ((d + 15) / 16) * 16; }

// asynchronous on `stream`; 0 on success (else refine_launch_last_error)
int launch_refine(const RefineArgs &a, int num_cus, void *stream);
const char *refine_launch_last_error();

}  // namespace wann
