// wann_refdump.h -- the text the product prints in the reference's name: the message for a window outside the index's label
// range and the QueryParams::verbose dump.  Host data in, lines out to a FILE * (production: stdout); no HIP header, so the
// words are tested without a device (host_sanitize_test.cpp).  The copies from the device, the one-dump-at-a-time lock and
// the flushes are the batch driver's (wann_batch.cpp).
#pragma once
#include <cstdint>
#include <cstdio>

#include "wann_device.h"

namespace wann_host {

// range_filter_tree.h:191-203, super_optimized_postfilter_tree.h:173-184: one line for every query whose window [ranges[2q],
// ranges[2q+1]] lies outside [first_label, last_label].  digits: the precision the reference's std::cout has by then (4 or 6).
void print_outside_range(FILE *out, const float *ranges, int64_t nq, float first_label, float last_label, int digits);

// The reference's dump (postfilter_vamana.h:155-185 + :230), per query and partition search, in query order, with the tree
// classes' own lines (range_filter_tree.h:452-457, super_optimized_postfilter_tree.h:226-267) around the searches.
struct VerboseDump {
  int64_t nq;
  int maxt;                       // task slots per query
  const wann::Task *tasks;        // [nq * maxt]
  const int32_t *qtask_cnt;       // [nq] tasks of each query
  const int32_t *vlog_n;          // [nq * maxt] records of each task's doubling loop
  const unsigned long long *vlog; // [nq * maxt * vlog_cap] (beam << 42 | unfiltered << 21 | frontier); null: no searches to dump
  int vlog_cap;
  const int64_t *vroute;          // [nq * vroute_words] the descent's entries (RouteArgs::vroute); null: none
  int vroute_words;
  const wann::PartDesc *parts;    // (their sizes: the n of a search's first line)
  long long per_query_ns;         // the figure of the super tree's "Time to do searcht" line
  long long k, beam_width, final_beam_multiply, postfiltering_max_beam;  // of the call's QueryParams
};
void print_verbose_dump(FILE *out, const VerboseDump &d);

}  // namespace wann_host
