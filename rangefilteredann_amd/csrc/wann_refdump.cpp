// wann_refdump.cpp -- the reference's words (wann_refdump.h): pure host text, no HIP.
#include "wann_refdump.h"

#include <algorithm>

using namespace wann;

namespace wann_host {

void print_outside_range(FILE *out, const float *ranges, int64_t nq, float first_label, float last_label, int digits) {
  for (int64_t q = 0; q < nq; q++)
    if (ranges[2 * (size_t)q + 1] < first_label || ranges[2 * (size_t)q] > last_label)
      fprintf(out, "Query range is entirely outside the index range (%.*g, %.*g) index range vs. (%.*g, %.*g) This shouldn't happen but does not directly "
              "impact correctness\n", digits, first_label, digits, last_label, digits, ranges[2 * (size_t)q], digits, ranges[2 * (size_t)q + 1]);
}

// what the descent noted for the query's task `task_index`, printed before that task (entries are in emission order).
// Returns whether the super tree's descent ended among them (its second timing line follows the query's searches).
static bool route_lines(FILE *out, const int64_t *rq, int task_index) {
  bool timed_search = false;
  const int64_t rwords = rq ? rq[0] : 0;
  for (int64_t o = 0; o + 7 <= rwords; o += 7) {
    const int64_t *e = rq + 1 + o;
    if (e[1] != task_index) continue;
    if (e[0] == 1) fprintf(out, "Testing bucket %lld\n", (long long)e[2]);
    else if (e[0] == 2)
      fprintf(out, "Query range = (%lld,%lld), smallest containing range (size %lld) = (%lld,%lld)\n", (long long)e[2], (long long)e[3], (long long)e[6],
              (long long)e[4], (long long)e[5]);
    else if (e[0] == 3) {
      fprintf(out, "Time to find bucket: 0ns\n");
      timed_search = true;
    } else if (e[0] == 4) fprintf(out, "Query range: %lld %lld\n", (long long)e[2], (long long)e[3]);
    else if (e[0] == 5) fprintf(out, "Searching bucket: %lld %lld\n", (long long)e[2], (long long)e[3]);
  }
  return timed_search;
}

// record j of a task's doubling loop: unfiltered return m_, frontier size f_
static void rec(const unsigned long long *task_log, int j, long long &m_, long long &f_) {
  const unsigned long long v = task_log[j];
  m_ = (long long)((v >> 21) & 0x1fffff);
  f_ = (long long)(v & 0x1fffff);
}

void print_verbose_dump(FILE *out, const VerboseDump &d) {
  for (int64_t q = 0; q < d.nq; q++) {
    const int64_t *rq = d.vroute ? d.vroute + (size_t)q * d.vroute_words : nullptr;
    bool timed_search = false;
    for (int i = 0; i <= d.qtask_cnt[(size_t)q]; i++) {
      timed_search |= route_lines(out, rq, i);
      if (i == d.qtask_cnt[(size_t)q]) break;
      const size_t ti = (size_t)q * d.maxt + i;
      const Task &t = d.tasks[ti];
      if (t.mode != T_GRAPH || !d.vlog) continue;
      const long long mult = (t.flags & 2) ? 1 : d.final_beam_multiply;
      fprintf(out, "Starting optimized postfiltering, beam size = %lld, k = %lld, final multiply = %lld, n = %d\n", d.beam_width, d.k, mult,
              d.parts[(size_t)t.part].n);
      long long beam = d.beam_width, frontier = 0;
      int e = 0;
      const int ne = std::min(d.vlog_n[ti], d.vlog_cap);
      const unsigned long long *task_log = d.vlog + ti * (size_t)d.vlog_cap;
      while (frontier < d.k && beam < d.postfiltering_max_beam && e < ne) {  // :161-172
        long long m_, f_;
        rec(task_log, e++, m_, f_);
        fprintf(out, "Unfiltered return = %lld\n", m_);
        frontier = f_;
        fprintf(out, "Finished a double, frontier size = %lld, beam size = %lld\n", frontier, beam);
        if (frontier < d.k) beam *= 2;
      }
      const long long fb = std::min<long long>(beam * mult, d.postfiltering_max_beam);
      if (fb > beam) {  // :173-181 (the final re-search; should its record be missing -- more searches than records -- the
        if (e < ne) {   // line below still names the beam the reference would)
          long long m_, f_;
          rec(task_log, e++, m_, f_);
          fprintf(out, "Unfiltered return = %lld\n", m_);
          frontier = f_;
        }
        beam = fb;
      }
      fprintf(out, "Final frontier size = %lld, final beam size %lld\n", frontier, beam);
    }
    if (timed_search) fprintf(out, "Time to do searcht: %lldns\n", d.per_query_ns);
  }
}

}  // namespace wann_host
