// window_ann_pybind.cpp -- pybind11 shim over the C ABI (include/wann.h) that re-exports the
// Python surface of the reference's `window_ann` module for the window-search path
// (python_bindings/python_bindings.cpp:111-157,204-213 of JoshEngels/RangeFilteredANN):
// same class names, constructor keywords, batch_search signatures and return tuple, so
// experiments/wrapper.py and run_our_method.py drive this engine unchanged.
//
// Everything computes on the GPU through libwann.so; without a gfx950 device constructors raise.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <optional>
#include <stdexcept>
#include <string>
#include <vector>
#include <cstdio>

#include "../../include/wann.h"
#include "wann_bf16.h"
#include "wann_f8.h"

namespace py = pybind11;
using namespace pybind11::literals;

namespace wannpy {

struct BuildParams {  // python_bindings.cpp:211-213
  long max_degree, limit;
  double alpha;
  std::string cache_path;
  BuildParams(long R, long L, double a, std::string c) : max_degree(R), limit(L), alpha(a), cache_path(std::move(c)) {}
};

struct QueryParams {  // python_bindings.cpp:204-209
  wann_query_params c{};
  QueryParams(long k, long beam, double cut, long limit, long degree_limit, long final_beam_multiply,
              long postfiltering_max_beam, std::optional<float> ratio, bool verbose) {
    c.k = k;
    c.beam_width = beam;
    c.cut = cut;
    c.limit = limit;
    c.degree_limit = degree_limit;
    c.final_beam_multiply = final_beam_multiply;
    c.postfiltering_max_beam = postfiltering_max_beam;
    c.has_min_query_to_bucket_ratio = ratio.has_value();
    c.min_query_to_bucket_ratio = ratio.value_or(0.f);
    c.verbose = verbose;
  }
};

static const BuildParams &default_build_params() {  // python_bindings.cpp:88
  static BuildParams bp(64, 500, 1.175, "index_cache");
  return bp;
}

[[noreturn]] static void raise_last(const char *what) {
  throw std::runtime_error(std::string(what) + ": " + wann_last_error());
}

using FArray = py::array_t<float, py::array::c_style | py::array::forcecast>;

// numpy has no bfloat16: any array numpy casts to float32 -> the uint16 bit patterns of its values rounded to bfloat16 (nearest,
// ties to even: float_to_bf16).  VALUES are rounded, whatever the array's dtype: an integer array is never read as bit patterns.
static py::array bf16_bits_of(const py::handle &a) {
  FArray f = FArray::ensure(a);
  if (!f) return py::array();
  py::array_t<uint16_t> out(std::vector<py::ssize_t>(f.shape(), f.shape() + f.ndim()));
  const float *src = f.data();
  uint16_t *dst = out.mutable_data();
  for (py::ssize_t i = 0, n = f.size(); i < n; i++) dst[i] = wann::float_to_bf16(src[i]);
  return std::move(out);
}

// numpy has no float8 either: any array numpy casts to float32 -> the uint8 bit patterns of its values rounded to OCP E4M3
// (nearest, ties to even; what rounds above 448, infinities and NaN become the NaN pattern: float_to_f8 -- an index refuses those).
// VALUES are rounded, whatever the array's dtype: a uint8 array is never read as bit patterns.
static py::array f8_bits_of(const py::handle &a) {
  FArray f = FArray::ensure(a);
  if (!f) return py::array();
  py::array_t<uint8_t> out(std::vector<py::ssize_t>(f.shape(), f.shape() + f.ndim()));
  const float *src = f.data();
  uint8_t *dst = out.mutable_data();
  for (py::ssize_t i = 0, n = f.size(); i < n; i++) dst[i] = wann::float_to_f8(src[i]);
  return std::move(out);
}

// any array -> a C-contiguous array of the element type `dtype` (py::array_t<T>::ensure semantics; float16, which pybind11 has no
// C++ type for, through numpy: astype rounds to nearest, ties to even; bfloat16: bf16_bits_of; float8: f8_bits_of)
static py::array as_elem(int dtype, const py::handle &a) {
  if (dtype == WANN_DTYPE_F8) return f8_bits_of(a);
  if (dtype == WANN_DTYPE_BF16) return bf16_bits_of(a);
  if (dtype == WANN_DTYPE_F16) return py::module_::import("numpy").attr("ascontiguousarray")(a, "dtype"_a = "float16");
  if (dtype == WANN_DTYPE_F32) return FArray::ensure(a);
  if (dtype == WANN_DTYPE_U8) return py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(a);
  return py::array_t<int8_t, py::array::c_style | py::array::forcecast>::ensure(a);
}
using NeighborsAndDistances = std::pair<py::array_t<unsigned int>, py::array_t<float>>;

class Index {
 public:
  Index(int kind, int metric, int dtype, py::array points, FArray labels, int32_t cutoff, double split,
        double shift, const BuildParams &bp)
      : kind_(kind), dtype_(dtype) {
    // py::array_t<T> semantics of the reference (python_bindings.cpp:113,121,...): any array is cast to T
    py::array pts = as_elem(dtype, points);
    if (!pts) throw std::runtime_error("points must be convertible to an array of the index's element type");
    if (pts.ndim() != 2) throw std::runtime_error("points numpy array must be 2-dimensional");           // tree_utils.h:46
    if (labels.ndim() != 1) throw std::runtime_error("filter data numpy array must be 1-dimensional");    // tree_utils.h:53
    if (labels.shape(0) != pts.shape(0))
      throw std::runtime_error("filter data numpy array must have the same number of elements as the points array");
    wann_build_params wb{bp.max_degree, bp.limit, bp.alpha, bp.cache_path.c_str()};
    const void *pp = pts.data();
    const float *lp = labels.data();
    int64_t n = pts.shape(0), d = pts.shape(1);
    {
      py::gil_scoped_release nogil;
      h_ = wann_index_create(kind, metric, dtype, pp, n, d, lp, cutoff, split, shift, &wb, device_from_env(), 0);
    }
    if (!h_) raise_last("index construction failed");
  }
  ~Index() { wann_index_destroy(h_); }
  Index(const Index &) = delete;
  Index &operator=(const Index &) = delete;

  static int device_from_env() {
    // one process per GPU: LOCAL_RANK selects the device unless WANN_DEVICE overrides it
    if (const char *e = getenv("WANN_DEVICE")) return atoi(e);
    int ndev = wann_device_count();
    if (const char *e = getenv("LOCAL_RANK")) return ndev > 0 ? atoi(e) % ndev : 0;
    return 0;
  }

  NeighborsAndDistances search(py::array queries_in, py::object filters, uint64_t nq, const std::string &method,
                               const QueryParams &qp) {
    FArray fr = FArray::ensure(filters);
    if (!fr) throw std::runtime_error("filters must be a sequence of (lo, hi) pairs");
    if (fr.ndim() != 2 || fr.shape(1) != 2 || (uint64_t)fr.shape(0) < nq)
      throw std::runtime_error("filters must have shape (num_queries, 2)");
    py::array queries = as_elem(dtype_, queries_in);
    if (!queries) throw std::runtime_error("queries must be convertible to an array of the index's element type");
    if (queries.ndim() != 2 || (uint64_t)queries.shape(0) < nq || queries.shape(1) != wann_dim(h_))
      throw std::runtime_error("queries must have shape (num_queries, dimension)");
    size_t k = (size_t)qp.c.k;
    py::array_t<unsigned int> ids({(size_t)nq, k});
    py::array_t<float> dists({(size_t)nq, k});
    const void *qptr = queries.data();
    const float *rptr = fr.data();
    unsigned int *ip = ids.mutable_data();
    float *dp = dists.mutable_data();
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_batch_search(h_, qptr, rptr, (int64_t)nq, method.c_str(), &qp.c, ip, dp);
    }
    if (rc) raise_last("batch_search failed");
    return std::make_pair(ids, dists);
  }

  // the wide host-buffer call (wann.h WIDE ROWS): batch_search's arguments, rows of `width` columns from the search that stops as
  // at query_params.k
  NeighborsAndDistances search_wide(py::array queries_in, py::object filters, uint64_t nq, const std::string &method, const QueryParams &qp,
                                    int64_t width) {
    FArray fr = FArray::ensure(filters);
    if (!fr) throw std::runtime_error("filters must be a sequence of (lo, hi) pairs");
    if (fr.ndim() != 2 || fr.shape(1) != 2 || (uint64_t)fr.shape(0) < nq)
      throw std::runtime_error("filters must have shape (num_queries, 2)");
    py::array queries = as_elem(dtype_, queries_in);
    if (!queries) throw std::runtime_error("queries must be convertible to an array of the index's element type");
    if (queries.ndim() != 2 || (uint64_t)queries.shape(0) < nq || queries.shape(1) != wann_dim(h_))
      throw std::runtime_error("queries must have shape (num_queries, dimension)");
    // (a width the library refuses gets empty rows: the call below fails before it touches them)
    const size_t w = (width >= 1 && width <= 1024) ? (size_t)width : 0;
    py::array_t<unsigned int> ids({(size_t)nq, w});
    py::array_t<float> dists({(size_t)nq, w});
    const void *qptr = queries.data();
    const float *rptr = fr.data();
    unsigned int *ip = ids.mutable_data();
    float *dp = dists.mutable_data();
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_batch_search_wide(h_, qptr, rptr, (int64_t)nq, method.c_str(), &qp.c, width, ip, dp);
    }
    if (rc) raise_last("batch_search_wide failed");
    return std::make_pair(ids, dists);
  }
  // ... and the device-resident one (ids / dists are num_queries x width)
  void search_device_wide(uint64_t q_ptr, uint64_t r_ptr, int64_t nq, int64_t query_id_base, const std::string &method, const QueryParams &qp,
                          int64_t width, uint64_t ids_ptr, uint64_t dists_ptr, uint64_t stream) {
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_batch_search_device_wide(h_, (const void *)q_ptr, (const float *)r_ptr, nq, query_id_base, method.c_str(), &qp.c, width,
                                         (uint32_t *)ids_ptr, (float *)dists_ptr, (void *)stream);
    }
    if (rc) raise_last("batch_search_device_wide failed");
  }

  // device-resident call: every *_ptr is a device address on this index's GPU (e.g. torch .data_ptr())
  void search_device(uint64_t q_ptr, uint64_t r_ptr, int64_t nq, int64_t query_id_base, const std::string &method,
                     const QueryParams &qp, uint64_t ids_ptr, uint64_t dists_ptr, uint64_t stream) {
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_batch_search_device(h_, (const void *)q_ptr, (const float *)r_ptr, nq, query_id_base, method.c_str(),
                                    &qp.c, (uint32_t *)ids_ptr, (float *)dists_ptr, (void *)stream);
    }
    if (rc) raise_last("batch_search_device failed");
  }

  // ... for queries that are not a contiguous range of their batch: query_ids_ptr = device array of their global row numbers (int64)
  void search_device_ids(uint64_t q_ptr, uint64_t r_ptr, int64_t nq, uint64_t qids_ptr, const std::string &method, const QueryParams &qp,
                         uint64_t ids_ptr, uint64_t dists_ptr, uint64_t stream) {
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_batch_search_device_ids(h_, (const void *)q_ptr, (const float *)r_ptr, nq, (const int64_t *)qids_ptr, method.c_str(), &qp.c,
                                        (uint32_t *)ids_ptr, (float *)dists_ptr, (void *)stream);
    }
    if (rc) raise_last("batch_search_device_ids failed");
  }

  // asynchronous device-resident call: returns a ticket at once; wait(ticket) blocks until that batch's rows are in place
  int64_t search_device_async(uint64_t q_ptr, uint64_t r_ptr, int64_t nq, int64_t query_id_base, const std::string &method,
                              const QueryParams &qp, uint64_t ids_ptr, uint64_t dists_ptr, uint64_t after_stream) {
    int64_t ticket = -1;
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_batch_search_device_async(h_, (const void *)q_ptr, (const float *)r_ptr, nq, query_id_base, method.c_str(), &qp.c,
                                          (uint32_t *)ids_ptr, (float *)dists_ptr, (void *)after_stream, &ticket);
    }
    if (rc) raise_last("batch_search_device_async failed");
    return ticket;
  }
  // predicted work per query (hops) of a batch of windows: what a cost-balanced shard cut balances
  py::array_t<float> predict_costs(py::array_t<float, py::array::c_style | py::array::forcecast> filters, const std::string &method,
                                   const QueryParams &qp) {
    if (filters.ndim() != 2 || filters.shape(1) != 2) throw std::runtime_error("filters must be (num_queries, 2)");
    const int64_t nq = filters.shape(0);
    py::array_t<float> out(nq);
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_predict_costs(h_, filters.data(), nq, method.c_str(), &qp.c, out.mutable_data());
    }
    if (rc) raise_last("predict_costs failed");
    return out;
  }
  py::dict wait(int64_t ticket) {
    wann_counters c;
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = wann_wait(h_, ticket, &c);
    }
    if (rc) raise_last("wait failed");
    py::dict d = counters_dict(c);
    d["half_rows"] = wann_last_half_rows(h_);
    d["byte_rows"] = wann_last_byte_rows(h_);
    d["scan_rows"] = wann_last_scan_rows(h_);
    d["dense_rows"] = wann_last_dense_rows(h_);
    return d;
  }
  // a row switch's setter (wann_set_*_rows): the setting now in force
  bool set_row_switch(int (*set)(wann_index *, int), bool on, const char *what) {
    const int rc = set(h_, on ? 1 : 0);
    if (rc < 0) raise_last(what);
    return rc != 0;
  }
  // float32 indexes with graphs whose points are all binary16 values: the beam searches read a half-precision copy of the rows
  // (wann_set_half_rows); returns the setting now in force -- False on an index without such a copy
  bool set_half_rows(bool on) { return set_row_switch(wann_set_half_rows, on, "set_half_rows failed"); }
  bool half_rows() const { return wann_half_rows(h_) != 0; }
  int64_t half_rows_bytes() const { return wann_half_rows_bytes(h_); }
  // ... and whose points are all integers 0 .. 255: the beam searches read a one-byte copy of the rows instead, once asked to
  // (wann_set_byte_rows, off by default); returns the setting now in force -- False on an index without such a copy
  bool set_byte_rows(bool on) { return set_row_switch(wann_set_byte_rows, on, "set_byte_rows failed"); }
  bool byte_rows() const { return wann_byte_rows(h_) != 0; }
  int64_t byte_rows_bytes() const { return wann_byte_rows_bytes(h_); }
  // the exact scans read the shadow copy the beam searches read (wann_set_scan_rows, off by default); returns the setting now
  // in force -- False on an index without a shadow copy
  bool set_scan_rows(bool on) { return set_row_switch(wann_set_scan_rows, on, "set_scan_rows failed"); }
  bool scan_rows() const { return wann_scan_rows(h_) != 0; }
  // the score launches of the dense path read the one-byte copy of a float32 index of byte-exact points (wann_set_dense_rows, off
  // by default); returns the setting now in force -- False on an index without a copy that path can read
  bool set_dense_rows(bool on) { return set_row_switch(wann_set_dense_rows, on, "set_dense_rows failed"); }
  bool dense_rows() const { return wann_dense_rows(h_) != 0; }
  int64_t dense_rows_bytes() const { return wann_dense_rows_bytes(h_); }

  // float16 / bfloat16 / float8 indexes: the full-precision points (any array numpy casts to float32, in the order of the array
  // the index was created from) as the row store of the refined calls (wann_set_refine_rows); None drops the store
  void set_refine_rows(py::object points) {
    int rc;
    if (points.is_none()) {
      rc = wann_set_refine_rows(h_, nullptr, 0, 0);
    } else {
      FArray pts = FArray::ensure(points);
      if (!pts) throw std::runtime_error("refine rows must be convertible to a float32 array");
      if (pts.ndim() != 2) throw std::runtime_error("refine rows numpy array must be 2-dimensional");
      const float *pp = pts.data();
      const int64_t n = pts.shape(0), d = pts.shape(1);
      py::gil_scoped_release nogil;
      rc = wann_set_refine_rows(h_, pp, n, d);
    }
    if (rc) raise_last("set_refine_rows failed");
  }
  int64_t refine_rows_bytes() const { return wann_refine_rows_bytes(h_); }
  // the refined host-buffer call: FLOAT32 queries (not rounded to the index's element type), refine_k >= k candidates from the
  // compact rows re-ranked against the refine rows
  // stop_k (None: refine_k, the search at k = refine_k): the search stops as at k = stop_k and the re-rank sees up to refine_k
  // entries of that frontier (wann_batch_search_refined_stop)
  NeighborsAndDistances search_refined(py::object queries_in, py::object filters, uint64_t nq, const std::string &method, const QueryParams &qp,
                                       int64_t refine_k, std::optional<int64_t> stop_k) {
    FArray fr = FArray::ensure(filters);
    if (!fr) throw std::runtime_error("filters must be a sequence of (lo, hi) pairs");
    if (fr.ndim() != 2 || fr.shape(1) != 2 || (uint64_t)fr.shape(0) < nq) throw std::runtime_error("filters must have shape (num_queries, 2)");
    FArray queries = FArray::ensure(queries_in);
    if (!queries) throw std::runtime_error("queries must be convertible to a float32 array");
    if (queries.ndim() != 2 || (uint64_t)queries.shape(0) < nq || queries.shape(1) != wann_dim(h_))
      throw std::runtime_error("queries must have shape (num_queries, dimension)");
    if (qp.c.k < 1) throw std::runtime_error("k must be in [1, 1024]");
    size_t k = (size_t)qp.c.k;
    py::array_t<unsigned int> ids({(size_t)nq, k});
    py::array_t<float> dists({(size_t)nq, k});
    const float *qptr = queries.data(), *rptr = fr.data();
    unsigned int *ip = ids.mutable_data();
    float *dp = dists.mutable_data();
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = stop_k ? wann_batch_search_refined_stop(h_, qptr, rptr, (int64_t)nq, method.c_str(), &qp.c, refine_k, *stop_k, ip, dp)
                  : wann_batch_search_refined(h_, qptr, rptr, (int64_t)nq, method.c_str(), &qp.c, refine_k, ip, dp);
    }
    if (rc) raise_last("batch_search_refined failed");
    return std::make_pair(ids, dists);
  }
  // ... and the device-resident one (every *_ptr a device address on this index's GPU; ids / dists are num_queries x k)
  void search_device_refined(uint64_t q_ptr, uint64_t r_ptr, int64_t nq, int64_t query_id_base, const std::string &method, const QueryParams &qp,
                             int64_t refine_k, uint64_t ids_ptr, uint64_t dists_ptr, uint64_t stream, std::optional<int64_t> stop_k) {
    int rc;
    {
      py::gil_scoped_release nogil;
      rc = stop_k ? wann_batch_search_device_refined_stop(h_, (const void *)q_ptr, (const float *)r_ptr, nq, query_id_base, method.c_str(), &qp.c,
                                                          refine_k, *stop_k, (uint32_t *)ids_ptr, (float *)dists_ptr, (void *)stream)
                  : wann_batch_search_device_refined(h_, (const void *)q_ptr, (const float *)r_ptr, nq, query_id_base, method.c_str(), &qp.c,
                                                     refine_k, (uint32_t *)ids_ptr, (float *)dists_ptr, (void *)stream);
    }
    if (rc) raise_last("batch_search_device_refined failed");
  }
  py::dict refine_counters() const {
    wann_refine_counters c;
    if (wann_get_refine_counters(h_, &c)) raise_last("refine_counters failed");
    py::dict d;
    d["refined_queries"] = c.refined_queries;
    d["refined_rows"] = c.refined_rows;
    d["refine_ms"] = c.refine_ms;
    return d;
  }

  // PrefilterIndex only: distinct wide windows on the matrix cores (wann_set_dense_windows); returns the previous setting
  bool set_dense_windows(bool on) {
    const int rc = wann_set_dense_windows(h_, on ? 1 : 0);
    if (rc < 0) raise_last("set_dense_windows failed");
    return rc != 0;
  }
  py::dict dense_window_counters() const {
    wann_dense_window_counters c;
    if (wann_get_dense_window_counters(h_, &c)) raise_last("dense_window_counters failed");
    py::dict d;
    d["queries"] = c.queries;
    d["unproven"] = c.unproven;
    d["rescued"] = c.rescued;
    d["groups"] = c.groups;
    d["tiles"] = c.tiles;
    d["passes"] = c.passes;
    d["handover_bytes"] = c.handover_bytes;
    return d;
  }
  // graph-backed tree indexes only: exact answers for windows of at most max_points points (wann_set_exact_windows; 0 = off);
  // returns the previous limit
  int64_t set_exact_windows(int64_t max_points) {
    const int64_t rc = wann_set_exact_windows(h_, max_points);
    if (rc < 0) raise_last("set_exact_windows failed");
    return rc;
  }
  py::dict exact_window_counters() const {
    wann_exact_window_counters c;
    if (wann_get_exact_window_counters(h_, &c)) raise_last("exact_window_counters failed");
    py::dict d;
    d["queries"] = c.queries;
    d["dense_queries"] = c.dense_queries;
    d["unproven"] = c.unproven;
    d["rescued"] = c.rescued;
    d["passes"] = c.passes;
    d["rows_scanned"] = c.rows_scanned;
    return d;
  }
  py::dict counters() const {
    wann_counters c;
    wann_get_counters(h_, &c);
    py::dict d = counters_dict(c);
    d["half_rows"] = wann_last_half_rows(h_);  // 1: the last batch's beam searches read the half-precision shadow rows
    d["byte_rows"] = wann_last_byte_rows(h_);  // 1: they read the one-byte shadow rows (then half_rows is 0)
    d["scan_rows"] = wann_last_scan_rows(h_);  // the rows its k_brute launch read: 0 the index's own, 1 the half rows, 2 the one-byte rows
    d["dense_rows"] = wann_last_dense_rows(h_);  // 1: a score launch of its dense path read the one-byte copy of the rows
    return d;
  }
  static py::dict counters_dict(const wann_counters &c) {
    py::dict d;
    d["beam_searches"] = c.beam_searches;
    d["hops"] = c.hops;
    d["dist_cmps"] = c.dist_cmps;
    d["brute_rows"] = c.brute_rows;
    d["label_reads"] = c.label_reads;
    d["rounds"] = c.rounds;
    d["spec_searches"] = c.spec_searches;
    d["spec_hops"] = c.spec_hops;
    d["spec_dist_cmps"] = c.spec_dist_cmps;
    d["gemm_queries"] = c.gemm_queries;
    d["gemm_unproven"] = c.gemm_unproven;
    d["gemm_rescued"] = c.gemm_rescued;
    d["deep_handoffs"] = c.deep_handoffs;
    d["lookaheads_used"] = c.lookaheads_used;
    d["big_searches"] = c.big_searches;
    d["big_hops"] = c.big_hops;
    d["packet_hops"] = c.packet_hops;
    d["own_scorings"] = c.own_scorings;
    d["prefetched_hops"] = c.prefetched_hops;
    d["poll_timeouts"] = c.poll_timeouts;
    d["lookaheads_issued"] = c.lookaheads_issued;
    d["recovered_continuations"] = c.recovered_continuations;
    d["device_ms"] = c.device_ms;
    d["search_kernel_ms"] = c.search_kernel_ms;
    return d;
  }
  std::vector<int64_t> levels() const {
    std::vector<int64_t> v;
    for (int64_t l = 0; l < wann_num_levels(h_); l++) v.push_back(wann_level_size(h_, l));
    return v;
  }
  std::pair<int64_t, int64_t> partition_range(int64_t level, int64_t idx) const {
    int64_t s, e;
    if (wann_partition_range(h_, level, idx, &s, &e)) raise_last("partition_range");
    return {s, e};
  }
  int64_t max_degree() const { return wann_max_degree(h_); }
  py::array_t<int32_t> partition_graph(int64_t level, int64_t idx, int64_t max_degree) const {
    auto [s, e] = partition_range(level, idx);
    py::array_t<int32_t> rows({(size_t)(e - s), (size_t)(max_degree + 1)});
    if (wann_partition_graph(h_, level, idx, rows.mutable_data(), e - s, max_degree)) raise_last("partition_graph");
    return rows;
  }
  int64_t device_bytes() const { return wann_device_bytes(h_); }
  int num_replicas() const { return wann_num_replicas(h_); }
  int64_t num_points() const { return wann_num_points(h_); }
  int64_t dim() const { return wann_dim(h_); }

 private:
  int kind_, dtype_;
  wann_index *h_ = nullptr;
};

template <int KIND, int METRIC, int DTYPE>
struct IndexT : Index {
  using Index::Index;
};

template <typename C>
static void common_defs(py::class_<C> &c) {
  c.def("batch_search_device", &C::search_device, "queries_ptr"_a, "filters_ptr"_a, "num_queries"_a,
        "query_id_base"_a, "query_method"_a, "query_params"_a, "ids_ptr"_a, "dists_ptr"_a, "stream"_a = 0)
      .def("batch_search_device_ids", &C::search_device_ids, "queries_ptr"_a, "filters_ptr"_a, "num_queries"_a, "query_ids_ptr"_a, "query_method"_a,
           "query_params"_a, "ids_ptr"_a, "dists_ptr"_a, "stream"_a = 0)
      .def("batch_search_device_async", &C::search_device_async, "queries_ptr"_a, "filters_ptr"_a, "num_queries"_a, "query_id_base"_a,
           "query_method"_a, "query_params"_a, "ids_ptr"_a, "dists_ptr"_a, "after_stream"_a = 0)
      .def("wait", &C::wait, "ticket"_a)
      .def("predict_costs", &C::predict_costs, "filters"_a, "query_method"_a, "query_params"_a)
      .def("counters", &C::counters)
      .def("levels", &C::levels)
      .def("partition_range", &C::partition_range)
      .def("partition_graph", &C::partition_graph, "level"_a, "idx"_a, "max_degree"_a)
      .def("device_bytes", &C::device_bytes)
      .def("set_half_rows", &C::set_half_rows, "on"_a)
      .def("half_rows", &C::half_rows)
      .def("half_rows_bytes", &C::half_rows_bytes)
      .def("set_byte_rows", &C::set_byte_rows, "on"_a)
      .def("byte_rows", &C::byte_rows)
      .def("byte_rows_bytes", &C::byte_rows_bytes)
      .def("set_scan_rows", &C::set_scan_rows, "on"_a)
      .def("scan_rows", &C::scan_rows)
      .def("set_dense_rows", &C::set_dense_rows, "on"_a)
      .def("dense_rows", &C::dense_rows)
      .def("dense_rows_bytes", &C::dense_rows_bytes)
      .def("set_refine_rows", &C::set_refine_rows, "points"_a.none(true))
      .def("refine_rows_bytes", &C::refine_rows_bytes)
      .def("batch_search_refined", &C::search_refined, "queries"_a, "filters"_a, "num_queries"_a, "query_method"_a, "query_params"_a,
           "refine_k"_a, py::kw_only(), "stop_k"_a = py::none())
      .def("batch_search_device_refined", &C::search_device_refined, "queries_ptr"_a, "filters_ptr"_a, "num_queries"_a, "query_id_base"_a,
           "query_method"_a, "query_params"_a, "refine_k"_a, "ids_ptr"_a, "dists_ptr"_a, "stream"_a = 0, py::kw_only(), "stop_k"_a = py::none())
      .def("batch_search_wide", &C::search_wide, "queries"_a, "filters"_a, "num_queries"_a, "query_method"_a, "query_params"_a, "width"_a)
      .def("batch_search_wide",
           [](C &self, py::array q, py::object f, uint64_t nq, const QueryParams &qp, int64_t width) { return self.search_wide(q, f, nq, "", qp, width); },
           "queries"_a, "filters"_a, "num_queries"_a, "query_params"_a, "width"_a)
      .def("batch_search_device_wide", &C::search_device_wide, "queries_ptr"_a, "filters_ptr"_a, "num_queries"_a, "query_id_base"_a,
           "query_method"_a, "query_params"_a, "width"_a, "ids_ptr"_a, "dists_ptr"_a, "stream"_a = 0)
      .def("refine_counters", &C::refine_counters)
      .def("max_degree", &C::max_degree)
      .def("num_replicas", &C::num_replicas)
      .def("num_points", &C::num_points)
      .def("dim", &C::dim);
}

template <int METRIC, int DTYPE>
static void add_variant(py::module_ &m, const std::string &agnostic) {
  {
    using C = IndexT<WANN_KIND_PREFILTER, METRIC, DTYPE>;
    py::class_<C> c(m, ("PrefilterIndex" + agnostic).c_str());
    c.def(py::init([](py::array points, FArray fv, const BuildParams &bp) {
            return new C(WANN_KIND_PREFILTER, METRIC, DTYPE, points, fv, 1000, 2, 0.5, bp);
          }),
          "points"_a, "filter_values"_a, "build_params"_a = default_build_params())
        .def("batch_search",
             [](C &self, py::array q, py::object f, uint64_t nq, const QueryParams &qp) { return self.search(q, f, nq, "", qp); },
             "queries"_a, "filters"_a, "num_queries"_a, "query_params"_a)
        .def("set_dense_windows", &C::set_dense_windows, "on"_a)
        .def("dense_window_counters", &C::dense_window_counters);
    common_defs(c);
  }
  {
    using C = IndexT<WANN_KIND_TREE_PREFILTER, METRIC, DTYPE>;
    py::class_<C> c(m, ("RangeFilterTreeIndex" + agnostic).c_str());
    c.def(py::init([](py::array points, FArray fv, int32_t cutoff, size_t split, const BuildParams &bp) {
            return new C(WANN_KIND_TREE_PREFILTER, METRIC, DTYPE, points, fv, cutoff, (double)split, 0.5, bp);
          }),
          "points"_a, "filter_values"_a, "cutoff"_a = 1000, "split_factor"_a = 2,
          "build_params"_a = default_build_params())
        .def("batch_search",
             [](C &self, py::array q, py::object f, uint64_t nq, const std::string &method, const QueryParams &qp) {
               return self.search(q, f, nq, method, qp);
             },
             "queries"_a, "filters"_a, "num_queries"_a, "query_method"_a, "query_params"_a);
    common_defs(c);
  }
  {
    using C = IndexT<WANN_KIND_POSTFILTER, METRIC, DTYPE>;
    py::class_<C> c(m, ("PostfilterVamanaIndex" + agnostic).c_str());
    c.def(py::init([](py::array points, FArray fv, const BuildParams &bp) {
            return new C(WANN_KIND_POSTFILTER, METRIC, DTYPE, points, fv, 1000, 2, 0.5, bp);
          }),
          "points"_a, "filters"_a, "build_params"_a = default_build_params())
        .def("batch_search",
             [](C &self, py::array q, py::object f, uint64_t nq, const QueryParams &qp) { return self.search(q, f, nq, "", qp); },
             "queries"_a, "filters"_a, "num_queries"_a, "query_params"_a);
    common_defs(c);
  }
  {
    using C = IndexT<WANN_KIND_TREE_VAMANA, METRIC, DTYPE>;
    py::class_<C> c(m, ("VamanaRangeFilterTreeIndex" + agnostic).c_str());
    c.def(py::init([](py::array points, FArray fv, int32_t cutoff, size_t split, const BuildParams &bp) {
            return new C(WANN_KIND_TREE_VAMANA, METRIC, DTYPE, points, fv, cutoff, (double)split, 0.5, bp);
          }),
          "points"_a, "filter_values"_a, "cutoff"_a = 1000, "split_factor"_a = 2,
          "build_params"_a = default_build_params())
        .def("batch_search",
             [](C &self, py::array q, py::object f, uint64_t nq, const std::string &method, const QueryParams &qp) {
               return self.search(q, f, nq, method, qp);
             },
             "queries"_a, "filters"_a, "num_queries"_a, "query_method"_a, "query_params"_a)
        .def("set_exact_windows", &C::set_exact_windows, "max_points"_a)
        .def("exact_window_counters", &C::exact_window_counters);
    common_defs(c);
  }
  {
    using C = IndexT<WANN_KIND_SUPER, METRIC, DTYPE>;
    py::class_<C> c(m, ("SuperOptimizedPostfilterTreeIndex" + agnostic).c_str());
    c.def(py::init([](py::array points, FArray fv, int32_t cutoff, float split, float shift, const BuildParams &bp) {
            return new C(WANN_KIND_SUPER, METRIC, DTYPE, points, fv, cutoff, (double)split, (double)shift, bp);
          }),
          "points"_a, "filter_values"_a, "cutoff"_a = 1000, "split_factor"_a = 2, "shift_factor"_a = 0.5,
          "build_params"_a = default_build_params())
        .def("batch_search",
             [](C &self, py::array q, py::object f, uint64_t nq, const QueryParams &qp) { return self.search(q, f, nq, "", qp); },
             "queries"_a, "filters"_a, "num_queries"_a, "query_params"_a)
        .def("set_exact_windows", &C::set_exact_windows, "max_points"_a)
        .def("exact_window_counters", &C::exact_window_counters);
    common_defs(c);
  }
}

// ---- unfiltered VamanaIndex<T,Point> (ParlayANN/python/vamana_index.cpp:42-76, python_bindings.cpp:92-109) -------------
// The reference's constructor is VamanaIndex(data_path, index_path, num_points, dimensions) but its binding names the
// arguments "index_path", "data_path" in that order: the FIRST argument (keyword index_path) is the point file and the
// second (keyword data_path) the graph file.  Kept as is: positional and keyword calls behave like the reference's.
template <int METRIC, int DTYPE>
struct VamanaIndexT {
  wann_vamana *h = nullptr;
  VamanaIndexT(const std::string &first_called_index_path, const std::string &second_called_data_path, size_t num_points, size_t dimensions) {
    h = wann_vamana_open(METRIC, DTYPE, first_called_index_path.c_str(), second_called_data_path.c_str(), 0);
    if (!h) raise_last("VamanaIndex");
    // (the reference asserts these; assert() is compiled out of its release build)
    (void)num_points;
    (void)dimensions;
  }
  ~VamanaIndexT() { wann_vamana_close(h); }
  VamanaIndexT(const VamanaIndexT &) = delete;
  NeighborsAndDistances search_raw(const void *q, uint64_t nq, uint64_t knn, uint64_t beam) {
    py::array_t<unsigned int> ids({(size_t)nq, (size_t)knn});
    py::array_t<float> dists({(size_t)nq, (size_t)knn});
    if (wann_vamana_batch_search(h, q, (int64_t)nq, (int64_t)knn, (int64_t)beam, ids.mutable_data(), dists.mutable_data()))
      raise_last("batch_search");
    return {std::move(ids), std::move(dists)};
  }
  NeighborsAndDistances batch_search(py::array queries, uint64_t nq, uint64_t knn, uint64_t beam) {
    const int64_t d = wann_vamana_dim(h);
    if (DTYPE == WANN_DTYPE_F32) {
      FArray q = FArray::ensure(queries);
      if (!q || q.ndim() != 2 || q.shape(1) != d || (uint64_t)q.shape(0) < nq) throw std::runtime_error("queries must be a (num_queries, dimensions) array");
      return search_raw(q.data(), nq, knn, beam);
    }
    if (DTYPE == WANN_DTYPE_U8) {
      auto q = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(queries);
      if (!q || q.ndim() != 2 || q.shape(1) != d || (uint64_t)q.shape(0) < nq) throw std::runtime_error("queries must be a (num_queries, dimensions) array");
      return search_raw(q.data(), nq, knn, beam);
    }
    auto q = py::array_t<int8_t, py::array::c_style | py::array::forcecast>::ensure(queries);
    if (!q || q.ndim() != 2 || q.shape(1) != d || (uint64_t)q.shape(0) < nq) throw std::runtime_error("queries must be a (num_queries, dimensions) array");
    return search_raw(q.data(), nq, knn, beam);
  }
  // queries from a point file (uint32 n, uint32 d, data)
  NeighborsAndDistances batch_search_from_string(const std::string &path, uint64_t nq, uint64_t knn, uint64_t beam) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open query file " + path);
    uint32_t head[2] = {0, 0};
    const size_t esz = (size_t)wann::element_bytes(DTYPE);
    std::vector<unsigned char> raw;
    bool ok = fread(head, 4, 2, f) == 2 && (int64_t)head[1] == wann_vamana_dim(h) && head[0] >= nq;
    if (ok) {
      raw.resize((size_t)nq * head[1] * esz);
      ok = raw.empty() || fread(raw.data(), 1, raw.size(), f) == raw.size();
    }
    fclose(f);
    if (!ok) throw std::runtime_error("query file does not hold num_queries points of the index's dimension: " + path);
    return search_raw(raw.data(), nq, knn, beam);
  }
  // ground truth file: int32 n, int32 width, n*width uint32 ids, n*width float distances (types.h:33-74); recall counts
  // every ground-truth point tied with the k-th distance (vamana_index.cpp:104-132) and is printed like the reference prints it
  double check_recall(const std::string &gfile, py::array_t<unsigned int, py::array::c_style | py::array::forcecast> neighbors, int k) {
    FILE *f = fopen(gfile.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open ground truth file " + gfile);
    int32_t head[2] = {0, 0};
    if (fread(head, 4, 2, f) != 2 || head[0] < 0 || head[1] < k) {
      fclose(f);
      throw std::runtime_error("bad ground truth file " + gfile);
    }
    const size_t n = (size_t)head[0], w = (size_t)head[1];
    std::vector<uint32_t> ids(n * w);
    std::vector<float> ds(n * w);
    const bool ok = fread(ids.data(), 4, n * w, f) == n * w && fread(ds.data(), 4, n * w, f) == n * w;
    fclose(f);
    if (!ok) throw std::runtime_error("truncated ground truth file " + gfile);
    if (neighbors.ndim() != 2 || (size_t)neighbors.shape(0) < n || neighbors.shape(1) < k) throw std::runtime_error("neighbors must be (n, >= k)");
    long correct = 0;
    for (size_t i = 0; i < n; i++) {
      size_t cnt = (size_t)k;
      while (cnt < w && ds[i * w + cnt] == ds[i * w + k - 1]) cnt++;
      for (size_t l = 0; l < cnt; l++)
        for (int j = 0; j < k; j++)
          if (neighbors.at(i, j) == ids[i * w + l]) {
            correct++;
            break;
          }
    }
    const double recall = (float)correct / (float)((size_t)k * n);
    py::print("Recall:", recall);
    return recall;
  }
};

template <int METRIC, int DTYPE>
static void add_vamana(py::module_ &m, const std::string &lower, const std::string &cls) {
  m.def(("build_vamana_" + lower + "_index").c_str(),
        [](const std::string &distance_metric, const std::string &data_file_path, const std::string &index_output_path, uint32_t graph_degree,
           uint32_t beam_width, float alpha) {
          (void)distance_metric;  // (unused by the reference too: the variant fixes the metric)
          if (wann_vamana_build_file(METRIC, DTYPE, data_file_path.c_str(), index_output_path.c_str(), graph_degree, beam_width, alpha, 0))
            raise_last("build_vamana_index");
        },
        "distance_metric"_a, "data_file_path"_a, "index_output_path"_a, "graph_degree"_a, "beam_width"_a, "alpha"_a);
  using V = VamanaIndexT<METRIC, DTYPE>;
  py::class_<V>(m, cls.c_str())
      .def(py::init<const std::string &, const std::string &, size_t, size_t>(), "index_path"_a, "data_path"_a, "num_points"_a, "dimensions"_a)
      .def("batch_search", &V::batch_search, "queries"_a, "num_queries"_a, "knn"_a, "beam_width"_a)
      .def("batch_search_from_string", &V::batch_search_from_string, "queries"_a, "num_queries"_a, "knn"_a, "beam_width"_a)
      .def("check_recall", &V::check_recall, "gFile"_a, "neighbors"_a, "k"_a);
}

}  // namespace wannpy

PYBIND11_MODULE(_window_ann, m) {
  using namespace wannpy;
  m.doc() = "WindowANN Python bindings -- MI355X (gfx950) engine";
  m.attr("__version__") = "mi355x-dev";

  py::module_ defaults = m.def_submodule("defaults");  // python_bindings.cpp:169-175
  defaults.attr("METRIC") = "Euclidian";
  defaults.attr("ALPHA") = 1.2;
  defaults.attr("GRAPH_DEGREE") = 64;
  defaults.attr("BEAMWIDTH") = 128;

  py::class_<QueryParams>(m, "QueryParams")
      .def(py::init<long, long, double, long, long, long, long, std::optional<float>, bool>(), "k"_a, "beam_width"_a,
           "cut"_a, "limit"_a, "degree_limit"_a, "final_beam_multiply"_a, "postfiltering_max_beam"_a,
           "min_query_to_bucket_ratio"_a, "verbose"_a);
  py::class_<BuildParams>(m, "BuildParams")
      .def(py::init<long, long, double, std::string>(), "max_degree"_a, "limit"_a, "alpha"_a, "cache_path"_a);

  add_variant<WANN_METRIC_L2, WANN_DTYPE_F32>(m, "FloatEuclidian");
  add_variant<WANN_METRIC_MIPS, WANN_DTYPE_F32>(m, "FloatMips");
  add_variant<WANN_METRIC_L2, WANN_DTYPE_U8>(m, "UInt8Euclidian");
  add_variant<WANN_METRIC_MIPS, WANN_DTYPE_U8>(m, "UInt8Mips");
  add_variant<WANN_METRIC_L2, WANN_DTYPE_I8>(m, "Int8Euclidian");
  add_variant<WANN_METRIC_MIPS, WANN_DTYPE_I8>(m, "Int8Mips");
  // not a type of the reference: float16 points (wann.h WANN_DTYPE_F16), rows of the float32 index on the upcast points
  add_variant<WANN_METRIC_L2, WANN_DTYPE_F16>(m, "Float16Euclidian");
  add_variant<WANN_METRIC_MIPS, WANN_DTYPE_F16>(m, "Float16Mips");
  // likewise bfloat16 points (wann.h WANN_DTYPE_BF16): constructors and host batch_search take any array numpy casts to float32
  // and round its values to bfloat16 (a torch.bfloat16 tensor t passes through t.float().numpy() exactly)
  add_variant<WANN_METRIC_L2, WANN_DTYPE_BF16>(m, "BFloat16Euclidian");
  add_variant<WANN_METRIC_MIPS, WANN_DTYPE_BF16>(m, "BFloat16Mips");
  // and float8 points (wann.h WANN_DTYPE_F8, OCP E4M3): the same, rounded to float8 -- values out of range become NaN patterns,
  // which the constructor (and a host batch_search) refuses with the offending row: data is never silently saturated
  add_variant<WANN_METRIC_L2, WANN_DTYPE_F8>(m, "Float8Euclidian");
  add_variant<WANN_METRIC_MIPS, WANN_DTYPE_F8>(m, "Float8Mips");

  // python_bindings.cpp:67-86: builder and index names of the unfiltered Vamana variants
  add_vamana<WANN_METRIC_L2, WANN_DTYPE_F32>(m, "float_euclidian", "VamanaFloatEuclidianIndex");
  add_vamana<WANN_METRIC_MIPS, WANN_DTYPE_F32>(m, "float_mips", "VamanaFloatMipsIndex");
  add_vamana<WANN_METRIC_L2, WANN_DTYPE_U8>(m, "uint8_euclidian", "VamanaUInt8EuclidianIndex");
  add_vamana<WANN_METRIC_MIPS, WANN_DTYPE_U8>(m, "uint8_mips", "VamanaUInt8MipsIndex");
  add_vamana<WANN_METRIC_L2, WANN_DTYPE_I8>(m, "int8_euclidian", "VamanaInt8EuclidianIndex");
  add_vamana<WANN_METRIC_MIPS, WANN_DTYPE_I8>(m, "int8_mips", "VamanaInt8MipsIndex");

  // experiments/wrapper.py:245 spells the uint8 classes "Uint8" while the reference registers "UInt8"
  // (python_bindings.cpp:74-79), so its uint8 constructors raise AttributeError there; both spellings resolve here.
  for (const char *cls : {"PrefilterIndex", "RangeFilterTreeIndex", "PostfilterVamanaIndex", "VamanaRangeFilterTreeIndex",
                          "SuperOptimizedPostfilterTreeIndex"})
    for (const char *metric : {"Euclidian", "Mips"})
      m.attr((std::string(cls) + "Uint8" + metric).c_str()) = m.attr((std::string(cls) + "UInt8" + metric).c_str());

  // what a bfloat16 index stores of `a`: its values rounded to bfloat16, as uint16 bit patterns / as the float32 values they widen to
  m.def("bfloat16_bits", [](py::object a) {
    py::array b = bf16_bits_of(a);
    if (!b) throw std::runtime_error("bfloat16_bits: not convertible to a float32 array");
    return b;
  }, "a"_a);
  m.def("bfloat16_round", [](py::object a) {
    FArray f = FArray::ensure(a);
    if (!f) throw std::runtime_error("bfloat16_round: not convertible to a float32 array");
    py::array_t<float> out(std::vector<py::ssize_t>(f.shape(), f.shape() + f.ndim()));
    const float *src = f.data();
    float *dst = out.mutable_data();
    for (py::ssize_t i = 0, n = f.size(); i < n; i++) dst[i] = wann::bf16_to_float(wann::float_to_bf16(src[i]));
    return out;
  }, "a"_a);
  // what a float8 index stores of `a`: its values rounded to OCP E4M3, as uint8 bit patterns / as the float32 values they widen to
  m.def("float8_bits", [](py::object a) {
    py::array b = f8_bits_of(a);
    if (!b) throw std::runtime_error("float8_bits: not convertible to a float32 array");
    return b;
  }, "a"_a);
  m.def("float8_round", [](py::object a) {
    FArray f = FArray::ensure(a);
    if (!f) throw std::runtime_error("float8_round: not convertible to a float32 array");
    py::array_t<float> out(std::vector<py::ssize_t>(f.shape(), f.shape() + f.ndim()));
    const float *src = f.data();
    float *dst = out.mutable_data();
    for (py::ssize_t i = 0, n = f.size(); i < n; i++) dst[i] = wann::f8_to_float(wann::float_to_f8(src[i]));
    return out;
  }, "a"_a);
  m.def("device_count", [] { return wann_device_count(); });
  m.def("abi_version", [] { return wann_abi_version(); });
  // the byte of a one-byte shadow row (the device copy) at which element `e` of the row is stored; -1 for a negative e
  m.def("byte_row_position", [](int64_t e) { return wann_byte_row_position(e); }, py::arg("element"));
  // the half of a half shadow row (the device copy) at which element `e` of the row is stored; -1 for a negative e
  m.def("half_row_position", [](int64_t e) { return wann_half_row_position(e); }, py::arg("element"));
  m.def(
      "build_cache_shard",
      [](int kind, int metric, FArray points, FArray labels, int32_t cutoff, double split, double shift,
         const BuildParams &bp, int shard, int nshards, int threads) {
        if (points.ndim() != 2 || labels.ndim() != 1) throw std::runtime_error("bad shapes");
        wann_build_params wb{bp.max_degree, bp.limit, bp.alpha, bp.cache_path.c_str()};
        const float *pp = points.data();
        const float *lp = labels.data();
        int64_t n = points.shape(0), d = points.shape(1);
        int rc;
        {
          py::gil_scoped_release nogil;
          rc = wann_build_cache_shard(kind, metric, WANN_DTYPE_F32, pp, n, d, lp, cutoff, split, shift, &wb, shard,
                                      nshards, threads);
        }
        if (rc) raise_last("build_cache_shard failed");
      },
      "kind"_a, "metric"_a, "points"_a, "filter_values"_a, "cutoff"_a, "split_factor"_a, "shift_factor"_a,
      "build_params"_a, "shard"_a, "nshards"_a, "threads"_a = 0);
  m.def(
      "raw_beam_search",
      [](int metric, FArray points, py::array_t<int32_t, py::array::c_style | py::array::forcecast> graph_rows,
         int64_t subset_start, FArray queries, py::array_t<int64_t, py::array::c_style | py::array::forcecast> query_ids,
         int64_t beam, int64_t limit, int64_t degree_limit, int device) {
        if (points.ndim() != 2 || graph_rows.ndim() != 2 || queries.ndim() != 2) throw std::runtime_error("bad shapes");
        int64_t n = points.shape(0), d = points.shape(1), sn = graph_rows.shape(0), md = graph_rows.shape(1) - 1;
        int64_t nq = queries.shape(0);
        py::array_t<int32_t> ids({(size_t)nq, (size_t)beam});
        py::array_t<float> dists({(size_t)nq, (size_t)beam});
        py::array_t<int32_t> sizes((size_t)nq);
        py::array_t<int64_t> hops((size_t)nq), cmps((size_t)nq);
        int rc = wann_raw_beam_search(metric, points.data(), n, d, graph_rows.data(), md, subset_start, sn,
                                      queries.data(), nq, query_ids.data(), beam, limit, degree_limit,
                                      ids.mutable_data(), dists.mutable_data(), sizes.mutable_data(),
                                      hops.mutable_data(), cmps.mutable_data(), device);
        if (rc) raise_last("raw_beam_search failed");
        return py::make_tuple(ids, dists, sizes, hops, cmps);
      },
      "metric"_a, "points"_a, "graph_rows"_a, "subset_start"_a, "queries"_a, "query_ids"_a, "beam"_a,
      "limit"_a = 10000000, "degree_limit"_a = 10000, "device"_a = 0);
  // raw_beam_search over points of any element type (dtype: 0 float32, 1 uint8, 2 int8, 3 float16, 5 bfloat16 -- there `points` is a
  // uint16 array of BIT PATTERNS, as float16 takes np.float16 -- 8 float8: a uint8 array of bit patterns); queries stay float32
  m.def(
      "raw_beam_search_typed",
      [](int metric, int dtype, py::array points_in, py::array_t<int32_t, py::array::c_style | py::array::forcecast> graph_rows,
         int64_t subset_start, FArray queries, py::array_t<int64_t, py::array::c_style | py::array::forcecast> query_ids,
         int64_t beam, int64_t limit, int64_t degree_limit, int device) {
        if ((dtype < WANN_DTYPE_F32 || dtype > WANN_DTYPE_F16) && dtype != WANN_DTYPE_BF16 && dtype != WANN_DTYPE_F8) throw std::runtime_error("unknown dtype");
        if (dtype == WANN_DTYPE_F8 && !py::isinstance<py::array_t<uint8_t>>(points_in))
          throw std::runtime_error("dtype 8 takes the points as a uint8 array of float8 (E4M3) bit patterns");
        if (dtype == WANN_DTYPE_BF16 && !py::isinstance<py::array_t<uint16_t>>(points_in))
          throw std::runtime_error("dtype 5 takes the points as a uint16 array of bfloat16 bit patterns");
        py::array points = dtype == WANN_DTYPE_BF16 ? py::array(py::array_t<uint16_t, py::array::c_style>::ensure(points_in))
                         : dtype == WANN_DTYPE_F8 ? py::array(py::array_t<uint8_t, py::array::c_style>::ensure(points_in)) : as_elem(dtype, points_in);
        if (points.ndim() != 2 || graph_rows.ndim() != 2 || queries.ndim() != 2) throw std::runtime_error("bad shapes");
        int64_t n = points.shape(0), d = points.shape(1), sn = graph_rows.shape(0), md = graph_rows.shape(1) - 1;
        int64_t nq = queries.shape(0);
        if (queries.shape(1) != d) throw std::runtime_error("queries must have the points' dimension");
        py::array_t<int32_t> ids({(size_t)nq, (size_t)beam});
        py::array_t<float> dists({(size_t)nq, (size_t)beam});
        py::array_t<int32_t> sizes((size_t)nq);
        py::array_t<int64_t> hops((size_t)nq), cmps((size_t)nq);
        int rc = wann_raw_beam_search_typed(metric, dtype, points.data(), n, d, graph_rows.data(), md, subset_start, sn,
                                            queries.data(), nq, query_ids.data(), beam, limit, degree_limit,
                                            ids.mutable_data(), dists.mutable_data(), sizes.mutable_data(),
                                            hops.mutable_data(), cmps.mutable_data(), device);
        if (rc) raise_last("raw_beam_search_typed failed");
        return py::make_tuple(ids, dists, sizes, hops, cmps);
      },
      "metric"_a, "dtype"_a, "points"_a, "graph_rows"_a, "subset_start"_a, "queries"_a, "query_ids"_a, "beam"_a,
      "limit"_a = 10000000, "degree_limit"_a = 10000, "device"_a = 0);
}
