"""CPU: the restatement of the wide call (wide_util.restate) against the oracle's ordinary call -- the yardstick for the
util the GPU tests of tests/test_gpu_wide.py compare the engine with.  The PREFIX PROPERTY (include/wann.h WIDE ROWS): the
first s columns of the wide row at (stop_k = s, width = W) are the ordinary call's row at k = s, ids and distance bits.  The
cases are also checked to be worth running: many rows hold more than s entries, and many differ from the ordinary call at
k = W -- so neither "forward to the call at k = s" nor "forward to the call at k = W" restates the wide call."""
import numpy as np
import pytest

import refine_util as ru
import wide_util as wu

_built = {}


def _oracle_index(orc, kind, metric, cache):
    if (kind, metric) not in _built:
        X, Q, labels, W = wu.data()
        _built[kind, metric] = getattr(orc, kind + "Float" + metric)(X, labels, **wu.kwargs_of(orc, kind, cache))
    return _built[kind, metric]


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("wide_restatement")) + "/"


def test_one_level_call_is_one_level(oracle, cache):
    """the building block: the oracle counts ONE search per graph-searched query for a one-level call, at every beam"""
    X, Q, labels, W = wu.data()
    idx = _oracle_index(oracle, "PostfilterVamanaIndex", "Euclidian", cache)
    for b in (4, 16, 64, 99):
        wu.search(idx, Q, W, wu.NQ, "", wu.qp(oracle, 64, b, 1, b + 1))
        assert idx.last_counters["searches"] == wu.NQ, (b, idx.last_counters)


@pytest.mark.parametrize("params", wu.PARAMS, ids=lambda p: "s%d_W%d_B%d_x%d_max%d" % p)
@pytest.mark.parametrize("metric", ("Euclidian", "Mips"))
@pytest.mark.parametrize("kind,method", wu.KINDS)
def test_prefix_property(oracle, cache, kind, method, metric, params):
    s, width, B, mult, max_beam = params
    X, Q, labels, W = wu.data()
    idx = _oracle_index(oracle, kind, metric, cache)
    pad = ru.pad_id_of(kind)
    (ids, dists), levels = wu.restate(oracle, idx, Q, W, wu.NQ, method, s, width, B, mult, max_beam, pad)
    at_s = wu.search(idx, Q, W, wu.NQ, method, wu.qp(oracle, s, B, mult, max_beam))
    at_w = wu.search(idx, Q, W, wu.NQ, method, wu.qp(oracle, width, B, mult, max_beam))
    assert np.array_equal(ids[:, :s], at_s[0]) and np.array_equal(dists[:, :s].view(np.uint32), at_s[1].view(np.uint32))
    cnt = ru.candidate_counts(ids, dists, pad)
    more = int((cnt > s).sum())
    differ = int(((ids != at_w[0]) | (dists.view(np.uint32) != at_w[1].view(np.uint32))).any(axis=1).sum())
    print(f"{kind}{metric} {params}: {levels} level calls, {more} rows hold more than s entries, {differ} differ from the call at k = W")
    # pads are a suffix, and a row is never longer than its level's frontier allows
    is_pad = (ids == np.uint32(pad)) & (dists == ru.FLT_MAX)
    assert np.array_equal(is_pad, np.arange(width)[None, :] >= cnt[:, None])
    if (kind, metric) in wu.RECORDED:  # (recorded when the restatement was first run: at least 68 and 94)
        assert more >= 50 and differ >= 50
