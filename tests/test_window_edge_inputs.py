"""CPU: window_edge_util's sites are what tests/test_gpu_dense_window_edges.py takes them for (no GPU, no engine)."""
import numpy as np

import window_edge_util as we


def test_sites_reach_the_table_edges():
    st = we.Sites(5064, 64)  # (the constructor asserts every placement's windows on both paths)
    assert st.n % 64 == 37 and 50000 < st.n < 60000 and st.hi[-1] == st.n - 1
    assert sorted(st.m.tolist()) == [16, 17, 32, 33, 63, 64, 65, 127, 129, 257]
    assert sorted({st.level(s) for s in range(st.S)}) == [4, 5, 6, 7, 8]
    lo_on, hi_on = st.lo % 64 == 0, st.hi % 64 == 0
    s16 = int(np.nonzero(st.m == 16)[0][0])
    assert lo_on[s16] and hi_on[s16] and st.hi[s16] - st.lo[s16] == 1024
    assert (lo_on & ~hi_on).sum() == 1 and (~lo_on & hi_on).sum() == 1 and (lo_on & hi_on).sum() == 1
    rest = ~lo_on & ~hi_on
    rest[-1] = False  # (the last site's end is n - 1)
    assert ((st.lo[rest] % 64 >= 1) & (st.lo[rest] % 64 <= 24) & ((st.hi[rest] - 1) % 64 >= 39) & ((st.hi[rest] - 1) % 64 <= 62)).all()
    for pl in we.IN_WINDOW:
        for s, pos in st.outliers(pl).items():
            assert all(st.lo[s] <= p < st.hi[s] for p in pos)
    out = st.outliers("outside")
    assert all(len(out[s]) == 2 for s in range(st.S - 1)) and out[st.S - 1] == [64 * st.b0[-1] - 1]
    for s, pos in out.items():
        assert [p // 64 for p in pos] == [st.b0[s] - 1, st.b1[s] + 1][:len(pos)]
    # the cover path: no two windows of a site alike where an end can shrink by a position a query
    a, b = st.positions("cover")
    for s in st.sites_of("cover"):
        q = slice(s * we.REP, (s + 1) * we.REP)
        assert len({(x, y) for x, y in zip(a[q], b[q])}) == we.REP


def test_tail_shares():
    for share, trimmed in (((1, 5), True), ((3, 10), False)):
        st = we.Sites(5064, 64, share)
        t = len(st.tail_pos)
        assert t == st.n * share[0] // share[1] and (t < st.n / 4) == trimmed and st.tail_pos[-1] == st.n - 1
