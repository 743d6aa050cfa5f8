"""The listing limit on every seam of the ordered compaction that the change feed, idle expiry and the hot-object report's tie
pass share (rio_gp_changes_dev, rio_gp_expire_dev, rio_gp_top_rows_dev), against the plain restatements (tests/spec_changes.py,
spec_expire.py, spec_top.py) only.

One table of 9 * 1024 + 77 rows: ten tiles of 1 024 rows, four to a workgroup, so three workgroups with the last tile partial.
Two hit patterns, every row and every seventh row, and the limit `cap` on each side of a lane's quad (4), a step (256), a tile
(1 024), a workgroup (4 096) and the total: the listing is the restatement's first min(cap, total) rows, the count is the
total, nothing is written past the listing, and a second call lists exactly the remainder."""
import numpy as np
import pytest

import spec_changes
import spec_expire
import spec_top

NONE = 0xFFFFFFFF
N, M = 9 * 1024 + 77, 8
PATTERNS = {"every_row": 1, "every_seventh_row": 7}


def _caps(total, most=None):
    caps = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, total - 1, total, total + 1]
    return [c for c in caps if most is None or c <= most]


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


@pytest.fixture(scope="module", params=sorted(PATTERNS))
def table(gp, request):
    """(handle, A, load, hit rows): the hit rows sit on a node and carry load 3, the others have no node and load 1."""
    step = PATTERNS[request.param]
    hit = np.arange(0, N, step)
    A = np.full(N, NONE, np.uint32)
    A[hit] = (hit % M).astype(np.uint32)
    load = np.ones(N, np.uint32)
    load[hit] = 3
    g = gp.GpuPlacement(N, M)
    g.set_nodes(None, np.ones(M, np.uint8), m=M)
    g.set_objects(N, load, np.zeros(N, np.uint32))
    g.set_assign(A)
    yield g, A, load, hit
    g.close()


def _dev(k, cap):
    import torch
    d = [torch.full((cap + 8,), -1, dtype=torch.int32, device="cuda") for _ in range(k)]
    torch.cuda.synchronize()
    return d


def _host(d):
    return [x.cpu().numpy().view(np.uint32) for x in d]


def _listed(got, want, cap):
    """`want` in front, nothing written behind it (the arrays hold cap + 8 words)."""
    k = len(want)
    assert k <= cap
    return np.array_equal(got[:k], want) and (got[k:] == NONE).all()


@pytest.mark.gpu
def test_the_change_feed_at_every_seam(table):
    g, A, load, hit = table
    total = len(hit)
    for cap in _caps(total):
        g.changes_reset()
        B = np.full(N, NONE, np.uint32)
        for c in (cap, N):                               # the first min(cap, total) rows, then exactly the remainder
            wr, wo, wn, wt, B = spec_changes.dense(B, A, N, c)
            d = _dev(3, c)
            assert g.changes_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), cap=c) == wt, (cap, c)
            got = _host(d)
            assert _listed(got[0], wr, c) and _listed(got[1], wo, c) and _listed(got[2], wn, c), (cap, c)
        assert wt == max(total - cap, 0) and len(wr) == wt
        assert g.changes_dev() == 0


@pytest.mark.gpu
def test_idle_expiry_at_every_seam(table):
    g, A, load, hit = table
    total = len(hit)
    S = np.zeros(N, np.uint32)                           # nobody has been seen: every placed row is idle below cutoff 1
    for cap in _caps(total):
        g.set_assign(A)                                  # the table as it was
        cur = A
        for c in (cap, N):
            wr, wn, wi, wf, cur = spec_expire.expire(cur, S, load, N, 1, c)
            d = _dev(2, c)
            assert g.expire_dev(1, d[0].data_ptr(), d[1].data_ptr(), cap=c) == (wi, wf), (cap, c)
            got = _host(d)
            assert _listed(got[0], wr, c) and _listed(got[1], wn, c), (cap, c)
            assert np.array_equal(g.get_assign(), cur), (cap, c)
        assert wi == max(total - cap, 0) and len(wr) == wi
        assert g.expire_dev(1) == (0, 0)
    g.set_assign(A)


@pytest.mark.gpu
@pytest.mark.parametrize("placed", [False, True])
def test_the_tie_pass_of_the_hot_object_report_at_every_seam(gp, table, placed):
    g, A, load, hit = table
    total = len(hit)
    flags = gp.TOP_PLACED if placed else 0               # min_key 3: the candidates are the hit rows, every key is 3
    for cap in _caps(total, gp.TOP_MAX):
        wr, wk, wn, wc, ws = spec_top.top_rows(A, load, None, N, flags, 0, 3, cap)
        assert wc == total and (wk == 3).all() and np.array_equal(wr, hit[:cap])
        d = _dev(3, cap)
        assert g.top_rows_dev(flags, 0, 3, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), cap) == (wc, ws), cap
        got = _host(d)
        assert _listed(got[0], wr, cap) and _listed(got[1], wk, cap) and _listed(got[2], wn, cap), cap
