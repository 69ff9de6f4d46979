"""The aligned identity crop's kernel alone, through zr_identity_align_async, against zr_face_align_host
(itself pinned to the numpy restatement by tests/test_align_cpu.py): the view and the record of every row,
bit for bit.

Rows: n = 6 (2 streams of 3 slots) and n = 130 (past two wavefronts), with L = 468 (the fixture meshes,
moved, scaled and turned per row; the default five-point settings) and L = 6 (random sets, a group that
names index L - 1).  Due and not-due rows are mixed, and a not-due row's view and record keep their sentinel
bytes; some due rows are degenerate (coincident points, a non-finite coordinate) and max_residual lies
between the rows' residuals, so both kinds of fallback occur and keep the view select would have written.
The streams have different frame sizes, and the frame index of a rewritten view is the one it held."""
import ctypes as C
import math

import numpy as np
import pytest

import align_ref as AR
import test_align_cpu as TA

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 0xA5A5A5A5


def _script(n, K, L, seed):
    """(template, groups, landmarks [n][L][3], due [n], frame sizes per stream)."""
    rng = np.random.default_rng(seed)
    if L == 468:
        mesh, _, _ = TA.fixture()
        template, groups = AR.TEMPLATE, AR.GROUPS
        lm = np.empty((n, L, 3), f32)
        for i in range(n):
            m = mesh[i % 3].copy()
            ang, s = rng.uniform(-math.pi, math.pi), rng.uniform(0.3, 3.0)
            c, sn = math.cos(ang), math.sin(ang)
            x, y = m[:, 0] - 96.0, m[:, 1] - 96.0
            m[:, 0] = s * (c * x - sn * y) + rng.uniform(0, 480)
            m[:, 1] = s * (sn * x + c * y) + rng.uniform(0, 360)
            # a sheared copy now and then: the residual grows past the limit
            if i % 5 == 2:
                m[:, 0] += 0.6 * (m[:, 1] - m[:, 1].mean())
            lm[i] = m
    else:
        template = [(float(f32(x)), float(f32(y))) for x, y in rng.uniform(10, 100, (5, 2))]
        groups = [[0], [1, 5], [2], [3, 4], [5]]
        lm = (rng.normal(0, 50, (n, L, 3)) + 200).astype(f32)
        t = np.array(template, f32)
        for i in range(0, n, 2):   # every other row a noisy similarity of the template: small residuals
            ang, s = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 2.0)
            c, sn = math.cos(ang), math.sin(ang)
            pts = np.zeros((6, 2))
            pts[:5] = s * np.stack([c * t[:, 0] - sn * t[:, 1], sn * t[:, 0] + c * t[:, 1]], 1) + 150
            pts[5] = pts[4]
            lm[i, :, :2] = (pts + rng.normal(0, 0.5, (6, 2))).astype(f32)
    for i in range(n):
        if i % 13 == 4:
            lm[i, :, :2] = lm[i, 0, :2]       # coincident face points
        if i % 17 == 9:
            lm[i, groups[1][0], 0] = math.inf
        if i % 19 == 11:
            lm[i, groups[2][0], 1] = math.nan
    due = np.array([0 if i % 4 == 1 else 1 for i in range(n)], np.int32)
    sizes = [(480 + 16 * s, 360 + 8 * s) for s in range(n // K + 1)]
    return template, groups, lm, due, sizes


def _limit(template, groups, lm, due):
    """A max_residual between the due rows' residuals (the median gap), taken from the restatement."""
    res = sorted(float(r["residual"]) for r in (AR.fit(template, groups, lm[i]) for i in range(len(lm)) if due[i])
                 if r["flags"] == AR.ALIGNED)
    mid = len(res) // 2
    assert res[mid - 1] < res[mid]
    return float(f32((res[mid - 1] + res[mid]) / 2))


def _run(n, K, L, totals=True):
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    template, groups, lm, due, sizes = _script(n, K, L, 1000 * n + L)
    limit = _limit(template, groups, lm, due)
    cfg = _lib.AlignCfg.make(template, groups, 112, 112, limit)
    state = np.zeros(n, np.dtype(_lib.TrackState))
    views = np.zeros(n, AR.VIEW_DESC)
    views.view(np.uint32)[:] = SENTINEL
    for i in range(n):
        state["frame_w"][i], state["frame_h"][i] = sizes[i // K]
        state["tracked"][i] = 1
        if due[i]:   # what select leaves: a bounding crop on the row's frame
            views[i]["f"] = [50, 40, 10 + i, 20, 100, 80, 1, 0]
            views[i]["frame"], views[i]["pad"] = i // K, 0
    recs = np.full(n * 4, SENTINEL, np.uint32)
    d_state, d_lm, d_due, d_views, d_recs = b(state), b(lm), b(due), b(views), b(recs)
    d_tot = b(np.array([1000, 2000], np.uint64))
    _lib.check(lib.zr_identity_align_async(C.byref(cfg), d_state.ptr, n, d_lm.ptr, L, d_due.ptr, d_views.ptr,
                                           d_recs.ptr, d_tot.ptr if totals else None, None))
    _lib.synchronize()
    got_v, got_r = d_views.download((n,), AR.VIEW_DESC), d_recs.download((n,), AR.RECORD)
    aligned = fallback = 0
    kinds = set()
    for i in range(n):
        if not due[i]:
            assert got_v[i].tobytes() == views[i].tobytes() and got_r[i].tobytes() == recs[4 * i:4 * i + 4].tobytes(), \
                ("a row that is not due is not written", i)
            continue
        want_v = views[i:i + 1].copy()
        want_r = np.zeros(1, AR.RECORD)
        w, h = sizes[i // K]
        rc = lib.zr_face_align_host(C.byref(cfg), lm[i].ctypes.data, L, 3, w, h, i // K, want_v.ctypes.data,
                                    want_r.ctypes.data)
        assert rc == 0
        assert got_r[i].tobytes() == want_r[0].tobytes(), ("record", i, got_r[i], want_r[0])
        assert got_v[i].tobytes() == want_v[0].tobytes(), ("view", i, got_v[i], want_v[0])
        flags = int(want_r[0]["flags"])
        kinds.add(flags)
        if flags & AR.ALIGNED:
            aligned += 1
            assert got_v[i].tobytes() != views[i].tobytes()
        else:
            fallback += 1
            assert got_v[i].tobytes() == views[i].tobytes(), ("a fallback keeps select's view", i)
    assert d_tot.download((2,), np.uint64).tolist() == ([1000 + aligned, 2000 + fallback] if totals else [1000, 2000])
    assert d_lm.download(lm.shape, f32).tobytes() == lm.tobytes() and d_due.download((n,), np.int32).tolist() == due.tolist()
    return kinds, aligned, fallback, got_v


@pytest.mark.parametrize("L", [468, 6])
@pytest.mark.parametrize("n", [6, 130])
def test_align_bits(n, L):
    kinds, aligned, fallback, views = _run(n, 3, L)
    assert aligned > 0 and AR.FALLBACK | AR.FAIL_RESIDUAL in kinds
    if n == 130:   # the script holds the cases
        assert kinds == {AR.ALIGNED, AR.FALLBACK | AR.FAIL_RESIDUAL, AR.FALLBACK | AR.FAIL_DEGENERATE}
        assert fallback > 0 and (views["f"][:, 7] != 0).any(), "rotated views occur"


def test_null_totals_are_accepted():
    _run(130, 3, 6, totals=False)


def test_refusals_launch_nothing():
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    n, K, L = 6, 3, 6
    template, groups, lm, due, sizes = _script(n, K, L, 5)
    due[:] = 1
    state = np.zeros(n, np.dtype(_lib.TrackState))
    state["frame_w"], state["frame_h"] = 480, 360
    views = np.full(n * 10, SENTINEL, np.uint32)
    recs = np.full(n * 4, SENTINEL, np.uint32)
    d_state, d_lm, d_due, d_views, d_recs = b(state), b(lm), b(due), b(views), b(recs)
    d_tot = b(np.array([11, 22], np.uint64))

    def call(nn=n, LL=L, template=template, groups=groups, ow=112, oh=112, max_residual=math.inf, num_points=None,
             raw_group=None, **kw):
        a = dict(state=d_state.ptr, lm=d_lm.ptr, due=d_due.ptr, views=d_views.ptr, recs=d_recs.ptr)
        a.update(kw)
        cfg = _lib.AlignCfg.make(template, groups, ow, oh, max_residual)
        if num_points is not None:
            cfg.num_points = num_points
        if raw_group is not None:
            cfg.group[raw_group[0]][raw_group[1]] = raw_group[2]
        return lib.zr_identity_align_async(C.byref(cfg), a["state"], nn, a["lm"], LL, a["due"], a["views"], a["recs"],
                                           d_tot.ptr, None)

    bad = [call(**{k: None}) for k in ("state", "lm", "due", "views", "recs")]
    bad.append(lib.zr_identity_align_async(None, d_state.ptr, n, d_lm.ptr, L, d_due.ptr, d_views.ptr, d_recs.ptr,
                                           d_tot.ptr, None))
    bad += [call(nn=0), call(nn=(1 << 24) + 1), call(LL=0), call(num_points=1), call(num_points=9), call(ow=0),
            call(oh=0), call(raw_group=(0, 0, -1)), call(raw_group=(1, 1, 6)), call(raw_group=(3, 1, -2)),
            call(LL=5),   # the groups name index 5
            call(template=[(math.nan, 1.0)] + template[1:]), call(template=template[:4] + [(1.0, -math.inf)]),
            call(template=[(3.0, 4.0)] * 5), call(max_residual=math.nan)]
    assert bad == [-1] * len(bad), bad
    _lib.synchronize()
    assert d_views.download((n * 10,), np.uint32).tolist() == views.tolist()
    assert d_recs.download((n * 4,), np.uint32).tolist() == recs.tolist()
    assert d_tot.download((2,), np.uint64).tolist() == [11, 22]
    # the same call is accepted once the arguments are right (the sentinel views carry a frame index, kept)
    assert call() == 0
    _lib.synchronize()
    assert sum(d_tot.download((2,), np.uint64).tolist()) == 33 + n
    assert (d_views.download((n,), AR.VIEW_DESC)["frame"] == SENTINEL).all()
