"""The face quality gate's kernels alone, through zr_identity_quality_async and
zr_identity_quality_mask_async, against zaru_amd.host.face_quality (zr_face_quality_host, itself pinned to
the numpy restatement by tests/test_quality_cpu.py): the whole record of every row and d_due, bit for bit.

Rows: n = 1 and n = 65 with K = 1, n = 3 and n = 66 with K = 3 (the entry refuses an n that is no multiple of
the slots, so K = 3 takes the multiples of 3 on either side of a wavefront; 65 with K = 3 is checked to be
refused).  The rows cycle through the views and frames of the CPU file -- three frames of different sizes,
views inside, down-sampled, half and wholly outside, rotated -- and through: due and not due; tracked with a
`src` that is the row's own slot, a higher slot (the object moved down), -1 (a newcomer to a vacated slot),
out of range, and untracked; a view whose frame index is past the table.  Every grid of the CPU file, and
128 x 128 = 16384 pixels."""
import ctypes as C
import math

import numpy as np
import pytest

import quality_ref as QR
import test_quality_cpu as TQ

pytestmark = pytest.mark.gpu

f32 = np.float32
VIEW_DESC = np.dtype([("f", f32, 8), ("frame", np.uint32), ("pad", np.uint32)])
EMBED = (55.0, 0.5, 1.0, -math.inf)          # the flat views, the small and the outside ones fail
LEARN = (55.0, 1.0, 1000.0, -math.inf)       # the views that leave the frame are held back
FRAME_ORDER = ("noise", "flat", "checker")


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


def host_scene():
    """The frames and the views as descriptors (no device needed)."""
    from zaru_amd import _lib
    frames = TQ.frames()
    views = []
    for name, (fname, _) in TQ.views().items():
        _, hv = TQ.host_view(name)
        z = (C.c_float * 5)(*hv.zr_view())
        d = np.zeros(1, VIEW_DESC)
        _lib.check(_lib.lib().zr_view_describe(z, 1, FRAME_ORDER.index(fname), d.ctypes.data))
        views.append((name, fname, hv, d[0]))
    return {"frames": frames, "views": views}


@pytest.fixture(scope="module")
def scene():
    """host_scene with the frames on the device, each its own size, tightly packed."""
    from zaru_amd import _lib
    sc = host_scene()
    frames = sc["frames"]
    sc["bufs"] = {k: _lib.DeviceBuffer.from_array(frames[k]) for k in FRAME_ORDER}
    sc["table"] = (_lib.Frame * 3)(*[_lib.Frame(sc["bufs"][k].ptr, frames[k].shape[1], frames[k].shape[0],
                                                frames[k].shape[1] * 4) for k in FRAME_ORDER])
    return sc


def _rows(scene, n, K, seed):
    """The script of n rows: (due, tracked, src, view index, frame past the table)."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        j = i % K
        kind = (i // 2) % 5
        src = [j, min(j + 1, K - 1) if K > 1 else 0, -1, K + (i % 3) * 40, j][kind]
        rows.append({"due": i % 4 != 3 or n == 1, "tracked": kind != 4 or i % 2 == 0, "src": src,
                     "view": (i * 7 + i // 9) % len(scene["views"]), "past": i % 11 == 5})
    records = np.zeros(n, np.dtype(_records_dtype()))
    records["size"], records["inside"] = rng.uniform(1, 99, n), rng.uniform(0, 1, n)
    records["sharpness"], records["frontal"] = rng.uniform(0, 5000, n), rng.uniform(-1, 1, n)
    records["flags"], records["samples"] = rng.choice([1 | 2, 1 | 2 | 4, 1 | 64], n), rng.integers(0, 12100, n)
    records["rejected"] = rng.choice([0, 1, 7, 0xFFFFFFFE, 0xFFFFFFFF], n)
    return rows, records


def _records_dtype():
    from zaru_amd import _lib
    return _lib.FaceQuality


def _incoming(rows, records, i, K):
    r = rows[i]
    if r["tracked"] and 0 <= r["src"] < K:
        return records[(i // K) * K + r["src"]]
    return np.zeros(1, records.dtype)[0]


def _expected(H, scene, rows, records, K, ow, oh, poses, embed, learn, cache):
    out = np.zeros(len(rows), records.dtype)
    due = np.zeros(len(rows), np.int32)
    measured = rejected = 0
    for i, r in enumerate(rows):
        inc = _incoming(rows, records, i, K)
        if not r["due"]:
            out[i] = inc
            continue
        name, fname, hv, desc = scene["views"][r["view"]]
        pose = None if poses is None else poses[i]
        if r["past"]:   # a 0 x 0 frame: every pixel outside
            m = {"size": np.fmin(desc["f"][4], desc["f"][5]), "inside": f32(0), "sharpness": f32(0), "samples": 0,
                 "frontal": pose[20] if pose is not None and pose.view(np.uint32)[7] else f32(math.nan)}
            q = QR.judge(m, embed, learn, int(inc["rejected"]))
        else:
            key = (name, ow, oh)
            if key not in cache:
                cache[key] = H.face_quality(scene["frames"][fname], hv, ow, oh)
            m = dict(cache[key])
            m["frontal"] = pose[20] if pose is not None and pose.view(np.uint32)[7] else f32(math.nan)
            q = QR.judge(m, embed, learn, int(inc["rejected"]))
        for k in QR.KEYS:
            out[k][i] = q[k]
        measured += 1
        rejected += 0 if q["flags"] & QR.EMBED else 1
        due[i] = 1 if q["flags"] & QR.EMBED else 0
    return out, due, measured, rejected


def _run(H, scene, n, K, ow, oh, with_pose, embed=EMBED, learn=LEARN, cache=None, counters=True, n_frames=3):
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    rows, records = _rows(scene, n, K, 100 * n + K)
    state = np.zeros(n, np.dtype(_lib.TrackState))
    state["tracked"] = [1 if r["tracked"] else 0 for r in rows]
    src = np.array([r["src"] for r in rows], np.int32)
    views = np.zeros(n, VIEW_DESC)
    for i, r in enumerate(rows):
        views[i] = scene["views"][r["view"]][3]
        if r["past"]:
            views[i]["frame"] = n_frames + (i % 2) * 1000
        if not r["due"]:
            views[i]["f"] = math.nan   # a row that is not due has no crop: it must not be read as one
            views[i]["frame"] = 0xFFFFFFFF
    poses = None
    if with_pose:
        rng = np.random.default_rng(7 * n + K)
        poses = rng.uniform(-1, 1, (n, 21)).astype(f32)
        poses.view(np.uint32)[:, 7] = [0 if i % 3 == 1 else 1 for i in range(n)]
        poses[:, 20] = rng.choice([0.3, 0.6, 0.95], n)
    due0 = np.array([1 if r["due"] else 0 for r in rows], np.int32)
    d_state, d_src, d_views, d_in, d_due = b(state), b(src), b(views), b(records), b(due0)
    sentinel = np.full(n * 8, 0xA5A5A5A5, np.uint32)
    d_out = b(sentinel)
    d_pose = b(poses) if with_pose else None
    d_cnt = b(np.array([1000, 2000], np.uint64))
    cfg = _lib.QualityCfg(K, ow, oh, _lib.QualityTier(*embed), _lib.QualityTier(*learn))
    _lib.check(lib.zr_identity_quality_async(C.byref(cfg), scene["table"], n_frames, d_state.ptr, n, d_src.ptr,
                                             d_views.ptr, d_pose.ptr if with_pose else None, d_in.ptr, d_out.ptr,
                                             d_due.ptr, d_cnt.ptr if counters else None,
                                             d_cnt.ptr + 8 if counters else None, None))
    _lib.synchronize()
    want, want_due, measured, rejected = _expected(H, scene, rows, records, K, ow, oh, poses, embed, learn,
                                                   {} if cache is None else cache)
    got = d_out.download((n,), records.dtype)
    for i in range(n):
        assert got[i].tobytes() == want[i].tobytes(), ("row", i, rows[i], got[i], want[i])
    got_due = d_due.download((n,), np.int32)
    assert got_due.tolist() == want_due.tolist()
    assert d_cnt.download((2,), np.uint64).tolist() == ([1000 + measured, 2000 + rejected] if counters else [1000, 2000])
    assert d_in.download((n,), records.dtype).tobytes() == records.tobytes(), "the incoming records are only read"
    return rows, got, got_due, (d_out, records.dtype)


SHAPES = [(1, 1), (65, 1), (3, 3), (66, 3)]
CACHE = {}


@pytest.mark.parametrize("grid", TQ.GRIDS + [(128, 128)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}k{s[1]}")
def test_measure_bits(H, scene, shape, grid):
    n, K = shape
    rows, got, due, _ = _run(H, scene, n, K, grid[0], grid[1], with_pose=False, cache=CACHE)
    if n >= 65 and grid == (112, 112):   # the script holds the cases
        flags = got["flags"][[i for i, r in enumerate(rows) if r["due"]]]
        assert (flags & QR.LEARN).any() and ((flags & QR.EMBED != 0) & (flags & QR.LEARN == 0)).any()
        for bit in (QR.FAIL_SIZE, QR.FAIL_INSIDE, QR.FAIL_SHARPNESS):
            assert (flags & bit).any(), bit
        assert any(r["due"] and r["past"] for r in rows) and any(not r["due"] for r in rows)
        assert 0xFFFFFFFF in got["rejected"] and 0 < due.sum() < n


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}k{s[1]}")
def test_measure_with_pose_and_frontal_tiers(H, scene, shape):
    """frontal is rot[8] of a valid pose and NaN otherwise; 0.6 passes the embed tier's 0.5 and misses the
    learn tier's 0.9, an invalid pose fails both."""
    n, K = shape
    embed, learn = (-math.inf, -math.inf, -math.inf, 0.5), (-math.inf, -math.inf, -math.inf, 0.9)
    rows, got, due, _ = _run(H, scene, n, K, 7, 5, with_pose=True, embed=embed, learn=learn, counters=False)
    if n >= 65:
        d = [i for i, r in enumerate(rows) if r["due"]]
        assert {int(f) for f in got["flags"][d]} == {QR.MEASURED | QR.FAIL_FRONTAL, QR.MEASURED | QR.EMBED,
                                                     QR.MEASURED | QR.EMBED | QR.LEARN}
        assert np.isnan(got["frontal"][d]).any()


def test_all_skip_tiers_keep_every_due_row(H, scene):
    rows, got, due, _ = _run(H, scene, 66, 3, 112, 112, with_pose=False, embed=QR.SKIP, learn=QR.SKIP, cache=CACHE)
    assert due.tolist() == [1 if r["due"] else 0 for r in rows]
    assert all(int(f) == 7 for f, r in zip(got["flags"], rows) if r["due"])


def test_a_frame_table_of_one(H, scene):
    """With one frame in the table the views of frames 1 and 2 sample nothing, as those past it do."""
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    n, K = 66, 3
    rows, records = _rows(scene, n, K, 100 * n + K)
    state = np.zeros(n, np.dtype(_lib.TrackState))
    state["tracked"] = [1 if r["tracked"] else 0 for r in rows]
    src = np.array([r["src"] for r in rows], np.int32)
    views = np.zeros(n, VIEW_DESC)
    for i, r in enumerate(rows):
        views[i] = scene["views"][r["view"]][3]   # frames 1 and 2 keep their index: past a table of one
        if r["past"]:
            views[i]["frame"] = 1 + i
        r["past"] = r["past"] or scene["views"][r["view"]][1] != "noise"
    assert any(r["due"] and r["past"] for r in rows) and any(r["due"] and not r["past"] for r in rows)
    due0 = np.array([1 if r["due"] else 0 for r in rows], np.int32)
    d_state, d_src, d_views, d_in, d_due = b(state), b(src), b(views), b(records), b(due0)
    d_out = b(np.zeros(n * 8, np.uint32))
    cfg = _lib.QualityCfg(K, 7, 5, _lib.QualityTier(*EMBED), _lib.QualityTier(*LEARN))
    _lib.check(lib.zr_identity_quality_async(C.byref(cfg), scene["table"], 1, d_state.ptr, n, d_src.ptr, d_views.ptr,
                                             None, d_in.ptr, d_out.ptr, d_due.ptr, None, None, None))
    _lib.synchronize()
    want, want_due, _, _ = _expected(H, scene, rows, records, K, 7, 5, None, EMBED, LEARN, {})
    got = d_out.download((n,), records.dtype)
    for i in range(n):
        assert got[i].tobytes() == want[i].tobytes(), ("row", i, rows[i])
    assert d_due.download((n,), np.int32).tolist() == want_due.tolist()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}k{s[1]}")
def test_learn_mask(H, scene, shape):
    """On the gate's own output and list, and on a list that names every row (records that were carried,
    default or rejected among them)."""
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    n, K = shape
    rows, got, due, (d_q, dtype) = _run(H, scene, n, K, 112, 112, with_pose=False, cache=CACHE)
    packed = np.full(n, -1, np.int32)
    packed[due != 0] = np.arange(int(due.sum()))
    every = np.arange(n, dtype=np.int32)[::-1].copy()
    every[::7] = -1
    for of in (packed, every):
        d_of, d_learn, d_held = b(of), b(np.full(n, 12345, np.int32)), b(np.array([500], np.uint64))
        _lib.check(lib.zr_identity_quality_mask_async(n, d_of.ptr, d_q.ptr, d_learn.ptr, d_held.ptr, None))
        _lib.synchronize()
        learn = (got["flags"] & QR.LEARN) != 0
        want = np.where((of >= 0) & learn, of, -1)
        assert d_learn.download((n,), np.int32).tolist() == want.tolist()
        assert d_held.download((1,), np.uint64)[0] == 500 + int(((of >= 0) & ~learn).sum())
        assert d_of.download((n,), np.int32).tolist() == of.tolist()
        _lib.check(lib.zr_identity_quality_mask_async(n, d_of.ptr, d_q.ptr, d_learn.ptr, None, None))   # no counter
        _lib.synchronize()
        assert d_learn.download((n,), np.int32).tolist() == want.tolist()
    if n >= 65:
        assert ((every >= 0) & ~learn).any() and ((every >= 0) & learn).any()


def test_refusals_launch_nothing(H, scene):
    """Every refusal, with real buffers: the outputs keep their bytes."""
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    n, K = 6, 3
    state = np.zeros(n, np.dtype(_lib.TrackState))
    state["tracked"] = 1
    views = np.zeros(n, VIEW_DESC)
    views[:] = scene["views"][0][3]
    sent_out, sent_due = np.full(n * 8, 0xA5A5A5A5, np.uint32), np.ones(n, np.int32)
    d_state, d_src, d_views = b(state), b(np.zeros(n, np.int32)), b(views)
    d_in, d_out, d_due = b(np.zeros(n * 8, np.uint32)), b(sent_out), b(sent_due)
    d_cnt, d_pose = b(np.array([11, 22], np.uint64)), b(np.zeros((n, 21), f32))
    frontal = (-math.inf, -math.inf, -math.inf, 0.5)

    def call(slots=K, ow=7, oh=5, embed=QR.SKIP, learn=QR.SKIP, nn=n, frames=scene["table"], nf=3, pose=None, **kw):
        a = dict(state=d_state.ptr, src=d_src.ptr, views=d_views.ptr, rin=d_in.ptr, rout=d_out.ptr, due=d_due.ptr)
        a.update(kw)
        cfg = _lib.QualityCfg(slots, ow, oh, _lib.QualityTier(*embed), _lib.QualityTier(*learn))
        return lib.zr_identity_quality_async(C.byref(cfg), frames, nf, a["state"], nn, a["src"], a["views"], pose,
                                             a["rin"], a["rout"], a["due"], d_cnt.ptr, d_cnt.ptr + 8, None)

    bad = [call(**{k: None}) for k in ("state", "src", "views", "rin", "rout", "due")]
    bad += [call(frames=None), call(nn=0), call(nn=(1 << 24) + 3), call(slots=0), call(slots=65), call(slots=4),
            call(nn=65, slots=3), call(ow=0), call(oh=0), call(ow=129, oh=128), call(embed=(math.nan,) + QR.SKIP[1:]),
            call(learn=QR.SKIP[:3] + (math.nan,)), call(rin=d_out.ptr), call(embed=frontal), call(learn=frontal),
            call(nf=0)]
    assert bad == [-1] * len(bad)
    d_learn = b(np.full(n, 777, np.int32))
    bad = [lib.zr_identity_quality_mask_async(n, None, d_out.ptr, d_learn.ptr, d_cnt.ptr, None),
           lib.zr_identity_quality_mask_async(n, d_due.ptr, None, d_learn.ptr, d_cnt.ptr, None),
           lib.zr_identity_quality_mask_async(n, d_due.ptr, d_out.ptr, None, d_cnt.ptr, None),
           lib.zr_identity_quality_mask_async(0, d_due.ptr, d_out.ptr, d_learn.ptr, d_cnt.ptr, None),
           lib.zr_identity_quality_mask_async((1 << 24) + 1, d_due.ptr, d_out.ptr, d_learn.ptr, d_cnt.ptr, None)]
    assert bad == [-1] * len(bad)
    _lib.synchronize()
    assert d_out.download((n * 8,), np.uint32).tolist() == sent_out.tolist()
    assert d_due.download((n,), np.int32).tolist() == sent_due.tolist()
    assert d_cnt.download((2,), np.uint64).tolist() == [11, 22] and d_learn.download((n,), np.int32).tolist() == [777] * n
    # the same calls are accepted once the argument is right: a frontal tier with the pose records
    assert call(embed=frontal, pose=d_pose.ptr) == 0
    _lib.synchronize()
    assert d_cnt.download((2,), np.uint64).tolist() == [11 + n, 22 + n]   # valid == 0 everywhere: NaN fails
