"""Tiled detection on the device: zr_detect_merge_async and zr_due_compact_tiles_async alone against
the restatements of tests/tiled_ref.py (bit for bit), what they and set_detection_tiles refuse, the
host TiledDetector on the scene the CPU oracle pins (tests/test_tiled_cpu.py), and
DeviceMultiTracker with tiles against MultiTrackerRef(detect=TiledDetector.detect)."""
import ctypes as C

import numpy as np
import pytest

import multi_tracker_ref as MR
import tiled_ref as TR
from tiled_ref import random_tiles, tie_case

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = 0xA5A5A5A5  # the bits of every float an entry must leave alone


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


@pytest.fixture(scope="module")
def L():
    from zaru_amd import _lib
    _lib.lib()
    return _lib


# ---- the merge kernel alone ---------------------------------------------------------------------------
def run_merge(L, counts, dets, due, ndue, cfg, dcap, with_optional=True):
    """counts [n][T], dets [n][T][cap][20].  Returns (count [n], dets [n][dcap][20] as u32, ties [n][2],
    dropped [n]) with sentinels where nothing was written."""
    n = len(counts)
    d_tc, d_td = L.DeviceBuffer.from_array(np.asarray(counts, np.int32)), L.DeviceBuffer.from_array(np.asarray(dets, f32))
    d_due = L.DeviceBuffer.from_array(np.asarray(list(due) + [0] * (n - len(due)), np.int32))
    d_ndue = L.DeviceBuffer.from_array(np.array([ndue], np.int32))
    d_count = L.DeviceBuffer.from_array(np.full(n, -7, np.int32))
    d_dets = L.DeviceBuffer.from_array(np.full((n, dcap, 20), SENT, np.uint32))
    d_ties = L.DeviceBuffer.from_array(np.full((n, 2), -9, np.int32))
    d_drop = L.DeviceBuffer.from_array(np.full(n, -11, np.int32))
    rc = L.lib().zr_detect_merge_async(d_tc.ptr, d_td.ptr, d_due.ptr, d_ndue.ptr, n, C.byref(cfg), d_count.ptr,
                                       d_dets.ptr, dcap, d_ties.ptr if with_optional else None,
                                       d_drop.ptr if with_optional else None, None)
    L.check(rc)
    L.synchronize()
    return (d_count.download((n,), np.int32), d_dets.download((n, dcap, 20), np.uint32),
            d_ties.download((n, 2), np.int32), d_drop.download((n,), np.int32))


def check_merge(L, counts, dets, cap, keypoints=6, remove=False, due=None, ndue=None, dcap=None, iou=0.3):
    counts, dets = np.asarray(counts, np.int32), np.asarray(dets, f32)
    n, T = counts.shape
    due = list(range(n)) if due is None else due
    ndue = len(due) if ndue is None else ndue
    want = [TR.merge(counts[s], dets[s], cap, keypoints, iou, remove) for s in range(n)]
    dcap = max(1, max(len(w[0]) for w in want)) if dcap is None else dcap
    cfg = L.DetMergeCfg(tiles=T, tile_cap=cap, keypoints=keypoints, iou=iou, mode=1 if remove else 0)
    count, out, ties, dropped = run_merge(L, counts, dets, due, ndue, cfg, dcap)
    merged = set(due[:max(0, min(ndue, n))])
    for s in range(n):
        if s not in merged:  # not due: every output still holds its sentinel
            assert count[s] == -7 and np.all(out[s] == SENT) and ties[s].tolist() == [-9, -9] and dropped[s] == -11, s
            continue
        rows, t, d = want[s]
        k = min(len(rows), dcap)
        assert count[s] == len(rows), (s, count[s], len(rows))    # exact, whatever dcap is
        assert TR.same_f32(out[s, :k].view(f32), rows[:k]), (s, out[s, :k].view(f32), rows[:k])
        assert np.all(out[s, k:] == SENT), s                      # nothing written past the list or dcap
        assert ties[s].tolist() == list(t), (s, ties[s], t)
        assert dropped[s] == d, (s, dropped[s], d)
    return want


def _row(conf, cx, cy, w, h, angle=0.1, keypoints=6, seed=0):
    r = np.zeros(20, f32)
    r[:6] = conf, angle, cx, cy, w, h
    r[6:6 + 2 * keypoints] = np.random.default_rng(seed).uniform(0, 900, 2 * keypoints)
    return r


def duplicates_case():
    """T = 3, tile_cap = 4: two faces that two tiles report each, and one only tile 2 sees."""
    dets = np.zeros((1, 3, 4, 20), f32)
    dets[0, 0, 0] = _row(0.91, 300, 200, 80, 84, seed=1)
    dets[0, 1, 0] = _row(0.83, 304, 203, 78, 80, seed=2)      # the first face again
    dets[0, 1, 1] = _row(0.72, 620, 310, 64, 66, seed=3)
    dets[0, 2, 0] = _row(0.88, 618, 308, 66, 66, seed=4)      # the second face again
    dets[0, 2, 1] = _row(0.55, 100, 420, 50, 52, seed=5)      # the singleton
    return [[1, 2, 2]], dets


def test_merge_duplicates_across_tiles(L):
    counts, dets = duplicates_case()
    (rows, ties, dropped), = check_merge(L, counts, dets, 4)
    assert len(rows) == 3 and ties == (5, 0) and dropped == 0
    assert [round(float(c), 2) for c in rows[:, 0]] == [0.91, 0.88, 0.55]
    assert 300 < rows[0, 2] < 304 and 618 < rows[1, 2] < 620      # weighted centres lie between the pair's


def test_merge_counts_clamped(L):
    """Counts above tile_cap (the excess is counted, rows past the cap are not read as candidates) and
    negative counts (nothing)."""
    rng = np.random.default_rng(31)
    _, dets = random_tiles(rng, 4, 5, 6, clusters=3)
    want = check_merge(L, [[9, -3, 5, 2], [-1, -1, 0, 700]], np.stack([dets, dets]), 5)
    assert want[0][2] == 4 and want[0][1][0] == 12 and want[1][2] == 695 and want[1][1][0] == 5


def test_merge_all_counts_zero(L):
    rng = np.random.default_rng(32)
    _, dets = random_tiles(rng, 3, 4, 6)
    (rows, ties, dropped), = check_merge(L, [[0, 0, 0]], dets[None], 4)
    assert len(rows) == 0 and ties == (0, 0) and dropped == 0


def big_group_case():
    """T = 5, tile_cap = 26: a union of 65 and one of 130 candidates (past one wavefront in the sort),
    80 of the 130 on one face, so one group's compaction passes a wavefront too."""
    rng = np.random.default_rng(33)
    _, a = random_tiles(rng, 5, 26, 6, clusters=5)
    _, b = random_tiles(rng, 5, 26, 6, clusters=5)
    flat = b.reshape(130, 20)
    on_face = rng.permutation(130)[:80]
    flat[on_face, 2:4] = np.array([500, 300]) + rng.uniform(-2, 2, (80, 2))
    flat[on_face, 4:6] = 70
    for t in range(5):
        b[t] = b[t][np.argsort(-b[t, :, 0], kind="stable")]
    return [[26, 13, 0, 26, 0], [26] * 5], np.stack([a, b])


def test_merge_past_one_wavefront(L):
    counts, dets = big_group_case()
    want = check_merge(L, counts, dets, 26)
    assert want[0][1] == (65, 0) and want[1][1] == (130, 0)
    rows, _ = TR.union(counts[1], dets[1], 26)
    on_face = rows[(np.abs(rows[:, 2] - 500) <= 2) & (rows[:, 4] == 70)]
    seed = on_face[np.argmax(on_face[:, 0])]
    group = sum(1 for r in rows if TR.iou(seed[2:6], r[2:6]) >= f32(0.3)) - 1
    assert group >= 70, group
    assert len(want[1][0]) <= 130 - group


@pytest.mark.parametrize("remove", [False, True])
def test_merge_full_union(L, remove):
    """T = 16, tile_cap = 64: all 1024 candidates."""
    rng = np.random.default_rng(34)
    counts, dets = random_tiles(rng, 16, 64, 6, clusters=12, counts=[64] * 16)
    (rows, ties, dropped), = check_merge(L, counts[None], dets[None], 64, remove=remove)
    assert ties == (1024, 0) and dropped == 0 and 1 <= len(rows) < 200


def test_merge_remove_mode(L):
    counts, dets = duplicates_case()
    (rows, _, _), = check_merge(L, counts, dets, 4, remove=True)
    assert len(rows) == 3
    assert TR.same_f32(rows[0], dets[0, 0, 0]) and TR.same_f32(rows[1], dets[0, 2, 0])  # the seeds as they are


@pytest.mark.parametrize("remove", [False, True])
def test_merge_nan_iou(L, remove):
    """Two zero-area boxes at one place in different tiles: their IoU is 0 / 0.  Average leaves the
    second ungrouped, Remove drops it."""
    dets = np.zeros((1, 2, 2, 20), f32)
    dets[0, 0, 0] = _row(0.9, 100, 100, 0, 0, seed=6)
    dets[0, 1, 0] = _row(0.8, 100, 100, 0, 0, seed=7)
    dets[0, 1, 1] = _row(0.7, 300, 300, 50, 50, seed=8)
    (rows, _, _), = check_merge(L, [[1, 2]], dets, 2, remove=remove)
    assert len(rows) == (2 if remove else 3)


@pytest.mark.parametrize("remove", [False, True])
def test_merge_ties_keep_union_order(L, remove):
    counts, dets = tie_case()     # 18 candidates: within what the reference's sort pins
    (_, ties, _), = check_merge(L, counts[None], dets[None], 6, remove=remove)
    assert ties == (18, 3)


@pytest.mark.parametrize("keypoints", [0, 6, 7])
def test_merge_keypoints(L, keypoints):
    """The palm detector's 7 keypoints fill the record; with 6 (and 0) the fields past them are 0 even
    where the input rows hold something there."""
    rng = np.random.default_rng(35)
    counts, dets = random_tiles(rng, 3, 8, 7, clusters=3)
    want = check_merge(L, counts[None], dets[None], 8, keypoints=keypoints)
    assert np.all(want[0][0][:, 6 + 2 * keypoints:] == 0) and len(want[0][0]) >= 1
    check_merge(L, counts[None], dets[None], 8, keypoints=keypoints, remove=True)


def test_merge_dcap_below_count(L):
    rng = np.random.default_rng(36)
    counts, dets = random_tiles(rng, 4, 8, 6, clusters=6, counts=[8] * 4)
    want = check_merge(L, counts[None], dets[None], 8, dcap=2)
    assert len(want[0][0]) > 2


def test_merge_only_due_streams(L):
    """n = 5 with d_due = [1, 3]: the other streams' outputs keep their sentinels; and *d_ndue below
    the list's length, above n and negative."""
    rng = np.random.default_rng(37)
    cs, ds = zip(*[random_tiles(rng, 3, 6, 6, clusters=3) for _ in range(5)])
    counts, dets = np.stack(cs), np.stack(ds)
    check_merge(L, counts, dets, 6, due=[1, 3])
    check_merge(L, counts, dets, 6, due=[4, 0, 2], ndue=2)
    check_merge(L, counts, dets, 6, due=[3, 1, 0, 2, 4], ndue=1000)   # clamped to n
    check_merge(L, counts, dets, 6, due=[3, 1], ndue=-4)              # nothing
    # without the optional outputs
    cfg = L.DetMergeCfg(tiles=3, tile_cap=6, keypoints=6, iou=0.3, mode=0)
    count, out, ties, dropped = run_merge(L, counts, dets, [2], 1, cfg, 18, with_optional=False)
    rows = TR.merge(counts[2], dets[2], 6, 6)[0]
    assert count[2] == len(rows) and TR.same_f32(out[2, :len(rows)].view(f32), rows)
    assert np.all(ties == -9) and np.all(dropped == -11)


# ---- the tile compaction alone ------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 1025])
@pytest.mark.parametrize("pattern", ["mixed", "all", "none"])
def test_due_compact_tiles_alone(L, n, T, pattern):
    rng = np.random.default_rng(n * 10 + T)
    pending = {"mixed": rng.integers(-1, 2, n), "all": np.full(n, 3), "none": np.zeros(n)}[pattern].astype(np.int32)
    if pattern == "mixed":
        pending[0] = 1
    tm = rng.integers(1, 2 ** 31, (T, 10), dtype=np.int64).astype(np.uint32)  # any bits: copied as they are
    d_p, d_tm = L.DeviceBuffer.from_array(pending), L.DeviceBuffer.from_array(tm)
    d_due = L.DeviceBuffer.from_array(np.full(n, -7, np.int32))
    d_slots = L.DeviceBuffer.from_array(np.full(n * T, -7, np.int32))
    d_views = L.DeviceBuffer.from_array(np.full((n * T, 10), SENT, np.uint32))
    d_n = L.DeviceBuffer.from_array(np.array([-5, -5], np.int32))
    d_tot = L.DeviceBuffer.from_array(np.array([1000, 5000], np.uint64))
    due, slots, views, ndue, nviews = TR.compact_tiles(pending, tm)
    for call in (1, 2):  # the totals accumulate
        L.check(L.lib().zr_due_compact_tiles_async(d_p.ptr, n, d_tm.ptr, T, d_due.ptr, d_n.ptr, d_slots.ptr, d_views.ptr,
                                                   d_n.ptr + 4, d_tot.ptr, d_tot.ptr + 8, None))
        L.synchronize()
        assert d_n.download((2,), np.int32).tolist() == [ndue, nviews]
        assert d_tot.download((2,), np.uint64).tolist() == [1000 + call * ndue, 5000 + call * nviews]
        got_due, got_slots = d_due.download((n,), np.int32), d_slots.download((n * T,), np.int32)
        got_views = d_views.download((n * T, 10), np.uint32)
        assert np.array_equal(got_due[:ndue], due) and np.all(got_due[ndue:] == -7)
        assert np.array_equal(got_slots[:nviews], slots) and np.all(got_slots[nviews:] == -7)
        assert np.array_equal(got_views[:nviews], views)        # the templates, byte for byte, but for `frame`
        assert np.all(got_views[nviews:] == SENT)                # entries past the counts untouched
    # without the totals
    L.check(L.lib().zr_due_compact_tiles_async(d_p.ptr, n, d_tm.ptr, T, d_due.ptr, d_n.ptr, d_slots.ptr, d_views.ptr,
                                               d_n.ptr + 4, None, None, None))
    L.synchronize()
    assert d_tot.download((2,), np.uint64).tolist() == [1000 + 2 * ndue, 5000 + 2 * nviews]
    if pattern == "none":
        assert ndue == 0
    if pattern == "all":
        assert nviews == n * T


def test_due_compact_tiles_equals_due_compact(L):
    """One tile: the existing entry's outputs."""
    n = 1500
    rng = np.random.default_rng(5)
    pending = rng.integers(0, 2, n).astype(np.int32)
    tm = rng.integers(1, 2 ** 31, (1, 10), dtype=np.int64).astype(np.uint32)
    d_p, d_tm = L.DeviceBuffer.from_array(pending), L.DeviceBuffer.from_array(tm)
    outs = []
    for tiled in (False, True):
        d_due, d_views = L.DeviceBuffer.from_array(np.full(n, -7, np.int32)), L.DeviceBuffer.from_array(np.full((n, 10), SENT, np.uint32))
        d_n, d_slots = L.DeviceBuffer.from_array(np.array([-5, -5], np.int32)), L.DeviceBuffer(n * 4)
        if tiled:
            L.check(L.lib().zr_due_compact_tiles_async(d_p.ptr, n, d_tm.ptr, 1, d_due.ptr, d_n.ptr, d_slots.ptr, d_views.ptr,
                                                       d_n.ptr + 4, None, None, None))
        else:
            L.check(L.lib().zr_due_compact_async(d_p.ptr, n, tm.ctypes.data, d_due.ptr, d_n.ptr, d_views.ptr, None, None))
        L.synchronize()
        outs.append((d_due.download((n,), np.int32), d_views.download((n, 10), np.uint32), d_n.download((1,), np.int32)))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


# ---- refusals -----------------------------------------------------------------------------------------
def test_entries_refuse_and_write_nothing(L):
    lib = L.lib()
    n, T, cap = 2, 3, 4
    d_out = L.DeviceBuffer.from_array(np.full(4096, SENT, np.uint32))   # every output of every refused call
    d_in = L.DeviceBuffer.from_array(np.ones(4096, np.int32))
    o, i = d_out.ptr, d_in.ptr
    # zr_due_compact_tiles_async(pending, n, templates, tiles, due, ndue, slots, views, nviews, total_s, total_v, stream)
    good = [i, n, i, T, o, o + 64, o + 128, o + 1024, o + 68, None, None, None]
    for k in (0, 2, 4, 5, 6, 7, 8):
        a = list(good)
        a[k] = None
        assert lib.zr_due_compact_tiles_async(*a) == -1, k
    for nn, tt in ((0, T), (n, 0), (n, 17)):
        a = list(good)
        a[1], a[3] = nn, tt
        assert lib.zr_due_compact_tiles_async(*a) == -1, (nn, tt)
    # zr_detect_merge_async(tile_count, tile_dets, due, ndue, n, cfg, count, dets, dcap, ties, dropped, stream)
    cfg = L.DetMergeCfg(tiles=T, tile_cap=cap, keypoints=6, iou=0.3, mode=0)

    def merge(c=cfg, nn=n, dcap=8, null=None):
        a = [i, i, i, i, nn, None if c is None else C.byref(c), o, o + 1024, dcap, o + 64, o + 128, None]
        if null is not None:
            a[null] = None
        return lib.zr_detect_merge_async(*a)

    for k in (0, 1, 2, 3, 6, 7):
        assert merge(null=k) == -1, k
    assert merge(c=None) == -1 and merge(nn=0) == -1 and merge(dcap=0) == -1
    for field, value in (("tiles", 0), ("tiles", 17), ("tile_cap", 0), ("tile_cap", 257), ("keypoints", -1),
                         ("keypoints", 8)):
        bad = L.DetMergeCfg.from_buffer_copy(cfg)
        setattr(bad, field, value)
        assert merge(bad) == -1, (field, value)
    assert merge(L.DetMergeCfg(tiles=16, tile_cap=65, keypoints=6, iou=0.3, mode=0)) == -1   # 1040 > 1024
    L.synchronize()
    assert np.all(d_out.download((4096,), np.uint32) == SENT)


def test_set_detection_tiles_refusals(H):
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    assert dev.detection_tiles() == []
    tiles = H.detection_tiles(960, 540, 2, 1)
    dev.set_detection_tiles(tiles, 32)
    r = H.Rect.from_center(100.0, 100.0, 50.0, 50.0)
    for rects, cap in (([r] * 17, 4), (tiles, 0), (tiles, 257), ([r] * 5, 205), ([r] * 16, 65)):
        with pytest.raises(RuntimeError):
            dev.set_detection_tiles(rects, cap)
        assert dev.detection_tiles() == tiles     # what was set stays
    with pytest.raises(RuntimeError):
        H.TiledDetector("face", [])
    with pytest.raises(RuntimeError):
        H.TiledDetector("face", [r] * 17)
    with pytest.raises(RuntimeError):
        H.TiledDetector("face", tiles).set_tile_cap(400)
    dev.set_detection_tiles([])
    assert dev.detection_tiles() == [] and dev.detector_views() == 0 and dev.dropped_tile_detections() == [0]


# ---- the host TiledDetector on the scene ----------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return TR.scene_frame(), TR.gray_frame()


@pytest.fixture(scope="module")
def tiles(H):
    t = H.detection_tiles(TR.SCENE_W, TR.SCENE_H, 2, 1, 0.25, True)
    assert TR.same_f32(np.array([r.tuple() for r in t], f32), TR.scene_tiles())
    return t


def test_tiled_detector_finds_what_the_full_frame_misses(H, scene, tiles):
    import track_kernels_ref as KR
    frame, gray = scene
    assert H.Detector("face").detect(frame) == []
    tiled = H.TiledDetector("face", tiles)
    got = tiled.detect(frame)
    per_want, want = TR.oracle_tiled(frame, TR.scene_tiles())
    print("tiled:", [(d.confidence(), d.bounding_rect().tuple()) for d in got])
    print("oracle:", [(d.conf, d.rect.tuple()) for d in want])
    assert len(got) == 2 and len(want) == 2
    per = tiled.tile_detections(frame)
    assert [len(p) for p in per] == [len(p) for p in per_want] and len(per[0]) == 0
    # test_gpu_host_api.py::test_detector_detects_face's bar: 1e-2 input pixels, here of a tile whose
    # letterbox side is the tile's width
    side = max(tiles[1].width(), tiles[1].height())
    tol = 1e-2 * side / 128.0
    for g, w in zip(got, want):
        assert np.allclose(g.bounding_rect().tuple(), w.rect.tuple(), rtol=0, atol=tol), (g.bounding_rect().tuple(), w.rect.tuple())
    # the merged list is tiled_ref.merge of the tiles' own lists, bit for bit
    cap = 8
    rows = np.zeros((3, cap, 20), f32)
    for t, p in enumerate(per):
        rows[t, :len(p)] = KR.det_rows(p, host=True)
    assert TR.same_f32(TR.merge([len(p) for p in per], rows, cap, 6)[0], KR.det_rows(got, host=True))
    assert tiled.ties() == (sum(len(p) for p in per), 0) and tiled.dropped() == 0
    assert tiled.detect(gray) == [] and all(p == [] for p in tiled.tile_detections(gray))
    # the full-frame tile's own list is the plain detector's (the merge then averages each lone
    # detection with itself, x * c / c, which may move a last bit: that is process() run twice)
    big = np.repeat(np.repeat(TR.face_patch(192), 2, axis=0), 2, axis=1)
    f = TR.gray_frame()
    f[60:60 + 384, 100:100 + 384] = big
    plain = H.Detector("face").detect(f)
    one = H.TiledDetector("face", tiles[:1])
    assert len(plain) >= 1 and TR.same_f32(KR.det_rows(plain, host=True), KR.det_rows(one.tile_detections(f)[0], host=True))
    # two roundings of 2^-24 each
    assert np.allclose(KR.det_rows(plain, host=True), KR.det_rows(one.detect(f), host=True), rtol=3e-7, atol=0)


# ---- the loop -------------------------------------------------------------------------------------------
def _record(objs, count, pending):
    return (int(count), bool(pending),
            [(int(o["id"]), np.asarray(o["rect"], f32).tobytes(), f32(o["angle"]).tobytes(),
              np.ascontiguousarray(o["landmarks"], f32).tobytes(), f32(o["confidence"]).tobytes()) for o in objs])


def _ref_objects(ref):
    return [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
             "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in ref.objects()]


def _dev_objects(dev, s):
    return [{"id": o["id"], "rect": o["view_rect"].rect().tuple(), "angle": o["view_rect"].rotation_radians(),
             "landmarks": o["landmarks"], "confidence": o["confidence"]} for o in dev.objects(s)]


STEPS = 5


def _run(H, L, video, tiles_at):
    """video [steps][streams] frames; tiles_at(step) -> rects or None (leave as it is).  Returns the
    tracker and per step its streams' records and object counts."""
    n = len(video[0])
    h, w = video[0][0].shape[:2]
    dev = H.DeviceMultiTracker("face", "facemesh", n, 4)
    bufs = [L.DeviceBuffer.from_array(np.stack(fr)) for fr in video]
    records, counts = [], []
    for t, buf in enumerate(bufs):
        rects = tiles_at(t)
        if rects is not None:
            dev.set_detection_tiles(rects)
        dev.step([(buf.ptr + s * h * w * 4, w, h, w * 4) for s in range(n)], 33.0 * t)
        dev.synchronize()
        c, p = dev.object_counts(), dev.detection_pending()
        records.append([_record(_dev_objects(dev, s), c[s], p[s]) for s in range(n)])
        counts.append(c)
    return dev, records, counts


def test_loop_tracks_the_small_faces(H, L, scene, tiles):
    video = [list(scene)] * STEPS
    tiled = H.TiledDetector("face", tiles)
    refs = [MR.MultiTrackerRef(H, "face", "facemesh", 4, detect=tiled.detect) for _ in range(2)]
    dev, records, counts = _run(H, L, video, lambda t: tiles if t == 0 else None)
    compared = 0
    for t in range(STEPS):
        for s in range(2):
            refs[s].step(video[t][s], 33.0 * t)
            want, got = _record(_ref_objects(refs[s]), len(refs[s].objs), refs[s].pending), records[t][s]
            assert got[:2] == want[:2], (t, s, got[:2], want[:2])
            assert [o[0] for o in got[2]] == [o[0] for o in want[2]], (t, s)
            for g, w in zip(got[2], want[2]):
                assert g == w, (t, s, g[0], [a == b for a, b in zip(g, w)])
                compared += 1
    print("counts:", counts, "compared:", compared)
    assert compared >= 6, compared
    assert [c[0] for c in counts] == [0] + [2] * (STEPS - 1), counts   # both faces from the step after the detection
    assert all(c[1] == 0 for c in counts), counts
    frames = dev.detector_frames()
    assert frames == sum(r.detector_frames for r in refs)
    assert dev.detector_views() == len(tiles) * frames
    assert dev.dropped_tile_detections() == [0, 0] and dev.dropped_detections() == [0, 0]
    assert dev.detection_tiles() == tiles
    # the packed export agrees with objects() under tiling
    packed = dev.objects_packed()
    listed = [o for s in range(2) for o in dev.objects(s)]
    assert packed["count"] == len(listed) == 2 and packed["stream_offsets"].tolist() == [0, 2, 2]
    for k, o in enumerate(listed):
        assert packed["id"][k] == o["id"] and packed["stream"][k] == 0
        assert np.array_equal(packed["landmarks"][k], o["landmarks"])
        assert packed["view_rect"][k, :4].tolist() == list(o["view_rect"].rect().tuple())
        assert packed["confidence"][k] == f32(o["confidence"])


def test_loop_without_tiles_sees_nobody(H, L, scene):
    """The same video through a tracker without tiles: the faces are too small for the full-frame
    pass, so no object exists at any step."""
    dev, records, counts = _run(H, L, [list(scene)] * STEPS, lambda t: None)
    assert all(c == [0, 0] for c in counts), counts
    assert all(r[2] == [] for step in records for r in step)
    assert dev.detector_views() == 0 and dev.detector_frames() == 2 * STEPS


def test_tiles_off_again_is_the_untiled_loop(H, L, scene, tiles):
    """A tracker that was tiled only while no face was in view, then switched off, and a fresh untiled
    tracker give equal records on the frames that follow (a face large enough for the full frame)."""
    gray = scene[1]
    face = gray.copy()
    face[60:60 + 384, 100:100 + 384] = np.repeat(np.repeat(TR.face_patch(192), 2, axis=0), 2, axis=1)
    video = [[gray]] * 2 + [[face]] * 4
    a, rec_a, counts_a = _run(H, L, video, lambda t: tiles if t == 0 else [] if t == 2 else None)
    b, rec_b, counts_b = _run(H, L, video, lambda t: None)
    assert rec_a == rec_b
    assert counts_b[-1] == [1] and rec_b[-1][0][2] != []     # the face is found and tracked: not a vacuous match
    assert a.detector_views() == 2 * len(tiles) and b.detector_views() == 0
    assert a.detector_frames() == b.detector_frames()
