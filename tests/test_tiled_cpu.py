"""CPU-side checks of tiled detection: the restatements of tests/tiled_ref.py (the oracle of
tests/test_gpu_tiled.py) against the host pieces the suite already pins, the grid's known answers,
the premise of the GPU tests on the CPU oracle -- two small faces that the full-frame pass does not
find and the tiles do -- and what the two new C entry points refuse before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import zaru_amd.host as H
from zaru_amd import _lib

import multi_tracker_ref as MR
import tiled_ref as TR

f32 = np.float32


# ---- the grid -----------------------------------------------------------------------------------------
def _host_tiles(*a):
    return np.array([r.tuple() for r in H.detection_tiles(*a)], f32)


def test_grid_known_answers():
    t = TR.detection_tiles(960, 540, 2, 1, 0.25, True)
    assert t.shape == (3, 4)
    assert t[0].tolist() == [480.0, 270.0, 960.0, 540.0]                 # the full frame first
    w = 960.0 / 1.75
    assert np.allclose(t[1], [w / 2, 270.0, w, 540.0], rtol=0, atol=1e-3)        # [0, 548.57] x [0, 540]
    assert np.allclose(t[2], [960.0 - w / 2, 270.0, w, 540.0], rtol=0, atol=1e-3)  # [411.43, 960] x [0, 540]
    t = TR.detection_tiles(1920, 1080, 3, 2, 0.25, False)
    assert t.shape == (6, 4)
    w, h = 1920.0 / 2.5, 1080.0 / 1.75
    assert np.allclose(t[:, 2], w, atol=1e-3) and np.allclose(t[:, 3], h, atol=1e-3)
    x0, y0 = t[:, 0] - t[:, 2] / 2, t[:, 1] - t[:, 3] / 2
    assert np.allclose(x0, [0, 0.75 * w, 1920 - w] * 2, atol=1e-3)     # row-major, stride (1 - overlap) * size
    assert np.allclose(y0, [0] * 3 + [1080 - h] * 3, atol=1e-3)
    # the last column and row end at the frame's edge
    assert np.allclose((t[:, 0] + t[:, 2] / 2)[[2, 5]], 1920.0, atol=1e-3)
    assert np.allclose((t[:, 1] + t[:, 3] / 2)[3:], 1080.0, atol=1e-3)
    assert len(TR.detection_tiles(1920, 1080, 3, 2)) == 7                # overlap 0.25 and the full frame by default
    assert len(TR.detection_tiles(100, 100, 1, 1, 0.0, False)) == 1


@pytest.mark.parametrize("args", [(960, 540, 2, 1, 0.25, True), (1920, 1080, 3, 2, 0.25, True),
                                  (1920, 1080, 3, 2, 0.25, False), (641, 479, 4, 3, 0.1, True),
                                  (1280, 720, 5, 3, 0.5, True), (300, 200, 1, 1, 0.0, True), (333, 777, 4, 4, 0.33, False)])
def test_grid_restatement_equals_host(args):
    assert TR.same_f32(TR.detection_tiles(*args), _host_tiles(*args))


@pytest.mark.parametrize("args", [(960, 540, 0, 1, 0.25, True), (960, 540, 1, 0, 0.25, True),
                                  (960, 540, 2, 2, -0.1, True), (960, 540, 2, 2, 1.0, True),
                                  (960, 540, 2, 2, float("nan"), True), (960, 540, 4, 4, 0.25, True),
                                  (960, 540, 17, 1, 0.25, False)])
def test_grid_refusals(args):
    with pytest.raises(RuntimeError):
        H.detection_tiles(*args)
    with pytest.raises(ValueError):
        TR.detection_tiles(*args)
    assert len(H.detection_tiles(960, 540, 4, 4, 0.25, False)) == 16


# ---- the merge against NonMaxSuppression::process -------------------------------------------------------
def _host_process(rows, keypoints, iou, remove):
    nms = H.NonMaxSuppression()
    nms.set_iou_thresh(iou)
    nms.set_mode(H.SuppressionMode.Remove if remove else H.SuppressionMode.Average)
    return TR.from_detections(nms.process(TR.to_detections(H, rows, keypoints)))


@pytest.mark.parametrize("remove", [False, True])
@pytest.mark.parametrize("seed,T,cap,keypoints", [(1, 3, 4, 6), (2, 5, 26, 6), (3, 2, 9, 7), (4, 7, 16, 6), (5, 1, 30, 6)])
def test_merge_ref_equals_host_nms(seed, T, cap, keypoints, remove):
    rng = np.random.default_rng(seed)
    counts, dets = TR.random_tiles(rng, T, cap, keypoints, clusters=min(6, max(2, T * cap // 6)))
    rows, dropped = TR.union(counts, dets, cap)
    assert len(set(rows[:, 0].tolist())) == len(rows)  # distinct confidences: the order is the reference's
    got, ties, _ = TR.merge(counts, dets, cap, keypoints, 0.3, remove)
    want = _host_process(rows, keypoints, 0.3, remove)
    assert dropped == 0 and ties == (len(rows), 0)
    assert 0 < len(got) < len(rows) or len(rows) <= 1     # something was merged
    assert TR.same_f32(got, want)


@pytest.mark.parametrize("remove", [False, True])
def test_merge_ref_ties_keep_union_order(remove):
    counts, dets = TR.tie_case()
    rows, _ = TR.union(counts, dets, 6)
    got, ties, _ = TR.merge(counts, dets, 6, 6, 0.3, remove)
    assert ties == (18, 3)
    assert TR.same_f32(got, _host_process(rows, 6, 0.3, remove))


def test_union_clamps_and_counts_dropped():
    rng = np.random.default_rng(4)
    _, dets = TR.random_tiles(rng, 3, 4, 6)
    rows, dropped = TR.union([7, -3, 2], dets, 4)
    assert dropped == 3 and len(rows) == 6
    assert np.array_equal(rows, np.concatenate([dets[0], dets[2][:2]]))


def test_nan_iou_decides_as_the_comparisons_do():
    dets = np.zeros((2, 2, 20), f32)
    dets[0, 0, :6] = 0.9, 0.0, 100, 100, 0, 0   # two zero-area boxes at one place: IoU = 0 / 0
    dets[1, 0, :6] = 0.8, 0.0, 100, 100, 0, 0
    dets[1, 1, :6] = 0.7, 0.0, 300, 300, 50, 50
    avg, _, _ = TR.merge([1, 2], dets, 2, 6, 0.3, False)
    rem, _, _ = TR.merge([1, 2], dets, 2, 6, 0.3, True)
    assert len(avg) == 3 and len(rem) == 2      # Average leaves the second ungrouped; Remove drops it
    rows, _ = TR.union([1, 2], dets, 2)
    assert TR.same_f32(avg, _host_process(rows, 6, 0.3, False)) and TR.same_f32(rem, _host_process(rows, 6, 0.3, True))


# ---- the tile compaction --------------------------------------------------------------------------------
def test_compact_tiles_restatement():
    tm = np.arange(30, dtype=np.uint32).reshape(3, 10) + 100
    due, slots, views, ndue, nviews = TR.compact_tiles([0, 5, 0, -1], tm)
    assert due.tolist() == [1, 3] and (ndue, nviews) == (2, 6)
    assert slots.tolist() == [3, 4, 5, 9, 10, 11]
    assert views[:, 8].tolist() == [1, 1, 1, 3, 3, 3]
    want = np.tile(tm, (2, 1))
    assert np.array_equal(np.delete(views, 8, axis=1), np.delete(want, 8, axis=1))
    # one tile: due_compact_kernel's restatement
    import track_kernels_ref as KR
    d1, _, v1, n1, _ = TR.compact_tiles([1, 0, 1], tm[:1])
    d0, v0, n0 = KR.compact([1, 0, 1], tm[0])
    assert np.array_equal(d1, d0) and np.array_equal(v1, v0) and n1 == n0


# ---- the scene on the CPU oracle: the premise of the GPU tests -------------------------------------------
@pytest.fixture(scope="module")
def scene():
    tiles = TR.scene_tiles()
    return TR.oracle_tiled(TR.scene_frame(), tiles), TR.oracle_tiled(TR.gray_frame(), tiles)


def test_scene_full_frame_finds_nothing_tiles_find_both(scene):
    (per, merged), (per_gray, merged_gray) = scene
    print("per tile:", [[(d.conf, d.rect.tuple()) for d in p] for p in per])
    print("merged:", [(d.conf, d.rect.tuple()) for d in merged])
    assert len(per[0]) == 0                              # the full-frame pass sees neither face
    assert len(per[1]) >= 1 and len(per[2]) >= 1
    assert len(merged) == 2
    # each merged box lies on the face it stands for (centre within the patch, size of its order)
    for d, (size, x0, y0) in zip(sorted(merged, key=lambda d: d.rect.cx), TR.FACES):
        assert x0 < d.rect.cx < x0 + size and y0 < d.rect.cy < y0 + size, (d.rect.tuple(), size, x0, y0)
        assert 0.3 * size < d.rect.w < size and 0.3 * size < d.rect.h < size
    assert merged[0].conf >= merged[1].conf              # most confident first
    assert all(len(p) == 0 for p in per_gray) and len(merged_gray) == 0


def test_scene_merge_ref_equals_oracle_nms(scene):
    """The union of the oracle's per-tile lists through tiled_ref.merge gives the oracle's own NMS."""
    import track_kernels_ref as KR
    (per, merged), _ = scene
    cap = 8
    dets = np.zeros((3, cap, 20), f32)
    for t, p in enumerate(per):
        dets[t, :len(p)] = KR.det_rows(p, host=False)
    got, _, dropped = TR.merge([len(p) for p in per], dets, cap, 6)
    assert dropped == 0 and TR.same_f32(got, KR.det_rows(merged, host=False))


# ---- the bookkeeping is indifferent to where detections come from ------------------------------------------
class _FakeTracker:
    def __init__(self):
        self.roi = None

    def set_roi_padding(self, p):
        pass

    def set_loss_threshold(self, t):
        pass

    def set_roi(self, roi):
        self.roi = roi

    def track(self, frame):
        return {"updated_roi": self.roi, "landmarks": self.roi.rect().center[0], "confidence": 1.0}


def test_tracker_ref_with_scripted_tiled_detect():
    """A detect() that merges scripted per-tile lists: a face both tiles report starts one object, a
    face one tile reports another, and the next detection of the same faces starts none."""
    dets = np.zeros((2, 4, 20), f32)
    dets[0, 0, :6] = 0.9, 0.0, 300, 200, 80, 80     # tile 0 and tile 1 see the same face
    dets[1, 0, :6] = 0.8, 0.0, 303, 201, 80, 80
    dets[1, 1, :6] = 0.7, 0.0, 700, 150, 70, 70     # only tile 1 sees this one
    calls = []

    def detect(frame):
        rows, _, _ = TR.merge([1, 2], dets, 4, 6)
        calls.append(len(rows))
        return TR.to_detections(H, rows, 6)

    ref = MR.MultiTrackerRef(H, "face", "facemesh", 4, make_tracker=_FakeTracker, detect=detect)
    ref.interval = 40.0
    seen = []
    for k in range(5):
        ref.step({}, 15.0 * k)
        seen.append((ref.ids(), ref.pending))
    assert calls == [2, 2]
    assert seen == [([], True), ([0, 1], False), ([0, 1], False), ([0, 1], True), ([0, 1], False)], seen
    assert ref.filtered == 2 and ref.detector_frames == 2
    assert ref.objs[0].roi.rect().center[0] != 300.0   # the merged box, not tile 0's


# ---- the C entries refuse before they touch a device ----------------------------------------------------------
def test_new_entry_points_refuse_bad_arguments():
    lib = _lib.lib()
    p = 4096  # stands for a device pointer: none of these calls gets as far as using it
    # zr_due_compact_tiles_async(pending, n, templates, tiles, due, ndue, slots, views, nviews, total_s, total_v, stream)
    good = [p, 8, p, 3, p, p, p, p, p, None, None, None]
    assert C.sizeof(_lib.DetMergeCfg) == 20
    for i in (0, 2, 4, 5, 6, 7, 8):
        a = list(good)
        a[i] = None
        assert lib.zr_due_compact_tiles_async(*a) == -1, i
    for n, t in ((0, 3), (8, 0), (8, 17), (2 ** 25, 3)):
        a = list(good)
        a[1], a[3] = n, t
        assert lib.zr_due_compact_tiles_async(*a) == -1, (n, t)
    # zr_detect_merge_async(tile_count, tile_dets, due, ndue, n, cfg, count, dets, dcap, ties, dropped, stream)
    cfg = _lib.DetMergeCfg(tiles=3, tile_cap=64, keypoints=6, iou=0.3, mode=0)

    def merge(c=cfg, n=4, dcap=896, null=None):
        a = [p, p, p, p, n, None if c is None else C.byref(c), p, p, dcap, None, None, None]
        if null is not None:
            a[null] = None
        return lib.zr_detect_merge_async(*a)

    for i in (0, 1, 2, 3, 6, 7):
        assert merge(null=i) == -1, i
    assert merge(c=None) == -1 and merge(n=0) == -1 and merge(dcap=0) == -1
    for field, value in (("tiles", 0), ("tiles", 17), ("tile_cap", 0), ("tile_cap", 257), ("keypoints", -1),
                         ("keypoints", 8), ("mode", 2)):
        bad = _lib.DetMergeCfg.from_buffer_copy(cfg)
        setattr(bad, field, value)
        assert merge(bad) == -1, (field, value)
    assert merge(_lib.DetMergeCfg(tiles=16, tile_cap=65, keypoints=6, iou=0.3, mode=0)) == -1   # 1040 > 1024
    assert merge(_lib.DetMergeCfg(tiles=5, tile_cap=205, keypoints=6, iou=0.3, mode=0)) == -1   # 1025 > 1024
