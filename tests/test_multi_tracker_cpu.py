"""CPU-side checks of the multi-object tracker: the oracle of tests/test_gpu_multi_tracker.py
(tests/multi_tracker_ref.py) pinned against a hand-written expectation, and what the three new C
entry points refuse before they touch a device."""
import ctypes as C

import zaru_amd.host as H
from zaru_amd import _lib

import multi_tracker_ref as MR


def _rect(cx, cy, w=40.0, h=40.0):
    return H.Rect.from_center(cx, cy, w, h)


class _FakeTracker:
    """A LandmarkTracker whose estimates the frame scripts: a frame is {"lose": {cx, ...},
    "move": {cx: Rect}, "dets": [...]}, keyed by the centre x of the RoI the tracker holds."""

    def __init__(self, log):
        self.roi, self.log = None, log

    def set_roi_padding(self, p):
        self.log.append(("padding", p))

    def set_loss_threshold(self, t):
        self.log.append(("loss", t))

    def set_roi(self, roi):
        self.roi = roi

    def track(self, frame):
        cx = self.roi.rect().center[0]
        if cx in frame.get("lose", ()):
            return None
        if cx in frame.get("move", {}):
            self.roi = H.RotatedRect(frame["move"][cx], self.roi.rotation_radians())
        return {"updated_roi": self.roi, "landmarks": cx, "confidence": 1.0}


def test_oracle_bookkeeping_matches_hand_written_expectation():
    D = H.Detection
    log = []
    frames = [
        # step 0: nothing tracked -> a detection runs on this frame and is taken at step 1;
        # C lies on A, so the sweep removes it and swap_remove moves D into its place
        {"dets": [D(0.9, _rect(100.0, 100.0), 0.5), D(0.9, _rect(300.0, 100.0), 0.0),
                  D(0.8, _rect(104.0, 100.0), 0.0), D(0.7, _rect(200.0, 300.0), 0.0)]},
        {},
        {"lose": {100.0}},                       # A's estimate on this frame is below the threshold
        {"dets": [], "move": {50.0: _rect(300.0, 100.0)}},  # G drifts onto B
        {},
    ]
    injected = {2: [D(0.9, _rect(300.0, 100.0), 0.0), D(0.9, _rect(400.0, 300.0), 0.0)],   # E on B (filtered), F
                3: [D(0.9, _rect(50.0, 300.0), 0.0), D(0.9, _rect(450.0, 50.0), 0.0)]}    # G, and H past the 4 slots
    ref = MR.MultiTrackerRef(H, "face", "facemesh", 4, make_tracker=lambda: _FakeTracker(log),
                             detect=lambda f: f["dets"])
    ref.interval = 40.0
    ref.loss = -1.0
    got = []
    for k, f in enumerate(frames):
        ref.step(f, 15.0 * k, injected.get(k, ()))
        got.append((ref.ids(), [o.id for o in ref.objects()], ref.pending, ref.dropped))
    assert got == [
        ([], [], True, 0),                 # 0 ms: empty -> detect; the clock moves to 40 ms
        ([0, 1, 3], [], False, 0),         # ids 0..3 start, 2 is swept, 3 takes its place; no result yet
        ([0, 1, 3, 4], [0, 1, 3], False, 0),   # E filtered against B, F starts as 4
        ([1, 3, 4, 5], [1, 3, 4], True, 1),    # A lost; G starts as 5, H finds no slot; 45 ms >= 40 ms -> detect
        ([1, 3, 4], [1, 3, 4], False, 0),      # G moved onto B: swept (the later one leaves)
    ], got
    assert (ref.filtered, ref.swept, ref.detector_frames, ref.next_id) == (1, 2, 2, 6)
    assert ref.next_det == 80.0
    # faces: the RoI is the detection's rect, unrotated, with the LandmarkTracker's default padding
    assert ("padding", 0.3) in log and ("loss", -1.0) in log
    assert ref.objs[0].roi.rotation_radians() == 0.0
    # the palm defaults: grow 1.5 and the detection's angle
    palm = MR.MultiTrackerRef(H, "palm", "hand", 4, make_tracker=lambda: _FakeTracker(log), detect=lambda f: [])
    palm.step({}, 0.0, [D(0.9, _rect(100.0, 100.0), 0.5)])
    assert palm.objs[0].roi.rect() == _rect(100.0, 100.0).grow_rel(1.5)
    assert palm.objs[0].roi.rotation_radians() == 0.5 and ("padding", 0.4) in log


def test_new_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    p = 4096  # stands for a device pointer: none of these calls gets as far as using it
    # zr_slot_compact_async(counts, n_streams, slots, views, dense_views, dense_of, nactive, total, stream)
    good = [p, 8, 4, p, p, p, p, p, None]
    for i in (0, 3, 4, 5, 6):
        a = list(good)
        a[i] = None
        assert lib.zr_slot_compact_async(*a) == -1, i
        assert b"null" in lib.zr_last_error()
    for n, k in ((0, 4), (8, 0), (8, 65), (2 ** 30, 2), (2 ** 31 - 1, 2), (2 ** 40, 1)):
        a = list(good)
        a[1], a[2] = n, k
        assert lib.zr_slot_compact_async(*a) == -1, (n, k)
    # zr_multi_manage_async: the configuration
    cfg = _lib.MultiCfg(slots=4, iou_thresh=0.3, det_grow=0.0, use_angle=0, interval_ms=300.0, aspect_w=1, aspect_h=1)

    def manage(c, n=2, dcap=896, state=p):
        return lib.zr_multi_manage_async(state, p, p, p, p, p, p, p, p, p, dcap, p, n, None if c is None else C.byref(c),
                                         0.0, 1, p, None, None)

    assert manage(None) == -1
    assert manage(cfg, state=None) == -1
    for field, value in (("slots", 0), ("slots", 65), ("det_grow", -0.5), ("det_grow", float("nan")),
                         ("interval_ms", -1.0), ("aspect_w", 0), ("aspect_h", -1)):
        bad = _lib.MultiCfg.from_buffer_copy(cfg)
        setattr(bad, field, value)
        assert manage(bad) == -1, (field, value)
    assert manage(cfg, dcap=0) == -1 and manage(cfg, n=2 ** 23) == -1
    assert C.sizeof(_lib.MultiCfg) == 32
    # zr_track_update_indexed_async: zr_track_update_async's checks
    tc = _lib.TrackCfg(kind=0, num_landmarks=468, in_w=192, in_h=192, aspect_w=1, aspect_h=1, loss_thresh=0.5,
                       padding=0.3, rois_per_frame=4)

    def update(c, state=p, n=8, lm=p, lm_stride=1404, flag=p, flag_stride=1, views=p):
        return lib.zr_track_update_indexed_async(state, n, C.byref(c), lm, lm_stride, flag, flag_stride, p, p, views, None)

    assert update(tc, state=None) == -1 and update(tc, n=0) == -1 and update(tc, views=None) == -1
    assert update(tc, lm=None) == -1 and update(tc, flag=None) == -1 and update(tc, flag_stride=0) == -1
    assert update(tc, lm_stride=1403) == -4  # ZR_ERR_SHAPE: fewer floats per image than the extract reads
    for field, value in (("kind", 4), ("num_landmarks", 263), ("padding", -0.1), ("rois_per_frame", -1)):
        bad = _lib.TrackCfg.from_buffer_copy(tc)
        setattr(bad, field, value)
        assert update(bad) == -1, (field, value)
