"""The oracle of the device multi-object tracker: a Python restatement of HandTracker::track
(crates/zaru/src/hand/tracking.rs:115-219) for any (detector, landmarker), one host
``zaru_amd.host.LandmarkTracker`` per object.

Schedule as DeviceHandTracker / DeviceMultiTracker run it: a detection requested at step t runs on
step t's frame and is taken at step t + 1 (the reference's worker finishing within a frame), and an
object's estimate on step t's frame is consumed at step t + 1 (the reference's promise handles).
The host trackers are synchronous, so the estimate is made at the end of step t and kept.

``make_tracker`` and ``detect`` are replaceable, so the bookkeeping can be pinned without a GPU
(tests/test_multi_tracker_cpu.py)."""

DEFAULTS = {
    # detector -> (det_grow, use_angle, roi_padding): examples/facemesh.rs:49-54 with
    # LandmarkTracker::DEFAULT_ROI_PADDING for faces; tracking.rs:34,136,159 for the palm
    "face": (0.0, False, 0.3),
    "face_full": (0.0, False, 0.3),
    "palm": (1.5, True, 0.4),
}


class _Object:
    def __init__(self, oid, roi, tracker):
        self.id = oid
        self.roi = roi          # TrackedHand::roi
        self.tracker = tracker
        self.pending = None     # the estimate made on the last frame, consumed by the next step
        self.lm = None          # TrackedHand::lm


class MultiTrackerRef:
    def __init__(self, H, detector="face", landmarker="facemesh", slots=4, make_tracker=None, detect=None):
        self.H = H
        self.slots = slots
        self.det_grow, self.use_angle, self.padding = DEFAULTS[detector]
        self.iou = 0.30000001192092896  # HandTracker::DEFAULT_IOU_THRESH, 0.3f32
        self.interval = 300.0    # HandTracker::DEFAULT_REDETECT_INTERVAL
        self.loss = None         # LandmarkTracker's default
        self.make_tracker = make_tracker or (lambda: H.LandmarkTracker(landmarker))
        if detect is None:
            det = H.Detector(detector)
            detect = det.detect
        self.detect = detect
        self.objs = []
        self.next_id = 0
        self.next_det = None     # the clock starts at the first step
        self.det_result = None   # the running detection's result (taken by the next step)
        self.dropped = 0
        self.detector_frames = 0
        self.filtered = 0        # detections the IoU filter removed, summed
        self.swept = 0           # objects the de-duplication sweep removed, summed

    def _start(self, roi):
        t = self.make_tracker()
        t.set_roi_padding(self.padding)
        if self.loss is not None:
            t.set_loss_threshold(self.loss)
        t.set_roi(roi)
        o = _Object(self.next_id, roi, t)
        self.next_id += 1
        return o

    def step(self, frame, now_ms, injected=()):
        H = self.H
        if self.next_det is None:
            self.next_det = now_ms
        # retain_mut (116-127): lost objects leave, the others take their result
        kept = []
        for o in self.objs:
            if o.pending is None:
                continue
            o.lm = o.pending
            o.roi = o.pending["updated_roi"]
            kept.append(o)
        self.objs = kept
        # the finished detection (129-134), the injected ones first
        dets = list(injected)
        if self.det_result is not None:
            dets += list(self.det_result)
            self.det_result = None
        # retain (140-156) against the objects that existed before this step's new ones
        rois = [o.roi.rect() for o in self.objs]
        keep = []
        for d in dets:
            grown = d.bounding_rect().grow_rel(self.det_grow)
            if any(r.iou(grown) >= self.iou for r in rois):
                self.filtered += 1
                continue
            keep.append((d, grown))
        # extend (158-194); the device's slots are bounded and report the overflow
        self.dropped = 0
        for d, grown in keep:
            if len(self.objs) >= self.slots:
                self.dropped += 1
                continue
            self.objs.append(self._start(H.RotatedRect(grown, d.angle() if self.use_angle else 0.0)))
        # the swap_remove sweep (196-208)
        idx = H.HandTracker.dedupe_rois([o.roi.rect() for o in self.objs], self.iou)
        self.swept += len(self.objs) - len(idx)
        self.objs = [self.objs[i] for i in idx]
        # (re)detection (210-218): none is running here, the last one was taken above
        self.pending = len(self.objs) == 0 or now_ms >= self.next_det
        if self.pending:
            self.next_det += self.interval
            self.det_result = self.detect(frame)
            self.detector_frames += 1
        # every object's worker on this frame
        for o in self.objs:
            o.pending = o.tracker.track(frame)

    def objects(self):
        """HandTracker::hands: the objects that have a result, in order."""
        return [o for o in self.objs if o.lm is not None]

    def ids(self):
        return [o.id for o in self.objs]
