"""The oracle of the eye refinement (zaru_amd.host.EyeRefiner, DeviceMultiTracker.set_eye_refinement).

Two layers:

  * a numpy / ``oracle`` restatement of the semantics -- the eye rects of a face mesh
    (face/landmark/mediapipe.rs:146-192), the crop, the view the Estimator samples of it
    (landmark.rs:320-323), the un-mirroring (face/eye.rs:121-125) and the iris diameter
    (eye.rs:105-114) -- and the independent chain of the whole refinement through the oracle's
    preprocessing and its f32 network (``refine_chain``);
  * ``MultiEyeRef``: tests/multi_tracker_ref.py's MultiTrackerRef with the eyes of every object, the
    way tests/multi_identity_ref.py carries identities.  After a step's tracker updates (the
    estimates made on the previous frame, ``_Object.pending``) and before its bookkeeping, every
    tracked object's eyes are refined from *this* step's frame at the place those landmarks give.

``refine`` is replaceable, so the bookkeeping can be pinned without a GPU (tests/test_eye_cpu.py)."""
import numpy as np

f32 = np.float32
LEFT = (145, 33, 133, 159)      # LeftEyeBottom, OuterCorner, InnerCorner, Top: the reference's order
RIGHT = (374, 362, 263, 386)    # RightEyeBottom, InnerCorner, OuterCorner, Top
CORNERS = (33, 263)
GROW = 0.65
SIDE = 64                       # iris_landmark.onnx: 64 x 64, ColorMapper::linear(-1..=1)


def face_angle(O, lm):
    a, b = lm[CORNERS[1]], lm[CORNERS[0]]
    return O.signed_angle_to((f32(a[0] - b[0]), f32(a[1] - b[1])), (1.0, 0.0))


def eye_rects(O, lm):
    """(left, right) as oracle RRects; None for an invalid eye."""
    lm = np.asarray(lm, f32)
    out = []
    for idx in (LEFT, RIGHT):
        used = lm[list(idx) + list(CORNERS), :2]
        if not np.isfinite(used).all():
            out.append(None)
            continue
        r = O.rrect_bounding(face_angle(O, lm), [lm[i, :2] for i in idx])
        out.append(r if (r.rect.w > 0 and r.rect.h > 0) else None)
    return tuple(out)


def crop_rect(O, eye, grow=GROW):
    return O.RRect(O.grow_to_fit_aspect(O.grow_rel(eye.rect, grow), SIDE, SIDE), eye.rad)


def network_view(O, crop, W, Hh):
    """(the view the network samples, the Estimator's map-out rect): ViewData::view twice."""
    view = O.view_compose(O.view_full(W, Hh), crop)
    lrect = O.grow_to_fit_aspect(O.Rect.from_top_left(0, 0, view.rect.w, view.rect.h), SIDE, SIDE)
    return O.view_compose(view, lrect), lrect


def flip(pos, width=SIDE):
    """EyeLandmarks::flip_horizontal_in_place: x = -(x - half) + half, one rounding per operation."""
    p = np.array(pos, f32)
    half = f32(f32(width) / f32(2.0))
    p[:, 0] = (-(p[:, 0] - half)).astype(f32) + half
    return p


def iris_diameter(pos):
    p = np.asarray(pos, f32)
    radius = f32(0.0)
    for k in range(1, 5):
        d = (p[0] - p[k]).astype(f32)
        d2 = f32(f32(f32(f32(0.0) + f32(d[0] * d[0])) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
        radius = f32(radius + np.sqrt(d2, dtype=f32))
    return f32(f32(radius / f32(4.0)) * f32(2.0))


def refine_chain(O, net, img, lm, grow=GROW, mirror=True):
    """The independent chain on one face: O.preproc on the composed view -> mirror the tensor for the
    right eye -> the oracle's f32 network -> extract -> un-mirror -> O.estimator_map -> O.transform_out.
    net: O.Net(iris_landmark.onnx, f64=False).  mirror=False leaves the right eye's mirroring out (of
    the tensor and of the landmarks).  Returns {side: None | {landmarks, iris_diameter, crop, per_px}}."""
    Hh, W = img.shape[:2]
    out = {}
    for side, eye in zip(("left", "right"), eye_rects(O, lm)):
        if eye is None:
            out[side] = None
            continue
        crop = crop_rect(O, eye, grow)
        view, lrect = network_view(O, crop, W, Hh)
        x = O.preproc(img, view, SIDE, SIDE, -1.0, 1.0)
        flipped = side == "right" and mirror
        if flipped:
            x = np.ascontiguousarray(x[:, :, ::-1])
        outs = net.run(x[None])
        pos = np.concatenate([outs[1].reshape(5, 3), outs[0].reshape(71, 3)]).astype(f32)
        if flipped:
            pos = flip(pos)
        pos = O.estimator_map(pos, lrect, SIDE)
        for j in range(pos.shape[0]):
            pos[j, 0], pos[j, 1] = O.transform_out(crop, pos[j, 0], pos[j, 1])
        out[side] = {"landmarks": pos, "iris_diameter": iris_diameter(pos), "crop": crop,
                     "per_px": f32(lrect.w / f32(SIDE))}
    return out


class MultiEyeRef:
    def __init__(self, tracker, refine):
        """tracker: a MultiTrackerRef.  refine(frame, landmarks) -> {"left": ..., "right": ...}, each None
        or a result."""
        self.tracker = tracker
        self.refine = refine
        self.images = 0        # valid eyes, summed: eye_images()
        self.lost = 0          # objects that left because their estimate was below the loss threshold
        self.last_tracked = []

    def step(self, frame, now_ms, injected=()):
        self.last_tracked = []
        for o in self.tracker.objs:
            if o.pending is None:  # lost: it leaves in this step's bookkeeping, with no landmarks
                self.lost += 1
                continue
            o.eyes = self.refine(frame, o.pending["landmarks"])
            self.images += sum(1 for side in ("left", "right") if o.eyes[side] is not None)
            self.last_tracked.append(o.id)
        self.tracker.step(frame, now_ms, injected)

    def objects(self):
        """(object, eyes) for the objects that have a result, in order."""
        return [(o, getattr(o, "eyes", None)) for o in self.tracker.objects()]
