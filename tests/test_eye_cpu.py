"""Eye refinement, the parts that need no GPU:

  * zaru_amd.host.face_eye_rects / eye_crop_rect / eye_crop_view / EyeLandmarks against the oracle's
    rect geometry (O.rrect_bounding, O.grow_rel, O.grow_to_fit_aspect, O.view_compose) and
    tests/eye_ref.py's numpy restatement, bit for bit, on the three golden meshes and seeded random ones;
  * the validity rule;
  * tests/eye_ref.py's MultiEyeRef bookkeeping on a hand-written timeline with a stub estimator;
  * the argument refusals of zr_eye_select_async / zr_eye_crop_async / zr_eye_commit_async.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
import zaru_amd.host as H
from zaru_amd import _lib

import eye_ref as ER
import multi_tracker_ref as MR

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(*v):
    return np.array(v, f32).tobytes()


def _hrect(r):
    return _bits(*r.rect().tuple(), r.rotation_radians())


def _orect(r):
    return _bits(*r.rect.tuple(), r.rad)


def _rotated(lm, deg, centre):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    out = np.array(lm, np.float64)
    xy = out[:, :2] - centre
    out[:, 0] = c * xy[:, 0] - s * xy[:, 1] + centre[0]
    out[:, 1] = s * xy[:, 0] + c * xy[:, 1] + centre[1]
    return np.ascontiguousarray(out, f32)


def meshes():
    g = np.load(os.path.join(GOLDEN, "sad_linus_mesh.npz"))
    out = {"golden%d" % i: np.ascontiguousarray(g["landmarks"][i], f32) for i in range(3)}
    out["golden0_rot40"] = _rotated(out["golden0"], 40.0, (96.0, 96.0))
    out["golden1_rot-155"] = _rotated(out["golden1"], -155.0, (20.0, 130.0))
    rng = np.random.default_rng(3)
    out["random468"] = rng.uniform(-50, 700, (468, 3)).astype(f32)
    out["random478"] = rng.uniform(0, 2000, (478, 3)).astype(f32)
    out["tiny"] = (rng.uniform(0, 1e-3, (468, 3)) + 300.0).astype(f32)
    return out


MESHES = meshes()


@pytest.mark.parametrize("name", sorted(MESHES))
def test_rects_crops_and_views_are_the_oracles_bits(name):
    lm = MESHES[name]
    got = H.face_eye_rects(lm)
    want = ER.eye_rects(O, lm)
    for side, g, w in zip(("left", "right"), got, want):
        assert (g is None) == (w is None), (name, side)
        if w is None:
            continue
        assert _hrect(g) == _orect(w), (name, side, g.rect().tuple(), w.rect.tuple())
        for grow in (ER.GROW, 0.0, 1.25):
            crop = ER.crop_rect(O, w, grow)
            assert _hrect(H.eye_crop_rect(g, grow)) == _orect(crop), (name, side, grow)
            for W, Hh in ((192, 192), (480, 360), (1919, 1081)):
                view, _ = ER.network_view(O, crop, W, Hh)
                assert _bits(*H.eye_crop_view(g, W, Hh, grow).zr_view()) == _orect(view), (name, side, grow, W)
        assert _hrect(H.eye_crop_rect(g)) == _orect(ER.crop_rect(O, w)), "the default grow is 0.65"
    assert H.EYE_CROP_GROW == f32(0.65)


@pytest.mark.parametrize("i", range(3))
def test_left_is_left_of_right_on_the_golden_faces(i):
    """mediapipe.rs:586: left_eye().center().x < right_eye().center().x; and the crop is square, 2.3 x
    the rect's long side."""
    left, right = H.face_eye_rects(MESHES["golden%d" % i])
    assert left.rect().center[0] < right.rect().center[0]
    for r in (left, right):
        w, h = r.rect().size
        assert w > h > 0
        crop = H.eye_crop_rect(r)
        assert crop.rotation_radians() == r.rotation_radians() and crop.rect().center == r.rect().center
        cw, ch = crop.rect().size
        assert abs(cw / w - 2.3) < 1e-5 and abs(ch - cw) <= 4 * np.spacing(f32(cw))


def test_invalid_eyes():
    lm = MESHES["golden0"]
    for idx in ER.LEFT:
        for c in (0, 1):
            bad = lm.copy()
            bad[idx, c] = np.nan
            left, right = H.face_eye_rects(bad)
            # 33 is also the face's corner: both eyes need it
            assert left is None and (right is None) == (idx == 33), (idx, c)
    bad = lm.copy()
    bad[386, 1] = np.inf
    left, right = H.face_eye_rects(bad)
    assert left is not None and right is None
    bad = lm.copy()
    bad[145, 2] = np.nan  # z is not used
    assert all(r is not None for r in H.face_eye_rects(bad))
    bad = lm.copy()
    bad[[145, 133, 159]] = bad[33]  # four coincident points: width (and height) 0
    left, right = H.face_eye_rects(bad)
    assert left is None and right is not None
    assert ER.eye_rects(O, bad)[0] is None
    bad = np.zeros((468, 3), f32)  # everything coincides: the angle is atan2(0, 0) = 0, both rects empty
    assert H.face_eye_rects(bad) == (None, None)
    with pytest.raises(RuntimeError):
        H.face_eye_rects(lm[:386])
    with pytest.raises(RuntimeError):
        H.eye_crop_rect(H.face_eye_rects(lm)[0], -0.1)


def test_eye_landmarks():
    rng = np.random.default_rng(8)
    p = rng.uniform(0, 64, (76, 3)).astype(f32)
    e = H.EyeLandmarks(p)
    assert e.positions().tobytes() == p.tobytes()
    assert e.iris_center().tobytes() == p[0].tobytes()
    assert e.iris_contour().tobytes() == p[1:5].tobytes() and e.eye_contour().tobytes() == p[5:].tobytes()
    assert _bits(e.iris_diameter()) == _bits(ER.iris_diameter(p))
    e.flip_horizontal_in_place(64)
    assert e.positions().tobytes() == ER.flip(p, 64).tobytes()
    assert np.array_equal(e.positions()[:, 1:], p[:, 1:])
    # twice is the identity on dyadic values (every step is exact), for an odd width too
    d = (rng.integers(-4096, 4096, (76, 3)) / 16.0).astype(f32)
    for width in (64, 63):
        e = H.EyeLandmarks(d)
        e.flip_horizontal_in_place(width)
        assert not np.array_equal(e.positions(), d)
        e.flip_horizontal_in_place(width)
        assert e.positions().tobytes() == d.tobytes(), width
    # a known answer: the centre at the origin, the contour at distances 1, 2, 3, 4
    k = np.zeros((76, 3), f32)
    k[1, 0], k[2, 1], k[3, 2], k[4, 0] = 1.0, -2.0, 3.0, -4.0
    assert H.EyeLandmarks(k).iris_diameter() == 5.0


def test_map_out_is_flip_map_transform():
    """eye_map_out against the oracle's estimator_map / transform_out (f32, the same order) for both
    parities, on a rotated crop that is not square to the last bit."""
    rng = np.random.default_rng(9)
    raw = rng.uniform(-8, 72, (76, 3)).astype(f32)
    for name in ("golden0_rot40", "random468"):
        for side, rect in zip(("left", "right"), H.face_eye_rects(MESHES[name])):
            crop = H.eye_crop_rect(rect)
            ocrop = O.RRect(O.Rect(*crop.rect().tuple()), crop.rotation_radians())
            lrect = O.grow_to_fit_aspect(O.Rect.from_top_left(0, 0, ocrop.rect.w, ocrop.rect.h), 64, 64)
            for right in (False, True):
                got = H.eye_map_out(raw, right, crop)
                want = O.estimator_map(ER.flip(raw) if right else raw, lrect, 64)
                for j in range(76):
                    want[j, 0], want[j, 1] = O.transform_out(ocrop, want[j, 0], want[j, 1])
                assert got["landmarks"].tobytes() == want.tobytes(), (name, side, right)
                assert _bits(got["iris_diameter"]) == _bits(ER.iris_diameter(want))
                assert _hrect(got["crop"]) == _hrect(crop)


class _FakeTracker:
    """tests/test_multi_tracker_cpu.py's: estimates scripted by the frame, keyed by the RoI's centre x."""

    def __init__(self):
        self.roi = None

    def set_roi_padding(self, p):
        pass

    def set_loss_threshold(self, t):
        pass

    def set_roi(self, roi):
        self.roi = roi

    def track(self, frame):
        cx = self.roi.rect().center[0]
        if cx in frame.get("lose", ()):
            return None
        return {"updated_roi": self.roi, "landmarks": cx, "confidence": 1.0}


def test_oracle_bookkeeping_with_a_stub_estimator():
    """Eyes are made for the objects that have landmarks at the step, from that step's frame and the
    previous frame's landmarks; a lost object gets none; the count is of valid eyes."""
    D = H.Detection
    rect = lambda cx: H.Rect.from_center(cx, 100.0, 40.0, 40.0)
    frames = [{"name": 0, "dets": [D(0.9, rect(100.0), 0.0), D(0.9, rect(300.0), 0.0)]},
              {"name": 1}, {"name": 2, "lose": {100.0}}, {"name": 3}, {"name": 4}]
    calls = []

    def refine(frame, lm):
        calls.append((frame["name"], lm))
        # the object at 300 has no valid right eye
        return {"left": {"frame": frame["name"], "lm": lm}, "right": None if lm == 300.0 else {"frame": frame["name"]}}

    t = MR.MultiTrackerRef(H, "face", "facemesh", 3, make_tracker=_FakeTracker, detect=lambda f: f.get("dets", []))
    t.interval, t.loss = 1000.0, -1.0
    ref = ER.MultiEyeRef(t, refine)
    seen = []
    for k, f in enumerate(frames):
        ref.step(f, 15.0 * k, [D(0.9, rect(200.0), 0.0)] if k == 2 else ())
        seen.append([(o.id, None if e is None else (e["left"]["frame"], e["left"]["lm"], e["right"] is None))
                     for o, e in ref.objects()])
    assert seen == [
        [],                                           # step 0: detection runs on frame 0
        [],                                           # step 1: ids 0, 1 start; no result yet
        [(0, (2, 100.0, False)), (1, (2, 300.0, True))],   # their estimates on frame 1, refined on frame 2
        [(1, (3, 300.0, True)), (2, (3, 200.0, False))],   # 0 lost on frame 2: leaves; 2 (injected) has a result
        [(1, (4, 300.0, True)), (2, (4, 200.0, False))],
    ], seen
    assert calls == [(2, 100.0), (2, 300.0), (3, 300.0), (3, 200.0), (4, 300.0), (4, 200.0)], calls
    assert ref.images == 2 + 1 + 1 + 2 + 1 + 2 and ref.lost == 1


def test_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    p = 4096  # stands for a device pointer: none of these calls gets as far as using it
    cfg = _lib.EyeCfg(slots=4, num_landmarks=468, aspect_w=1, aspect_h=1, in_w=64, in_h=64, crop_grow=0.65)
    assert C.sizeof(_lib.EyeCfg) == 28

    def select(c, n=8, args=(p, p, p, p, p)):
        a = list(args)
        return lib.zr_eye_select_async(None if c is None else C.byref(c), a[0], n, a[1], a[2], a[3], a[4], None)

    def commit(c, n=8, s0=213, s1=15, args=(p, p, p, p, p, p, p)):
        a = list(args)
        return lib.zr_eye_commit_async(None if c is None else C.byref(c), n, a[0], a[1], a[2], s0, s1, a[3], a[4], a[5],
                                       a[6], None)

    for fn, nargs in ((select, 5), (commit, 7)):
        assert fn(None) == -1
        for i in range(nargs):
            a = [p] * nargs
            a[i] = None
            assert fn(cfg, args=a) == -1, (fn.__name__, i)
            assert b"null" in lib.zr_last_error()
        for n in (0, 2 ** 24 + 4, 6):  # 6: not a multiple of the 4 slots
            assert fn(cfg, n=n) == -1, (fn.__name__, n)
        for field, value in (("slots", 0), ("slots", 65), ("num_landmarks", 386), ("num_landmarks", 21),
                             ("aspect_w", 0), ("aspect_h", -1), ("in_w", 0), ("in_h", 0), ("crop_grow", -0.01),
                             ("crop_grow", float("nan"))):
            bad = _lib.EyeCfg.from_buffer_copy(cfg)
            setattr(bad, field, value)
            assert fn(bad) == -1, (fn.__name__, field, value)
    assert commit(cfg, s0=212) == -1 and commit(cfg, s1=14) == -1
    short = _lib.EyeCfg.from_buffer_copy(cfg)
    short.num_landmarks = 386
    assert select(short) == -1 and b"386" in lib.zr_last_error()

    frame = _lib.Frame(rgba=p, width=64, height=48, row_stride=256)

    def crop(frames=frame, n_frames=1, args=(p, p, p, p), entries=16, w=64, h=64):
        a = list(args)
        return lib.zr_eye_crop_async(None if frames is None else C.byref(frames), n_frames, a[0], a[1], entries, a[2],
                                     a[3], w, h, None)

    assert crop(frames=None) == -1 and crop(n_frames=0) == -1
    for i in range(4):
        a = [p] * 4
        a[i] = None
        assert crop(args=a) == -1, i
    assert crop(entries=0) == -1 and crop(entries=2 ** 25 + 1) == -1
    assert crop(w=0) == -1 and crop(h=0) == -1 and crop(w=4097) == -1
    assert crop(args=(p, p, p, p + 2)) == -1 and b"aligned" in lib.zr_last_error()
    for field, value in (("rgba", None), ("width", 0), ("height", 0)):
        bad = _lib.Frame.from_buffer_copy(frame)
        setattr(bad, field, value)
        assert crop(frames=bad) == -1, field
