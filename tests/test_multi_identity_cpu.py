"""Recognition inside DeviceMultiTracker, the parts that need no GPU:

  * zaru_amd.host.landmark_crop_view against a numpy-f32 restatement of Rect::bounding -> grow_rel ->
    grow_to_fit_aspect -> ViewData::view, bit for bit;
  * the schedule of tests/multi_identity_ref.py on a hand-written timeline, for the three kinds of
    interval;
  * the argument refusals of zr_identity_select_async / _compact_async / _commit_async.
"""
import ctypes as C
import math

import numpy as np
import pytest

import zaru_amd.host as H
from zaru_amd import _lib

import multi_identity_ref as IR

f32 = np.float32


def crop_ref(pts, W, Hh, aw, ah, grow):
    """The crop as (cx, cy, w, h, rad) in f32, one rounding per operation."""
    x, y = pts[:, 0].astype(f32), pts[:, 1].astype(f32)
    x0, y0, x1, y1 = x.min(), y.min(), x.max(), y.max()
    # Rect::bounding -> span -> from_top_left (rect.rs:49-68)
    w, h = f32(x1 - x0), f32(y1 - y0)
    cx, cy = f32(x0 + f32(w * f32(0.5))), f32(y0 + f32(h * f32(0.5)))
    # grow_rel (rect.rs:84-93)
    g = f32(grow)
    l, t = f32(w * g), f32(h * g)
    w, h = f32(f32(w + l) + l), f32(f32(h + t) + t)
    # grow_to_fit_aspect (rect.rs:104-117)
    a = f32(f32(aw) / f32(ah))
    tw = f32(h * a)
    if tw >= w:
        w = f32(w + f32(tw - w))
    else:
        h = f32(h + f32(f32(w / a) - h))
    # ViewData::full(W, H).view(RotatedRect(crop, 0)) (image/mod.rs:201-210): the centre through the
    # full view's transform_out (a rotation by 0 around its middle), then move_to(top left)
    hw, hh = f32(f32(W) * f32(0.5)), f32(f32(Hh) * f32(0.5))
    px = f32(f32(f32(cx - hw) + hw) + f32(hw - f32(f32(W) * f32(0.5))))
    py = f32(f32(f32(cy - hh) + hh) + f32(hh - f32(f32(Hh) * f32(0.5))))
    tlx, tly = f32(px - f32(w * f32(0.5))), f32(py - f32(h * f32(0.5)))
    return np.array([f32(tlx + f32(w * f32(0.5))), f32(tly + f32(h * f32(0.5))), w, h, 0.0], f32)


def _point_sets():
    rng = np.random.default_rng(5)
    sets = {
        "wide": np.c_[rng.uniform(40, 400, 468), rng.uniform(100, 140, 468), rng.uniform(-5, 5, 468)],
        "tall": np.c_[rng.uniform(200, 230, 21), rng.uniform(-30, 500, 21), rng.uniform(-5, 5, 21)],
        "single": np.array([[123.25, 77.5, 0.0]]),
        "equal": np.tile(np.array([[300.0, 200.0, 1.0]]), (65, 1)),
        "outside": np.c_[rng.uniform(-200, 900, 478), rng.uniform(-100, 700, 478), np.zeros(478)],
        "tiny": np.c_[rng.uniform(10, 10.001, 64), rng.uniform(20, 20.001, 64), np.zeros(64)],
    }
    return {k: np.ascontiguousarray(v, f32) for k, v in sets.items()}


@pytest.mark.parametrize("aspect", [(1, 1), (4, 3), (9, 16)])
@pytest.mark.parametrize("grow", [0.4, 0.0, 1.5])
def test_landmark_crop_view_bits(aspect, grow):
    for name, pts in _point_sets().items():
        for W, Hh in ((480, 360), (1919, 1081)):
            got = np.array(H.landmark_crop_view(pts, W, Hh, aspect[0], aspect[1], grow).zr_view(), f32)
            want = crop_ref(pts, W, Hh, aspect[0], aspect[1], grow)
            assert got.tobytes() == want.tobytes(), (name, W, Hh, got, want)
            # x, y pairs without z give the same crop
            xy = np.ascontiguousarray(pts[:, :2])
            assert np.array(H.landmark_crop_view(xy, W, Hh, *aspect, grow).zr_view(), f32).tobytes() == want.tobytes()


def test_landmark_crop_view_is_the_embedders_crop_of_the_bounding_rect():
    """With the default grow it is FaceEmbedder::crop_view's arithmetic: rect.grow_rel(0.4) fitted to
    the aspect, as a view of the whole image."""
    pts = _point_sets()["wide"]
    rect = H.Rect.bounding([(float(p[0]), float(p[1])) for p in pts])
    want = H.ViewData.full(640, 480).view_rect(rect.grow_rel(0.4).grow_to_fit_aspect(112, 112)).zr_view()
    assert H.landmark_crop_view(pts, 640, 480, 112, 112).zr_view() == want
    assert H.landmark_crop_view(pts, 640, 480, 1, 1, 0.4).zr_view() == want


def test_landmark_crop_view_refusals():
    pts = _point_sets()["single"]
    for bad in (lambda: H.landmark_crop_view(np.zeros((0, 3), f32), 10, 10, 1, 1),
                lambda: H.landmark_crop_view(np.zeros((4, 1), f32), 10, 10, 1, 1),
                lambda: H.landmark_crop_view(np.zeros(6, f32), 10, 10, 1, 1),
                lambda: H.landmark_crop_view(pts, 10, 10, 0, 1),
                lambda: H.landmark_crop_view(pts, 10, 10, 1, 0)):
        with pytest.raises(RuntimeError):
            bad()


# ---- the schedule ----------------------------------------------------------------------------
class _Obj:
    def __init__(self, oid):
        self.id = oid
        self.pending = None
        self.lm = None


class _Timeline:
    """Stands for MultiTrackerRef: objects appear at scripted steps; each has landmarks from the
    step after it started."""

    def __init__(self, starts):
        self.starts, self.objs, self.k = starts, [], 0

    def step(self, frame, now_ms, injected=()):
        for o in self.objs:
            o.lm = o.pending
        for oid in self.starts.get(self.k, []):
            self.objs.append(_Obj(oid))
        for o in self.objs:  # every object's estimate on this frame, consumed by the next step
            o.pending = {"landmarks": [(1.0 + o.id, 2.0, 0.0), (3.0 + o.id, 5.0, 0.0)]}
        self.k += 1

    def objects(self):
        return [o for o in self.objs if o.lm is not None]


def _due_steps(interval, steps=9, nan_at=None):
    tl = _Timeline({0: [0], 2: [1]})
    calls = []
    ref = IR.MultiIdentityRef(H, tl, lambda frame, rect: calls.append((frame, rect.tuple())) or [0.0] * 128,
                              lambda e: (IR.NO_MATCH, math.inf), interval=interval)
    due = []
    for k in range(steps):
        if nan_at == k:
            for o in tl.objs:
                if o.pending:
                    o.pending["landmarks"][-1] = (math.nan, 5.0, 0.0)
        ref.step(k, 15.0 * k)
        due.append(list(ref.last_due))
    assert ref.images == sum(len(d) for d in due) == len(calls)
    return due, ref


def test_schedule_on_a_timeline():
    """Clock 15 ms per step; object 0 starts at step 0 (first landmarks at step 1), object 1 at step 2
    (first at step 3)."""
    every, _ = _due_steps(0.0)
    assert every == [[], [0], [0], [0, 1], [0, 1], [0, 1], [0, 1], [0, 1], [0, 1]]
    # 40 ms: embedded at 15 -> next 55 -> due at 60 (step 4), not at 45 (step 3); then 100 -> 105 (7)
    forty, ref = _due_steps(40.0)
    assert forty == [[], [0], [], [1], [0], [], [1], [0], []]
    assert [i["embeddings"] for _, i in ref.objects()] == [3, 2]
    once, ref = _due_steps(math.inf)
    assert once == [[], [0], [], [1], [], [], [], [], []]
    assert [i["embeddings"] for _, i in ref.objects()] == [1, 1]
    # an object whose landmarks are not finite is not embedded, and is due again once they are
    nan, _ = _due_steps(math.inf, nan_at=1)
    assert nan == [[], [], [0], [1], [], [], [], [], []]
    # the crop's rect is the landmarks' bounding rect
    assert H.Rect.bounding([(1.0, 2.0), (3.0, 5.0)]).tuple() == (2.0, 3.5, 2.0, 3.0)


def test_known_threshold():
    assert IR.known(7, f32(0.5), 0.5) == 7                 # <= is known
    assert IR.known(7, f32(0.5), float(np.nextafter(f32(0.5), f32(0)))) == IR.NO_MATCH
    assert IR.known(7, f32(0.5), math.inf) == 7
    assert IR.known(7, f32(0.5), math.nan) == IR.NO_MATCH and IR.known(7, math.nan, math.inf) == IR.NO_MATCH
    assert IR.known(IR.NO_MATCH, math.inf, math.inf) == IR.NO_MATCH   # an empty gallery
    assert IR.NO_MATCH == H.NO_MATCH


# ---- refusals ----------------------------------------------------------------------------------
def _icfg(**kw):
    v = dict(slots=4, num_landmarks=468, aspect_w=1, aspect_h=1, crop_grow=0.4, threshold=math.inf, interval_ms=1000.0)
    v.update(kw)
    return _lib.IdentityCfg(**v)


def test_identity_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    assert C.sizeof(_lib.IdentityState) == 24 and _lib.IdentityState.next_ms.offset == 16
    p, q = 4096, 8192  # stand for device pointers: none of these calls gets as far as using them
    names = ("state", "lm", "src", "sin", "ein", "sout", "eout", "due", "views")

    def select(c=_icfg(), n=8, now=0.0, **kw):
        a = dict(state=p, lm=p, src=p, sin=p, ein=p, sout=q, eout=q, due=p, views=p)
        a.update(kw)
        return lib.zr_identity_select_async(None if c is None else C.byref(c), a["state"], n, a["lm"], a["src"], now,
                                            a["sin"], a["ein"], a["sout"], a["eout"], a["due"], a["views"], None)

    assert select(c=None) == -1
    for name in names:
        assert select(**{name: None}) == -1, name
    assert select(n=0) == -1 and select(n=(1 << 24) + 4) == -1
    for n, slots in ((8, 0), (8, 65), (8, -1), (8, 3), (9, 4), (130, 64)):
        assert select(c=_icfg(slots=slots), n=n) == -1, (n, slots)
    for field, value in (("num_landmarks", 0), ("aspect_w", 0), ("aspect_h", -1), ("crop_grow", -0.1),
                         ("crop_grow", math.nan), ("interval_ms", -1.0), ("interval_ms", math.nan)):
        assert select(c=_icfg(**{field: value})) == -1, (field, value)
    assert select(now=math.nan) == -1
    assert select(sin=p, sout=p) == -1 and select(ein=p, eout=p) == -1   # in == out
    assert select(ein=p + 4) == -1 and select(eout=q + 4) == -1          # float2 accesses

    def compact(n=8, **kw):
        a = dict(due=p, views=p, dviews=q, of=p, ndue=p, valid=p, total=p)
        a.update(kw)
        return lib.zr_identity_compact_async(a["due"], a["views"], n, a["dviews"], a["of"], a["ndue"], a["valid"],
                                             a["total"], None)

    for name in ("due", "views", "dviews", "of", "ndue", "valid"):
        assert compact(**{name: None}) == -1, name
    assert compact(n=0) == -1 and compact(n=(1 << 24) + 1) == -1

    def commit(c=_icfg(), n=8, now=0.0, **kw):
        a = dict(of=p, idx=p, dist=p, dense=p, sout=q, eout=q)
        a.update(kw)
        return lib.zr_identity_commit_async(None if c is None else C.byref(c), n, a["of"], a["idx"], a["dist"],
                                            a["dense"], now, a["sout"], a["eout"], None)

    assert commit(c=None) == -1 and commit(n=0) == -1 and commit(now=math.nan) == -1
    for name in ("of", "idx", "dist", "dense", "sout", "eout"):
        assert commit(**{name: None}) == -1, name
    for n, slots in ((8, 0), (8, 65), (9, 4)):
        assert commit(c=_icfg(slots=slots), n=n) == -1, (n, slots)
    assert commit(c=_icfg(interval_ms=-5.0)) == -1 and commit(dense=p + 4) == -1
    # thresholds and an infinite interval are settings, not errors: checked on the GPU, where they run
