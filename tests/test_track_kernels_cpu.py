"""CPU-side checks of tests/track_kernels_ref.py, the restatements tests/test_gpu_track_kernels.py
holds the bookkeeping kernels to: on the GPU tests' own scenario table they equal the pieces the
suite already pins (HandTracker.filter_detections / dedupe_rois, tests/multi_tracker_ref.py), the
table covers every branch it is meant to, host and oracle agree on a NaN IoU in NMS, and the
kernels' entry points refuse bad arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import zaru_amd.host as H
from zaru_amd import _lib

import multi_tracker_ref as MR
import track_kernels_ref as R

f32 = np.float32
CONFIGS = {"faces": dict(K=5, dcap=6, iou=0.3, grow=0.0, use_angle=0, interval=40.0, aw=1, ah=1),
           "hands": dict(K=5, dcap=6, iou=0.3, grow=1.5, use_angle=1, interval=40.0, aw=1, ah=1)}
NOW = 1000.0


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def steps(request):
    """Both steps of the GPU test, by the restatement: [(inputs, now, init_clock, outputs, trace)]."""
    cfg = CONFIGS[request.param]
    a1 = R.scenarios(cfg)
    o1, t1 = R.manage(a1, cfg, NOW, 1)
    a2, now2 = R.second_step(o1, cfg)
    o2, t2 = R.manage(a2, cfg, now2, 0)
    return cfg, [(a1, NOW, 1, o1, t1), (a2, now2, 0, o2, t2)]


def _hrect(v):
    return H.Rect.from_center(float(v[0]), float(v[1]), float(v[2]), float(v[3]))


def test_scenario_table_covers_every_branch(steps):
    cfg, ((a1, _, _, o1, t1), (a2, _, _, o2, t2)) = steps
    first, second = R.coverage(t1), R.coverage(t2)
    for b in R.BRANCHES:
        if b in ("nhands_over", "nhands_under"):
            assert first[b] == 1, (b, first)          # the two clamp streams
        elif b == "not_due":
            assert first[b] == 0 and second[b] >= 3   # init_clock = 1 makes every stream due
        else:
            assert first[b] >= 3, (b, first)
    for b in ("compact", "untracked", "count_clamped", "count_negative", "newcomer", "dropped", "sweep_last",
              "sweep_move", "due", "not_due"):
        assert second[b] >= 3, (b, second)
    # a clock exactly at `now` is due
    assert sum(1 for s in range(len(t2)) if a2["next_det"][s] == steps[1][1][1] and o2["det_pending"][s]) >= 3
    # the clamp streams sit in the middle of the table and behave as K and 0 hands
    S, K = len(t1), cfg["K"]
    for s in (R.NHANDS_OVER_AT, R.NHANDS_UNDER_AT):
        assert 1 < s < S - 2
    assert (a1["nhands"][R.NHANDS_OVER_AT], a1["nhands"][R.NHANDS_UNDER_AT]) == (K + 3, -2)
    assert (o1["nhands"][R.NHANDS_OVER_AT], o1["nhands"][R.NHANDS_UNDER_AT]) == (K, 0)
    # the NaN rows: an object is started (the reference discards on >= only) and the sweep keeps it
    for s, t in enumerate(t1):
        if t["tags"] & {"nan_zero", "nan_inf"}:
            assert "nan_sweep" in t["tags"] and o1["nhands"][s] > len(t["rois"]), s
            assert np.isnan(H.Rect.iou(_hrect(t["rois"][-1]), _hrect(t["dets"][0][2:6]).grow_rel(cfg["grow"])))
    assert S == 150 and S > 2 * 64 and S % 64 != 0


def test_manage_filter_and_sweep_equal_the_host_pieces(steps):
    cfg, both = steps
    thr = float(f32(cfg["iou"]))
    for a, now, init, o, trace in both:
        for s, t in enumerate(trace):
            rects = [_hrect(r) for r in t["pre_sweep"]]
            assert H.HandTracker.dedupe_rois(rects, thr) == t["survivors"], s
            if cfg["grow"] == 1.5:   # filter_detections grows by the palm's 1.5
                dets = [H.Detection(float(d[0]), _hrect(d[2:6]), float(d[1])) for d in t["dets"]]
                assert H.HandTracker.filter_detections([_hrect(r) for r in t["rois"]], dets, thr) == t["keep"], s


class _FakeTracker:
    def set_roi_padding(self, p):
        pass

    def set_roi(self, roi):
        pass

    def track(self, frame):
        return None


def _rrect(v):
    return H.RotatedRect(_hrect(v), float(v[4]))


def test_manage_equals_multi_tracker_ref(steps):
    cfg, both = steps
    K, dcap = cfg["K"], cfg["dcap"]
    for a, now, init, o, _ in both:
        for s in range(len(a["nhands"])):
            ref = MR.MultiTrackerRef(H, "face", "facemesh", K, make_tracker=_FakeTracker, detect=lambda f: [])
            ref.det_grow, ref.use_angle, ref.interval = cfg["grow"], bool(cfg["use_angle"]), cfg["interval"]
            ref.iou = float(f32(cfg["iou"]))
            ref.next_id, ref.next_det = int(a["next_id"][s]), None if init else float(a["next_det"][s])
            for h in range(min(max(int(a["nhands"][s]), 0), K)):
                st, i = a["state"][s * K + h], s * K + h
                obj = MR._Object(int(a["ids"][i]), _rrect(a["hroi"][i]), _FakeTracker())
                if st["active"]:
                    obj.pending = {"updated_roi": _rrect(st["updated"] if st["tracked"] else a["hroi"][i])}
                ref.objs.append(obj)
            if a["det_pending"][s]:
                ref.det_result = [H.Detection(float(d[0]), _hrect(d[2:6]), float(d[1]))
                                  for d in a["dets"][s, :max(min(int(a["count"][s]), dcap), 0)]]
            ref.step({}, now)
            n = int(o["nhands"][s])
            assert ref.ids() == [int(v) for v in o["ids"][s * K:s * K + n]], s
            got = np.array([[*x.roi.rect().tuple(), x.roi.rotation_radians()] for x in ref.objs], f32).reshape(n, 5)
            assert R.same_f32(got, o["hroi"][s * K:s * K + n]), s
            assert (ref.pending, ref.dropped, ref.next_id, ref.next_det) == \
                (bool(o["det_pending"][s]), int(o["dropped"][s]), int(o["next_id"][s]), float(o["next_det"][s])), s


def test_next_view_equals_the_host_views():
    """next_view against the host's own chain (Rect.grow_to_fit_aspect, ViewData.view twice)."""
    rng = np.random.default_rng(3)
    for k in range(40):
        roi = np.array([*rng.uniform(-50, 700, 2), *rng.uniform(0, 300, 2), rng.uniform(-3.2, 3.2)], f32)
        if k % 10 == 0:
            roi[2:4] = 0.0
        fw, fh, (aw, ah) = 640 + k, 480 - k, ((1, 1), (4, 3), (3, 5))[k % 3]
        vr = H.RotatedRect(_hrect(roi).grow_to_fit_aspect(aw, ah), float(roi[4]))
        view = H.ViewData.full(fw, fh).view(vr)
        local = H.Rect.from_top_left(0.0, 0.0, *view.rect.rect().size).grow_to_fit_aspect(aw, ah)
        view_rect, loc, desc = R.next_view(roi, fw, fh, aw, ah, k)
        assert R.same_f32(view_rect, np.array([*vr.rect().tuple(), vr.rotation_radians()], f32))
        assert R.same_f32(loc, np.array([*local.top_left(), local.width()], f32))
        assert R.same_views(desc, R.describe(view.view_rect(local).zr_view(), k))


def test_total_key_orders_as_total_cmp():
    vals = np.array([-np.nan, -np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan], f32)
    vals[0] = np.array(0xFFC00000, np.uint32).view(f32)
    vals[-1] = np.array(0x7FC00000, np.uint32).view(f32)
    keys = [R.total_key(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("remove", [True, False])
def test_nms_nan_iou_host_equals_oracle(remove):
    """Host and oracle agree, bit for bit, on the frame of tests/test_gpu_detpost_nan_iou.py:
    Remove mode drops a candidate whose IoU with the seed is NaN, Average leaves it ungrouped."""
    boxes, logits, (w, h) = R.nms_nan_frame(H.anchors("face"))
    host = R.det_rows(H.detect_post("face", boxes, logits, w, h, remove=remove), True)
    orc = R.det_rows(O.detect_post(O.FACE, boxes, logits, w, h, 128, 128, remove=remove), False)
    assert len(host) == (4 if remove else 6)
    assert np.array_equal(host.view(np.uint32), orc.view(np.uint32))
    # the seven confidences are distinct, and the zero-size boxes give a NaN IoU with each other
    conf = np.sort(host[:, 0])
    assert (np.diff(conf) > 0).all()
    assert np.isnan(O.iou(O.Rect(5.0, 5.0, 0.0, 0.0), O.Rect(5.0, 5.0, 0.0, 0.0)))
    assert np.isnan(O.iou(O.Rect(5.0, 5.0, 0.0, 0.0), O.Rect(9.0, 1.0, 0.0, 0.0)))


def test_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    p = 4096  # stands for a device pointer: none of these calls gets as far as using it

    def refused(fn, good, nullable=(), ranges=()):
        for i, v in enumerate(good):
            if v == p and i not in nullable:
                a = list(good)
                a[i] = None
                assert fn(*a) == -1, (fn.__name__, i)
        for i, v in ranges:
            a = list(good)
            a[i] = v
            assert fn(*a) == -1, (fn.__name__, i, v)

    # zr_due_compact_async(pending, n, template, due, ndue, due_views, total, stream) and its twin
    tmpl = (C.c_uint32 * 10)()
    for fn in (lib.zr_due_compact_async, lib.zr_track_lost_compact_async):
        refused(fn, [p, 8, C.addressof(tmpl), p, p, p, p, None], nullable=(6,),
                ranges=[(1, 0), (1, 2 ** 24 + 1), (2, None)])
    # zr_track_reseed_best_async(count, dets, dcap, fsize, n, cfg, state, views, reseeded, stream)
    tc = _lib.TrackCfg(kind=0, num_landmarks=468, in_w=192, in_h=192, aspect_w=1, aspect_h=1, loss_thresh=0.5,
                       padding=0.3, rois_per_frame=4)
    bad_w, bad_h, bad_r = (_lib.TrackCfg.from_buffer_copy(tc) for _ in range(3))
    bad_w.aspect_w, bad_h.aspect_h, bad_r.rois_per_frame = 0, -2, 65
    refused(lib.zr_track_reseed_best_async, [p, p, 8, p, 4, C.addressof(tc), p, p, p, None], nullable=(8,),
            ranges=[(2, 0), (2, 65537), (4, 2 ** 24 + 1), (5, None), (5, C.addressof(bad_w)), (5, C.addressof(bad_h))])
    # zr_track_seed_detections_async(count, dets, dcap, forced, nforced, fsize, n, cfg, grow, use_angle, state,
    #                                seed_copy, views, stream): forced and nforced come together or not at all
    good = [p, p, 8, p, p, p, 4, C.addressof(tc), 0.0, 0, p, p, p, None]
    refused(lib.zr_track_seed_detections_async, good, nullable=(11,),
            ranges=[(2, 0), (6, 2 ** 23), (7, None), (7, C.addressof(bad_w)), (7, C.addressof(bad_h)),
                    (7, C.addressof(bad_r)), (8, -0.5), (8, float("nan"))])
    # zr_detect_post_mapped_async(logits, boxes, anchors, letterbox, n, map, nframes, cfg, count, dets, dcap, ties, stream)
    class DetCfg(C.Structure):
        _fields_ = [("face", C.c_int), ("anchors", C.c_int), ("params", C.c_int), ("keypoints", C.c_int),
                    ("in_w", C.c_int), ("in_h", C.c_int), ("thresh", C.c_float), ("iou", C.c_float), ("mode", C.c_int)]
    dc = DetCfg(1, 896, 16, 6, 128, 128, 0.5, 0.3, 0)
    bads = []
    for field, value in (("anchors", 0), ("keypoints", 2), ("keypoints", 8), ("params", 15), ("in_w", 0), ("in_h", -1),
                         ("mode", 2), ("mode", -1), ("anchors", 2 ** 16)):
        b = DetCfg.from_buffer_copy(dc)
        setattr(b, field, value)
        bads.append(b)
    refused(lib.zr_detect_post_mapped_async, [p, p, p, p, 4, p, p, C.addressof(dc), p, p, 8, p, None], nullable=(11,),
            ranges=[(4, 2 ** 24 + 1), (7, None), (10, 65537)] + [(7, C.addressof(b)) for b in bads])
    # zr_hand_manage_async and the pointers of zr_multi_manage_async(state, ids, roi, src, n, next_id, next_det,
    # det_pending, count, dets, dcap, fsize, n, cfg, now, init_clock, views, dropped, stream)
    class HandCfg(C.Structure):
        _fields_ = [("slots", C.c_int), ("iou_thresh", C.c_float), ("palm_grow", C.c_float),
                    ("interval_ms", C.c_double), ("aspect_w", C.c_int), ("aspect_h", C.c_int)]
    hc = HandCfg(4, 0.3, 1.5, 300.0, 1, 1)
    mc = _lib.MultiCfg(slots=4, iou_thresh=0.3, det_grow=0.0, use_angle=0, interval_ms=300.0, aspect_w=1, aspect_h=1)
    hbad = []
    for field, value in (("slots", 0), ("slots", 65), ("palm_grow", -0.5), ("palm_grow", float("nan")),
                         ("interval_ms", -1.0), ("interval_ms", float("nan")), ("aspect_w", 0), ("aspect_h", -1)):
        b = HandCfg.from_buffer_copy(hc)
        setattr(b, field, value)
        hbad.append(b)
    good = [p, p, p, p, p, p, p, p, p, p, 8, p, 2, C.addressof(hc), 0.0, 1, p, p, None]
    refused(lib.zr_hand_manage_async, good, nullable=(17,),
            ranges=[(10, 0), (10, 65537), (12, 2 ** 23), (13, None)] + [(13, C.addressof(b)) for b in hbad])
    good[13] = C.addressof(mc)
    refused(lib.zr_multi_manage_async, good, nullable=(17,), ranges=[(10, 65537)])
    assert C.sizeof(HandCfg) == 32 and C.sizeof(DetCfg) == 36 and R.STATE.itemsize == 92
