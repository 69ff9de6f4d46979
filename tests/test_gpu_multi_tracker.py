"""The device multi-object tracker (zaru_amd.host.DeviceMultiTracker: K objects per stream with
ids, for any detector / landmark network pair) and its three entry points -- zr_multi_manage_async,
zr_slot_compact_async, zr_track_update_indexed_async -- against

  * tests/multi_tracker_ref.py, the Python restatement of crates/zaru/src/hand/tracking.rs:115-219
    over one host LandmarkTracker per object (bit for bit: ids, RoIs, landmarks, confidence);
  * itself with the compaction of the live slots switched off (no bit may change);
  * DeviceHandTracker, whose loop the ("palm", "hand") instance must reproduce;
  * numpy restatements of the two new kernels' contracts.
"""
import ctypes as C
import os

import numpy as np
import pytest

import multi_tracker_ref as MR

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FW, FH = 480, 360


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


def _noise(n, seed, h=FH, w=FW):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8) for _ in range(n)]


def _det(H, d):
    conf, (cx, cy, w, h), angle = d
    return H.Detection(conf, H.Rect.from_center(cx, cy, w, h), angle)


def _record(objs, count, pending):
    """One stream's step as comparable values: the floats as their bits."""
    return (int(count), bool(pending),
            [(int(o["id"]), np.asarray(o["rect"], np.float32).tobytes(), np.float32(o["angle"]).tobytes(),
              np.ascontiguousarray(o["landmarks"], np.float32).tobytes(), np.float32(o["confidence"]).tobytes())
             for o in objs])


def _ref_objects(ref):
    return [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
             "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in ref.objects()]


def _dev_objects(dev, s):
    return [{"id": o["id"], "rect": o["view_rect"].rect().tuple(), "angle": o["view_rect"].rotation_radians(),
             "landmarks": o["landmarks"], "confidence": o["confidence"]} for o in dev.objects(s)]


# ---- the face script: 3 streams x 4 slots, 7 steps of noise frames -------------------------------
S, K, STEPS = 3, 4, 7
# per step, per stream: (confidence, (cx, cy, w, h), angle) handed to both sides; face detections
# start a tracker on the rect itself (no grow), so they are face-sized
FACE_SCRIPT = {
    0: {0: [(0.9, (200.0, 180.0, 80.0, 88.0), 0.3)],
        1: [(0.9, (100.0, 100.0, 60.0, 60.0), 0.0), (0.8, (104.0, 101.0, 60.0, 60.0), 0.1)],  # a pair: the sweep
        2: [(0.9, (300.0, 200.0, 100.0, 80.0), -0.2), (0.7, (120.0, 260.0, 72.0, 72.0), 0.5)]},
    2: {1: [(0.6, (330.0, 250.0, 88.0, 88.0), 1.0)]},        # a late newcomer
    4: {2: [(0.9, (300.0, 60.0, 60.0, 60.0), 0.0)]},
}
# (step, stream): a detection placed exactly on the RoI that stream's first object holds when the
# step's filter runs (known to the oracle one step ahead), followed by a newcomer
ON_TOP = {(2, 0): (0.9, (420.0, 60.0, 50.0, 50.0), 0.0), (4, 2): None}


@pytest.fixture(scope="module")
def face_frames():
    return [_noise(STEPS, 10 + s) for s in range(S)]


@pytest.fixture(scope="module")
def face_oracle(H, face_frames):
    """The oracle's run of the face script, once: per step and stream its record, and the
    injections as they were made (the on-top ones depend on the oracle's state)."""
    refs = []
    for s in range(S):
        r = MR.MultiTrackerRef(H, "face", "facemesh", K)
        r.loss = -1.0
        r.interval = 40.0
        refs.append(r)
    records, injected = [], []
    for k in range(STEPS):
        row, inj = [], {}
        for s in range(S):
            dets = list(FACE_SCRIPT.get(k, {}).get(s, []))
            if (k, s) in ON_TOP:
                first = refs[s].objs[0]
                assert first.pending is not None  # loss threshold -1: never lost
                roi = first.pending["updated_roi"]
                dets.insert(0, (0.9, tuple(roi.rect().tuple()), 0.0))
                if ON_TOP[(k, s)] is not None:
                    dets.append(ON_TOP[(k, s)])
            inj[s] = dets
            refs[s].step(face_frames[s][k], 15.0 * k, [_det(H, d) for d in dets])
            row.append(_record(_ref_objects(refs[s]), len(refs[s].objs), refs[s].pending))
        records.append(row)
        injected.append(inj)
    return {"records": records, "injected": injected, "filtered": sum(r.filtered for r in refs),
            "swept": sum(r.swept for r in refs), "detector_frames": sum(r.detector_frames for r in refs)}


def _run_face_device(H, face_frames, injected, compact):
    from zaru_amd._lib import DeviceBuffer
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    dev.set_compact(compact)
    bufs = [DeviceBuffer.from_array(np.stack([face_frames[s][k] for s in range(S)])) for k in range(STEPS)]
    fb = FH * FW * 4
    records, total = [], 0
    for k in range(STEPS):
        for s in range(S):
            if injected[k][s]:
                dev.inject_detections(s, [_det(H, d) for d in injected[k][s]])
        dev.step([(bufs[k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)], 15.0 * k)
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        total += sum(counts)
        records.append([_record(_dev_objects(dev, s), counts[s], pend[s]) for s in range(S)])
    return {"records": records, "object_steps": total, "landmark_images": dev.landmark_images(),
            "detector_frames": dev.detector_frames(), "dropped": dev.dropped_objects()}


@pytest.fixture(scope="module")
def face_device_on(H, face_frames, face_oracle):
    return _run_face_device(H, face_frames, face_oracle["injected"], True)


def test_scripted_parity_faces(face_oracle, face_device_on):
    """Every step, every stream: object_counts, detection_pending, ids, view_rect (rect and angle),
    landmarks and confidence equal the oracle's, bit for bit."""
    compared = 0
    for k in range(STEPS):
        for s in range(S):
            want, got = face_oracle["records"][k][s], face_device_on["records"][k][s]
            assert got[0] == want[0], ("count", k, s, got[0], want[0])
            assert got[1] == want[1], ("pending", k, s)
            assert [o[0] for o in got[2]] == [o[0] for o in want[2]], ("ids", k, s)
            for g, w in zip(got[2], want[2]):
                assert g[1] == w[1], ("rect", k, s, g[0])
                assert g[2] == w[2], ("angle", k, s, g[0])
                assert g[3] == w[3], ("landmarks", k, s, g[0])
                assert g[4] == w[4], ("confidence", k, s, g[0])
                compared += 1
    print("object-steps compared:", compared, "filtered:", face_oracle["filtered"], "swept:", face_oracle["swept"])
    assert compared >= 10, compared
    assert face_oracle["filtered"] >= 1 and face_oracle["swept"] >= 1, face_oracle
    assert face_device_on["detector_frames"] == face_oracle["detector_frames"]


def test_compaction_changes_no_bit(H, face_frames, face_oracle, face_device_on):
    off = _run_face_device(H, face_frames, face_oracle["injected"], False)
    assert off["records"] == face_device_on["records"]
    # on: the network ran on exactly the live objects; off: on every slot of every stream
    assert face_device_on["landmark_images"] == face_device_on["object_steps"]
    assert face_device_on["landmark_images"] < STEPS * S * K
    assert off["landmark_images"] == STEPS * S * K


def test_hand_instance_equals_device_hand_tracker(H):
    """DeviceMultiTracker("palm", "hand") with its palm defaults on the script of
    tests/test_gpu_device_hand_tracker.py: the same ids, RoIs and landmarks as DeviceHandTracker."""
    from zaru_amd._lib import DeviceBuffer
    frames = [_noise(STEPS, 10 + s) for s in range(S)]
    D = lambda c, r, a: (c, r, a)
    inject = {
        0: {0: [D(0.9, (200.0, 180.0, 40.0, 44.0), 0.3)],
            1: [D(0.9, (100.0, 100.0, 30.0, 30.0), 0.0), D(0.8, (104.0, 101.0, 30.0, 30.0), 0.1)],
            2: [D(0.9, (300.0, 200.0, 50.0, 40.0), -0.2), D(0.7, (120.0, 260.0, 36.0, 36.0), 0.5)]},
        2: {0: [D(0.9, (203.0, 182.0, 40.0, 44.0), 0.3), D(0.9, (380.0, 90.0, 30.0, 30.0), 0.0)],
            1: [D(0.6, (330.0, 250.0, 44.0, 44.0), 1.0)]},
        4: {2: [D(0.9, (128.0, 262.0, 36.0, 36.0), 0.5), D(0.9, (300.0, 60.0, 30.0, 30.0), 0.0)]},
    }
    hand = H.DeviceHandTracker(S, 4)
    multi = H.DeviceMultiTracker("palm", "hand", S, 4)
    for t in (hand, multi):
        t.set_loss_threshold(-1.0)
        t.set_redetect_interval(40.0)
    bufs = [DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)])) for k in range(STEPS)]
    fb = FH * FW * 4
    compared = 0
    for k in range(STEPS):
        for s in range(S):
            dets = [_det(H, d) for d in inject.get(k, {}).get(s, [])]
            if dets:
                hand.inject_detections(s, dets)
                multi.inject_detections(s, dets)
        fr = [(bufs[k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)]
        hand.step(fr, 15.0 * k)
        multi.step(fr, 15.0 * k)
        hand.synchronize()
        multi.synchronize()
        assert multi.object_counts() == hand.hand_counts(), k
        assert multi.detection_pending() == hand.detection_pending(), k
        for s in range(S):
            want, got = hand.hands(s), multi.objects(s)
            assert [o["id"] for o in got] == [h["id"] for h in want], (k, s)
            for g, w in zip(got, want):
                assert g["view_rect"].rect() == w["view_rect"].rect(), (k, s, g["id"])
                assert (np.float32(g["view_rect"].rotation_radians()).tobytes() ==
                        np.float32(w["view_rect"].rotation_radians()).tobytes()), (k, s, g["id"])
                assert g["landmarks"].tobytes() == w["landmarks"].tobytes(), (k, s, g["id"])
                compared += 1
    assert compared >= 10, compared
    assert multi.detector_frames() == hand.palm_frames()


# ---- real detections: two faces in one frame, and a noise-only stream ----------------------------
RW, RH, RT, BLANK_FROM = 960, 480, 8, 4


def _patch():
    codes = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))["codes"][0]
    p = np.full((192, 192, 4), 255, np.uint8)
    p[..., :3] = codes.transpose(1, 2, 0)
    return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)  # 384 x 384


def _two_face_video():
    rng = np.random.default_rng(3)
    patch = _patch()
    frames = np.empty((RT, 2, RH, RW, 4), np.uint8)
    bg = rng.integers(0, 256, size=(2, RH, RW, 4), dtype=np.uint8)
    for t in range(RT):
        frames[t] = bg
        frames[t, 0, 48:48 + 384, 40:40 + 384] = patch
        if t < BLANK_FROM:  # the right face leaves: its place shows the background again
            frames[t, 0, 48:48 + 384, 536:536 + 384] = patch
    return frames


def test_real_detections_two_faces(H):
    from zaru_amd._lib import DeviceBuffer
    frames = _two_face_video()
    found = H.Detector("face").detect(frames[0, 0])
    print("faces in the two-face frame:", [(d.confidence(), d.bounding_rect().tuple()) for d in found])
    assert len(found) == 2, len(found)
    refs = [MR.MultiTrackerRef(H, "face", "facemesh", 4) for _ in range(2)]
    dev = H.DeviceMultiTracker("face", "facemesh", 2, 4)
    buf = DeviceBuffer.from_array(frames)
    fb = RH * RW * 4
    counts_seen, ids_seen, compared = [], [], 0
    for t in range(RT):
        now = 33.0 * t
        dev.step([(buf.ptr + (t * 2 + s) * fb, RW, RH, RW * 4) for s in range(2)], now)
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        for s in range(2):
            refs[s].step(frames[t, s], now)
            want = _record(_ref_objects(refs[s]), len(refs[s].objs), refs[s].pending)
            got = _record(_dev_objects(dev, s), counts[s], pend[s])
            assert got[:2] == want[:2], (t, s, got[:2], want[:2])
            assert [o[0] for o in got[2]] == [o[0] for o in want[2]], (t, s)
            for g, w in zip(got[2], want[2]):
                assert g == w, (t, s, g[0], [a == b for a, b in zip(g, w)])
                compared += 1
        counts_seen.append(counts[0])
        ids_seen.append([o["id"] for o in dev.objects(0)])
        # the noise stream never holds an object, so its detector runs on every frame
        assert counts[1] == 0 and pend[1] == 1, (t, counts, pend)
    print("counts:", counts_seen, "ids:", ids_seen)
    assert compared >= 6, compared
    assert counts_seen[1:BLANK_FROM + 1] == [2] * BLANK_FROM, counts_seen   # both faces, from the step after the detection
    assert ids_seen[2] == [0, 1], ids_seen
    assert counts_seen[BLANK_FROM + 1:] == [1] * (RT - BLANK_FROM - 1), counts_seen  # the blanked face is lost
    left = ids_seen[BLANK_FROM + 1]
    assert len(left) == 1 and all(i == left for i in ids_seen[BLANK_FROM + 1:]), ids_seen  # the survivor keeps its id
    assert dev.detector_frames() == sum(r.detector_frames for r in refs)


def test_capacity(H):
    from zaru_amd._lib import DeviceBuffer
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    dev.set_loss_threshold(-1.0)
    f = _noise(2, 3)
    dev.inject_detections(0, [_det(H, (0.9, (60.0 + 150.0 * i, 100.0, 60.0, 60.0), 0.0)) for i in range(3)])
    drops = []
    for k in range(2):
        b = DeviceBuffer.from_array(f[k])
        dev.step([(b.ptr, FW, FH, FW * 4)], 10.0 * k)
        dev.synchronize()
        drops.append(dev.dropped_objects())
    assert drops[0] == [1], drops
    assert dev.object_counts() == [2]
    assert [o["id"] for o in dev.objects(0)] == [0, 1]
    assert dev.dropped_detections() == [0]
    assert dev.detection_capacity() == 896  # BlazeFace short range's anchors


# ---- the two kernels alone ------------------------------------------------------------------------
def _compact_ref(counts, views, K):
    S = len(counts)
    dense_of = np.full(S * K, -1, np.int32)
    dense = []
    for s in range(S):
        for h in range(min(max(int(counts[s]), 0), K)):
            dense_of[s * K + h] = len(dense)
            dense.append(views[s * K + h])
    return dense_of, np.array(dense, np.uint32).reshape(-1, 10), len(dense)


@pytest.mark.parametrize("case", ["mixed", "one", "empty"])
def test_slot_compact_alone(case):
    from zaru_amd import _lib
    lib = _lib.lib()
    Kc = 4
    rng = np.random.default_rng(17)
    if case == "mixed":   # 1500 streams: past one 1024 chunk, no multiple of 64
        counts = rng.integers(0, Kc + 1, 1500).astype(np.int32)
        counts[0] = 0
        counts[-1] = 0
        counts[100:300] = 0        # a run of idle streams, across wavefronts
        counts[1000:1100] = Kc     # full streams, across the chunk boundary
        counts[700] = Kc + 3       # clamped to the slots
        counts[701] = -2           # clamped to 0
    elif case == "one":
        counts = np.array([3], np.int32)
    else:
        counts = np.zeros(130, np.int32)
    Sc = len(counts)
    views = rng.integers(1, 2 ** 31, (Sc * Kc, 10), dtype=np.int64).astype(np.uint32)  # any bits: copied as they are
    sentinel = np.full((Sc * Kc, 10), 0xA5A5A5A5, np.uint32)
    d_counts, d_views = _lib.DeviceBuffer.from_array(counts), _lib.DeviceBuffer.from_array(views)
    d_dense, d_of = _lib.DeviceBuffer.from_array(sentinel), _lib.DeviceBuffer.from_array(np.full(Sc * Kc, 77, np.int32))
    d_n, d_total = _lib.DeviceBuffer.from_array(np.array([-5], np.int32)), _lib.DeviceBuffer.from_array(np.array([1000], np.uint64))
    _lib.check(lib.zr_slot_compact_async(d_counts.ptr, Sc, Kc, d_views.ptr, d_dense.ptr, d_of.ptr, d_n.ptr, d_total.ptr, None))
    _lib.synchronize()
    want_of, want_dense, n = _compact_ref(counts, views, Kc)
    assert d_n.download((1,), np.int32)[0] == n
    assert d_total.download((1,), np.uint64)[0] == 1000 + n
    assert np.array_equal(d_of.download((Sc * Kc,), np.int32), want_of)
    got = d_dense.download((Sc * Kc, 10), np.uint32)
    assert np.array_equal(got[:n], want_dense)
    assert np.array_equal(got[n:], sentinel[n:])  # nothing written past the count
    if case == "empty":
        assert n == 0
    # without the running total
    _lib.check(lib.zr_slot_compact_async(d_counts.ptr, Sc, Kc, d_views.ptr, d_dense.ptr, d_of.ptr, d_n.ptr, None, None))
    _lib.synchronize()
    assert d_n.download((1,), np.int32)[0] == n and d_total.download((1,), np.uint64)[0] == 1000 + n


def test_track_update_indexed():
    """Five RoIs, one inactive; the estimates stored shuffled, found through the index: states,
    views and landmarks equal zr_track_update_async on the unshuffled estimates."""
    from zaru_amd import _lib
    lib = _lib.lib()
    n, L = 5, 468
    lm_stride, flag_stride = 3 * L + 5, 2
    rng = np.random.default_rng(23)
    cfg = _lib.TrackCfg(kind=0, num_landmarks=L, in_w=192, in_h=192, aspect_w=1, aspect_h=1, loss_thresh=0.5,
                        padding=0.3, rois_per_frame=1)
    st = (_lib.TrackState * n)()
    for i in range(n):
        st[i].roi[:] = [200.0 + 30 * i, 180.0 + 10 * i, 120.0 + 5 * i, 130.0, 0.1 * i]
        st[i].active = 0 if i == 2 else 1
        st[i].frame_w, st[i].frame_h = 640, 480
    lm = rng.uniform(20.0, 170.0, (n, lm_stride)).astype(np.float32)
    flag = rng.uniform(1.0, 4.0, (n, flag_stride)).astype(np.float32)
    flag[4, 0] = -3.0  # lost now: sigmoid < 0.5
    # where each RoI's estimate is stored; RoI 2 is inactive and holds none
    index = np.array([3, 0, -1, 1, 2], np.int32)
    lm_sh = rng.uniform(-1e6, 1e6, (n, lm_stride)).astype(np.float32)
    flag_sh = rng.uniform(-1e6, 1e6, (n, flag_stride)).astype(np.float32)
    for i in range(n):
        if index[i] >= 0:
            lm_sh[index[i]] = lm[i]
            flag_sh[index[i]] = flag[i]

    def run(lm_a, flag_a, idx):
        d_st = _lib.DeviceBuffer.from_array(np.frombuffer(bytes(st), np.uint8))
        d_views = _lib.DeviceBuffer(n * 40)
        _lib.check(lib.zr_track_seed_async(d_st.ptr, n, C.byref(cfg), d_views.ptr, None))
        d_lm, d_flag = _lib.DeviceBuffer.from_array(lm_a), _lib.DeviceBuffer.from_array(flag_a)
        d_out = _lib.DeviceBuffer.from_array(np.zeros((n, L, 3), np.float32))
        if idx is None:
            _lib.check(lib.zr_track_update_async(d_st.ptr, n, C.byref(cfg), d_lm.ptr, lm_stride, d_flag.ptr, flag_stride,
                                                 d_out.ptr, d_views.ptr, None))
        else:
            d_idx = _lib.DeviceBuffer.from_array(idx)
            _lib.check(lib.zr_track_update_indexed_async(d_st.ptr, n, C.byref(cfg), d_lm.ptr, lm_stride, d_flag.ptr,
                                                         flag_stride, d_idx.ptr, d_out.ptr, d_views.ptr, None))
        _lib.synchronize()
        return (d_st.download((n * C.sizeof(_lib.TrackState),), np.uint8), d_views.download((n, 10), np.uint32),
                d_out.download((n, L, 3), np.uint32))

    want = run(lm, flag, None)
    got = run(lm_sh, flag_sh, index)
    for w, g, name in zip(want, got, ("states", "views", "lm_out")):
        assert np.array_equal(w, g), name
    states = np.frombuffer(want[0].tobytes(), np.dtype(_lib.TrackState))
    assert list(states["tracked"]) == [1, 1, 0, 1, 0] and list(states["active"]) == [1, 1, 0, 1, 0]
    # the identity index is the plain call
    ident = run(lm, flag, np.arange(n, dtype=np.int32))
    for w, g in zip(want, ident):
        assert np.array_equal(w, g)
    # an active RoI whose estimate is nowhere (index out of range) is lost, not read
    bad = index.copy()
    bad[0], bad[3] = -1, n
    lost = np.frombuffer(run(lm_sh, flag_sh, bad)[0].tobytes(), np.dtype(_lib.TrackState))
    assert list(lost["tracked"]) == [0, 1, 0, 0, 0] and list(lost["active"]) == [0, 1, 0, 0, 0]


def test_pose(H):
    """With the canonical mesh as reference every object's pose is the host ProcrustesAnalyzer's on
    that object's landmarks; objects without a result have none (they are not listed)."""
    import procrustes_ref as R
    from zaru_amd._lib import DeviceBuffer
    mesh = R.canonical_mesh()
    analyzer = H.ProcrustesAnalyzer(mesh)
    dev = H.DeviceMultiTracker("face", "facemesh", 2, 3)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(1e9)
    dev.set_pose_reference(mesh)
    f = [_noise(4, 40 + s) for s in range(2)]
    script = {0: {0: [(0.9, (120.0, 120.0, 90.0, 90.0), 0.0), (0.9, (340.0, 200.0, 120.0, 110.0), 0.0)],
                  1: [(0.9, (240.0, 180.0, 150.0, 150.0), 0.0)]},
              2: {1: [(0.9, (80.0, 80.0, 60.0, 60.0), 0.0)]}}
    posed = 0
    for k in range(4):
        for s, dets in script.get(k, {}).items():
            dev.inject_detections(s, [_det(H, d) for d in dets])
        b = DeviceBuffer.from_array(np.stack([f[s][k] for s in range(2)]))
        dev.step([(b.ptr + s * FH * FW * 4, FW, FH, FW * 4) for s in range(2)], 10.0 * k)
        dev.synchronize()
        for s in range(2):
            objs = dev.objects(s)
            assert len(objs) <= dev.object_counts()[s]
            for o in objs:
                want = analyzer.analyze(o["landmarks"][:len(mesh)], flip_y=True).pose().view(np.uint32)
                assert np.array_equal(o["pose"].view(np.uint32), want), (k, s, o["id"])
                assert o["pose"].view(np.uint32)[7] == 1
                posed += 1
        if k == 0:
            assert all(dev.objects(s) == [] for s in range(2))  # started this step: no result, no pose
    assert posed >= 6, posed
    # without a reference there is no pose key
    dev.set_pose_reference(None)
    assert all("pose" not in o for s in range(2) for o in dev.objects(s))


def test_rejections(H):
    from zaru_amd._lib import DeviceBuffer
    for lm in ("iris", "eye", "face68_pfld", "face68_peppa"):
        with pytest.raises(RuntimeError):
            H.DeviceMultiTracker("face", lm, 1, 4)
    for slots in (0, 65):
        with pytest.raises(RuntimeError):
            H.DeviceMultiTracker("face", "facemesh", 1, slots)
    with pytest.raises(RuntimeError):
        H.DeviceMultiTracker("face", "facemesh", 0, 4)
    dev = H.DeviceMultiTracker("face", "facemesh", 2, 2)
    dev.set_loss_threshold(-1.0)
    f = _noise(2, 5)
    small = np.ascontiguousarray(f[0][:200, :300])
    b0, b1, bs = DeviceBuffer.from_array(f[0]), DeviceBuffer.from_array(f[1]), DeviceBuffer.from_array(small)
    good = [(b0.ptr, FW, FH, FW * 4), (b1.ptr, FW, FH, FW * 4)]
    dev.inject_detections(0, [_det(H, (0.9, (200.0, 180.0, 80.0, 80.0), 0.0))])
    dev.step(good, 0.0)
    dev.synchronize()

    def snapshot():
        return (dev.object_counts(), dev.detection_pending(), dev.landmark_images(), dev.detector_frames(),
                [[(o["id"], o["landmarks"].tobytes()) for o in dev.objects(s)] for s in range(2)])

    before = snapshot()
    with pytest.raises(RuntimeError):
        dev.step(good[:1], 10.0)                                      # a wrong frame count
    with pytest.raises(RuntimeError):
        dev.step([], 10.0)
    with pytest.raises(RuntimeError):
        dev.step_host([f[0], f[1]], 10.0)                             # host-resident frames
    with pytest.raises(RuntimeError):
        dev.step([good[0], (bs.ptr, 300, 200, 300 * 4)], 10.0)        # mixed frame sizes
    assert snapshot() == before
    with pytest.raises(RuntimeError):
        dev.inject_detections(2, [])
    with pytest.raises(RuntimeError):
        dev.objects(2)
    for bad in (dev.set_det_grow, dev.set_roi_padding, dev.set_redetect_interval):
        with pytest.raises(RuntimeError):
            bad(-1.0)
    # the loop goes on after the refused calls
    dev.step(good, 10.0)
    dev.synchronize()
    assert dev.object_counts()[0] == 1 and [o["id"] for o in dev.objects(0)] == [0]
