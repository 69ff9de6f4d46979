"""The face quality gate inside DeviceMultiTracker (set_identity_quality), against
tests/quality_ref.py's MultiQualityRef at every step, stream and object, bit for bit: tracking, identity,
the quality record, the counters and the gallery.

The script, at the shape of tests/test_gpu_multi_all_features.py: S = 2 streams of K = 3 slots, 10 steps of
480 x 360 frames 15 ms apart, every object embedded at every step (identify interval 0), injected detections,
the golden MobileFaceNet, enrolment and gallery refinement on.  Stream 0's frames are one noise image (a still
scene, so an object's looks stay within the identity threshold and its row is refined), stream 1's one flat
colour (alpha 255); one of stream 0's objects is injected at the frame's corner, so its crop leaves
the frame.  The oracle's measure is zaru_amd.host.face_quality, which tests/test_quality_cpu.py pins to the
numpy restatement bit for bit; the pose is the host ProcrustesAnalyzer's (tests/test_gpu_multi_tracker.py
pins the loop's pose to it).

The thresholds come from a run with every minimum -inf (`setup`): the gate changes neither the tracking nor
which objects are due at an interval of 0, so that run measures exactly the crops the gated run will.
  embed tier: min_sharpness 0.5 -- the flat stream's sharpness is exactly 0, noise is in the thousands -- and
              min_inside halfway between the smallest and the largest fraction stream 0 shows;
  learn tier: min_frontal and min_size at the lower sixth of what the embed tier's survivors show, so most
              looks teach and a few are held back.
test_script_contains_the_cases asserts the outcome instead of assuming it."""
import math

import numpy as np
import pytest

import multi_enrol_ref as ER
import multi_identity_ref as IR
import multi_tracker_ref as MR
import procrustes_ref as PR
import quality_ref as QR
import recognition_util as RU
import test_gpu_multi_identity as TI
import test_gpu_multi_template as TT

pytestmark = pytest.mark.gpu

f32 = np.float32
S, K, STEPS, CLOCK = 2, 3, 10, 15.0
FW, FH = 480, 360
SCRIPT = {
    0: {0: [(0.9, (200.0, 180.0, 80.0, 88.0), 0.3), (0.8, (24.0, 24.0, 80.0, 80.0), 0.0)],   # the second: a corner
        1: [(0.9, (100.0, 100.0, 60.0, 60.0), 0.0)]},
    3: {0: [(0.7, (380.0, 250.0, 64.0, 64.0), 1.0)], 1: [(0.6, (300.0, 200.0, 90.0, 90.0), 0.0)]},
}
GALLERY_IDS = [7, 1000, 2 ** 40 + 3]
FIRST_ID, CAPACITY, MAX_SAMPLES = 5000, 16, 64
# between two looks at one object (its crop drifts over a still image: 3 to 6) and the random rows (about 11)
THRESHOLD = 7.0
PACKED_KEYS_GATE_OFF = {"count", "stream_offsets", "stream", "slot", "id", "flags", "view_rect", "confidence",
                        "landmarks", "pose", "identity_id", "identity_distance", "identity_embeddings",
                        "identity_enrolled", "identity_present", "embedding"}


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


@pytest.fixture(scope="module")
def frames():
    flat = np.empty((FH, FW, 4), np.uint8)
    flat[...] = (120, 90, 60, 255)
    noise = TI._noise(1, 30)[0]   # a still scene: two looks at one object differ by the drift of its crop alone
    noise[..., 3] = 255
    return [[noise.copy() for _ in range(STEPS)], [flat.copy() for _ in range(STEPS)]]


@pytest.fixture(scope="module")
def model():
    return RU.model_bytes(TI.GOLDEN)


@pytest.fixture(scope="module")
def embed(H, model):
    raw = IR.host_embed(H.FaceEmbedder(model))
    cache = {}

    def fn(frame, rect):
        key = (id(frame), rect.tuple())
        if key not in cache:
            cache[key] = raw(frame, rect)
        return cache[key]
    return fn


@pytest.fixture(scope="module")
def gallery_rows():
    return np.random.default_rng(78).standard_normal((3, 128)).astype(f32)


def _injected(k):
    return [list(SCRIPT.get(k, {}).get(s, [])) for s in range(S)]


def _quality_record(q):
    return QR.bits(QR.DEFAULT if q is None else q)


def _oracle_run(H, frames, embed, rows, embed_tier, learn_tier):
    mesh = PR.canonical_mesh()
    analyzer = H.ProcrustesAnalyzer(mesh)
    measured = {}

    def measure(frame, view, pose):
        key = (id(frame), view.zr_view())
        if key not in measured:
            measured[key] = H.face_quality(frame, view, 112, 112)
        m = dict(measured[key])
        m["frontal"] = pose[20] if pose.view(np.uint32)[7] else f32(math.nan)
        return m

    trackers = []
    for s in range(S):
        t = MR.MultiTrackerRef(H, "face", "facemesh", K)
        t.loss, t.interval = -1.0, 40.0
        trackers.append(t)
    gal = ER.GalleryRef(CAPACITY, rows, GALLERY_IDS, FIRST_ID)
    ref = QR.MultiQualityRef(
        H, trackers, embed, TT._make_match(H), gal, embed_tier=embed_tier, learn_tier=learn_tier, measure=measure,
        pose_of=lambda lm: analyzer.analyze(np.asarray(lm, f32)[:len(mesh)], flip_y=True).pose(),
        crop=lambda lm, frame: H.landmark_crop_view(np.ascontiguousarray(lm, f32), FW, FH, 1, 1, 0.4),
        interval=0.0, threshold=THRESHOLD, refine=True, max_samples=MAX_SAMPLES, enrol=True)
    out = {"track": [], "identity": [], "quality": [], "counters": [], "ref": ref, "gallery": gal}
    for k in range(STEPS):
        ref.step([frames[s][k] for s in range(S)], CLOCK * k, [[TI._det(H, d) for d in dets] for dets in _injected(k)])
        out["track"].append([TI._track_record(
            [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
              "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in trackers[s].objects()],
            len(trackers[s].objs), trackers[s].pending) for s in range(S)])
        objs = [ref.objects(s) for s in range(S)]
        out["identity"].append([[(o.id, TT.TE._record(i, i and i["flags"] & ER.ENROLLED)) for o, i, _ in objs[s]]
                                for s in range(S)])
        out["quality"].append([[(o.id, _quality_record(q)) for o, _, q in objs[s]] for s in range(S)])
        out["counters"].append((ref.images, ref.measured, ref.rejected, ref.held_back, gal.enrolled_total,
                                ref.refined_total))
    return out


def _tier(H, t):
    return H.FaceQualityGate(*t)


def _device_run(H, frames, model, rows, tiers, pose=True, steps=STEPS):
    """tiers: None (the gate never set) or (embed, learn)."""
    from zaru_amd._lib import DeviceBuffer
    gallery = TI._gallery(H, rows, GALLERY_IDS)
    gallery.reserve(CAPACITY)
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    if pose:
        dev.set_pose_reference(PR.canonical_mesh())
    dev.set_recognition(model, gallery)
    dev.set_identify_interval(0.0)
    dev.set_identity_threshold(THRESHOLD)
    dev.set_gallery_refinement(gallery, MAX_SAMPLES)
    dev.set_enrolment(gallery, FIRST_ID)
    if tiers is not None:
        dev.set_identity_quality(_tier(H, tiers[0]), _tier(H, tiers[1]))
    out = {"track": [], "identity": [], "quality": [], "counters": [], "packed": [], "dev": dev, "gallery": gallery,
           "bufs": []}
    fb = FH * FW * 4
    for k in range(steps):
        buf = DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)]))
        out["bufs"].append(buf)
        for s, dets in enumerate(_injected(k)):
            if dets:
                dev.inject_detections(s, [TI._det(H, d) for d in dets])
        dev.step([(buf.ptr + s * fb, FW, FH, FW * 4) for s in range(S)], CLOCK * k)
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        objs = [dev.objects(s) for s in range(S)]
        out["track"].append([TI._track_record(
            [{"id": o["id"], "rect": o["view_rect"].rect().tuple(), "angle": o["view_rect"].rotation_radians(),
              "landmarks": o["landmarks"], "confidence": o["confidence"]} for o in objs[s]], counts[s], pend[s])
            for s in range(S)])
        out["identity"].append([[(o["id"], TT.TE._record(o["identity"], o["identity"] and o["identity"]["enrolled"]))
                                 for o in objs[s]] for s in range(S)])
        out["quality"].append([[(o["id"], _quality_record(o["quality"]) if "quality" in o else None) for o in objs[s]]
                               for s in range(S)])
        out["counters"].append((dev.identity_images(), dev.quality_measured_total(), dev.quality_rejected_total(),
                                dev.quality_held_back_total(), dev.enrolled_total(), dev.refined_total()))
        out["packed"].append(dev.objects_packed())
    return out


@pytest.fixture(scope="module")
def setup(H, frames, embed, gallery_rows):
    """The oracle with every minimum -inf, and the tiers chosen from what it measured."""
    plain = _oracle_run(H, frames, embed, gallery_rows, QR.SKIP, QR.SKIP)
    # every measurement of the run, from the oracle's per-step records
    seen = [(k, s, oid, np.frombuffer(bits[0], f32), bits[3])
            for k in range(STEPS) for s in range(S) for oid, bits in plain["quality"][k][s] if bits[1] & QR.MEASURED]
    assert len(seen) >= 20
    inside0 = [float(m[1]) for _, s, _, m, _ in seen if s == 0]
    min_inside = (min(inside0) + max(inside0)) / 2
    embed_tier = (-math.inf, min_inside, 0.5, -math.inf)
    alive = [m for _, _, _, m, _ in seen if m[1] >= f32(min_inside) and m[2] >= f32(0.5)]
    frontal = sorted(float(m[3]) for m in alive if not math.isnan(m[3]))
    min_frontal = frontal[len(frontal) // 6]
    sizes = sorted(float(m[0]) for m in alive if m[3] >= f32(min_frontal))
    min_size = sizes[len(sizes) // 6]
    learn_tier = (min_size, -math.inf, -math.inf, min_frontal)
    print("embed tier", embed_tier, "learn tier", learn_tier)
    for k, s, oid, m, n in seen:
        dist = [np.frombuffer(rec[1], f32)[0] for i, rec in plain["identity"][k][s] if i == oid and rec is not None]
        print(f"step {k} stream {s} object {oid}: size {m[0]:.2f} inside {m[1]:.4f} sharpness {m[2]:.1f} "
              f"frontal {m[3]:.4f} samples {n} distance {dist}")
    return {"plain": plain, "seen": seen, "tiers": (embed_tier, learn_tier)}


@pytest.fixture(scope="module")
def gated(H, frames, embed, model, gallery_rows, setup):
    want = _oracle_run(H, frames, embed, gallery_rows, *setup["tiers"])
    got = _device_run(H, frames, model, gallery_rows, setup["tiers"])
    return want, got


def test_script_contains_the_cases(setup, gated):
    want, _ = gated
    embed_tier, learn_tier = setup["tiers"]
    kinds = {c[3] for c in want["ref"].cases}
    assert kinds == {"reject", "held", "learn"}, kinds
    m = np.array([x[3] for x in setup["seen"]])
    # every criterion passes somewhere and fails somewhere
    assert (m[:, 1] >= f32(embed_tier[1])).any() and (m[:, 1] < f32(embed_tier[1])).any()     # inside
    assert (m[:, 2] >= f32(0.5)).any() and (m[:, 2] == 0).any()                                # sharpness
    assert (m[:, 0] >= f32(learn_tier[0])).any() and (m[:, 0] < f32(learn_tier[0])).any()     # size
    assert (m[:, 3] >= f32(learn_tier[3])).any() and (m[:, 3] < f32(learn_tier[3])).any()     # frontal
    flags = {bits[1] for k in range(STEPS) for s in range(S) for _, bits in want["quality"][k][s]}
    assert any(f & QR.FAIL_INSIDE for f in flags) and any(f & QR.FAIL_SHARPNESS for f in flags)
    # the flat stream is never embedded; stream 0 is enrolled and refined; somebody was rejected twice running
    assert all(rec is None for k in range(STEPS) for _, rec in want["identity"][k][1])
    assert want["gallery"].enrolled_total > 0 and want["ref"].refined_total > 0 and want["ref"].held_back > 0
    assert max(bits[2] for k in range(STEPS) for s in range(S) for _, bits in want["quality"][k][s]) >= 2
    # a crop left the frame
    assert min(float(x[3][1]) for x in setup["seen"] if x[1] == 0) < 1.0


def test_loop_equals_the_oracle(gated):
    want, got = gated
    for k in range(STEPS):
        for s in range(S):
            assert got["track"][k][s] == want["track"][k][s], ("tracking", k, s)
            assert got["identity"][k][s] == want["identity"][k][s], ("identity", k, s)
            assert got["quality"][k][s] == want["quality"][k][s], ("quality", k, s)
        assert got["counters"][k] == want["counters"][k], ("counters", k, got["counters"][k], want["counters"][k])


def test_packed_quality_is_objects(H, gated):
    _, got = gated
    n = 0
    for k in range(1, STEPS):
        p = got["packed"][k]
        assert set(p) == PACKED_KEYS_GATE_OFF | {"quality"}
        flat = [bits for s in range(S) for _, bits in got["quality"][k][s]]
        assert p["count"] == len(flat) and p["quality"].shape == (len(flat),)
        assert [QR.bits(q) for q in p["quality"]] == flat
        assert all(int(f) & 16 for f in p["flags"])   # ZR_EXPORT_QUALITY
        assert (p["quality"]["reserved"] == 0).all()
        n += len(flat)
    assert n > 10


def test_gallery_holds_no_trace_of_held_back_objects(gated):
    want, got = gated
    rows, ids = got["gallery"].rows()
    ref = want["gallery"]
    assert list(ids) == list(ref.ids) and len(ids) > len(GALLERY_IDS)
    for r in range(len(ids)):
        assert np.asarray(rows[r], f32).tobytes() == ref.rows[r].tobytes(), ("gallery row", r)
    assert list(got["gallery"].row_updates()) == list(want["ref"].updates)


def test_gate_made_a_difference(setup, gated):
    want, _ = gated
    plain = setup["plain"]
    assert plain["counters"][-1][0] > want["counters"][-1][0]            # embeddings made
    assert (plain["gallery"].enrolled_total, plain["ref"].refined_total) != \
        (want["gallery"].enrolled_total, want["ref"].refined_total)


def test_all_skip_tiers_change_nothing(H, frames, model, gallery_rows, setup):
    """With both tiers all -inf the identities, the gallery and the tracking are bit for bit those of a run
    without the gate -- and of the oracle's; the gate-off run reports no quality anywhere."""
    off = _device_run(H, frames, model, gallery_rows, None)
    on = _device_run(H, frames, model, gallery_rows, (QR.SKIP, QR.SKIP))
    plain = setup["plain"]
    for k in range(STEPS):
        for s in range(S):
            assert on["track"][k][s] == off["track"][k][s] == plain["track"][k][s], ("tracking", k, s)
            assert on["identity"][k][s] == off["identity"][k][s] == plain["identity"][k][s], ("identity", k, s)
            assert on["quality"][k][s] == plain["quality"][k][s], ("quality", k, s)
            assert all(q is None for _, q in off["quality"][k][s])
        assert on["counters"][k][0] == off["counters"][k][0] and on["counters"][k][4:] == off["counters"][k][4:]
        assert on["counters"][k] == plain["counters"][k] and off["counters"][k][1:4] == (0, 0, 0)
        # today's keys: nothing of the gate, and (from the first step with a result on) exactly this set
        assert set(off["packed"][k]) == set(on["packed"][k]) - {"quality"} and "quality" not in off["packed"][k]
        assert k == 0 or set(off["packed"][k]) == PACKED_KEYS_GATE_OFF
        for key in set(off["packed"][k]) - {"flags"}:
            assert np.asarray(on["packed"][k][key]).tobytes() == np.asarray(off["packed"][k][key]).tobytes(), (k, key)
        assert ((np.asarray(on["packed"][k]["flags"]) & ~np.uint32(16)) == off["packed"][k]["flags"]).all()
    ra, ia = on["gallery"].rows()
    rb, ib = off["gallery"].rows()
    assert list(ia) == list(ib) and np.asarray(ra, f32).tobytes() == np.asarray(rb, f32).tobytes()
    assert list(on["gallery"].row_updates()) == list(off["gallery"].row_updates())
    assert not off["dev"].identity_quality() and on["dev"].identity_quality()
    assert on["counters"][-1][2:4] == (0, 0) and on["counters"][-1][1] == on["counters"][-1][0] > 0


def test_set_recognition_turns_the_gate_off(H, frames, model, gallery_rows, setup):
    from zaru_amd._lib import DeviceBuffer
    run = _device_run(H, frames, model, gallery_rows, setup["tiers"], steps=3)
    dev = run["dev"]
    assert dev.identity_quality() and any("quality" in o for s in range(S) for o in dev.objects(s))
    measured = dev.quality_measured_total()
    dev.set_recognition(model, run["gallery"])
    dev.set_identify_interval(0.0)
    assert not dev.identity_quality()
    buf = DeviceBuffer.from_array(np.stack([frames[s][3] for s in range(S)]))
    dev.step([(buf.ptr + s * FH * FW * 4, FW, FH, FW * 4) for s in range(S)], CLOCK * 3)
    dev.synchronize()
    objs = [o for s in range(S) for o in dev.objects(s)]
    assert objs and all("quality" not in o for o in objs) and "quality" not in dev.objects_packed()
    assert dev.quality_measured_total() == measured           # the counter survives, and nothing was measured
    assert all(o["identity"] is not None for o in dev.objects(1))   # the flat stream is embedded again
    # needs recognition; None turns it off; a NaN minimum is refused
    dev.set_identity_quality(_tier(H, setup["tiers"][0]))
    assert dev.identity_quality()
    dev.set_identity_quality(None)
    assert not dev.identity_quality()
    with pytest.raises(RuntimeError):
        dev.set_identity_quality(H.FaceQualityGate(min_size=math.nan))
    dev.set_recognition(b"", None)
    with pytest.raises(RuntimeError):
        dev.set_identity_quality(_tier(H, setup["tiers"][0]))


def test_frontal_tier_without_pose_reference_is_refused_at_step(H, frames, model, gallery_rows):
    from zaru_amd._lib import DeviceBuffer
    run = _device_run(H, frames, model, gallery_rows, (QR.SKIP, QR.SKIP), pose=False, steps=2)
    dev = run["dev"]
    assert all(math.isnan(o["quality"]["frontal"]) for s in range(S) for o in dev.objects(s))
    dev.set_identity_quality(H.FaceQualityGate(), H.FaceQualityGate(min_frontal=0.5))
    before = (dev.landmark_images(), dev.identity_images(), dev.detector_frames(), dev.object_counts())
    buf = DeviceBuffer.from_array(np.stack([frames[s][2] for s in range(S)]))
    fr = [(buf.ptr + s * FH * FW * 4, FW, FH, FW * 4) for s in range(S)]
    with pytest.raises(RuntimeError):
        dev.step(fr, CLOCK * 2)
    dev.synchronize()
    assert (dev.landmark_images(), dev.identity_images(), dev.detector_frames(), dev.object_counts()) == before
    dev.set_pose_reference(PR.canonical_mesh())
    dev.step(fr, CLOCK * 2)   # with a reference the same step runs
    dev.synchronize()
    assert dev.landmark_images() > before[0] and dev.quality_measured_total() > 0
