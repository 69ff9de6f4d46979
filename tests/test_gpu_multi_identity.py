"""Recognition of the tracked faces inside DeviceMultiTracker (set_recognition) and its three entry
points -- zr_identity_select_async, zr_identity_compact_async, zr_identity_commit_async -- against

  * tests/multi_identity_ref.py: tests/multi_tracker_ref.py's oracle with an identity per object made
    by the host API (FaceEmbedder.embed on the landmarks' bounding rect, Gallery.match), bit for bit:
    id, distance, embeddings count and the 128 floats, at every step, stream and object;
  * itself with recognition off (no bit of the tracking may move);
  * numpy restatements of the three kernels' contracts on synthetic states (no network).

The script is tests/test_gpu_multi_tracker.py's face script (a swept duplicate pair, a late newcomer,
an on-top detection that is filtered) with two more events.  Each places a large detection around a
stream's first object: it passes the IoU filter (the object's RoI is a fifth of it), shrinks onto
the object with its first estimate, and is swept at the next step.  On stream 0 a newcomer started
right after it then moves down into its slot; on stream 1 a newcomer of that very step takes the slot.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import multi_identity_ref as IR
import multi_tracker_ref as MR
import recognition_util as RU

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FW, FH = 480, 360
S, K, STEPS, CLOCK = 3, 4, 8, 15.0
f32 = np.float32

# per step, per stream: (confidence, (cx, cy, w, h), angle)
SCRIPT = {
    0: {0: [(0.9, (200.0, 180.0, 80.0, 88.0), 0.3)],
        1: [(0.9, (100.0, 100.0, 60.0, 60.0), 0.0), (0.8, (104.0, 101.0, 60.0, 60.0), 0.1)],  # a pair: the sweep
        2: [(0.9, (300.0, 200.0, 100.0, 80.0), -0.2), (0.7, (120.0, 260.0, 72.0, 72.0), 0.5)]},
    2: {1: [(0.6, (330.0, 250.0, 88.0, 88.0), 1.0)]},        # a late newcomer
    3: {0: [(0.8, (60.0, 300.0, 60.0, 60.0), 0.0)]},         # starts behind stream 0's AROUND object
    4: {1: [(0.8, (400.0, 80.0, 56.0, 56.0), 0.0)],          # starts in the step stream 1's AROUND object leaves
        2: [(0.9, (300.0, 60.0, 60.0, 60.0), 0.0)]},
}
# (step, stream): a detection exactly on the RoI the stream's first object holds when the step's
# filter runs (known to the oracle one step ahead): filtered; then a newcomer
ON_TOP = {(2, 0): (0.9, (420.0, 60.0, 50.0, 50.0), 0.0), (4, 2): None}
# (step, stream): a square detection centred on that RoI with 5 times its area (IoU 0.2: kept)
AROUND = {(3, 0), (3, 1)}
GALLERY_IDS = [7, 1000, 2 ** 40 + 3]
GROW_AT, GROWN_ID = 4, 555   # rows added before this step, past the gallery's capacity of 64


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(FH, FW, 4), dtype=np.uint8) for _ in range(n)]


def _det(H, d):
    conf, (cx, cy, w, h), angle = d
    return H.Detection(conf, H.Rect.from_center(cx, cy, w, h), angle)


def _track_record(objs, count, pending):
    return (int(count), bool(pending),
            [(int(o["id"]), np.asarray(o["rect"], f32).tobytes(), f32(o["angle"]).tobytes(),
              np.ascontiguousarray(o["landmarks"], f32).tobytes(), f32(o["confidence"]).tobytes()) for o in objs])


def _identity_record(i):
    if i is None:
        return None
    return (int(i["id"]), f32(i["distance"]).tobytes(), int(i["embeddings"]),
            np.ascontiguousarray(i["embedding"], f32).tobytes())


@pytest.fixture(scope="module")
def frames():
    return [_noise(STEPS, 10 + s) for s in range(S)]


@pytest.fixture(scope="module")
def model():
    return RU.model_bytes(GOLDEN)


@pytest.fixture(scope="module")
def embed(H, model, frames):
    """FaceEmbedder.embed per (frame, rect), kept: the oracle's runs share their crops."""
    embedder = H.FaceEmbedder(model)
    raw = IR.host_embed(embedder)
    cache = {}

    def fn(frame, rect):
        key = (id(frame), rect.tuple())
        if key not in cache:
            cache[key] = raw(frame, rect)
        return cache[key]
    return fn


def _gallery(H, rows, ids):
    g = H.Gallery()
    if len(ids):
        g.add(np.ascontiguousarray(rows, f32), list(ids))
    return g


def _oracle_run(H, frames, embed, gallery, interval, threshold, grow=None):
    """The oracle over the script.  grow: (rows, ids) added to the gallery before step GROW_AT."""
    refs = []
    for s in range(S):
        r = MR.MultiTrackerRef(H, "face", "facemesh", K)
        r.loss = -1.0
        r.interval = 40.0
        refs.append(IR.MultiIdentityRef(H, r, embed, IR.host_match(gallery), interval, threshold))
    out = {"track": [], "identity": [], "injected": [], "images": [], "due": [], "tracked": [], "slots": []}
    for k in range(STEPS):
        if grow is not None and k == GROW_AT:
            gallery.add(np.ascontiguousarray(grow[0], f32), list(grow[1]))
        inj = {}
        for s in range(S):
            t = refs[s].tracker
            dets = list(SCRIPT.get(k, {}).get(s, []))
            if (k, s) in ON_TOP or (k, s) in AROUND:
                first = t.objs[0]
                assert first.pending is not None  # loss threshold -1: never lost
                cx, cy, w, h = first.pending["updated_roi"].rect().tuple()
                if (k, s) in ON_TOP:
                    dets.insert(0, (0.9, (cx, cy, w, h), 0.0))
                    if ON_TOP[(k, s)] is not None:
                        dets.append(ON_TOP[(k, s)])
                else:
                    side = float(f32(math.sqrt(5.0 * w * h)))
                    dets.insert(0, (0.9, (cx, cy, side, side), 0.0))
            inj[s] = dets
            refs[s].step(frames[s][k], CLOCK * k, [_det(H, d) for d in dets])
        out["injected"].append(inj)
        out["track"].append([_track_record(
            [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
              "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in refs[s].tracker.objects()],
            len(refs[s].tracker.objs), refs[s].tracker.pending) for s in range(S)])
        out["identity"].append([[(o.id, _identity_record(i)) for o, i in refs[s].objects()] for s in range(S)])
        out["images"].append(sum(r.images for r in refs))
        out["due"].append([list(r.last_due) for r in refs])
        out["tracked"].append([list(r.last_tracked) for r in refs])
        out["slots"].append([r.tracker.ids() for r in refs])
    out["swept"] = [r.tracker.swept for r in refs]
    out["filtered"] = [r.tracker.filtered for r in refs]
    return out


def _device_run(H, frames, injected, model=None, gallery=None, interval=None, threshold=None, grow=None,
                filt=None, pose=None):
    from zaru_amd._lib import DeviceBuffer
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    if filt is not None:
        dev.set_filter(filt)
    if pose is not None:
        dev.set_pose_reference(pose)
    if model is not None:
        dev.set_recognition(model, gallery)
        if interval is not None:
            dev.set_identify_interval(interval)
        if threshold is not None:
            dev.set_identity_threshold(threshold)
    bufs = [DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)])) for k in range(STEPS)]
    fb = FH * FW * 4
    out = {"track": [], "identity": [], "images": [], "pose": [], "objects": []}
    for k in range(STEPS):
        if grow is not None and k == GROW_AT:
            gallery.add(np.ascontiguousarray(grow[0], f32), list(grow[1]))
        for s in range(S):
            if injected[k][s]:
                dev.inject_detections(s, [_det(H, d) for d in injected[k][s]])
        dev.step([(bufs[k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)], CLOCK * k)
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        objs = [dev.objects(s) for s in range(S)]
        out["objects"].append(objs)
        out["track"].append([_track_record(
            [{"id": o["id"], "rect": o["view_rect"].rect().tuple(), "angle": o["view_rect"].rotation_radians(),
              "landmarks": o["landmarks"], "confidence": o["confidence"]} for o in objs[s]], counts[s], pend[s])
            for s in range(S)])
        out["identity"].append([[(o["id"], _identity_record(o["identity"])) for o in objs[s]] for s in range(S)])
        out["pose"].append([[o["pose"].tobytes() if "pose" in o else None for o in objs[s]] for s in range(S)])
        out["images"].append(dev.identity_images())
    return out


# ---- the oracle's four runs ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_empty(H, frames, embed):
    """Interval 0 against an empty gallery: every embedding the script can produce."""
    return _oracle_run(H, frames, embed, _gallery(H, [], []), 0.0, math.inf)


def _embedding_of(run, k, s, oid):
    for i, rec in run["identity"][k][s]:
        if i == oid and rec is not None:
            return np.frombuffer(rec[3], f32)
    raise AssertionError(("no embedding", k, s, oid))


@pytest.fixture(scope="module")
def gallery_rows(oracle_empty):
    """Two rows are the oracle's own embeddings of scripted objects (distance exactly 0 at that step),
    one is random; and the rows that later grow the gallery past its capacity of 64, one of them the
    embedding of stream 1's late newcomer at step GROW_AT + 1."""
    rng = np.random.default_rng(77)
    first = [oracle_empty["slots"][STEPS - 1][s][0] for s in range(S)]
    rows = np.stack([_embedding_of(oracle_empty, 1, 0, first[0]), _embedding_of(oracle_empty, 3, 2, first[2]),
                     rng.standard_normal(128).astype(f32)])
    late = oracle_empty["slots"][2][1][-1]  # started at step 2
    more = rng.standard_normal((70, 128)).astype(f32)
    more[66] = _embedding_of(oracle_empty, GROW_AT + 1, 1, late)
    more_ids = [10_000 + i for i in range(70)]
    more_ids[66] = GROWN_ID
    return {"rows": rows, "more": (more, more_ids), "first": first, "late": late}


@pytest.fixture(scope="module")
def oracle_every(H, frames, embed, gallery_rows):
    """Interval 0, the default threshold, the gallery grown before step GROW_AT."""
    return _oracle_run(H, frames, embed, _gallery(H, gallery_rows["rows"], GALLERY_IDS), 0.0, math.inf,
                       grow=gallery_rows["more"])


@pytest.fixture(scope="module")
def known_distance(oracle_every, gallery_rows):
    """The distance of stream 1's first object at its first embedding (step 1) to its nearest row."""
    for i, rec in oracle_every["identity"][1][1]:
        if i == gallery_rows["first"][1]:
            d = np.frombuffer(rec[1], f32)[0]
            assert np.isfinite(d) and d > 0 and rec[0] in GALLERY_IDS
            return d, rec[0]
    raise AssertionError("stream 1's first object has no identity at step 1")


@pytest.fixture(scope="module")
def oracle_forty(H, frames, embed, gallery_rows, known_distance):
    """Interval 40 ms, the threshold exactly the known distance."""
    return _oracle_run(H, frames, embed, _gallery(H, gallery_rows["rows"], GALLERY_IDS), 40.0, float(known_distance[0]))


@pytest.fixture(scope="module")
def oracle_once(H, frames, embed, gallery_rows, known_distance):
    """Interval +inf, the threshold just below the known distance."""
    return _oracle_run(H, frames, embed, _gallery(H, gallery_rows["rows"], GALLERY_IDS), math.inf,
                       float(np.nextafter(known_distance[0], f32(0))))


def _compare(want, got):
    compared = 0
    for k in range(STEPS):
        for s in range(S):
            assert got["track"][k][s] == want["track"][k][s], ("tracking", k, s)
            w, g = want["identity"][k][s], got["identity"][k][s]
            assert [i for i, _ in g] == [i for i, _ in w], ("ids", k, s)
            for (oid, wr), (_, gr) in zip(w, g):
                assert (gr is None) == (wr is None), ("identified", k, s, oid)
                if wr is None:
                    continue
                assert gr[0] == wr[0], ("identity id", k, s, oid, gr[0], wr[0])
                assert gr[1] == wr[1], ("distance", k, s, oid, np.frombuffer(gr[1], f32), np.frombuffer(wr[1], f32))
                assert gr[2] == wr[2], ("embeddings", k, s, oid, gr[2], wr[2])
                assert gr[3] == wr[3], ("embedding", k, s, oid)
                compared += 1
        assert got["images"][k] == want["images"][k], ("identity_images", k, got["images"][k], want["images"][k])
    return compared


# ---- the cases the script must contain, on the oracle side --------------------------------------------
def _slot(run, k, s, oid):
    ids = run["slots"][k][s]
    return ids.index(oid) if oid in ids else None


def _identity_at(run, k, s, oid):
    for i, rec in run["identity"][k][s]:
        if i == oid:
            return rec
    return "absent"


def test_script_contains_the_cases(oracle_empty, oracle_every, oracle_forty, oracle_once, gallery_rows, known_distance):
    print("slots per step:", oracle_once["slots"])
    print("due per step (once):", oracle_once["due"], "(forty):", oracle_forty["due"])
    # the existing script's events
    assert oracle_once["swept"][1] >= 2 and oracle_once["swept"][0] >= 1, oracle_once["swept"]
    assert all(f >= 1 for f in (oracle_once["filtered"][0], oracle_once["filtered"][2])), oracle_once["filtered"]
    # stream 0: the object started behind the AROUND one moves to a lower slot when that one leaves, after
    # it was identified -- and keeps identity, count and embedding for the rest of the run
    around, mover = oracle_once["slots"][3][0][-2:]
    assert _slot(oracle_once, 4, 0, around) is None                              # swept at step 4
    assert _slot(oracle_once, 4, 0, mover) == _slot(oracle_once, 3, 0, around)   # into its slot
    assert _slot(oracle_once, 4, 0, mover) < _slot(oracle_once, 3, 0, mover)
    recs = [_identity_at(oracle_once, k, 0, mover) for k in range(4, STEPS)]
    assert recs[0] not in (None, "absent") and recs[0][2] == 1 and all(r == recs[0] for r in recs), "mover"
    # stream 1: a newcomer of step 4 takes the slot the AROUND object -- identified in that step -- vacates;
    # it has no result at step 4, and from step 5 on its own identity
    around1 = oracle_once["slots"][3][1][-1]
    newcomer = oracle_once["slots"][4][1][-1]
    assert around1 in oracle_once["due"][4][1] and _slot(oracle_once, 4, 1, around1) is None
    assert _slot(oracle_once, 4, 1, newcomer) == _slot(oracle_once, 3, 1, around1)
    assert _identity_at(oracle_once, 4, 1, newcomer) == "absent"
    own = _identity_at(oracle_once, 5, 1, newcomer)
    assert own not in (None, "absent") and own[2] == 1
    assert own[3] == _identity_at(oracle_empty, 5, 1, newcomer)[3]               # its own crop's embedding
    # a step at which no object is due, and one at which every live object is
    quiet = [k for k in range(1, STEPS) if not any(oracle_once["due"][k])]
    assert quiet and all(oracle_once["images"][k] == oracle_once["images"][k - 1] for k in quiet), quiet
    still = [k for k in quiet if oracle_once["slots"][k] == oracle_once["slots"][k - 1]]
    assert still and all(oracle_once["identity"][k] == oracle_once["identity"][k - 1] for k in still), (quiet, still)
    full = [k for k in range(STEPS) if any(oracle_every["tracked"][k]) and
            oracle_every["due"][k] == oracle_every["tracked"][k]]
    assert len(full) == STEPS - 1, full   # interval 0: every step that has landmarks
    # 40 ms on the 15 ms clock: embedded at step a, again at a + 3 (45 >= 40), not at a + 2 (30)
    again = 0
    for s in range(S):
        steps_of = {}
        for k in range(STEPS):
            for oid in oracle_forty["due"][k][s]:
                steps_of.setdefault(oid, []).append(k)
        for oid, ks in steps_of.items():
            assert all(b - a == 3 for a, b in zip(ks, ks[1:])), (s, oid, ks)
            again += len(ks) - 1
    assert again >= 4, again
    # +inf: exactly one embedding per object that ever had a result
    had = {(s, i) for k in range(STEPS) for s in range(S) for i in oracle_once["tracked"][k][s]}
    assert oracle_once["images"][-1] == len(had) and len(had) >= 8
    assert oracle_every["images"][-1] > oracle_forty["images"][-1] > oracle_once["images"][-1]
    # the gallery rows made of the oracle's own embeddings: distance exactly 0 at that step
    for k, s, gid in ((1, 0, GALLERY_IDS[0]), (3, 2, GALLERY_IDS[1])):
        rec = _identity_at(oracle_every, k, s, gallery_rows["first"][s])
        assert rec[0] == gid and np.frombuffer(rec[1], f32)[0] == 0.0, (k, s, rec[:3])
    # the grown gallery: the late newcomer's next embedding matches a row past the old capacity
    rec = _identity_at(oracle_every, GROW_AT + 1, 1, gallery_rows["late"])
    assert rec[0] == GROWN_ID and np.frombuffer(rec[1], f32)[0] == 0.0
    assert _identity_at(oracle_every, GROW_AT - 1, 1, gallery_rows["late"])[0] in GALLERY_IDS
    # the thresholds: exactly the distance is known, just below is not; the distance is reported either way
    d, gid = known_distance
    at, below = (_identity_at(r, 1, 1, gallery_rows["first"][1]) for r in (oracle_forty, oracle_once))
    assert at[0] == gid and below[0] == IR.NO_MATCH and at[1] == below[1] == f32(d).tobytes()
    # the empty gallery: unknown, +inf, the embedding still there
    for k in range(STEPS):
        for s in range(S):
            for _, rec in oracle_empty["identity"][k][s]:
                assert rec is not None and rec[0] == IR.NO_MATCH and rec[1] == f32(math.inf).tobytes()
                assert any(np.frombuffer(rec[3], f32) != 0)


# ---- the device against the oracle ------------------------------------------------------------------
def test_empty_gallery(H, frames, model, oracle_empty):
    got = _device_run(H, frames, oracle_empty["injected"], model, _gallery(H, [], []), 0.0, None)
    assert _compare(oracle_empty, got) >= 30


def test_every_step_and_the_grown_gallery(H, frames, model, oracle_every, gallery_rows):
    g = _gallery(H, gallery_rows["rows"], GALLERY_IDS)
    got = _device_run(H, frames, oracle_every["injected"], model, g, 0.0, None, grow=gallery_rows["more"])
    assert len(g) == 73
    assert _compare(oracle_every, got) >= 30


def test_interval_40ms_threshold_equal(H, frames, model, oracle_forty, gallery_rows, known_distance):
    got = _device_run(H, frames, oracle_forty["injected"], model, _gallery(H, gallery_rows["rows"], GALLERY_IDS),
                      40.0, float(known_distance[0]))
    assert _compare(oracle_forty, got) >= 30


def test_interval_inf_threshold_below(H, frames, model, oracle_once, gallery_rows, known_distance):
    got = _device_run(H, frames, oracle_once["injected"], model, _gallery(H, gallery_rows["rows"], GALLERY_IDS),
                      math.inf, float(np.nextafter(known_distance[0], f32(0))))
    assert _compare(oracle_once, got) >= 30


def test_recognition_moves_no_bit_of_the_tracking(H, frames, oracle_every):
    """Recognition off on the same script: the tracking the recognition runs compared equal to."""
    off = _device_run(H, frames, oracle_every["injected"])
    assert off["track"] == oracle_every["track"]
    assert all(rec is None for k in range(STEPS) for s in range(S) for _, rec in off["identity"][k][s])
    assert off["images"] == [0] * STEPS


def test_filter_and_pose_unchanged_and_the_crop_follows_the_filtered_landmarks(H, frames, model, embed, oracle_every):
    import procrustes_ref as R
    mesh = R.canonical_mesh()
    g = _gallery(H, [], [])
    runs = [_device_run(H, frames, oracle_every["injected"], m, g, 0.0, None, filt=H.OneEuro(1.0, 0.05), pose=mesh)
            for m in (None, model)]
    assert runs[0]["track"] == runs[1]["track"] and runs[0]["pose"] == runs[1]["pose"]
    assert runs[0]["track"] != oracle_every["track"]  # the filter did move the landmarks
    assert any(p is not None for row in runs[1]["pose"][STEPS - 1] for p in row)
    # objects() reports the landmarks the step consumed -- the filtered ones -- and with interval 0 the
    # embedding was made from them in this step's frame
    checked = 0
    for k in range(1, STEPS):
        for s in range(S):
            for o in runs[1]["objects"][k][s]:
                rect = H.Rect.bounding([(float(p[0]), float(p[1])) for p in o["landmarks"]])
                want = embed(frames[s][k], rect)
                assert o["identity"]["embedding"].tobytes() == want.tobytes(), (k, s, o["id"])
                checked += 1
    assert checked >= 30, checked


def test_set_recognition_resets_and_turns_off(H, frames, model):
    from zaru_amd._lib import DeviceBuffer
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(1e9)
    g = _gallery(H, [], [])
    dev.set_recognition(model, g)
    dev.set_identify_interval(math.inf)
    dev.inject_detections(0, [_det(H, (0.9, (200.0, 180.0, 80.0, 88.0), 0.0))])
    bufs = [DeviceBuffer.from_array(f) for f in frames[0][:6]]

    def step(k):
        dev.step([(bufs[k].ptr, FW, FH, FW * 4)], CLOCK * k)
        dev.synchronize()
        return dev.objects(0)

    assert step(0) == []
    one = step(1)[0]["identity"]
    assert one["embeddings"] == 1 and one["id"] == H.NO_MATCH and dev.identity_images() == 1
    assert step(2)[0]["identity"]["embedding"].tobytes() == one["embedding"].tobytes() and dev.identity_images() == 1
    # again (as after Gallery.clear()): every object starts over and is embedded at the next step
    g.clear()
    g.add(one["embedding"][None], [42])
    dev.set_recognition(model, g)
    assert dev.objects(0)[0]["identity"] is None
    two = step(3)[0]["identity"]
    assert two["embeddings"] == 1 and two["id"] == 42 and dev.identity_images() == 2
    # off: no identity, no more embeddings, the tracking goes on
    dev.set_recognition(b"", None)
    assert step(4)[0]["identity"] is None and dev.identity_images() == 2
    for bad in (lambda: dev.set_identify_interval(-1.0), lambda: dev.set_identify_interval(math.nan),
                lambda: dev.set_identity_crop_grow(-0.5), lambda: dev.set_recognition(b"not a model", g),
                lambda: dev.set_recognition(model, H.Gallery(0, 64))):
        with pytest.raises(RuntimeError):
            bad()
    assert len(step(5)) == 1


# ---- the kernels alone, on synthetic states ------------------------------------------------------------
def _describe(views, frame):
    from zaru_amd import _lib
    v = np.ascontiguousarray(views, f32).reshape(-1, 5)
    out = np.zeros((len(v), 10), np.uint32)
    _lib.check(_lib.lib().zr_view_describe(v.ctypes.data, len(v), frame, out.ctypes.data))
    return out


@pytest.mark.parametrize("Kc", [1, 4])
@pytest.mark.parametrize("L", [1, 21, 64, 65, 468])
def test_select_alone(H, L, Kc):
    from zaru_amd import _lib
    lib = _lib.lib()
    Sc = 5
    n = Sc * Kc
    W, Hh, aw, ah, grow, now = 640, 480, 4, 3, 0.4, 100.0
    rng = np.random.default_rng(1000 + 10 * L + Kc)
    lm = np.c_[rng.uniform(-100, 800, n * L), rng.uniform(-80, 600, n * L), rng.uniform(-9, 9, n * L)]
    lm = np.ascontiguousarray(lm, f32).reshape(n, L, 3)
    lm[..., 2].flat[::7] = np.nan      # z is never looked at
    st = (_lib.TrackState * n)()
    for i in range(n):
        st[i].tracked, st[i].active, st[i].frame_w, st[i].frame_h = 1, 1, W, Hh
    src = rng.integers(0, Kc, n).astype(np.int32)
    sin = np.zeros(n, np.dtype(_lib.IdentityState))
    sin["row"], sin["distance"] = rng.integers(0, 50, n), rng.uniform(0, 2, n)
    sin["embeddings"] = rng.integers(1, 9, n)
    sin["next_ms"] = np.where(rng.random(n) < 0.5, now - 1.0, now + 1.0)   # due, not yet due
    ein = rng.standard_normal((n, 128)).astype(f32)
    # the special rows
    r = list(range(n))
    st[r[0]].tracked = 0                           # not tracked: default state, not due
    lm[r[1], L - 1, 1] = np.nan                    # a NaN in the last landmark: carried, not due
    sin["next_ms"][(r[1] // Kc) * Kc + src[r[1]]] = now - 1.0
    src[r[2]], src[r[3]] = -1, Kc                  # new objects: default state, due
    lm[r[4], :, :2] = (300.25, 200.5)              # all points equal: w = h = 0
    sin["next_ms"][(r[4] // Kc) * Kc + src[r[4]]] = now   # now >= next: due at equality
    sin["embeddings"][(r[n - 1] // Kc) * Kc + src[r[n - 1]]] = 0   # never embedded: due whatever next_ms says
    sin["next_ms"][(r[n - 1] // Kc) * Kc + src[r[n - 1]]] = now + 50.0
    cfg = _lib.IdentityCfg(Kc, L, aw, ah, grow, math.inf, 1000.0)
    d = {k: _lib.DeviceBuffer.from_array(v) for k, v in (
        ("st", np.frombuffer(bytes(st), np.uint8)), ("lm", lm), ("src", src), ("sin", sin), ("ein", ein),
        ("sout", np.full(n * 24, 0xA5, np.uint8)), ("eout", np.full((n, 128), 7.0, f32)),
        ("due", np.full(n, 9, np.int32)), ("views", np.full((n, 10), 0xA5A5A5A5, np.uint32)))}
    _lib.check(lib.zr_identity_select_async(C.byref(cfg), d["st"].ptr, n, d["lm"].ptr, d["src"].ptr, now, d["sin"].ptr,
                                            d["ein"].ptr, d["sout"].ptr, d["eout"].ptr, d["due"].ptr, d["views"].ptr,
                                            None))
    _lib.synchronize()
    sout = d["sout"].download((n,), np.dtype(_lib.IdentityState))
    eout, due = d["eout"].download((n, 128), f32), d["due"].download((n,), np.int32)
    views = d["views"].download((n, 10), np.uint32)
    default = np.zeros(1, np.dtype(_lib.IdentityState))
    default["row"], default["distance"] = -1, np.inf
    n_due = 0
    for i in range(n):
        tracked = st[i].tracked != 0
        have = tracked and 0 <= src[i] < Kc
        j = (i // Kc) * Kc + src[i]
        want_s = sin[j:j + 1] if have else default
        assert sout[i:i + 1].tobytes() == want_s.tobytes(), ("state", i)
        assert eout[i].tobytes() == (ein[j] if have else np.zeros(128, f32)).tobytes(), ("embedding", i)
        want_due = bool(tracked and (want_s["embeddings"][0] == 0 or now >= want_s["next_ms"][0])
                        and np.isfinite(lm[i, :, :2]).all())
        assert due[i] == int(want_due), ("due", i, due[i], want_due)
        if want_due:
            v = H.landmark_crop_view(lm[i], W, Hh, aw, ah, grow).zr_view()
            assert views[i].tobytes() == _describe([v], i // Kc)[0].tobytes(), ("view", i, views[i].view(f32)[:8], v)
            n_due += 1
        else:
            assert (views[i] == 0xA5A5A5A5).all(), ("a view written for a row that is not due", i)
    assert due[r[0]] == 0 and due[r[1]] == 0 and due[r[2]] == 1 and due[r[3]] == 1 and due[r[4]] == 1
    assert due[n - 1] == 1 and n_due < n


@pytest.mark.parametrize("case", ["none", "all", "mixed"])
def test_compact_alone(case):
    from zaru_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(31)
    n = {"none": 130, "all": 70, "mixed": 2500}[case]   # mixed: past two 1024-row chunks, no multiple of 64
    if case == "none":
        due = np.zeros(n, np.int32)
    elif case == "all":
        due = np.ones(n, np.int32)
    else:
        due = (rng.random(n) < 0.55).astype(np.int32)   # ~1375 due: the count crosses a chunk of rows too
        due[0] = due[-1] = 1
        due[100:300] = 0
        due[1000:1100] = 1
        due[2040:2060] = 5                               # any non-zero flag counts
    views = rng.integers(1, 2 ** 31, (n, 10), dtype=np.int64).astype(np.uint32)
    sentinel = np.full((n, 10), 0xA5A5A5A5, np.uint32)
    b = _lib.DeviceBuffer.from_array
    d_due, d_views, d_dense = b(due), b(views), b(sentinel)
    d_of, d_valid = b(np.full(n, 77, np.int32)), b(np.full(n, 77, np.int32))
    d_n, d_total = b(np.array([-5], np.int32)), b(np.array([1000], np.uint64))
    _lib.check(lib.zr_identity_compact_async(d_due.ptr, d_views.ptr, n, d_dense.ptr, d_of.ptr, d_n.ptr, d_valid.ptr,
                                             d_total.ptr, None))
    _lib.synchronize()
    rows = np.flatnonzero(due)
    m = len(rows)
    want_of = np.full(n, -1, np.int32)
    want_of[rows] = np.arange(m)
    assert d_n.download((1,), np.int32)[0] == m and d_total.download((1,), np.uint64)[0] == 1000 + m
    assert np.array_equal(d_of.download((n,), np.int32), want_of)
    assert np.array_equal(d_valid.download((n,), np.int32), (np.arange(n) < m).astype(np.int32))
    got = d_dense.download((n, 10), np.uint32)
    assert np.array_equal(got[:m], views[rows]) and np.array_equal(got[m:], sentinel[m:])
    if case == "mixed":
        assert m > 1024
    # without the running total
    _lib.check(lib.zr_identity_compact_async(d_due.ptr, d_views.ptr, n, d_dense.ptr, d_of.ptr, d_n.ptr, d_valid.ptr,
                                             None, None))
    _lib.synchronize()
    assert d_n.download((1,), np.int32)[0] == m and d_total.download((1,), np.uint64)[0] == 1000 + m


@pytest.mark.parametrize("threshold", [math.inf, 0.75, float(np.nextafter(f32(0.75), f32(0))), math.nan])
def test_commit_alone(threshold):
    """Rows 0..5 are due in this order of packed images: 2, 0, 3, 1, 4, 5; rows 6, 7 are not."""
    from zaru_amd import _lib
    lib = _lib.lib()
    n, now, interval = 8, 60.0, 40.0
    rng = np.random.default_rng(8)
    of = np.array([2, 0, 3, 1, 4, 5, -1, -1], np.int32)
    best = np.array([5, -1, 9, 3, 8, 2, 1, 1], np.int32)                  # by packed image
    dist = np.array([0.5, np.inf, 0.75, 1.25, np.nan, 0.0, 0.1, 0.1], f32)
    dense = rng.standard_normal((n, 128)).astype(f32)
    sout = np.zeros(n, np.dtype(_lib.IdentityState))
    sout["row"], sout["distance"], sout["embeddings"] = 11, 3.0, np.arange(n)
    sout["next_ms"] = 5.0
    eout = rng.standard_normal((n, 128)).astype(f32)
    cfg = _lib.IdentityCfg(4, 468, 1, 1, 0.4, threshold, interval)
    b = _lib.DeviceBuffer.from_array
    d_of, d_best, d_dist, d_dense, d_s, d_e = b(of), b(best), b(dist), b(dense), b(sout), b(eout)
    _lib.check(lib.zr_identity_commit_async(C.byref(cfg), n, d_of.ptr, d_best.ptr, d_dist.ptr, d_dense.ptr, now,
                                            d_s.ptr, d_e.ptr, None))
    _lib.synchronize()
    got_s, got_e = d_s.download((n,), np.dtype(_lib.IdentityState)), d_e.download((n, 128), f32)
    for i in range(n):
        k = of[i]
        if k < 0:
            assert got_s[i:i + 1].tobytes() == sout[i:i + 1].tobytes() and got_e[i].tobytes() == eout[i].tobytes()
            continue
        known = best[k] >= 0 and float(dist[k]) <= threshold   # False for a NaN on either side
        assert got_s["row"][i] == (best[k] if known else -1), (i, got_s["row"][i])
        assert got_s["distance"][i:i + 1].tobytes() == dist[k:k + 1].tobytes()
        assert got_s["embeddings"][i] == sout["embeddings"][i] + 1 and got_s["next_ms"][i] == now + interval
        assert got_e[i].tobytes() == dense[k].tobytes()
    # row 0 took image 2 (distance 0.75), row 1 image 0 (0.5), row 5 image 5 (0.0): <= is known
    assert got_s["row"][0] == (9 if threshold >= 0.75 else -1)
    assert (got_s["row"][1], got_s["row"][5]) == ((-1, -1) if math.isnan(threshold) else (5, 2))
    assert got_s["row"][3] == -1 and got_s["row"][4] == -1   # no row; a NaN distance


def test_refusals_launch_nothing(H, model):
    """Bad arguments with real device buffers: ZR_ERR_INVALID_ARGUMENT, and no buffer is touched."""
    from zaru_amd import _lib
    lib = _lib.lib()
    n = 8
    buf = _lib.DeviceBuffer.from_array(np.full(n * 128 * 4, 0x5A, np.uint8))
    other = _lib.DeviceBuffer.from_array(np.full(n * 128 * 4, 0x5A, np.uint8))
    p, q = buf.ptr, other.ptr
    ok = _lib.IdentityCfg(4, 2, 1, 1, 0.4, math.inf, 1000.0)
    calls = [
        lambda c=ok, nn=n, a=p: lib.zr_identity_select_async(C.byref(c), a, nn, p, p, 0.0, p, p, q, q, p, p, None),
        lambda c=ok, nn=n, a=p: lib.zr_identity_commit_async(C.byref(c), nn, a, p, p, p, 0.0, q, q, None),
    ]
    for call in calls:
        assert call(a=None) == -1 and call(nn=0) == -1
        for slots in (0, 65):
            assert call(c=_lib.IdentityCfg(slots, 2, 1, 1, 0.4, math.inf, 1000.0)) == -1
    assert lib.zr_identity_compact_async(None, p, n, q, p, p, p, None, None) == -1
    assert lib.zr_identity_compact_async(p, p, 0, q, p, p, p, None, None) == -1
    _lib.synchronize()
    for b in (buf, other):
        assert (b.download((n * 128 * 4,), np.uint8) == 0x5A).all()
