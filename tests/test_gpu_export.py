"""Every stream's tracked objects as one packed batch: zr_multi_export_async alone against
tests/export_ref.py (bit for bit, on any payload), and DeviceMultiTracker.snapshot() /
objects_packed() against the tracker's own objects(s) -- the yardstick -- over short sequences of
every configuration: split by stream_offsets the packed arrays must equal [objects(s) for s], a
snapshot must hold a step's results while later steps run, and a tracker that never calls the new
methods must report what one that calls them every step reports."""
import ctypes as C
import os

import numpy as np
import pytest

import export_ref as XR

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SENT = 0xA5A5A5A5
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


# ---- the kernel alone --------------------------------------------------------------------------------
def _words(rng, *shape):
    """Any bits: NaN patterns, denormals, the sentinel's neighbours."""
    return rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(u32)


def _kernel_inputs(S, K, L, seed, all_zero=False):
    from zaru_amd import _lib
    rng = np.random.default_rng(seed)
    rows = S * K
    nobjects = np.zeros(S, np.int32) if all_zero else rng.integers(-2, K + 3, S).astype(np.int32)
    src = rng.integers(-1, K + 1, rows).astype(np.int32)
    tdt, idt = np.dtype(_lib.TrackState), np.dtype(_lib.IdentityState)
    assert tdt.itemsize == 92 and tdt.fields["confidence"][1] == 68 and idt.itemsize == 24
    state = _words(rng, rows, 23)
    ist_words = _words(rng, rows, 6)
    ist_words[:, 2] = rng.choice(np.array([0, 0, 1, 5, 2 ** 31], u32), rows)   # embeddings: 0 = not embedded yet
    ist = np.zeros(rows, XR.IDENT)
    ist["row"] = ist_words[:, 0].view(np.int32)
    ist["distance"], ist["embeddings"], ist["flags"] = ist_words[:, 1], ist_words[:, 2], ist_words[:, 3]
    host = dict(ids=rng.integers(0, 2 ** 63, rows, dtype=np.uint64), roi=_words(rng, rows, 5),
                confidence=np.ascontiguousarray(state[:, 17]), lm=_words(rng, rows, 3 * L), pose=_words(rng, rows, 21),
                ist=ist, emb=_words(rng, rows, 128),
                eye_valid=rng.choice(np.array([0, 1, 1, -3], np.int32), 2 * rows), eye_diam=_words(rng, 2 * rows),
                eye_crop=_words(rng, 2 * rows, 5), eye_lm=_words(rng, 2 * rows, 228))
    return nobjects, src, host, state, ist_words


GROUPS = {"pose": ("pose",), "identity": ("ist", "emb"), "eyes": ("eye_valid", "eye_diam", "eye_crop", "eye_lm")}


def _run_kernel(S, K, L, groups, seed, all_zero=False, misalign=0):
    """The outputs are regions of one sentinel-filled arena with guard gaps between them, the regions
    of the groups that are off included (but not passed): whatever the launch writes outside the
    first `count` records of the arrays it was given shows as a changed word."""
    from zaru_amd import _lib
    lib = _lib.lib()
    nobjects, src, host, state, ist_words = _kernel_inputs(S, K, L, seed, all_zero)
    rows = S * K
    keep = []

    def dev(a):
        keep.append(_lib.DeviceBuffer.from_array(a))
        return keep[-1].ptr

    sizes = [("count", 1), ("offsets", S + 1), ("header", rows * 12), ("lm", rows * 3 * L), ("pose", rows * 21),
             ("ident", rows * 4), ("emb", rows * 128), ("eye_valid", 2 * rows), ("eye_diam", 2 * rows),
             ("eye_crop", 2 * rows * 5), ("eye_lm", 2 * rows * 228)]
    at, total = {}, 64
    for name, n in sizes:
        at[name] = total + (misalign if name == "lm" else 0)
        total += (n + misalign + 63) // 64 * 64 + 64     # 256-byte aligned regions, 256 bytes of guard
    arena = _lib.DeviceBuffer.from_array(np.full(total, SENT, u32))
    out = lambda name: arena.ptr + 4 * at[name]
    a = _lib.MultiExportArgs()
    a.d_nobjects, a.d_src, a.d_ids, a.d_roi = dev(nobjects), dev(src), dev(host["ids"]), dev(host["roi"])
    a.d_state, a.d_landmarks = dev(state), dev(host["lm"])
    a.d_count, a.d_stream_offsets, a.d_header, a.d_out_landmarks = out("count"), out("offsets"), out("header"), out("lm")
    if "pose" in groups:
        a.d_pose, a.d_out_pose = dev(host["pose"]), out("pose")
    if "identity" in groups:
        a.d_id_state, a.d_id_emb, a.d_out_identity, a.d_out_emb = dev(ist_words), dev(host["emb"]), out("ident"), out("emb")
    if "eyes" in groups:
        a.d_eye_valid, a.d_eye_diam, a.d_eye_crop, a.d_eye_lm = (dev(host["eye_valid"]), dev(host["eye_diam"]),
                                                                 dev(host["eye_crop"]), dev(host["eye_lm"]))
        a.d_out_eye_valid, a.d_out_eye_diam, a.d_out_eye_crop, a.d_out_eye_lm = (out("eye_valid"), out("eye_diam"),
                                                                                 out("eye_crop"), out("eye_lm"))
    _lib.check(lib.zr_multi_export_async(C.byref(a), S, K, L, None))
    _lib.synchronize()
    got = arena.download((total,), u32)
    args = {k: v for k, v in host.items() if k in ("ids", "roi", "confidence", "lm")}
    for g in groups:
        args.update({k: host[k] for k in GROUPS[g]})
    ref = XR.export(K, nobjects, src, **args)
    want = np.full(total, SENT, u32)

    def put(name, values):
        w = np.ascontiguousarray(values).view(u32).reshape(-1)
        want[at[name]:at[name] + len(w)] = w

    put("count", np.array([ref["count"]], np.int32))
    put("offsets", ref["offsets"])
    for name in ("header", "lm", "pose", "ident", "emb", "eye_valid", "eye_diam", "eye_crop", "eye_lm"):
        if name in ref and ref["count"]:
            put(name, ref[name])
    return got, want, ref, at


@pytest.mark.parametrize("S,K,L,groups,misalign", [
    (3, 4, 21, (), 0),                                  # under one wavefront; rows not 16-byte aligned
    (300, 5, 468, ("pose", "identity", "eyes"), 0),     # 1,500 rows: past one 1,024 chunk, no multiple of 64
    (1100, 2, 21, ("pose",), 0),                        # stream count past one 1,024-stream chunk of the scan
    (2, 3, 468, ("identity", "eyes"), 1),               # aligned row length, unaligned base: the dword path
])
def test_kernel_alone(S, K, L, groups, misalign):
    got, want, ref, at = _run_kernel(S, K, L, groups, seed=S + L, misalign=misalign)
    assert got[at["count"]] == ref["count"] and ref["count"] > 0
    assert np.array_equal(got[at["offsets"]:at["offsets"] + S + 1].view(np.int32), ref["offsets"])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], [n for n, o in at.items() if o <= bad[0]][-1])
    flags = ref["header"]["flags"]
    if "identity" in groups:   # the case holds embedded and not yet embedded objects
        assert (flags & XR.IDENTITY).any() and not (flags & XR.IDENTITY).all()
    if "eyes" in groups:
        assert (flags & XR.EYE_LEFT).any() and not (flags & XR.EYE_LEFT).all()
    if S >= 300:               # skipped slots inside streams, so the order is not the slots' own
        assert ref["count"] < S * K and (ref["header"]["slot"] > 0).any()


def test_kernel_alone_nothing_to_export():
    S, K = 70, 4
    got, want, ref, at = _run_kernel(S, K, 21, ("pose", "identity", "eyes"), seed=9, all_zero=True)
    assert ref["count"] == 0 and got[at["count"]] == 0
    assert not got[at["offsets"]:at["offsets"] + S + 1].any()
    assert np.array_equal(got, want)   # count and offsets apart, every word is still the sentinel


# ---- the loop ----------------------------------------------------------------------------------------
FW, FH = 480, 360
S, K, STEPS = 3, 4, 6
# tests/test_gpu_multi_tracker.py's scripts: per step, per stream (confidence, (cx, cy, w, h), angle)
FACE_SCRIPT = {
    0: {0: [(0.9, (200.0, 180.0, 80.0, 88.0), 0.3), (0.8, (60.0, 290.0, 60.0, 60.0), 0.0)],
        1: [(0.9, (100.0, 100.0, 60.0, 60.0), 0.0), (0.8, (104.0, 101.0, 60.0, 60.0), 0.1)],
        2: [(0.9, (300.0, 200.0, 100.0, 80.0), -0.2), (0.7, (120.0, 260.0, 72.0, 72.0), 0.5),
            (0.8, (400.0, 80.0, 64.0, 64.0), 0.0)]},
    2: {1: [(0.6, (330.0, 250.0, 88.0, 88.0), 1.0)]},
    4: {2: [(0.9, (300.0, 300.0, 60.0, 60.0), 0.0)]},
}
HAND_SCRIPT = {
    0: {0: [(0.9, (200.0, 180.0, 40.0, 44.0), 0.3), (0.8, (60.0, 290.0, 30.0, 30.0), 0.0)],
        1: [(0.9, (100.0, 100.0, 30.0, 30.0), 0.0), (0.8, (104.0, 101.0, 30.0, 30.0), 0.1)],
        2: [(0.9, (300.0, 200.0, 50.0, 40.0), -0.2), (0.7, (120.0, 260.0, 36.0, 36.0), 0.5),
            (0.8, (400.0, 80.0, 32.0, 32.0), 0.0)]},
    2: {1: [(0.6, (330.0, 250.0, 44.0, 44.0), 1.0)]},
    4: {2: [(0.9, (300.0, 300.0, 30.0, 30.0), 0.0)]},
}
GALLERY_IDS = [7, 1000, 2 ** 40 + 3]
FIRST_ID = 5000
# feature switches per configuration
CONFIGS = {
    "plain": (),
    "filter_pose": ("filter", "pose"),
    "recognition": ("recognition",),
    "eyes": ("eyes",),
    "hand": ("hand",),
    "all": ("filter", "pose", "recognition", "eyes"),
}


@pytest.fixture(scope="module")
def frames():
    from zaru_amd._lib import DeviceBuffer
    rng = np.random.default_rng(61)
    return [DeviceBuffer.from_array(rng.integers(0, 256, (S, FH, FW, 4), dtype=np.uint8)) for _ in range(STEPS)]


@pytest.fixture(scope="module")
def model():
    import recognition_util as RU
    return RU.model_bytes(GOLDEN)


def _make(H, config, model):
    """The tracker of a configuration; never loses an object until the test says so."""
    on = CONFIGS[config]
    dev = H.DeviceMultiTracker("palm", "hand", S, K) if "hand" in on else H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    keep = None
    if "filter" in on:
        dev.set_filter(H.Ema(0.5))
    if "pose" in on:
        import procrustes_ref as R
        dev.set_pose_reference(R.canonical_mesh())
    if "recognition" in on:
        # three rows nothing matches, and a threshold only equal bits pass: every object is unknown at its
        # first embedding and is enrolled, so person ids come from rows the steps appended
        keep = H.Gallery()
        keep.add(np.random.default_rng(78).standard_normal((3, 128)).astype(f32), GALLERY_IDS)
        keep.reserve(32)
        dev.set_recognition(model, keep)
        dev.set_identify_interval(20.0)
        dev.set_identity_threshold(1e-6)
        dev.set_enrolment(keep, FIRST_ID)
    if "eyes" in on:
        dev.set_eye_refinement(True)
    return dev, keep


def _rect5(r):
    return np.array([*r.rect().tuple(), r.rotation_radians()], f32).tobytes()


def _from_objects(o):
    """One entry of objects(s) as comparable values: floats as their bits, absent fields absent."""
    rec = {"id": int(o["id"]), "view_rect": _rect5(o["view_rect"]), "confidence": f32(o["confidence"]).tobytes(),
           "landmarks": np.ascontiguousarray(o["landmarks"], f32).tobytes(), "identity": None, "eyes": None}
    if "pose" in o:
        rec["pose"] = np.ascontiguousarray(o["pose"], f32).tobytes()
    if o["identity"] is not None:
        i = o["identity"]
        rec["identity"] = (int(i["id"]), f32(i["distance"]).tobytes(), int(i["embeddings"]),
                           np.ascontiguousarray(i["embedding"], f32).tobytes(), bool(i["enrolled"]))
    if o["eyes"] is not None:
        rec["eyes"] = tuple(None if e is None else (np.ascontiguousarray(e["landmarks"], f32).tobytes(),
                                                    f32(e["iris_diameter"]).tobytes(), _rect5(e["crop"]))
                            for e in (o["eyes"]["left"], o["eyes"]["right"]))
    return rec


def _from_packed(p, n_streams=S):
    """objects_packed()'s dict split by stream_offsets into objects(s)'s shape; checks the dict's own
    invariants on the way (shapes, order, zeros where a part is absent)."""
    c, off = int(p["count"]), p["stream_offsets"]
    assert off.shape == (n_streams + 1,) and off[0] == 0 and off[-1] == c and (np.diff(off) >= 0).all()
    L = p["landmarks"].shape[1]
    assert p["landmarks"].shape == (c, L, 3) and p["view_rect"].shape == (c, 5)
    for name in ("stream", "slot", "id", "flags", "confidence"):
        assert p[name].shape == (c,), name
    assert ("pose" in p) == bool(c and (p["flags"] & XR.POSE).all()) or c == 0
    out = []
    for s in range(n_streams):
        rows = range(off[s], off[s + 1])
        assert all(p["stream"][k] == s for k in rows)
        assert all(p["slot"][a] < p["slot"][b] for a, b in zip(rows, rows[1:]))   # slot order
        objs = []
        for k in rows:
            rec = {"id": int(p["id"][k]), "view_rect": p["view_rect"][k].tobytes(), "confidence": p["confidence"][k].tobytes(),
                   "landmarks": p["landmarks"][k].tobytes(), "identity": None, "eyes": None}
            if "pose" in p:
                assert p["pose"].shape == (c, 21)
                rec["pose"] = p["pose"][k].tobytes()
            if "identity_id" in p:
                assert p["embedding"].shape == (c, 128)
                present = bool(p["identity_present"][k])
                assert present == bool(p["flags"][k] & XR.IDENTITY) == (p["identity_embeddings"][k] > 0)
                if present:
                    rec["identity"] = (int(p["identity_id"][k]), p["identity_distance"][k].tobytes(),
                                       int(p["identity_embeddings"][k]), p["embedding"][k].tobytes(),
                                       bool(p["identity_enrolled"][k]))
                else:   # absent: zeros, and no person
                    assert p["identity_id"][k] == 2 ** 64 - 1 and not p["embedding"][k].view(u32).any()
                    assert p["identity_distance"][k].tobytes() == bytes(4) and not p["identity_enrolled"][k]
            if "eye_valid" in p:
                assert p["eye_landmarks"].shape == (c, 2, 76, 3) and p["eye_crop"].shape == (c, 2, 5)
                eyes = []
                for side in range(2):
                    valid = int(p["eye_valid"][k, side])
                    assert valid in (0, 1) and valid == bool(p["flags"][k] & (XR.EYE_RIGHT if side else XR.EYE_LEFT))
                    if valid:
                        eyes.append((p["eye_landmarks"][k, side].tobytes(), p["iris_diameter"][k, side].tobytes(),
                                     p["eye_crop"][k, side].tobytes()))
                    else:
                        eyes.append(None)
                        assert not p["eye_landmarks"][k, side].view(u32).any() and not p["eye_crop"][k, side].view(u32).any()
                        assert p["iris_diameter"][k, side].tobytes() == bytes(4)
                rec["eyes"] = tuple(eyes)
            objs.append(rec)
        out.append(objs)
    return out


def _det(H, d):
    conf, (cx, cy, w, h), angle = d
    return H.Detection(conf, H.Rect.from_center(cx, cy, w, h), angle)


def _counters(dev):
    return (dev.landmark_images(), dev.detector_frames(), dev.identity_images(), dev.eye_images())


def _run(H, frames, model, config, loss_at=None, packed="every", steps=STEPS):
    """packed: "every" (objects_packed() after every step, beside objects(s)), "never" (objects(s) only),
    or a step t: snapshot() after step t, two more steps enqueued at once, then objects_packed()."""
    dev, gallery = _make(H, config, model)
    script = HAND_SCRIPT if "hand" in CONFIGS[config] else FACE_SCRIPT
    fb = FH * FW * 4
    out = {"objects": [], "packed": [], "raw": [], "counters": [], "counts": [], "dev": dev, "gallery": gallery}

    def step(k):
        for s, dets in script.get(k, {}).items():
            dev.inject_detections(s, [_det(H, d) for d in dets])
        if loss_at is not None:
            dev.set_loss_threshold(loss_at[1] if k == loss_at[0] else -1.0)
        dev.step([(frames[k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)], 15.0 * k)

    k = 0
    while k < steps:
        step(k)
        if packed == k:
            dev.snapshot()
            step(k + 1)
            step(k + 2)
            out["snapshot"] = _from_packed(dev.objects_packed())
            k += 2
        if packed == "every":
            raw = dev.objects_packed()
            out["raw"].append(raw)
            out["packed"].append(_from_packed(raw))
        dev.synchronize()
        out["counts"].append(dev.object_counts())
        out["objects"].append([[_from_objects(o) for o in dev.objects(s)] for s in range(S)])
        out["counters"].append(_counters(dev))
        k += 1
    return out


def _pick_loss(calm):
    """From a run that loses nothing: a step and a threshold that make an object leave while a later
    slot's object of its stream stays (an object is lost when its confidence < threshold), so the
    survivor moves down a slot and its results sit in the slot it left."""
    for k in range(2, STEPS):
        raw, before = calm["raw"][k], calm["packed"][k - 1]
        off, conf = raw["stream_offsets"], raw["confidence"]
        for s in range(S):
            c, ids = conf[off[s]:off[s + 1]], raw["id"][off[s]:off[s + 1]]
            seen = {o["id"] for o in before[s]}   # reported a step earlier too, so its slot then is known
            for i in range(len(c)):
                for j in range(i + 1, len(c)):
                    if c[i] < c[j] and int(ids[j]) in seen:
                        return k, float(c[j])
    return None


@pytest.mark.parametrize("config", ["plain", "filter_pose", "recognition", "eyes", "hand"])
def test_loop_equals_objects(H, frames, model, config):
    """After every step objects_packed() split by stream_offsets == [objects(s) for s], bit for bit and
    field for field, over a sequence that starts with nothing to report and holds a step in which an
    object leaves and a survivor changes slot."""
    calm = _run(H, frames, model, config)
    loss = _pick_loss(calm)
    assert loss is not None, "no step of the calm run has a less confident object ahead of a more confident one"
    run = _run(H, frames, model, config, loss_at=loss)
    on = CONFIGS[config]
    moved = compared = identified = enrolled = eyes_valid = 0
    where = {}
    for k in range(STEPS):
        raw = run["raw"][k]
        assert run["packed"][k] == run["objects"][k], (config, k)
        if k == 0:   # objects started, none with a result: src is -1 everywhere
            assert raw["count"] == 0 and not raw["stream_offsets"].any() and sum(run["counts"][0]) >= 5
        # absent features are absent keys: objects() reports them from the second step on
        assert ("pose" in raw) == ("pose" in on and k >= 1), (config, k)
        assert ("identity_id" in raw) == ("recognition" in on and k >= 1), (config, k)
        assert ("eye_valid" in raw) == ("eyes" in on and k >= 1), (config, k)
        assert raw["landmarks"].shape[1] == (21 if "hand" in on else 468)
        now = {}
        for s in range(S):
            for o, slot in zip(run["packed"][k][s], raw["slot"][raw["stream_offsets"][s]:raw["stream_offsets"][s + 1]]):
                now[(s, o["id"])] = int(slot)
                moved += (s, o["id"]) in where and where[(s, o["id"])] != int(slot)
                compared += 1
                identified += o["identity"] is not None
                enrolled += o["identity"] is not None and o["identity"][4] and o["identity"][0] >= FIRST_ID
                eyes_valid += o["eyes"] is not None and sum(e is not None for e in o["eyes"])
        where = now
    print(config, "loss at", loss, "records compared:", compared, "slot changes:", moved, "identified:", identified,
          "enrolled:", enrolled, "valid eyes:", eyes_valid)
    assert compared >= 15, compared
    # an object whose slot differs from the one it reported from a step earlier: src[j] != j
    assert moved >= 1, "no survivor changed its slot"
    assert sum(len(o) for o in run["objects"][loss[0]]) < sum(len(o) for o in calm["objects"][loss[0]])
    if "recognition" in on:
        assert identified >= 5 and enrolled >= 3, (identified, enrolled)
    if "eyes" in on:
        assert eyes_valid >= 5, eyes_valid


@pytest.fixture(scope="module")
def untouched(H, frames, model):
    """The everything-on tracker that never calls the new methods."""
    return _run(H, frames, model, "all", packed="never")


def test_snapshot_isolation(H, frames, model, untouched):
    """snapshot() after step t, steps t + 1 and t + 2 enqueued behind it, and only then objects_packed():
    the records are step t's; objects(s) afterwards are step t + 2's."""
    t = 2
    a = _run(H, frames, model, "all", packed=t, steps=t + 3)
    assert sum(len(o) for o in untouched["objects"][t]) >= 5
    assert a["snapshot"] == untouched["objects"][t]
    assert untouched["objects"][t] != untouched["objects"][t + 2]
    assert a["objects"][-1] == untouched["objects"][t + 2]
    assert a["counters"][-1] == untouched["counters"][t + 2]


def test_off_means_off(H, frames, model, untouched):
    """A tracker that calls objects_packed() after every step reports, over the same sequence, the same
    objects(s) and the same counters as one that never calls it."""
    every = _run(H, frames, model, "all")
    assert every["objects"] == untouched["objects"]
    assert every["counters"] == untouched["counters"]
    assert every["counts"] == untouched["counts"]
    assert every["packed"] == untouched["objects"]
    assert untouched["counters"][-1][2] > 0 and untouched["counters"][-1][3] > 0   # recognition and eyes ran
