"""Aligned identity crops inside DeviceMultiTracker (set_identity_alignment), against
tests/multi_align_ref.py's MultiAlignRef at every step, stream and object, bit for bit: tracking, identity,
embedding, the quality record, the gallery's rows and sample counts, and the counters.

The script is tests/test_gpu_multi_quality.py's: S = 2 streams of K = 3 slots, 10 steps of 480 x 360 frames
15 ms apart, every object embedded at every step (identify interval 0), injected detections, the golden
MobileFaceNet, enrolment, gallery refinement and the quality gate on.  The oracle crops with
aligned_crop_view -- which tests/test_align_cpu.py pins to the numpy restatement -- falling back to
landmark_crop_view, and embeds with FaceEmbedder.embed_views.

The settings come from a run with max_residual = +inf and every quality minimum -inf (`setup`): alignment
changes neither the tracking nor which objects are due at an interval of 0, so that run fits exactly the
landmarks the other runs will.
  max_residual: the midpoint between the two middle residuals it observed, so about half the rows fall back;
  embed tier:   min_sharpness 0.5 -- the flat stream's sharpness is exactly 0, noise is in the thousands;
  learn tier:   min_size between the two middle sizes stream 0's crops will have under that max_residual (an
                aligned crop's size is scale x 112, a bounding crop's its shorter side; the setup run saw
                both views of every row), so some looks teach and some are held back.
test_script_contains_the_cases asserts the outcome instead of assuming it."""
import math

import numpy as np
import pytest

import align_ref as AR
import multi_align_ref as MA
import multi_enrol_ref as ER
import multi_tracker_ref as MR
import quality_ref as QR
import recognition_util as RU
import test_gpu_multi_identity as TI
import test_gpu_multi_quality as TQ
import test_gpu_multi_template as TT

pytestmark = pytest.mark.gpu

f32 = np.float32
S, K, STEPS, CLOCK, FW, FH = TQ.S, TQ.K, TQ.STEPS, TQ.CLOCK, TQ.FW, TQ.FH


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


@pytest.fixture(scope="module")
def frames():
    flat = np.empty((FH, FW, 4), np.uint8)
    flat[...] = (120, 90, 60, 255)
    noise = TI._noise(1, 30)[0]
    noise[..., 3] = 255
    return [[noise.copy() for _ in range(STEPS)], [flat.copy() for _ in range(STEPS)]]


@pytest.fixture(scope="module")
def model():
    return RU.model_bytes(TI.GOLDEN)


@pytest.fixture(scope="module")
def embedder(H, model):
    return H.FaceEmbedder(model), {}   # and the cache of embedded views the oracle runs share


@pytest.fixture(scope="module")
def gallery_rows():
    return np.random.default_rng(78).standard_normal((3, 128)).astype(f32)


def _alignment(H, max_residual):
    a = H.FaceAlignment.facemesh_five_point()
    a.max_residual = max_residual
    return a


def _oracle_run(H, frames, embedder, rows, max_residual, tiers, off_from=None, steps=STEPS):
    """max_residual None: alignment never on.  off_from: the step before which alignment is switched off."""
    measured = {}

    def measure(frame, view, pose):
        key = (id(frame), view.zr_view())
        if key not in measured:
            measured[key] = H.face_quality(frame, view, 112, 112)
        return dict(measured[key])   # no pose reference is set: frontal is NaN

    trackers = []
    for s in range(S):
        t = MR.MultiTrackerRef(H, "face", "facemesh", K)
        t.loss, t.interval = -1.0, 40.0
        trackers.append(t)
    gal = ER.GalleryRef(TQ.CAPACITY, rows, TQ.GALLERY_IDS, TQ.FIRST_ID)
    crops = MA.AlignedCrops(H, embedder[0], None if max_residual is None else _alignment(H, max_residual), FW, FH,
                            cache=embedder[1])
    ref = MA.MultiAlignRef(H, trackers, crops, TT._make_match(H), gal, embed_tier=tiers[0], learn_tier=tiers[1],
                           measure=measure, interval=0.0, threshold=TQ.THRESHOLD, refine=True,
                           max_samples=TQ.MAX_SAMPLES, enrol=True)
    out = {"track": [], "identity": [], "quality": [], "counters": [], "ref": ref, "gallery": gal, "crops": crops}
    for k in range(steps):
        if off_from is not None and k == off_from:
            crops.alignment = None
        ref.step([frames[s][k] for s in range(S)], CLOCK * k, [[TI._det(H, d) for d in dets] for dets in TQ._injected(k)])
        out["track"].append([TI._track_record(
            [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
              "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in trackers[s].objects()],
            len(trackers[s].objs), trackers[s].pending) for s in range(S)])
        objs = [ref.objects(s) for s in range(S)]
        out["identity"].append([[(o.id, TT.TE._record(i, i and i["flags"] & ER.ENROLLED)) for o, i, _ in objs[s]]
                                for s in range(S)])
        out["quality"].append([[(o.id, TQ._quality_record(q)) for o, _, q in objs[s]] for s in range(S)])
        out["counters"].append((ref.images, ref.measured, ref.rejected, ref.held_back, gal.enrolled_total,
                                ref.refined_total, crops.aligned, crops.fallbacks))
    return out


def _device_run(H, frames, model, rows, max_residual, tiers, off_from=None, steps=STEPS):
    from zaru_amd._lib import DeviceBuffer
    gallery = TI._gallery(H, rows, TQ.GALLERY_IDS)
    gallery.reserve(TQ.CAPACITY)
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    dev.set_recognition(model, gallery)
    dev.set_identify_interval(0.0)
    dev.set_identity_threshold(TQ.THRESHOLD)
    dev.set_gallery_refinement(gallery, TQ.MAX_SAMPLES)
    dev.set_enrolment(gallery, TQ.FIRST_ID)
    dev.set_identity_quality(H.FaceQualityGate(*tiers[0]), H.FaceQualityGate(*tiers[1]))
    if max_residual is not None:
        dev.set_identity_alignment(_alignment(H, max_residual))
    assert dev.identity_alignment() == (max_residual is not None)
    out = {"track": [], "identity": [], "quality": [], "counters": [], "dev": dev, "gallery": gallery, "bufs": []}
    fb = FH * FW * 4
    for k in range(steps):
        if off_from is not None and k == off_from:
            dev.set_identity_alignment(None)
            assert not dev.identity_alignment()
        buf = DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)]))
        out["bufs"].append(buf)
        for s, dets in enumerate(TQ._injected(k)):
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
        out["quality"].append([[(o["id"], TQ._quality_record(o["quality"]) if "quality" in o else None) for o in objs[s]]
                               for s in range(S)])
        out["counters"].append((dev.identity_images(), dev.quality_measured_total(), dev.quality_rejected_total(),
                                dev.quality_held_back_total(), dev.enrolled_total(), dev.refined_total(),
                                dev.aligned_total(), dev.align_fallback_total()))
    return out


def _same(want, got, steps=STEPS):
    for k in range(steps):
        for s in range(S):
            assert got["track"][k][s] == want["track"][k][s], ("tracking", k, s)
            assert got["identity"][k][s] == want["identity"][k][s], ("identity and embedding", k, s)
            assert got["quality"][k][s] == want["quality"][k][s], ("quality", k, s)
        assert got["counters"][k] == want["counters"][k], ("counters", k, got["counters"][k], want["counters"][k])
    rows, ids = got["gallery"].rows()
    ref = want["gallery"]
    assert list(ids) == list(ref.ids)
    for r in range(len(ids)):
        assert np.asarray(rows[r], f32).tobytes() == ref.rows[r].tobytes(), ("gallery row", r)
    assert list(got["gallery"].row_updates()) == list(want["ref"].updates)


@pytest.fixture(scope="module")
def setup(H, frames, embedder, gallery_rows):
    """The oracle with no limit and no tier, and the settings chosen from what it saw."""
    plain = _oracle_run(H, frames, embedder, gallery_rows, math.inf, (QR.SKIP, QR.SKIP))
    fits = plain["crops"].fits
    assert len(fits) >= 20 and all(f["flags"] == AR.ALIGNED for f in fits)
    res = sorted({float(f["residual"]) for f in fits})
    mid = len(res) // 2
    max_residual = float(f32((res[mid - 1] + res[mid]) / 2))
    assert res[mid - 1] < max_residual < res[mid]
    stream0 = {id(f) for f in frames[0]}
    sizes = sorted({float(np.fmin(f32(v[2]), f32(v[3])))
                    for f in fits if f["frame"] in stream0
                    for v in [f["view"] if float(f["residual"]) <= max_residual else f["bounding"]]})
    assert len(sizes) >= 4
    min_size = float(f32((sizes[len(sizes) // 2 - 1] + sizes[len(sizes) // 2]) / 2))
    tiers = ((-math.inf, -math.inf, 0.5, -math.inf), (min_size, -math.inf, -math.inf, -math.inf))
    print("max_residual", max_residual, "of", res[0], "..", res[-1], "tiers", tiers)
    return {"plain": plain, "max_residual": max_residual, "tiers": tiers}


@pytest.fixture(scope="module")
def aligned(H, frames, embedder, model, gallery_rows, setup):
    want = _oracle_run(H, frames, embedder, gallery_rows, setup["max_residual"], setup["tiers"])
    got = _device_run(H, frames, model, gallery_rows, setup["max_residual"], setup["tiers"])
    return want, got


def test_script_contains_the_cases(setup, aligned):
    want, _ = aligned
    fits = want["crops"].fits
    flags = [f["flags"] for f in fits]
    assert AR.ALIGNED in flags and AR.FALLBACK | AR.FAIL_RESIDUAL in flags, set(flags)
    assert want["crops"].aligned > 0 and want["crops"].fallbacks > 0
    assert want["crops"].aligned + want["crops"].fallbacks == len(fits) == want["ref"].measured
    # an aligned view is rotated: sin_r != 0
    assert any(f["flags"] == AR.ALIGNED and AR.sinf(f32(f["view"][4])) != 0 for f in fits)
    assert all(f["view"] == f["bounding"] for f in fits if f["flags"] & AR.FALLBACK), "a fallback is the bounding crop"
    # the gate rejects (the flat stream), holds back and lets learn; stream 0 is enrolled and refined
    kinds = {c[3] for c in want["ref"].cases}
    assert kinds == {"reject", "held", "learn"}, kinds
    assert want["gallery"].enrolled_total > 0 and want["ref"].refined_total > 0
    # alignment made a difference to what was embedded
    plain_emb = [rec for k in range(STEPS) for _, rec in setup["plain"]["identity"][k][0]]
    off = [rec for k in range(STEPS) for _, rec in want["identity"][k][0]]
    assert plain_emb != off


def test_loop_equals_the_oracle(aligned):
    want, got = aligned
    _same(want, got)
    assert got["counters"][-1][6] > 0 and got["counters"][-1][7] > 0


def test_switching_off_returns_to_the_bounding_crop(H, frames, embedder, model, gallery_rows, setup, aligned):
    steps, off_from = 6, 4
    want = _oracle_run(H, frames, embedder, gallery_rows, setup["max_residual"], setup["tiers"], off_from, steps)
    got = _device_run(H, frames, model, gallery_rows, setup["max_residual"], setup["tiers"], off_from, steps)
    _same(want, got, steps)
    # the counters stop where the switch was thrown, while the embeddings go on
    assert got["counters"][steps - 1][6:] == got["counters"][off_from - 1][6:]
    assert got["counters"][steps - 1][1] > got["counters"][off_from - 1][1]
    # the run that stays aligned is the same up to the switch and differs from there on
    stays = aligned[0]
    assert stays["identity"][off_from - 1] == want["identity"][off_from - 1]
    assert stays["identity"][steps - 1][0] != want["identity"][steps - 1][0]


def test_alignment_needs_recognition_and_the_embedders_grid(H, model, gallery_rows):
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    with pytest.raises(RuntimeError):
        dev.set_identity_alignment(H.FaceAlignment.facemesh_five_point())
    assert not dev.identity_alignment() and dev.aligned_total() == 0 and dev.align_fallback_total() == 0
    dev.set_identity_alignment(None)   # off while off is accepted
    gallery = TI._gallery(H, gallery_rows, TQ.GALLERY_IDS)
    dev.set_recognition(model, gallery)
    with pytest.raises(RuntimeError):   # a grid that is not the embedder's input
        dev.set_identity_alignment(H.FaceAlignment(AR.TEMPLATE, AR.GROUPS, 96, 112))
    with pytest.raises(RuntimeError):   # an index past the landmarker's points
        dev.set_identity_alignment(H.FaceAlignment(AR.TEMPLATE, [[468]] + AR.GROUPS[1:]))
    with pytest.raises(RuntimeError):
        dev.set_identity_alignment(_alignment(H, math.nan))
    assert not dev.identity_alignment()
    dev.set_identity_alignment(H.FaceAlignment.facemesh_five_point())
    assert dev.identity_alignment()
    dev.set_recognition(model, gallery)   # every set_recognition turns it off
    assert not dev.identity_alignment()
