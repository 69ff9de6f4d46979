"""Iris and eye-contour refinement on the GPU: zaru_amd.host.EyeRefiner, the three entry points
zr_eye_select_async / zr_eye_crop_async / zr_eye_commit_async, and DeviceMultiTracker's
set_eye_refinement, against

  * tests/eye_ref.py's independent chain through the oracle's preprocessing and f32 network
    (max L2 <= 1e-3 network px, test_estimator_eye_and_68_point's bar for this network), and semantic
    bars on the three golden faces;
  * the host restatement (face_eye_rects, eye_crop_view, eye_map_out, EyeRefiner.mirrored_crop) and
    zr_preprocess_views_async, bit for bit, for the kernels alone on synthetic states;
  * EyeRefiner.refine on the reported landmarks, bit for bit, for the loop -- and the loop itself with
    refinement off for everything else it reports.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O

import eye_ref as ER
import multi_tracker_ref as MR

pytestmark = pytest.mark.gpu

f32 = np.float32
TOL = 1e-3   # network px


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


def codes_image(codes):
    """tests/test_gpu_host_api.py's: an RGBA image whose identity view reproduces the committed input."""
    c, h, w = codes.shape
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., :3] = codes.transpose(1, 2, 0)
    return img


def _l2(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64)[:, :2] - np.asarray(b, np.float64)[:, :2]) ** 2).sum(-1)).max())


def _eye_bits(e):
    """One eye of a result as comparable values (None stays None)."""
    if e is None:
        return None
    c = e["crop"]
    return (np.ascontiguousarray(e["landmarks"], f32).tobytes(), f32(e["iris_diameter"]).tobytes(),
            np.array([*c.rect().tuple(), c.rotation_radians()], f32).tobytes())


# ---- 1, 2: the golden faces ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "sad_linus_mesh.npz"))
    return [(codes_image(g["codes"][i]), np.ascontiguousarray(g["landmarks"][i], f32)) for i in range(3)]


@pytest.fixture(scope="module")
def refined(H, golden):
    r = H.EyeRefiner()
    return [r.refine(img, lm) for img, lm in golden]


@pytest.fixture(scope="module")
def chain(golden, models_dir):
    net = O.Net(os.path.join(models_dir, "iris_landmark.onnx"), f64=False)
    return [(ER.refine_chain(O, net, img, lm), ER.refine_chain(O, net, img, lm, mirror=False)) for img, lm in golden]


def test_refiner_against_the_oracle_chain(H, golden, refined, chain):
    for i in range(3):
        for side in ("left", "right"):
            got, want = refined[i][side], chain[i][0][side]
            assert got is not None and want is not None, (i, side)
            l2 = _l2(got["landmarks"], want["landmarks"]) / float(want["per_px"])
            dz = float(np.abs(got["landmarks"][:, 2] - want["landmarks"][:, 2]).max()) / float(want["per_px"])
            print("face", i, side, "max L2 (network px):", l2, "max |dz|:", dz)
            assert l2 <= TOL, (i, side, l2)
            crop = got["crop"]
            assert np.array([*crop.rect().tuple(), crop.rotation_radians()], f32).tobytes() == \
                np.array([*want["crop"].rect.tuple(), want["crop"].rad], f32).tobytes()
            # the diameter is the landmarks' own, in the reference's order
            assert f32(got["iris_diameter"]).tobytes() == ER.iris_diameter(got["landmarks"]).tobytes()


def _bars(H, eye, rect, where):
    w, h = rect.rect().size
    cx, cy = rect.transform_in(float(eye["landmarks"][0, 0]), float(eye["landmarks"][0, 1]))
    ratio = eye["iris_diameter"] / w
    print(where, "iris centre at", cx / w, cy / h, "of the eye rect; diameter / width", ratio)
    assert 0.0 <= cx <= w and 0.0 <= cy <= h, (where, cx, cy, w, h)
    assert 0.3 <= ratio <= 0.6, (where, ratio)


def test_semantic_bars(H, golden, refined, chain):
    for i, (img, lm) in enumerate(golden):
        rects = dict(zip(("left", "right"), H.face_eye_rects(lm)))
        for side in ("left", "right"):
            _bars(H, refined[i][side], rects[side], ("face", i, side))
        # a silently dropped flip cannot pass: without the mirroring the right eye is somewhere else
        want, unmirrored = chain[i][0]["right"], chain[i][1]["right"]
        l2 = _l2(refined[i]["right"]["landmarks"], unmirrored["landmarks"]) / float(want["per_px"])
        print("face", i, "right eye without the mirroring differs by", l2, "network px")
        assert l2 > TOL, (i, l2)
        assert _l2(unmirrored["landmarks"], want["landmarks"]) / float(want["per_px"]) > TOL


# ---- 3: the kernels alone ----------------------------------------------------------------------------------
def _describe(views, frame):
    from zaru_amd import _lib
    v = np.ascontiguousarray(views, f32).reshape(-1, 5)
    out = np.zeros((len(v), 10), np.uint32)
    _lib.check(_lib.lib().zr_view_describe(v.ctypes.data, len(v), frame, out.ctypes.data))
    return out


SENT = 0xA5A5A5A5


@pytest.mark.parametrize("n,slots,grow,n_frames", [(5, 5, 0.65, 1), (600, 4, 0.3, 100)])
def test_kernels_alone(H, n, slots, grow, n_frames):
    """select + compact + crop + commit on synthetic states.  n = 600 gives 1200 entries: past one
    1024-row compaction chunk and no multiple of 64; its streams 100..149 have no frame."""
    from zaru_amd import _lib
    lib = _lib.lib()
    b = _lib.DeviceBuffer.from_array
    W, Hh, L, ne = 160, 120, 468, 2 * n
    rng = np.random.default_rng(100 + n)
    # each face's points in a 40 x 30 box anywhere around the frame: eye rects of every angle, crops
    # inside the frame, hanging over its edges and wholly outside
    org = np.c_[rng.uniform(-30, 150, n), rng.uniform(-30, 110, n), np.zeros(n)]
    lm = (org[:, None, :] + rng.uniform(0, 1, (n, L, 3)) * (40.0, 30.0, 8.0)).astype(f32)
    st = np.zeros(n, np.dtype(_lib.TrackState))
    st["tracked"], st["active"], st["frame_w"], st["frame_h"] = 1, 1, W, Hh
    special = [1, 2, 3] + ([515, 516, 517, 599] if n == 600 else [])
    st["tracked"][[r for r in special if r % 514 == 1 or r == 599]] = 0   # untracked rows
    for r in special:
        if r % 514 == 2:
            lm[r, 145, 0] = np.nan                  # a NaN point of the left eye only
        if r % 514 == 3:
            lm[r, [145, 133, 159]] = lm[r, 33]      # a zero-width left eye
    lm[0, 0, :] = np.nan                            # a point no eye uses
    # row 4's left eye is centred 6 px inside the right edge: its crop hangs over it
    lm[4, :, :2] = ((135.0, 40.0) + rng.uniform(0, 1, (L, 2)) * (40.0, 30.0)).astype(f32)
    lm[4, [33, 133, 145, 159, 263], :2] = [(146.0, 50.0), (162.0, 51.0), (154.0, 55.0), (154.0, 46.0), (175.0, 52.0)]
    cfg = _lib.EyeCfg(slots, L, 1, 1, 64, 64, grow)
    d_st, d_lm = b(st), b(lm)
    d_valid, d_views = b(np.full(ne, 9, np.int32)), b(np.full((ne, 10), SENT, np.uint32))
    d_crop = b(np.full((ne, 5), SENT, np.uint32))
    _lib.check(lib.zr_eye_select_async(C.byref(cfg), d_st.ptr, n, d_lm.ptr, d_valid.ptr, d_views.ptr, d_crop.ptr, None))
    _lib.synchronize()
    valid, views = d_valid.download((ne,), np.int32), d_views.download((ne, 10), np.uint32)
    crops = d_crop.download((ne, 5), np.uint32)
    rects = []
    for i in range(n):
        rects += list(H.face_eye_rects(lm[i])) if st["tracked"][i] else [None, None]
    zviews = {}
    for e, r in enumerate(rects):
        assert valid[e] == int(r is not None), ("valid", e, valid[e])
        if r is None:
            assert (views[e] == SENT).all() and (crops[e] == SENT).all(), ("an invalid entry was written", e)
            continue
        zviews[e] = H.eye_crop_view(r, W, Hh, grow).zr_view()
        assert views[e].tobytes() == _describe([zviews[e]], (e // 2) // slots)[0].tobytes(), ("view", e)
        c = H.eye_crop_rect(r, grow)
        assert crops[e].tobytes() == np.array([*c.rect().tuple(), c.rotation_radians()], f32).tobytes(), ("crop", e)
    assert [valid[2 * r] for r in (1, 2, 3)] == [0, 0, 0] and [valid[2 * r + 1] for r in (1, 2, 3)] == [0, 1, 1]
    assert valid[0] == 1 and valid[1] == 1

    # compact: zr_identity_compact_async over the entries
    d_due_views, d_of = b(np.full((ne, 10), SENT, np.uint32)), b(np.full(ne, 77, np.int32))
    d_count, d_dv, d_total = b(np.array([-5], np.int32)), b(np.full(ne, 77, np.int32)), b(np.array([1000], np.uint64))
    _lib.check(lib.zr_identity_compact_async(d_valid.ptr, d_views.ptr, ne, d_due_views.ptr, d_of.ptr, d_count.ptr,
                                             d_dv.ptr, d_total.ptr, None))
    _lib.synchronize()
    due_of = d_of.download((ne,), np.int32)
    packed = np.flatnonzero(valid)
    m = len(packed)
    want_of = np.full(ne, -1, np.int32)
    want_of[packed] = np.arange(m)
    assert np.array_equal(due_of, want_of) and d_count.download((1,), np.int32)[0] == m
    assert d_total.download((1,), np.uint64)[0] == 1000 + m
    if n == 600:
        assert m > 1024 and m % 64 != 0, m

    # crop: every packed cell against the preprocessing's samples, cells past the count untouched
    imgs = [rng.integers(0, 256, (Hh, W, 4), dtype=np.uint8) for _ in range(3)]
    d_imgs = [b(im) for im in imgs]
    fr = (_lib.Frame * n_frames)(*[_lib.Frame(d_imgs[f % 3].ptr, W, Hh, W * 4) for f in range(n_frames)])
    cell = 64 * 64 * 4
    d_atlas = b(np.full(ne * cell, 0xEE, np.uint8))
    _lib.check(lib.zr_eye_crop_async(fr, n_frames, d_due_views.ptr, d_of.ptr, ne, d_count.ptr, d_atlas.ptr, 64, 64, None))
    _lib.synchronize()
    atlas = d_atlas.download((ne, 64, 64, 4), np.uint8)
    assert (atlas[m:] == 0xEE).all(), "a cell past the count was written"
    framed = [e for e in packed if (e // 2) // slots < n_frames]
    vz = (_lib.View * len(framed))(*[_lib.View(*zviews[e]) for e in framed])
    vf = np.array([(e // 2) // slots for e in framed], np.uint32)
    d_pre = _lib.DeviceBuffer(len(framed) * 3 * 64 * 64 * 4)
    _lib.check(lib.zr_preprocess_views_async(fr, n_frames, vz, vf.ctypes.data, len(framed), 64, 64, 0.0, 255.0,
                                             d_pre.ptr, None))
    _lib.synchronize()
    pre = np.rint(d_pre.download((len(framed), 3, 64, 64), f32)).astype(np.uint8).transpose(0, 2, 3, 1)
    inside = 0
    for j, e in enumerate(framed):
        want = pre[j][:, ::-1] if e & 1 else pre[j]
        assert np.array_equal(atlas[due_of[e]][..., :3], want), ("cell", e, due_of[e])
        inside += int(want.any())
    for e in packed:
        if (e // 2) // slots >= n_frames:   # a frame index past the table: Color::NONE
            assert not atlas[due_of[e]].any(), ("cell of a missing frame", e)
    assert inside >= 3 and (n_frames >= n // slots or len(framed) < m)
    # the whole RGBA pixel, and Color::NONE outside the frame, against the host's sampler
    refiner = H.EyeRefiner()
    for e in framed[:6] + framed[-6:] + [8, 9]:
        mir = refiner.mirrored_crop(imgs[((e // 2) // slots) % 3], rects[e], grow)
        assert np.array_equal(atlas[due_of[e]], mir if e & 1 else mir[:, ::-1]), ("rgba", e)
    over = atlas[due_of[8]]                      # row 4 hangs over the right edge
    assert over.any() and not over.reshape(-1, 4).any(axis=1).all()

    # commit on hand-made outputs, strides wider than the rows
    s0, s1 = 216, 16
    out0, out1 = rng.uniform(-8, 72, (ne, s0)).astype(f32), rng.uniform(-8, 72, (ne, s1)).astype(f32)
    d_elm, d_diam, d_ev = b(np.full((ne, 76, 3), 7.0, f32)), b(np.full(ne, 7.0, f32)), b(np.full(ne, 7, np.int32))
    d_o0, d_o1 = b(out0), b(out1)
    _lib.check(lib.zr_eye_commit_async(C.byref(cfg), n, d_of.ptr, d_o0.ptr, d_o1.ptr, s0, s1, d_crop.ptr, d_elm.ptr,
                                       d_diam.ptr, d_ev.ptr, None))
    _lib.synchronize()
    elm, diam, ev = d_elm.download((ne, 76, 3), f32), d_diam.download((ne,), f32), d_ev.download((ne,), np.int32)
    assert np.array_equal(ev, valid)
    for e in range(ne):
        k = due_of[e]
        if k < 0:
            assert not elm[e].any() and diam[e] == 0.0, ("an invalid entry keeps no result", e)
            continue
        if n == 600 and e % 7 and e not in (4, 5, 6, 7, 8, 9):
            continue
        raw = np.concatenate([out1[k, :15].reshape(5, 3), out0[k, :213].reshape(71, 3)])
        want = H.eye_map_out(raw, bool(e & 1), H.eye_crop_rect(rects[e], grow))
        assert elm[e].tobytes() == want["landmarks"].tobytes(), ("landmarks", e)
        assert diam[e:e + 1].tobytes() == f32(want["iris_diameter"]).tobytes(), ("diameter", e)
        if e & 1:   # un-mirrored: not what the left-eye arithmetic gives
            assert elm[e].tobytes() != H.eye_map_out(raw, False, H.eye_crop_rect(rects[e], grow))["landmarks"].tobytes()


def test_refusals_launch_nothing():
    """Bad arguments with real device buffers: ZR_ERR_INVALID_ARGUMENT, and no buffer is touched."""
    from zaru_amd import _lib
    lib = _lib.lib()
    buf = _lib.DeviceBuffer.from_array(np.full(1 << 20, 0x5A, np.uint8))
    p = buf.ptr
    ok = dict(slots=4, num_landmarks=468, aspect_w=1, aspect_h=1, in_w=64, in_h=64, crop_grow=0.65)
    bad_cfgs = [dict(ok, slots=0), dict(ok, slots=65), dict(ok, num_landmarks=386), dict(ok, crop_grow=-1.0),
                dict(ok, crop_grow=float("nan")), dict(ok, aspect_w=0)]
    for kw in bad_cfgs:
        c = _lib.EyeCfg(**kw)
        assert lib.zr_eye_select_async(C.byref(c), p, 8, p, p, p, p, None) == -1, kw
        assert lib.zr_eye_commit_async(C.byref(c), 8, p, p, p, 213, 15, p, p, p, p, None) == -1, kw
    c = _lib.EyeCfg(**ok)
    assert lib.zr_eye_select_async(C.byref(c), p, 6, p, p, p, p, None) == -1      # 6 rows, 4 slots
    assert lib.zr_eye_select_async(C.byref(c), None, 8, p, p, p, p, None) == -1
    assert lib.zr_eye_commit_async(C.byref(c), 8, p, p, p, 212, 15, p, p, p, p, None) == -1
    fr = _lib.Frame(p, 64, 64, 256)
    assert lib.zr_eye_crop_async(C.byref(fr), 0, p, p, 16, p, p, 64, 64, None) == -1
    assert lib.zr_eye_crop_async(C.byref(fr), 1, p, p, 0, p, p, 64, 64, None) == -1
    assert lib.zr_eye_crop_async(C.byref(fr), 1, p, p, 16, p, p + 1, 64, 64, None) == -1
    assert lib.zr_eye_crop_async(C.byref(fr), 1, p, None, 16, p, p, 64, 64, None) == -1
    _lib.synchronize()
    assert (buf.download((1 << 20,), np.uint8) == 0x5A).all()


# ---- 4: the loop ---------------------------------------------------------------------------------------
FW, FH = 480, 360
S, K, STEPS = 2, 3, 6
# tests/test_gpu_multi_tracker.py's face script on two streams: a pair that the sweep thins, a late
# newcomer; the loss comes from the loss threshold (below)
SCRIPT = {
    0: {0: [(0.9, (200.0, 180.0, 80.0, 88.0), 0.3), (0.8, (60.0, 290.0, 60.0, 60.0), 0.0)],
        1: [(0.9, (100.0, 100.0, 60.0, 60.0), 0.0), (0.8, (104.0, 101.0, 60.0, 60.0), 0.1)]},
    2: {1: [(0.6, (330.0, 250.0, 88.0, 88.0), 1.0)]},
}
# without a loss: stream 0's two objects report at steps 1..5, stream 1's survivor of the pair at 1..5,
# its newcomer at 3..5
RESULTS_WITHOUT_LOSS = 2 * 5 + 5 + 3


def _det(H, d):
    conf, (cx, cy, w, h), angle = d
    return H.Detection(conf, H.Rect.from_center(cx, cy, w, h), angle)


@pytest.fixture(scope="module")
def frames():
    return [[np.random.default_rng(40 + s).integers(0, 256, (FH, FW, 4), dtype=np.uint8) for _ in range(STEPS)]
            for s in range(S)]


@pytest.fixture(scope="module")
def refine(H):
    """EyeRefiner.refine per (frame, landmarks), kept: the oracle and the comparisons share their runs."""
    refiner = H.EyeRefiner()
    cache = {}

    def fn(frame, lm):
        lm = np.ascontiguousarray(lm, f32)
        key = (id(frame), lm.tobytes())
        if key not in cache:
            cache[key] = refiner.refine(frame, lm)
        return cache[key]
    return fn


def _oracle_run(H, frames, refine, loss, filt=None):
    def make():
        t = H.LandmarkTracker("facemesh")
        if filt is not None:
            t.set_filter(filt)
        return t
    refs = []
    for s in range(S):
        r = MR.MultiTrackerRef(H, "face", "facemesh", K, make_tracker=make)
        r.loss, r.interval = loss, 40.0
        refs.append(ER.MultiEyeRef(r, refine))
    out = {"images": [], "confidences": [], "results": 0}
    for k in range(STEPS):
        for s in range(S):
            refs[s].step(frames[s][k], 15.0 * k, [_det(H, d) for d in SCRIPT.get(k, {}).get(s, [])])
            out["confidences"] += [float(o.pending["confidence"]) for o in refs[s].tracker.objs
                                   if o.pending is not None and k < STEPS - 1]
            out["results"] += len(refs[s].objects())
        out["images"].append(sum(r.images for r in refs))
    out["lost"] = sum(r.lost for r in refs)
    out["swept"] = sum(r.tracker.swept for r in refs)
    return out


@pytest.fixture(scope="module")
def loss_threshold(H, frames):
    """Just above the least confident estimate of a run that loses nothing: that estimate's object is
    the script's one loss (an estimate made afterwards may fall below it too)."""
    none = lambda frame, lm: {"left": None, "right": None}
    calm = _oracle_run(H, frames, none, -1.0)
    assert calm["lost"] == 0 and calm["results"] == RESULTS_WITHOUT_LOSS and calm["swept"] >= 1, calm
    return float(np.nextafter(f32(min(calm["confidences"])), f32(np.inf)))


def _device_run(H, frames, loss, eyes, filt=None, compact=True, off_at=None):
    from zaru_amd._lib import DeviceBuffer
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(loss)
    dev.set_redetect_interval(40.0)
    dev.set_compact(compact)
    if filt is not None:
        dev.set_filter(filt)
    assert dev.eye_refinement() is False and dev.eye_images() == 0
    if eyes:
        dev.set_eye_refinement(True)
        assert dev.eye_refinement() is True
    bufs = [DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)])) for k in range(STEPS)]
    fb = FH * FW * 4
    out = {"track": [], "eyes": [], "images": []}
    for k in range(STEPS):
        if off_at is not None and k == off_at:
            dev.set_eye_refinement(False)
        for s in range(S):
            dets = SCRIPT.get(k, {}).get(s, [])
            if dets:
                dev.inject_detections(s, [_det(H, d) for d in dets])
        dev.step([(bufs[k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)], 15.0 * k)
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        objs = [dev.objects(s) for s in range(S)]
        out["track"].append([(int(counts[s]), bool(pend[s]), [
            (int(o["id"]), np.array([*o["view_rect"].rect().tuple(), o["view_rect"].rotation_radians()], f32).tobytes(),
             np.ascontiguousarray(o["landmarks"], f32).tobytes(), f32(o["confidence"]).tobytes(), o["identity"],
             "pose" in o) for o in objs[s]]) for s in range(S)])
        out["eyes"].append([[(o["landmarks"], o["eyes"]) for o in objs[s]] for s in range(S)])
        out["images"].append(dev.eye_images())
    return out


@pytest.mark.parametrize("variant", ["plain", "ema", "uncompacted"])
def test_loop(H, frames, refine, loss_threshold, variant):
    """Every step, stream and object: eyes == EyeRefiner.refine(this step's frame, the reported
    landmarks), bit for bit; everything else == the same run with refinement off; eye_images() == the
    oracle's count."""
    filt = H.Ema(0.5) if variant == "ema" else None
    kw = dict(filt=filt, compact=variant != "uncompacted")
    want = _oracle_run(H, frames, refine, loss_threshold, filt)
    off = _device_run(H, frames, loss_threshold, False, **kw)
    on = _device_run(H, frames, loss_threshold, True, **kw)
    assert on["track"] == off["track"], "refinement moved a bit of the tracking"
    assert all(e is None for step in off["eyes"] for stream in step for _, e in stream)
    assert off["images"] == [0] * STEPS
    compared = results = valid = 0
    for k in range(STEPS):
        for s in range(S):
            for lm, eyes in on["eyes"][k][s]:
                results += 1
                assert eyes is not None, ("no eyes", k, s)
                host = refine(frames[s][k], lm)
                for side in ("left", "right"):
                    assert _eye_bits(eyes[side]) == _eye_bits(host[side]), (variant, k, s, side)
                    compared += 1
                    valid += eyes[side] is not None
        assert on["images"][k] == want["images"][k], ("eye_images", k, on["images"][k], want["images"][k])
    print(variant, "object results:", results, "eyes compared:", compared, "valid:", valid, "lost:", want["lost"],
          "eye_images:", on["images"])
    assert results == want["results"] and compared == 2 * results
    # the threshold is the unfiltered run's: a filter moves the RoIs, so its estimates need not cross it
    assert (want["lost"] >= 1 or variant == "ema") and want["swept"] >= 1, want
    # one loss takes at most an object's five results; a second one (an estimate made after the first
    # loss may fall below the threshold too) as many again
    assert results >= RESULTS_WITHOUT_LOSS - 10 and valid >= results, (results, valid)
    assert on["images"][-1] >= valid   # the eyes of objects that left in the step are counted too


def test_toggling_off_mid_run(H, frames, loss_threshold):
    off = _device_run(H, frames, loss_threshold, False)
    half = _device_run(H, frames, loss_threshold, True, off_at=3)
    assert half["track"] == off["track"]
    for k in range(STEPS):
        for s in range(S):
            for _, eyes in half["eyes"][k][s]:
                assert (eyes is None) == (k >= 3), (k, s)
    assert half["images"][2] > 0 and half["images"][3:] == [half["images"][2]] * 3


# ---- 5: end to end on a real face ----------------------------------------------------------------------
def test_real_face_end_to_end(H, golden):
    from zaru_amd._lib import DeviceBuffer
    img, _ = golden[0]
    buf = DeviceBuffer.from_array(img)
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    dev.set_eye_refinement(True)
    dev.inject_detections(0, [H.Detection(0.9, H.Rect.from_top_left(0.0, 0.0, 192.0, 192.0), 0.0)])
    for k in range(3):
        dev.step([(buf.ptr, 192, 192, 192 * 4)], 15.0 * k)
    dev.synchronize()
    objs = dev.objects(0)
    assert len(objs) >= 1
    o = objs[0]
    assert o["confidence"] > 0.9 and o["eyes"] is not None
    rects = dict(zip(("left", "right"), H.face_eye_rects(o["landmarks"])))
    for side in ("left", "right"):
        assert o["eyes"][side] is not None, side
        _bars(H, o["eyes"][side], rects[side], ("tracked face", side))
    assert o["eyes"]["left"]["landmarks"][0, 0] < o["eyes"]["right"]["landmarks"][0, 0]
    assert dev.eye_images() >= 4


# ---- 6: refusals ---------------------------------------------------------------------------------------
def test_refusals(H):
    hand = H.DeviceMultiTracker("palm", "hand", 1, 2)
    with pytest.raises(RuntimeError):
        hand.set_eye_refinement(True)
    assert hand.eye_refinement() is False
    hand.set_eye_refinement(False)   # off is what it is already
    face = H.DeviceMultiTracker("face", "facemesh_v2", 1, 2)
    face.set_eye_refinement(True)    # V2 is allowed
    for bad in (-0.1, float("nan")):
        with pytest.raises(RuntimeError):
            face.set_eye_crop_grow(bad)
    face.set_eye_crop_grow(0.5)
    assert face.eye_refinement() is True and face.eye_images() == 0
