"""Every optional stage of DeviceMultiTracker in one run, through its switches: filter, pose,
recognition with enrolment, smoothing and refinement, eyes, detection tiles, a held snapshot, the
features set again and switched off, and a change of frame size.  The per-feature suites pin each
stage against its oracle; this pins their composition.  After every step the bytes of every array of
objects_packed(), the object counts, the counters and the gallery are hashed (SHA-256) and compared
with tests/golden/multi_all_features.json for equality.

The golden is this file's own record: `python tests/test_gpu_multi_all_features.py --record` on the
commit whose behaviour is to be kept writes it; the test never does."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
RECORD = os.path.join(GOLDEN, "multi_all_features.json")
f32 = np.float32

# the smallest shape with two streams, two objects in one of them, a free slot in both, and a tile
# grid larger than one
S, K, STEPS = 2, 3, 11
FW, FH = 480, 360
SMALL_W, SMALL_H = 320, 240   # the last step's frames
# per step, per stream (confidence, (cx, cy, w, h), angle): all inside the small frame too
SCRIPT = {
    0: {0: [(0.9, (150.0, 120.0, 80.0, 88.0), 0.3), (0.8, (60.0, 190.0, 60.0, 60.0), 0.0)],
        1: [(0.9, (100.0, 100.0, 60.0, 60.0), 0.0)]},
    2: {1: [(0.6, (230.0, 150.0, 72.0, 72.0), 1.0)]},
}
GALLERY_IDS = [7, 1000, 2 ** 40 + 3]
FIRST_ID = 5000
# between the distance of two looks at one object on these noise frames (about 3) and the distance to
# the random rows (the norm of a 128-vector of unit normals, about 11): the objects are unknown at
# first, enrolled, and known -- so their rows are refined -- from then on
THRESHOLD = 4.0
COUNTERS = ("detector_frames", "detector_views", "landmark_images", "identity_images", "eye_images",
            "enrolled_total", "enrol_dropped", "refined_total")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _packed(p, prefix):
    return {prefix + k: _sha(np.asarray(p[k])) for k in sorted(p)}


def run(H):
    """The schedule; one dict of digests per step."""
    import procrustes_ref as R
    import recognition_util as RU
    from zaru_amd._lib import DeviceBuffer

    model = RU.model_bytes(GOLDEN)
    rng = np.random.default_rng(61)
    sizes = [(FW, FH)] * (STEPS - 1) + [(SMALL_W, SMALL_H)]
    frames = [DeviceBuffer.from_array(rng.integers(0, 256, (S, h, w, 4), dtype=np.uint8)) for w, h in sizes]
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    gallery = None

    def recognise():
        dev.set_recognition(model, gallery)
        dev.set_identify_interval(20.0)
        dev.set_identity_threshold(THRESHOLD)

    out = []
    for k in range(STEPS):
        if k == 2:
            dev.set_filter(H.Ema(0.5))
            dev.set_pose_reference(R.canonical_mesh())
        if k == 3:
            gallery = H.Gallery()
            gallery.add(np.random.default_rng(78).standard_normal((3, 128)).astype(f32), GALLERY_IDS)
            gallery.reserve(16)
            recognise()
            dev.set_enrolment(gallery, FIRST_ID)
            dev.set_identity_smoothing(4)
            dev.set_gallery_refinement(gallery)
        if k == 4:
            dev.set_eye_refinement(True)
        if k == 5:
            dev.set_detection_tiles(H.detection_tiles(FW, FH, 2, 2), 8)
        if k == 8:
            recognise()   # the same model again: every identity starts over, enrolment and the rest are off
            dev.set_eye_refinement(False)
        if k == 9:
            dev.set_eye_refinement(True)
            dev.set_detection_tiles([])
        for s, dets in SCRIPT.get(k, {}).items():
            dev.inject_detections(s, [H.Detection(c, H.Rect.from_center(*r), a) for c, r, a in dets])
        (w, h), fb = sizes[k], sizes[k][0] * sizes[k][1] * 4
        dev.step([(frames[k].ptr + s * fb, w, h, w * 4) for s in range(S)], 15.0 * k)
        d, p = {}, None
        if k == 7:    # the snapshot taken after step 5, with two steps enqueued behind it
            d.update(_packed(dev.objects_packed(), "snapshot."))
        if k != 6:    # (a call at step 6 would consume the held snapshot)
            p = dev.objects_packed()
            d.update(_packed(p, "packed."))
        if k == 5:
            dev.snapshot()
        d["object_counts"] = _sha(np.asarray(dev.object_counts(), np.int32))
        counters = [int(getattr(dev, name)()) for name in COUNTERS]
        d["counters"] = _sha(np.asarray(counters, np.uint64))
        if gallery is not None:
            rows, ids = gallery.rows()
            d["gallery.rows"] = _sha(np.asarray(rows, f32))
            d["gallery.ids"] = _sha(np.asarray(ids, np.uint64))
            d["gallery.row_updates"] = _sha(np.asarray(gallery.row_updates(), np.uint32))
        out.append(d)
        print(k, dict(zip(COUNTERS, counters)), "objects", dev.object_counts(), "packed", p and p["count"],
              "distances", p and p.get("identity_distance"))
    return out, dict(zip(COUNTERS, counters))


def test_all_features_digests():
    import zaru_amd.host as H
    with open(RECORD) as f:
        want = json.load(f)
    got, counters = run(H)
    # the run is the one the golden was recorded for, and every stage did something in it
    assert len(got) == len(want) == STEPS
    assert all(counters[name] > 0 for name in COUNTERS if name != "enrol_dropped"), counters
    for k, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (k, sorted(set(g) ^ set(w)))
        for key in sorted(g):
            assert g[key] == w[key], f"step {k}: {key} differs from the recorded run"
    # the held snapshot is step 5's records, untouched by the two steps enqueued behind it
    for key, digest in got[7].items():
        if key.startswith("snapshot."):
            assert digest == got[5]["packed." + key[len("snapshot."):]], key
    assert got[7]["packed.landmarks"] != got[5]["packed.landmarks"]


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", nargs="?", const=RECORD, help="write the digests (default: the golden)")
    args = ap.parse_args()
    sys.path.append(REPO)
    import zaru_amd.host as H
    digests, _ = run(H)
    if args.record:
        with open(args.record, "w") as f:
            json.dump(digests, f, indent=1, sort_keys=True)
            f.write("\n")
        print("recorded", args.record)
