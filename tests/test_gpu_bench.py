"""One plain `bench.py` run at a small batch: --steps sets the timed steps, the result line
carries the headline figure and none of the --full legs, and --dump-outputs writes the last
step's results as float32 arrays that agree with the line's own counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, STEPS = 12, 3


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--batch", str(BATCH), "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["steps"] == STEPS and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "faces/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0 and out["value"] > 0
    # value = tracked faces over the timed steps / their wall time
    assert out["value"] == pytest.approx(out["tracked_per_step"] / (out["ms_per_step"] / 1e3), rel=1e-2)
    for leg in ("roofline", "kernels", "hand", "face_next", "tracking", "face_loop", "hand_tracking",
                "config5", "jpeg_source"):
        assert leg not in out, leg
    assert out["cpu_baseline"] is None

    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert sorted(got) == ["face_detections", "face_landmarks", "face_rois"]
    assert all(a.dtype == np.float32 and a.size > 0 for a in got.values())
    dets, rois, lms = got["face_detections"], got["face_rois"], got["face_landmarks"]
    # every frame is tracked on one ROI (its best detection, else the forced ROI)
    assert rois.shape == (BATCH, 16) and np.array_equal(rois[:, 0], np.arange(BATCH))
    assert lms.shape == (BATCH, 468, 3)
    assert dets.shape[1] == 7 + 2 * 6 and len(dets) == round(out["detections_per_step"])
    assert set(dets[:, 0]) >= set(rois[rois[:, 1] == 1, 0])
    tracked = rois[:, 2] == 1
    assert int(tracked.sum()) == round(out["tracked_per_step"]) > 0
    assert np.isfinite(lms).all() and lms[tracked].any(axis=(1, 2)).all() and not lms[~tracked].any()
    # a tracked face's landmarks lie around its ROI (the frame is 1920 x 1080)
    c = lms[tracked][:, :, :2].mean(axis=1)
    assert (np.abs(c - rois[tracked, 6:8]) < rois[tracked, 8:10]).all()
