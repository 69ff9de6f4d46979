"""bench.py's command line and --dump-outputs writer, without a GPU: a plain run switches every
leg beside the headline figure off, --full leaves them to the --no-* options, and dump_outputs
writes float32 arrays of a pipeline's last results (a stand-in pipeline here; the GPU run is
tests/test_gpu_bench.py)."""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

LEGS = ("cpu_baseline", "profile", "traffic", "hand", "next", "tracking", "jpeg", "c5")


@pytest.fixture(scope="module")
def bench():
    # importing bench.py sets GPU_MAX_HW_QUEUES for its own process: keep it out of this one
    before = os.environ.get("GPU_MAX_HW_QUEUES")
    mod = importlib.import_module("bench")
    if before is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    else:
        os.environ["GPU_MAX_HW_QUEUES"] = before
    return mod


def parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_every_other_leg_off(bench, monkeypatch):
    a = parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert all(getattr(a, "no_" + leg) for leg in LEGS)


def test_full_leaves_the_legs_to_their_own_options(bench, monkeypatch):
    a = parse(bench, monkeypatch, "--full")
    assert a.full and not any(getattr(a, "no_" + leg) for leg in LEGS)
    a = parse(bench, monkeypatch, "--full", "--no-jpeg", "--no-traffic", "--dump-outputs", "d")
    assert a.dump_outputs == "d"
    assert [leg for leg in LEGS if getattr(a, "no_" + leg)] == ["traffic", "jpeg"]


def test_steps_must_be_positive(bench, monkeypatch):
    with pytest.raises(SystemExit):
        parse(bench, monkeypatch, "--steps", "0")


class _Rect:
    def __init__(self, *t):
        self.t = t

    def tuple(self):
        return self.t


class _RRect:
    def __init__(self, rad, *t):
        self.r, self.rad = _Rect(*t), rad

    def rect(self):
        return self.r

    def rotation_radians(self):
        return self.rad


class _Det:
    def __init__(self, conf, angle, rect, kps):
        self.c, self.a, self.r, self.k = conf, angle, rect, kps

    def confidence(self):
        return self.c

    def angle(self):
        return self.a

    def bounding_rect(self):
        return self.r

    def keypoints(self):
        return self.k


class _Pipe:
    """Two frames: one detection and a tracked ROI on frame 1, a lost forced ROI on frame 0."""

    def __init__(self, world=False):
        self.lm = np.arange(12, dtype=np.float32).reshape(4, 3) + 0.5
        none = np.zeros((0, 3), np.float32)
        self.world = self.lm / 8 if world else none
        self.rois = [
            {"frame": 0, "from_detection": False, "tracked": False, "confidence": 0.25,
             "raw_handedness": 0.0, "tongue_out": 0.0, "landmarks": none, "world": none,
             "roi": _RRect(0.0, 10.0, 20.0, 30.0, 40.0), "next_roi": _RRect(9.0, 9.0, 9.0, 9.0, 9.0)},
            {"frame": 1, "from_detection": True, "tracked": True, "confidence": 0.75,
             "raw_handedness": 0.5, "tongue_out": 0.125, "landmarks": self.lm, "world": self.world,
             "roi": _RRect(0.5, 1.0, 2.0, 3.0, 4.0), "next_roi": _RRect(0.25, 5.0, 6.0, 7.0, 8.0)}]

    def detections(self):
        return [[], [_Det(0.875, 0.5, _Rect(1.0, 2.0, 3.0, 4.0), [(1.5, 2.5), (3.5, 4.5)])]]

    def num_rois(self):
        return len(self.rois)

    def roi(self, i):
        return self.rois[i]


def test_dump_outputs_writes_the_last_results_as_float32(bench, tmp_path):
    p = _Pipe()
    d = tmp_path / "out"
    bench.dump_outputs(str(d), [SimpleNamespace(kind="face", pipe=p)], 0, 1)
    got = {f: np.load(d / f) for f in sorted(os.listdir(d))}
    # a face network has no world landmarks: that array would be empty and is not written
    assert sorted(got) == ["face_detections.npy", "face_landmarks.npy", "face_rois.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["face_detections.npy"],
                          np.array([[1, 0.875, 0.5, 1, 2, 3, 4, 1.5, 2.5, 3.5, 4.5]], np.float32))
    want = np.array([[0, 0, 0, 0.25, 0, 0, 10, 20, 30, 40, 0, 0, 0, 0, 0, 0],
                     [1, 1, 1, 0.75, 0.5, 0.125, 1, 2, 3, 4, 0.5, 5, 6, 7, 8, 0.25]], np.float32)
    assert np.array_equal(got["face_rois.npy"], want)
    assert got["face_landmarks.npy"].shape == (2, 4, 3)
    assert not got["face_landmarks.npy"][0].any()  # the lost ROI has no estimate
    assert np.array_equal(got["face_landmarks.npy"][1], p.lm)


def test_dump_outputs_names_each_rank_when_there_are_several(bench, tmp_path):
    p = _Pipe(world=True)
    bench.dump_outputs(str(tmp_path), [SimpleNamespace(kind="hand", pipe=p)], 3, 4)
    assert sorted(os.listdir(tmp_path)) == ["hand_detections_rank3.npy", "hand_landmarks_rank3.npy",
                                            "hand_rois_rank3.npy", "hand_world_rank3.npy"]
    world = np.load(tmp_path / "hand_world_rank3.npy")
    assert world.dtype == np.float32 and world.shape == (2, 4, 3)
    assert not world[0].any() and np.array_equal(world[1], p.world)
