#!/usr/bin/env python3
"""What eye refinement costs inside the multi-object loop, on the MI355X (GPU only: fails without
one): DeviceMultiTracker ("face", "facemesh") at `--streams` x `--slots` (default 64 x 4) on 1080p
frames that carry one face patch per slot, a detection injected on each at the first step, so every
slot is live; refinement off and on.

Two trackers (off, on) alternate in one process, `--repeats` rounds after a warm-up of each, every
measurement device events on the tracker's stream around `--steps` enqueued steps.  Beside them the
floor: the eye network alone on the same streams x slots x 2 views -- an atlas of 64 x 64 cells and
its identity cell views through zr_cnn_estimate_device_views_count_async, which is how the loop runs
it -- timed the same way.  Reports ms per step off and on, the added ms, the floor, and the added
time minus the floor: what select / compact / crop / commit cost.

Writes one JSON document (default profiles/multi_eye_bench.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

FRAME_MS = 33.0


class Events:
    def __init__(self):
        from zaru_amd import _lib
        self.lib, self.check = _lib.lib(), _lib.check
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            self.check(self.lib.zr_event_create_timing(C.byref(e)))

    def time(self, stream, fn, reps):
        """ms per call of `reps` calls of fn() enqueued on `stream`."""
        self.check(self.lib.zr_event_record(self.ev[0], stream))
        for _ in range(reps):
            fn()
        self.check(self.lib.zr_event_record(self.ev[1], stream))
        self.check(self.lib.zr_event_synchronize(self.ev[1]))
        ms = C.c_float()
        self.check(self.lib.zr_event_elapsed(C.byref(ms), self.ev[0], self.ev[1]))
        return ms.value / reps


def build_video(streams, slots, sets, device):
    """1080p seeded noise with `slots` face patches per frame (bench.py's patch at half size), drifting a few pixels
    per frame; returns the tensor (kept alive by the caller), the frame lists and the patch rects of
    the first frame as (cx, cy, w, h)."""
    import torch

    import bench
    rng = np.random.default_rng(bench.WORKLOADS["face"][5])
    fs = bench.FrameSet(rng, 1, patch=bench.load_patch())
    dev = f"cuda:{device}"
    # every second pixel of the patch: a 288 px face, four of which fit across a 1080p frame
    patch = torch.from_numpy(np.ascontiguousarray(bench.load_patch()[::2, ::2])).to(dev)
    base = torch.from_numpy(fs.base).to(dev)
    ph, pw = patch.shape[:2]
    cols = 4
    pos = [(100 + (k // cols) * (ph + 60), 60 + (k % cols) * (pw + 150)) for k in range(slots)]
    if any(y + ph + 2 * sets > fs.h or x + pw + 3 * sets > fs.w for y, x in pos):
        raise SystemExit("bench_multi_eyes: too many slots for the frame")
    video = torch.empty((sets, streams, fs.h, fs.w, 4), dtype=torch.uint8, device=dev)
    for v in range(sets):
        for s in range(streams):
            video[v, s].copy_(base[s % len(fs.base)])
            for y, x in pos:
                y, x = min(fs.h - ph, y + 2 * v), min(fs.w - pw, x + 3 * v)
                video[v, s, y:y + ph, x:x + pw] = patch
    torch.cuda.synchronize(device)
    lists = [[(video[v, s].data_ptr(), fs.w, fs.h, fs.w * 4) for s in range(streams)] for v in range(sets)]
    rects = [(x + pw / 2.0, y + ph / 2.0, float(pw), float(ph)) for y, x in pos]
    return video, lists, f"{fs.w}x{fs.h}", rects


def network_floor(views, steps, repeats, timer, device):
    """The eye network alone on `views` cells of an atlas, as the loop runs it."""
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, Frame, View
    from zaru_amd.nn import NeuralNetwork, model_bytes
    lib = _lib.lib()
    nn = NeuralNetwork.from_onnx(model_bytes("iris_landmark")).on_device(device).load()
    rng = np.random.default_rng(4)
    atlas = DeviceBuffer.from_array(rng.integers(0, 256, (views * 64, 64, 4), dtype=np.uint8))
    cells = (View * views)(*[View(32.0, 64.0 * k + 32.0, 64.0, 64.0, 0.0) for k in range(views)])
    desc = np.zeros((views, 10), np.uint32)
    _lib.check(lib.zr_view_describe(cells, views, 0, desc.ctypes.data))
    d_cells, d_count = DeviceBuffer.from_array(desc), DeviceBuffer.from_array(np.array([views], np.int32))
    outs = [DeviceBuffer(views * 213 * 4), DeviceBuffer(views * 15 * 4)]
    ptrs = (C.c_void_p * 2)(outs[0].ptr, outs[1].ptr)
    frame = Frame(atlas.ptr, 64, 64 * views, 256)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))

    def run():
        _lib.check(lib.zr_cnn_estimate_device_views_count_async(nn._h, C.byref(frame), 1, d_cells.ptr, views, d_count.ptr,
                                                                -1.0, 1.0, ptrs, stream))
    for _ in range(20):
        run()
    ms = [timer.time(stream, run, steps) for _ in range(repeats)]
    _lib.check(lib.zr_stream_synchronize(stream))
    lib.zr_stream_destroy(stream)
    return {"views": views, "ms_per_pass": [round(x, 4) for x in ms], "median_ms_per_pass": round(statistics.median(ms), 4),
            "spread_ms": round(max(ms) - min(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_eye_bench.json"))
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--sets", type=int, default=2, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.repeats < 5 or args.steps < 200:
        raise SystemExit("bench_multi_eyes: at least five repeats of at least 200 steps")
    import bench  # noqa: F401  (its environment first, then torch brings the device up, then the library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_eyes: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_eyes: no GPU")
    S, K = args.streams, args.slots
    timer = Events()
    video, lists, frame, rects = build_video(S, K, args.sets, args.device)
    trackers, clocks = {}, {}
    for name in ("off", "on"):
        t = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
        if name == "on":
            t.set_eye_refinement(True)
        for s in range(S):
            t.inject_detections(s, [H.Detection(0.9, H.Rect.from_center(*r), 0.0) for r in rects])
        trackers[name], clocks[name] = t, 0

    def step(name):
        t = trackers[name]
        t.step(lists[clocks[name] % args.sets], FRAME_MS * clocks[name])
        clocks[name] += 1

    def leg(name):
        t = trackers[name]
        t.synchronize()
        e0 = t.eye_images()
        ms = timer.time(t.stream(), lambda: step(name), args.steps)
        t.synchronize()
        return {"ms": ms, "live": sum(t.object_counts()), "eyes": (t.eye_images() - e0) / args.steps}

    for name in trackers:  # warm-up: every path, every shape; the objects start here
        for _ in range(20):
            step(name)
        trackers[name].synchronize()
    runs = {name: [] for name in trackers}
    for _ in range(args.repeats):
        for name in trackers:
            runs[name].append(leg(name))
    legs = {}
    for name in trackers:
        ms = [r["ms"] for r in runs[name]]
        legs[name] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(statistics.median(ms), 4),
                      "spread_ms": round(max(ms) - min(ms), 4),
                      "live_objects": statistics.median(r["live"] for r in runs[name]),
                      "eye_images_per_step": round(statistics.median(r["eyes"] for r in runs[name]), 2)}
    floor = network_floor(2 * S * K, args.steps, args.repeats, timer, args.device)
    added = legs["on"]["median_ms_per_step"] - legs["off"]["median_ms_per_step"]
    res = {
        "tool": "tools/bench_multi_eyes.py", "streams": S, "slots": K, "frame": frame, "video_frames": args.sets,
        "steps_per_measurement": args.steps, "repeats": args.repeats, "frame_clock_ms": FRAME_MS,
        "timing": "device events on the tracker's stream around `steps` enqueued steps; the two trackers "
                  "alternate in one process after a warm-up of each; medians over the repeats",
        "legs": legs, "eye_network_alone": floor,
        "added_ms_per_step": round(added, 4),
        "added_minus_network_ms": round(added - floor["median_ms_per_pass"], 4),
    }
    del trackers, video
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
