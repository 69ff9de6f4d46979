#!/usr/bin/env python3
"""What tiled detection costs in the multi-object loop on the MI355X (GPU only: fails without one):
DeviceMultiTracker("face", "facemesh") at `--streams` x `--slots` (default 64 x 4) on
tools/bench_multi_face.py's video (1080p noise frames that each carry one face patch), with
detection_tiles(1920, 1080, 3, 2) -- the full frame and a 3 x 2 grid, T = 7 -- off and on, at the
default 300 ms redetection interval and with the detector on every step (interval 0).

Four trackers (off / on x default / every step) alternate in one process, `--rounds` rounds after a
warm-up of each; a round of a tracker is `--steps` steps (at least 200) between two device events
on the tracker's stream.  Reported per configuration: milliseconds per step (every round, median,
spread), detector frames and tile views per step, and the objects held.  The noise background gives
the detector phantom faces in some tiles, so the tiled trackers hold more objects than the untiled
ones: their step also pays for the landmark network on those.

`--kernel-stats CSV` adds the merge and tile-compaction kernels' own times from the kernel stats of
a separate `rocprofv3 --kernel-trace --stats` run of `--trace-run` (that mode only steps the
tiled every-step tracker, for the profiler).

`--parent-root DIR` (a built checkout of the parent commit) answers "tiling off costs nothing": the
off / default configuration alone, in a fresh process per run, the parent's package and this one
alternately, `--rounds` runs of each; the difference of the medians is reported beside the spread of
the parent's own runs.

Writes one JSON document (default profiles/multi_tiles_bench.json)."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_MS = 33.0
CONFIGS = (("off_default", False, None), ("on_default", True, None), ("off_every_step", False, 0.0),
           ("on_every_step", True, 0.0))
TILE_KERNELS = ("det_merge_kernel", "due_compact_tiles_kernel")


def bring_up(root, device):
    """bench.py's order: its environment (hardware queues) first, then torch brings the device up,
    then the library -- the package of `root`."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, REPO)
    import bench  # noqa: F401
    sys.path.insert(0, root)  # ahead of the path bench.py put in front
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_tiles: no GPU")
    torch.cuda.set_device(device)
    torch.zeros(1, device=f"cuda:{device}")
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_tiles: no GPU")
    if os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))) != os.path.abspath(root):
        raise SystemExit("bench_multi_tiles: the package did not come from " + root)
    return H, _lib


class Loop:
    """One tracker and its clock; `timed(steps)` is milliseconds per step between two device events."""

    def __init__(self, H, _lib, lists, streams, slots, tiles, interval, device):
        self.dev = H.DeviceMultiTracker("face", "facemesh", streams, slots, device)
        if interval is not None:
            self.dev.set_redetect_interval(interval)
        if tiles:
            self.dev.set_detection_tiles(tiles)
        self.tiled, self.lists, self.k, self.lib, self._lib = bool(tiles), lists, 0, _lib.lib(), _lib
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            _lib.check(self.lib.zr_event_create_timing(C.byref(e)))

    def step(self):
        self.dev.step(self.lists[self.k % len(self.lists)], FRAME_MS * self.k)
        self.k += 1

    def timed(self, steps):
        self.dev.synchronize()
        stream = C.c_void_p(self.dev.stream())
        self._lib.check(self.lib.zr_event_record(self.ev[0], stream))
        for _ in range(steps):
            self.step()
        self._lib.check(self.lib.zr_event_record(self.ev[1], stream))
        self._lib.check(self.lib.zr_event_synchronize(self.ev[1]))
        ms = C.c_float()
        self._lib.check(self.lib.zr_event_elapsed(C.byref(ms), self.ev[0], self.ev[1]))
        return ms.value / steps

    def counters(self):
        self.dev.synchronize()
        return (self.dev.detector_frames(), self.dev.detector_views() if self.tiled else 0,
                float(np.mean(self.dev.object_counts())))


def summary(ms):
    return {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(statistics.median(ms), 4),
            "spread_ms": round(max(ms) - min(ms), 4)}


def run_configs(args, names):
    H, _lib = bring_up(args.root, args.device)
    from bench_multi_face import build_video
    video, lists, frame = build_video(args.streams, args.sets, args.device)
    w, h = (int(v) for v in frame.split("x"))
    loops = {}
    for name, tiled, interval in CONFIGS:
        if name in names:
            tiles = H.detection_tiles(w, h, 3, 2) if tiled else []
            loops[name] = Loop(H, _lib, lists, args.streams, args.slots, tiles, interval, args.device)
    for lp in loops.values():      # warm-up: every launch shape, every allocation; the objects start here
        lp.timed(args.warmup)
    runs = {n: [] for n in loops}
    before = {n: lp.counters() for n, lp in loops.items()}
    for _ in range(args.rounds):
        for n, lp in loops.items():
            runs[n].append(lp.timed(args.steps))
    out = {}
    for n, lp in loops.items():
        f0, v0, _ = before[n]
        f1, v1, objs = lp.counters()
        steps = args.rounds * args.steps
        out[n] = dict(summary(runs[n]), detector_frames_per_step=round((f1 - f0) / steps, 3),
                      detector_views_per_step=round((v1 - v0) / steps, 3), objects_per_stream=round(objs, 3))
    del video
    return out, frame


def kernel_stats(path):
    """The tile kernels' rows of a rocprofv3 kernel stats CSV (Name, Calls, TotalDurationNs, AverageNs, ...)."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in TILE_KERNELS + ("det_post_kernel", "due_compact_kernel"):
                if k in row.get("Name", ""):
                    out[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3),
                              "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_tiles_bench.json"))
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--sets", type=int, default=2, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--root", default=REPO, help="the checkout whose zaru_amd package is measured")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit (see above)")
    ap.add_argument("--kernel-stats", help="kernel stats CSV of a rocprofv3 run of --trace-run")
    ap.add_argument("--off-only", action="store_true", help="one run of off_default; prints its ms per step")
    ap.add_argument("--trace-run", action="store_true", help="only step the tiled every-step tracker (for rocprofv3)")
    args = ap.parse_args()
    if args.off_only:
        args.rounds = 1
        res, _ = run_configs(args, ("off_default",))
        print(json.dumps({"ms_per_step": res["off_default"]["ms_per_step"][0]}))
        return
    if args.trace_run:
        args.rounds = 1
        run_configs(args, ("on_every_step",))
        return
    if args.steps < 200 or args.rounds < 3:
        raise SystemExit("bench_multi_tiles: at least 200 steps a round and three rounds")
    configs, frame = run_configs(args, [c[0] for c in CONFIGS])
    res = {"tool": "tools/bench_multi_tiles.py", "streams": args.streams, "slots": args.slots, "frame": frame,
           "tiles": "detection_tiles(w, h, 3, 2): the full frame + 3 x 2, overlap 0.25 (T = 7), tile_cap 64",
           "timing": "device events on the tracker's stream around `steps` steps; the four trackers alternate in one "
                     "process after a warm-up of each; the profiler off",
           "steps_per_round": args.steps, "rounds": args.rounds, "warmup_steps": args.warmup, "configs": configs,
           "tiling_adds_ms_per_step": {
               k: round(configs["on_" + k]["median_ms_per_step"] - configs["off_" + k]["median_ms_per_step"], 4)
               for k in ("default", "every_step")}}
    print(json.dumps(res["configs"]), file=sys.stderr, flush=True)
    if args.kernel_stats:
        res["kernels"] = dict(kernel_stats(args.kernel_stats),
                              source="rocprofv3 --kernel-trace --stats, a run of its own (--trace-run)")
    if args.parent_root:
        runs = {"parent": [], "this": []}
        for _ in range(args.rounds):
            for who, root in (("parent", os.path.abspath(args.parent_root)), ("this", REPO)):
                cmd = [sys.executable, os.path.abspath(__file__), "--off-only", "--root", root, "--streams",
                       str(args.streams), "--slots", str(args.slots), "--sets", str(args.sets), "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--device", str(args.device)]
                p = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600)
                runs[who].append(json.loads(p.stdout.decode().strip().splitlines()[-1])["ms_per_step"])
        parent, this = summary(runs["parent"]), summary(runs["this"])
        diff = round(this["median_ms_per_step"] - parent["median_ms_per_step"], 4)
        res["tiling_off_vs_parent"] = {
            "what": "off_default alone, a fresh process per run, parent and this change alternately",
            "parent": parent, "this": this, "difference_of_medians_ms": diff,
            "within_parent_spread": abs(diff) <= parent["spread_ms"]}
        print(json.dumps(res["tiling_off_vs_parent"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
