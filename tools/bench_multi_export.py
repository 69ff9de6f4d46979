#!/usr/bin/env python3
"""Reading the multi-object loop's results on the MI355X (GPU only: fails without one):
DeviceMultiTracker ("face", "facemesh", pose reference and eye refinement on unless --plain) at
1,024 streams x 4 slots and at 64 x 4 (`--shapes`), on tools/bench_multi_face.py's video: 1080p
noise frames that each carry one face patch, so one live object per stream after the warm-up.

Four legs alternate in one process, `--rounds` rounds after a warm-up of each, every leg a host
clock around `--steps` steps that ends with the device idle:
  no_read    the steps enqueued back to back, one synchronise at the end: the step with nobody reading;
  objects    after every step synchronize(), then objects(s) for every stream s;
  packed     after every step objects_packed();
  snapshot   after every step snapshot(), the next step enqueued at once, then objects_packed(): the
             host reads step t while the device runs step t + 1.
Per leg: milliseconds per step of the whole loop, the part of it the host spent inside the read-out
calls (for `packed` and `snapshot` that includes waiting for the step itself to finish; for `objects`
the wait is synchronize()'s and is reported beside it), what reading adds to the no_read step, and
the objects read per step.  The records of the last `packed` step are checked against objects(s).
Before the legs, zr_multi_export_async alone on synthetic arrays of each shape, with one and with
`slots` objects per stream: microseconds per call between device events, bytes per call computed
here from the record layout, and the rate.

Writes one JSON document (default profiles/multi_export_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

FRAME_MS = 33.0
LEGS = ("no_read", "objects", "packed", "snapshot")


def export_alone(streams, slots, live, reps, warmup, plain, L=468):
    """zr_multi_export_async alone (both launches) on synthetic arrays with `live` objects per stream,
    each gathered from the next slot of its stream: device events around `reps` back-to-back calls.
    Bytes per call: every record's payload read and written once, headers included; the scan's reads
    of counts and `src` are left out."""
    import ctypes as C

    from zaru_amd import _lib
    lib = _lib.lib()
    rows = streams * slots
    rng = np.random.default_rng(2)
    keep = []

    def dev(a):
        keep.append(_lib.DeviceBuffer.from_array(a))
        return keep[-1].ptr

    def out(nbytes):
        keep.append(_lib.DeviceBuffer(nbytes))
        return keep[-1].ptr

    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    a = _lib.MultiExportArgs()
    a.d_nobjects = dev(np.full(streams, live, np.int32))
    a.d_src = dev(np.tile((np.arange(slots, dtype=np.int32) + 1) % slots, streams))
    a.d_ids, a.d_roi = dev(np.arange(rows, dtype=np.uint64)), dev(f(rows, 5))
    a.d_state, a.d_landmarks = dev(np.zeros(rows * C.sizeof(_lib.TrackState), np.uint8)), dev(f(rows, L * 3))
    a.d_count, a.d_stream_offsets = out(4), out(4 * (streams + 1))
    a.d_header, a.d_out_landmarks = out(rows * 48), out(rows * L * 12)
    per_record = 48 + L * 12
    if not plain:
        a.d_pose, a.d_out_pose = dev(f(rows, 21)), out(rows * 84)
        a.d_eye_valid, a.d_eye_diam = dev(np.ones(2 * rows, np.int32)), dev(f(2 * rows))
        a.d_eye_crop, a.d_eye_lm = dev(f(2 * rows, 5)), dev(f(2 * rows, 228))
        a.d_out_eye_valid, a.d_out_eye_diam = out(8 * rows), out(8 * rows)
        a.d_out_eye_crop, a.d_out_eye_lm = out(40 * rows), out(2 * rows * 912)
        per_record += 84 + 2 * (4 + 4 + 20 + 912)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))

    def call():
        _lib.check(lib.zr_multi_export_async(C.byref(a), streams, slots, L, stream))
    for _ in range(warmup):
        call()
    _lib.check(lib.zr_event_record(ev[0], stream))
    for _ in range(reps):
        call()
    _lib.check(lib.zr_event_record(ev[1], stream))
    _lib.check(lib.zr_event_synchronize(ev[1]))
    ms = C.c_float()
    _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
    count = int(keep[6].download((1,), np.int32)[0])
    assert count == streams * live, count
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    us = 1e3 * ms.value / reps
    nbytes = 2 * count * per_record
    return {"streams": streams, "slots": slots, "live_per_stream": live, "records": count, "reps": reps,
            "pose_and_eyes": not plain, "bytes_per_record": per_record,
            "timing": "device events around `reps` back-to-back calls on one stream (two launches a call, gaps included)",
            "us_per_call": round(us, 3), "bytes_per_call": nbytes, "GB_per_s": round(nbytes / (us * 1e-6) / 1e9, 1)}


def run_shape(H, streams, slots, args, build_video):
    video, lists, frame = build_video(streams, args.sets, args.device)
    dev = H.DeviceMultiTracker("face", "facemesh", streams, slots, args.device)
    if not args.plain:
        dev.set_pose_reference(np.load(os.path.join(REPO, "tests", "golden", "canonical_face_mesh.npy")))
        dev.set_eye_refinement(True)
    clock = {"k": 0}

    def step():
        dev.step(lists[clock["k"] % args.sets], FRAME_MS * clock["k"])
        clock["k"] += 1

    def leg(name):
        dev.synchronize()
        read = wait = 0.0
        objects = 0
        t0 = time.perf_counter()
        if name == "snapshot":
            step()
        for k in range(args.steps):
            if name != "snapshot":
                step()
            if name == "objects":
                t = time.perf_counter()
                dev.synchronize()
                wait += time.perf_counter() - t
                t = time.perf_counter()
                objects += sum(len(dev.objects(s)) for s in range(streams))
                read += time.perf_counter() - t
            elif name == "packed":
                t = time.perf_counter()
                objects += int(dev.objects_packed()["count"])
                read += time.perf_counter() - t
            elif name == "snapshot":
                t = time.perf_counter()
                dev.snapshot()
                read += time.perf_counter() - t
                if k + 1 < args.steps:
                    step()
                t = time.perf_counter()
                objects += int(dev.objects_packed()["count"])
                read += time.perf_counter() - t
        dev.synchronize()
        el = time.perf_counter() - t0
        n = args.steps
        return {"ms": 1e3 * el / n, "read_ms": 1e3 * read / n, "wait_ms": 1e3 * wait / n, "objects": objects / n}

    for n in LEGS:   # warm-up: every path, every allocation; the objects start here
        leg(n)
    runs = {n: [] for n in LEGS}
    for _ in range(args.rounds):
        for n in LEGS:
            runs[n].append(leg(n))
    # the packed records are the per-stream ones
    step()
    packed = dev.objects_packed()
    dev.synchronize()
    off, same = packed["stream_offsets"], True
    for s in range(streams):
        objs = dev.objects(s)
        rows = range(off[s], off[s + 1])
        same = same and len(objs) == len(rows) and all(
            int(packed["id"][k]) == o["id"] and packed["landmarks"][k].tobytes() == o["landmarks"].tobytes()
            and ("pose" not in o or packed["pose"][k].tobytes() == o["pose"].tobytes()) for k, o in zip(rows, objs))
    if not same:
        raise SystemExit("bench_multi_export: objects_packed() differs from objects(s)")
    legs = {}
    base = statistics.median(r["ms"] for r in runs["no_read"])
    for n in LEGS:
        ms = [r["ms"] for r in runs[n]]
        med = statistics.median(ms)
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(med, 4),
                   "spread_ms": round(max(ms) - min(ms), 4),
                   "added_to_no_read_ms": round(med - base, 4),
                   "median_read_call_ms_per_step": round(statistics.median(r["read_ms"] for r in runs[n]), 4),
                   "objects_read_per_step": round(statistics.median(r["objects"] for r in runs[n]), 1)}
        if n == "objects":
            legs[n]["median_synchronize_ms_per_step"] = round(statistics.median(r["wait_ms"] for r in runs[n]), 4)
    added = {n: legs[n]["added_to_no_read_ms"] for n in LEGS}
    out = {"streams": streams, "slots": slots, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
           "rounds": args.rounds, "pose": not args.plain, "eyes": not args.plain,
           "bytes_per_record": 48 + 468 * 12 + (0 if args.plain else 84 + 2 * (4 + 4 + 20 + 912)),
           "legs": legs, "packed_equals_objects": True,
           "objects_over_packed_loop": round(legs["objects"]["median_ms_per_step"] / legs["packed"]["median_ms_per_step"], 3),
           "objects_over_snapshot_loop": round(legs["objects"]["median_ms_per_step"] / legs["snapshot"]["median_ms_per_step"], 3),
           "added_ms": added}
    del dev, video
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_export_bench.json"))
    ap.add_argument("--shapes", default="1024x4,64x4", help="streams x slots, comma separated")
    ap.add_argument("--sets", type=int, default=2, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=500, help="calls of the export alone")
    ap.add_argument("--plain", action="store_true", help="no pose reference and no eye refinement")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_multi_export: at least five rounds")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    # as bench.py orders it: its environment (hardware queues) first, then torch brings the
    # device up, then the library
    import bench  # noqa: F401
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_export: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import zaru_amd.host as H
    from bench_multi_face import build_video
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_export: no GPU")
    res = {"tool": "tools/bench_multi_export.py",
           "timing": "host clock around `steps` steps of a leg, ending in a stream synchronise; the legs alternate "
                     "in one process after a warm-up leg of each; medians over the rounds",
           "export_alone": [], "shapes": []}
    for streams, slots in shapes:
        for live in (1, slots):
            res["export_alone"].append(export_alone(streams, slots, live, args.reps, 20, args.plain))
            print(json.dumps(res["export_alone"][-1]), file=sys.stderr, flush=True)
        r = run_shape(H, streams, slots, args, build_video)
        print(json.dumps(r), file=sys.stderr, flush=True)
        res["shapes"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
