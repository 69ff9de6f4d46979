#!/usr/bin/env python3
"""What aligned identity crops cost inside the multi-object loop, on the MI355X (GPU only: fails without
one): tools/bench_multi_identity.py's `identify_1s` and `identify_every_step` legs -- DeviceMultiTracker
("face", "facemesh") at `--streams` x `--slots` (default 256 x 4) on tools/bench_multi_face.py's video,
MobileFaceNet and a gallery of `--gallery` random rows, the same leg discipline (a warm-up of each leg, then
`--pairs` alternating rounds, every leg a tracker of its own and a host clock around `--steps` enqueued steps
that ends in a stream synchronise) -- without alignment, or with `--align`:
set_identity_alignment(FaceAlignment.facemesh_five_point()) on both legs.

One process measures one setting, so that "off" here, "off" on another build of the project (run that build's
tools/bench_multi_identity.py) and "on" can alternate process by process.  With `--align` the kernel alone is
timed too, between device events (back-to-back calls on one stream) at streams x slots rows x 468 landmarks
with one due row per stream.

Prints one JSON document; `--out FILE` also writes it."""
import argparse
import ctypes as C
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
LEGS = {"identify_1s": 1000.0, "identify_every_step": 0.0}


def kernel_alone(streams, slots, reps, warmup, L=468):
    """Slot 0 of every stream due, its landmarks a fixture mesh scaled and turned; the others idle."""
    from zaru_amd import _lib
    from zaru_amd._lib import AlignCfg, DeviceBuffer, FaceAlignment, TrackState
    import zaru_amd.host as H
    lib = _lib.lib()
    n = streams * slots
    rng = np.random.default_rng(4)
    mesh = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))["landmarks"].astype(np.float32)
    st = (TrackState * n)()
    lm = np.zeros((n, L, 3), np.float32)
    for i in range(n):
        st[i].tracked, st[i].active, st[i].frame_w, st[i].frame_h = 1, 1, 1920, 1080
        ang, s = rng.uniform(-0.5, 0.5), rng.uniform(1.0, 3.0)
        m = mesh[i % 3]
        x, y = m[:, 0] - 96.0, m[:, 1] - 96.0
        lm[i, :, 0] = s * (np.cos(ang) * x - np.sin(ang) * y) + 960.0
        lm[i, :, 1] = s * (np.sin(ang) * x + np.cos(ang) * y) + 540.0
    b = DeviceBuffer.from_array
    state, d_lm = b(np.frombuffer(bytes(st), np.uint8)), b(lm)
    due0 = np.zeros(n, np.int32)
    due0[::slots] = 1
    due, views = b(due0), b(np.zeros((n, 10), np.float32))
    recs, totals = b(np.zeros(n, np.dtype(FaceAlignment))), b(np.zeros(2, np.uint64))
    cfg = AlignCfg.from_buffer_copy(H.FaceAlignment.facemesh_five_point().cfg_bytes())
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))

    def call():
        return lib.zr_identity_align_async(C.byref(cfg), state.ptr, n, d_lm.ptr, L, due.ptr, views.ptr, recs.ptr,
                                           totals.ptr, stream)
    for _ in range(warmup):
        _lib.check(call())
    _lib.check(lib.zr_event_record(ev[0], stream))
    for _ in range(reps):
        _lib.check(call())
    _lib.check(lib.zr_event_record(ev[1], stream))
    _lib.check(lib.zr_event_synchronize(ev[1]))
    ms = C.c_float()
    _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
    got = totals.download((2,), np.uint64).tolist()
    assert got == [streams * (reps + warmup), 0], got   # every due row aligned, every call
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return {"rows": n, "slots": slots, "landmarks": L, "due_rows": streams, "reps": reps, "warmup": warmup,
            "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)",
            "align_us_per_call": round(1e3 * ms.value / reps, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--align", action="store_true", help="aligned crops on in both legs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("bench_multi_align: at least five rounds")
    import bench  # noqa: F401  (its environment first, then torch brings the device up, then the library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_align: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import bench_multi_face
    import make_golden_recognition as mg
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_align: no GPU")
    S, K = args.streams, args.slots
    res = {"tool": "tools/bench_multi_align.py", "align": bool(args.align)}
    if args.align:
        res["kernel_alone"] = kernel_alone(S, K, args.reps, 50)
        print(json.dumps(res["kernel_alone"]), file=sys.stderr, flush=True)
    video, lists, frame = bench_multi_face.build_video(S, args.sets, args.device)
    model = mg.load_model_bytes()
    gallery = H.Gallery(args.device)
    rng = np.random.default_rng(3)
    gallery.add(rng.standard_normal((args.gallery, 128)).astype(np.float32), list(range(args.gallery)))
    trackers, clocks = {}, {}
    for name, interval in LEGS.items():
        t = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
        t.set_recognition(model, gallery)
        t.set_identify_interval(interval)
        if args.align:
            t.set_identity_alignment(H.FaceAlignment.facemesh_five_point())
        trackers[name], clocks[name] = t, 0

    def leg(name):
        t = trackers[name]
        t.synchronize()
        before = (t.identity_images(), t.aligned_total(), t.align_fallback_total())
        t0 = time.perf_counter()
        for _ in range(args.steps):
            t.step(lists[clocks[name] % args.sets], FRAME_MS * clocks[name])
            clocks[name] += 1
        t.synchronize()
        el = time.perf_counter() - t0
        after = (t.identity_images(), t.aligned_total(), t.align_fallback_total())
        per = [(a - b) / args.steps for a, b in zip(after, before)]
        return {"ms": 1e3 * el / args.steps, "live": sum(t.object_counts()), "embeddings": per[0], "aligned": per[1],
                "fallbacks": per[2]}

    for n in LEGS:  # warm-up: every path, every shape; the objects start and are first identified here
        leg(n)
    runs = {n: [] for n in LEGS}
    for _ in range(args.pairs):
        for n in LEGS:
            runs[n].append(leg(n))
    legs = {}
    for n in LEGS:
        ms = [r["ms"] for r in runs[n]]
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(statistics.median(ms), 4),
                   "spread_ms": round(max(ms) - min(ms), 4),
                   "live_objects": statistics.median(r["live"] for r in runs[n]),
                   "embeddings_per_step": [round(r["embeddings"], 2) for r in runs[n]],
                   "aligned_per_step": [round(r["aligned"], 2) for r in runs[n]],
                   "fallbacks_per_step": [round(r["fallbacks"], 2) for r in runs[n]]}
    res["loop"] = {
        "streams": S, "slots": K, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
        "rounds": args.pairs, "frame_clock_ms": FRAME_MS, "gallery_rows": args.gallery,
        "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; the legs "
                  "alternate in one process after a warm-up leg of each, each leg a tracker of its own",
        "legs": legs,
    }
    del trackers, video
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
