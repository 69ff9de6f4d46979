#!/usr/bin/env python3
"""What recognition costs inside the multi-object loop, on the MI355X (GPU only: fails without
one): DeviceMultiTracker ("face", "facemesh") at `--streams` x `--slots` (default 256 x 4) on
tools/bench_multi_face.py's video (1080p noise frames with one face patch each, so one live object
per stream after the warm-up), with MobileFaceNet (tests/golden) and a gallery of `--gallery` random
rows.

Four legs alternate in one process, `--pairs` rounds after a warm-up of each, every leg a tracker of
its own and a host clock around `--steps` enqueued steps that ends in a stream synchronise:
  track_only           no recognition: the baseline
  identify_once        set_identify_interval(+inf): in steady state every object is identified, so a
                       step pays the select / compact / commit launches and the embedding network's
                       and the match's launches at a device count of 0
  identify_1s          the default interval of 1000 ms on the 33 ms frame clock
  identify_every_step  interval 0: one MobileFaceNet pass over the live faces per step
Reports each leg's medians and spread, tracked faces/s, embeddings per step, the ratios to
track_only, and the three new kernels alone between device events (back-to-back calls on one
stream) at streams x slots rows x 468 landmarks with one due row per stream.

Writes one JSON document (default profiles/multi_identity_bench.json)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

FRAME_MS = 33.0
LEGS = {"track_only": None, "identify_once": math.inf, "identify_1s": 1000.0, "identify_every_step": 0.0}


def kernels_alone(streams, slots, reps, warmup, L=468):
    """Slot 0 of every stream tracked and due (never embedded), the others idle."""
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, IdentityCfg, IdentityState, TrackState
    lib = _lib.lib()
    n = streams * slots
    rng = np.random.default_rng(2)
    st = (TrackState * n)()
    for i in range(0, n, slots):
        st[i].tracked, st[i].active, st[i].frame_w, st[i].frame_h = 1, 1, 1920, 1080
    b = DeviceBuffer.from_array
    state = b(np.frombuffer(bytes(st), np.uint8))
    lm = b(rng.uniform(100.0, 900.0, (n, L, 3)).astype(np.float32))
    src = b(np.zeros(n, np.int32))
    sin = np.zeros(n, np.dtype(IdentityState))
    sin["row"], sin["distance"] = -1, np.inf
    states = [b(sin), b(sin)]
    embs = [b(np.zeros((n, 128), np.float32)), b(np.zeros((n, 128), np.float32))]
    due, views, dviews, due_of = DeviceBuffer(n * 4), DeviceBuffer(n * 40), DeviceBuffer(n * 40), DeviceBuffer(n * 4)
    ndue, valid = DeviceBuffer(4), DeviceBuffer(n * 4)
    best, dist = b(np.zeros(n, np.int32)), b(np.ones(n, np.float32))
    dense = b(rng.standard_normal((n, 128)).astype(np.float32))
    cfg = IdentityCfg(slots, L, 1, 1, 0.4, math.inf, 1000.0)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))
    calls = {
        # in and out stay as they are, so every call sees the same due rows
        "select": lambda: lib.zr_identity_select_async(C.byref(cfg), state.ptr, n, lm.ptr, src.ptr, 0.0, states[0].ptr,
                                                       embs[0].ptr, states[1].ptr, embs[1].ptr, due.ptr, views.ptr,
                                                       stream),
        "compact": lambda: lib.zr_identity_compact_async(due.ptr, views.ptr, n, dviews.ptr, due_of.ptr, ndue.ptr,
                                                         valid.ptr, None, stream),
        "commit": lambda: lib.zr_identity_commit_async(C.byref(cfg), n, due_of.ptr, best.ptr, dist.ptr, dense.ptr, 0.0,
                                                       states[1].ptr, embs[1].ptr, stream),
    }
    out = {"rows": n, "slots": slots, "landmarks": L, "due_rows": streams, "reps": reps, "warmup": warmup,
           "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)"}
    for name in ("select", "compact", "commit"):
        for _ in range(warmup):
            _lib.check(calls[name]())
        _lib.check(lib.zr_event_record(ev[0], stream))
        for _ in range(reps):
            _lib.check(calls[name]())
        _lib.check(lib.zr_event_record(ev[1], stream))
        _lib.check(lib.zr_event_synchronize(ev[1]))
        ms = C.c_float()
        _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
        out[name + "_us_per_call"] = round(1e3 * ms.value / reps, 3)
    assert ndue.download((1,), np.int32)[0] == streams
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_identity_bench.json"))
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
        raise SystemExit("bench_multi_identity: at least five rounds")
    import bench  # noqa: F401  (its environment first, then torch brings the device up, then the library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_identity: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import bench_multi_face
    import make_golden_recognition as mg
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_identity: no GPU")
    S, K = args.streams, args.slots
    res = {"tool": "tools/bench_multi_identity.py", "kernels_alone": kernels_alone(S, K, args.reps, 50)}
    print(json.dumps(res["kernels_alone"]), file=sys.stderr, flush=True)
    video, lists, frame = bench_multi_face.build_video(S, args.sets, args.device)
    model = mg.load_model_bytes()
    gallery = H.Gallery(args.device)
    rng = np.random.default_rng(3)
    gallery.add(rng.standard_normal((args.gallery, 128)).astype(np.float32), list(range(args.gallery)))
    trackers, clocks = {}, {}
    for name, interval in LEGS.items():
        t = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
        if interval is not None:
            t.set_recognition(model, gallery)
            t.set_identify_interval(interval)
        trackers[name], clocks[name] = t, 0

    def leg(name):
        t = trackers[name]
        t.synchronize()
        id0 = t.identity_images()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            t.step(lists[clocks[name] % args.sets], FRAME_MS * clocks[name])
            clocks[name] += 1
        t.synchronize()
        el = time.perf_counter() - t0
        return {"ms": 1e3 * el / args.steps, "live": sum(t.object_counts()),
                "embeddings": (t.identity_images() - id0) / args.steps}

    for n in LEGS:  # warm-up: every path, every shape; the objects start and are first identified here
        leg(n)
    runs = {n: [] for n in LEGS}
    for _ in range(args.pairs):
        for n in LEGS:
            runs[n].append(leg(n))
    legs = {}
    for n in LEGS:
        ms = [r["ms"] for r in runs[n]]
        med = statistics.median(ms)
        live = statistics.median(r["live"] for r in runs[n])
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(med, 4),
                   "spread_ms": round(max(ms) - min(ms), 4), "live_objects": live,
                   "tracked_faces_per_s": round(live / (med * 1e-3), 1),
                   "embeddings_per_step": [round(r["embeddings"], 2) for r in runs[n]]}
    base = legs["track_only"]["median_ms_per_step"]
    for n in LEGS:
        if n != "track_only":
            legs[n]["vs_track_only"] = {"delta_ms_per_step": round(legs[n]["median_ms_per_step"] - base, 4),
                                        "ratio": round(legs[n]["median_ms_per_step"] / base, 4)}
    res["loop"] = {
        "streams": S, "slots": K, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
        "rounds": args.pairs, "frame_clock_ms": FRAME_MS, "gallery_rows": args.gallery,
        "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; the legs "
                  "alternate in one process after a warm-up leg of each, each leg a tracker of its own",
        "legs": legs,
    }
    del trackers, video
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
