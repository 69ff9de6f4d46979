#!/usr/bin/env python3
"""Multi-face tracking on the MI355X (GPU only: fails without one): DeviceMultiTracker
("face", "facemesh") at `--streams` x `--slots` (default 256 x 4) on 1080p noise frames that each
carry one face patch, so one live object per stream after the warm-up.

Three legs alternate in one process, `--pairs` rounds after a warm-up of each, every leg a host
clock around `--steps` enqueued steps that ends in a stream synchronise:
  face_loop   DeviceFaceLoop ("face", "facemesh") at the same stream count and video: the nearest
              single-face capability (one RoI per stream, detector on loss only);
  compact_on  DeviceMultiTracker with the live slots packed (zr_slot_compact_async): the landmark
              network runs on the live objects;
  compact_off the same with the network on all streams x slots views (DeviceHandTracker's schedule).
  filter_ema, filter_one_euro (not in the default legs: `--legs`)  compact_on with a landmark
              filter set (set_filter): zr_lm_filter_indexed_async + the update on its positions
              instead of the plain update.
Reports each leg's medians and spread, tracked faces/s, landmark images and detector frames per
step, and the time of zr_slot_compact_async alone (device events around back-to-back calls).  With
a filter leg it also times zr_lm_filter_indexed_async alone at streams x slots rows x 468
landmarks, beside zr_lm_filter_async on the same shape: microseconds, bytes per call computed here
from the shapes and the state layout, and the rate.

Writes one JSON document (default profiles/multi_face_bench.json)."""
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

FRAME_MS = 33.0  # the clock handed to the tracker: 30 frames/s, so the 300 ms redetection fires every 10th step


def build_video(streams, sets, device):
    """bench.py's frames (seeded noise + the face patch), `sets` frames per stream with the patch
    drifting a few pixels per frame; returns the tensor (kept alive by the caller) and frame lists."""
    import torch

    import bench
    rng = np.random.default_rng(bench.WORKLOADS["face"][5])
    fs = bench.FrameSet(rng, streams, patch=bench.load_patch())
    dev = f"cuda:{device}"
    patch = torch.from_numpy(bench.load_patch()).to(dev)
    base = torch.from_numpy(fs.base).to(dev)
    ph, pw = patch.shape[:2]
    video = torch.empty((sets, streams, fs.h, fs.w, 4), dtype=torch.uint8, device=dev)
    for v in range(sets):
        for s in range(streams):
            video[v, s].copy_(base[s % len(fs.base)])
            y, x = fs.pos[s]
            y, x = min(fs.h - ph, y + 2 * v), min(fs.w - pw, x + 3 * v)
            video[v, s, y:y + ph, x:x + pw] = patch
    torch.cuda.synchronize(device)
    lists = [[(video[v, s].data_ptr(), fs.w, fs.h, fs.w * 4) for s in range(streams)] for v in range(sets)]
    return video, lists, f"{fs.w}x{fs.h}"


def compact_alone(streams, slots, reps, warmup):
    from zaru_amd import _lib
    lib = _lib.lib()
    counts = _lib.DeviceBuffer.from_array(np.ones(streams, np.int32))
    views = _lib.DeviceBuffer.from_array(np.zeros((streams * slots, 10), np.float32))
    dense = _lib.DeviceBuffer(streams * slots * 40)
    dense_of = _lib.DeviceBuffer(streams * slots * 4)
    nact = _lib.DeviceBuffer(4)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))

    def call():
        _lib.check(lib.zr_slot_compact_async(counts.ptr, streams, slots, views.ptr, dense.ptr, dense_of.ptr, nact.ptr,
                                             None, stream))
    for _ in range(warmup):
        call()
    _lib.check(lib.zr_event_record(ev[0], stream))
    for _ in range(reps):
        call()
    _lib.check(lib.zr_event_record(ev[1], stream))
    _lib.check(lib.zr_event_synchronize(ev[1]))
    ms = C.c_float()
    _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
    assert nact.download((1,), np.int32)[0] == streams
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return {"streams": streams, "slots": slots, "live_per_stream": 1, "reps": reps,
            "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)",
            "us_per_call": round(1e3 * ms.value / reps, 3)}


FILTER_LEGS = {"filter_ema": ("ema", 1, (0.6,)), "filter_one_euro": ("one_euro", 3, (1.0, 0.05, 1.0))}


def filter_alone(streams, slots, reps, warmup, L=468):
    """zr_lm_filter_indexed_async (every row live, the estimates in a shuffled dense order, every
    state gathered from another slot of its stream, the two state buffers swapping roles per call)
    and zr_lm_filter_async on the same rows.  Bytes per value: input read + position write, the
    primed word and the state floats read and written (the indexed form also writes the primed
    word); the per-row tables are left out."""
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, LmFilter, TrackCfg, TrackState
    lib = _lib.lib()
    n = streams * slots
    rng = np.random.default_rng(1)
    lm = DeviceBuffer.from_array(rng.normal(96.0, 40.0, (n, 3 * L)).astype(np.float32))
    flag = DeviceBuffer.from_array(np.ones((n, 1), np.float32))
    pos = DeviceBuffer(n * L * 3 * 4)
    st = (TrackState * n)()
    for i in range(n):
        st[i].active = 1
    state = DeviceBuffer.from_array(np.frombuffer(bytes(st), np.uint8))
    index = DeviceBuffer.from_array(rng.permutation(n).astype(np.int32))
    src = DeviceBuffer.from_array(np.tile((np.arange(slots, dtype=np.int32) + 1) % slots, streams))
    cfg = TrackCfg(0, L, 192, 192, 1, 1, 0.5, 0.3, slots)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))
    out = []
    for name, kind, p in (("none", 0, ()), ("ema", 1, (0.6,)), ("alpha_beta", 2, (0.5, 0.1)),
                          ("one_euro", 3, (1.0, 0.05, 1.0))):
        f = LmFilter.make(kind, *p)
        sb = _lib.lm_filter_state_size(f, L)
        bufs = [DeviceBuffer(max(4, n * sb)), DeviceBuffer(max(4, n * sb))]
        row = {"filter": name, "state_bytes_per_row": sb}
        for form in ("indexed", "plain"):
            for b in bufs:
                _lib.check(lib.zr_memset_async(b.ptr, 0, max(4, n * sb), stream))
            k = {"i": 0}

            def call():
                a, b = bufs[k["i"] & 1], bufs[1 - (k["i"] & 1)]
                k["i"] += 1
                if form == "indexed":
                    _lib.check(lib.zr_lm_filter_indexed_async(
                        C.byref(f), C.byref(cfg), state.ptr, n, slots, lm.ptr, 3 * L, flag.ptr, 1, index.ptr, src.ptr,
                        1.0 / 30.0, a.ptr if sb else None, b.ptr if sb else None, pos.ptr, stream))
                else:
                    _lib.check(lib.zr_lm_filter_async(C.byref(f), C.byref(cfg), state.ptr, n, lm.ptr, 3 * L, flag.ptr,
                                                      1, 1.0 / 30.0, a.ptr if sb else None, pos.ptr, stream))
            for _ in range(warmup):  # the first calls prime every value; the timed ones all filter
                call()
            _lib.check(lib.zr_event_record(ev[0], stream))
            for _ in range(reps):
                call()
            _lib.check(lib.zr_event_record(ev[1], stream))
            _lib.check(lib.zr_event_synchronize(ev[1]))
            ms = C.c_float()
            _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
            floats = {0: 0, 1: 1, 2: 2, 3: 2}[kind]
            per_value = 8 + 8 * floats + (0 if kind == 0 else 8 if form == "indexed" else 4)
            nbytes = n * L * 3 * per_value
            us = 1e3 * ms.value / reps
            row[form] = {"us_per_call": round(us, 3), "bytes_per_call": nbytes,
                         "GB_per_s": round(nbytes / (us * 1e-6) / 1e9, 1)}
        out.append(row)
        for b in bufs:
            b.free()
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return {"rows": n, "slots": slots, "landmarks": L, "values_per_call": n * L * 3, "reps": reps, "warmup": warmup,
            "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)",
            "kinds": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_face_bench.json"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--legs", default="face_loop,compact_on,compact_off",
                    help="the legs to run (a profiler run wants one); the comparisons need all three")
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("bench_multi_face: at least five rounds")
    # as bench.py orders it: its environment (hardware queues) first, then torch brings the
    # device up, then the library
    import bench  # noqa: F401
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_face: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_face: no GPU")
    S, K = args.streams, args.slots
    names = tuple(args.legs.split(","))
    known = ("face_loop", "compact_on", "compact_off") + tuple(FILTER_LEGS)
    if not names or any(n not in known for n in names):
        raise SystemExit("bench_multi_face: --legs takes " + ", ".join(known))
    res = {"tool": "tools/bench_multi_face.py", "slot_compact_alone": compact_alone(S, K, args.reps, 50)}
    print(json.dumps(res["slot_compact_alone"]), file=sys.stderr, flush=True)
    if any(n in FILTER_LEGS for n in names):
        res["lm_filter_indexed_alone"] = filter_alone(S, K, args.reps, 50)
        print(json.dumps(res["lm_filter_indexed_alone"]), file=sys.stderr, flush=True)
    video, lists, frame = build_video(S, args.sets, args.device)
    loop = H.DeviceFaceLoop("face", "facemesh", S, args.device)
    multi = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
    clock = {"k": 0, "filter": None}
    host_filter = {"ema": H.Ema, "one_euro": H.OneEuro}

    def leg(name):
        if name == "face_loop":
            loop.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                loop.step(lists[k % args.sets])
            loop.synchronize()
            el = time.perf_counter() - t0
            live = sum(1 for st in loop.states() if st["tracked"])
            return {"ms": 1e3 * el / args.steps, "live": live}
        multi.set_compact(name != "compact_off")
        want = FILTER_LEGS.get(name)
        if want != clock["filter"]:  # a filter leg starts from the default state, the others carry none
            multi.set_filter(None if want is None else host_filter[want[0]](*want[2]))
            clock["filter"] = want
        multi.synchronize()
        img0, det0 = multi.landmark_images(), multi.detector_frames()
        t0 = time.perf_counter()
        for k in range(args.steps):
            multi.step(lists[k % args.sets], FRAME_MS * clock["k"])
            clock["k"] += 1
        multi.synchronize()
        el = time.perf_counter() - t0
        return {"ms": 1e3 * el / args.steps, "live": sum(multi.object_counts()),
                "lm_images": (multi.landmark_images() - img0) / args.steps,
                "det_frames": (multi.detector_frames() - det0) / args.steps}

    for n in names:  # warm-up: every path, every shape; the objects start here
        leg(n)
    runs = {n: [] for n in names}
    for _ in range(args.pairs):
        for n in names:
            runs[n].append(leg(n))
    legs = {}
    for n in names:
        ms = [r["ms"] for r in runs[n]]
        med = statistics.median(ms)
        live = statistics.median(r["live"] for r in runs[n])
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(med, 4),
                   "median_us_per_step": round(1e3 * med, 1), "spread_ms": round(max(ms) - min(ms), 4),
                   "live_objects": live, "tracked_faces_per_s": round(live / (med * 1e-3), 1)}
        if n != "face_loop":
            legs[n]["landmark_images_per_step"] = round(statistics.median(r["lm_images"] for r in runs[n]), 2)
            legs[n]["detector_frames_per_step"] = round(statistics.median(r["det_frames"] for r in runs[n]), 2)
    res["loop"] = {
        "streams": S, "slots": K, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
        "rounds": args.pairs, "frame_clock_ms": FRAME_MS,
        "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; the legs "
                  "alternate in one process after a warm-up leg of each",
        "legs": legs,
    }
    for n in names:
        if n in FILTER_LEGS and "compact_on" in legs:
            on, fl = legs["compact_on"], legs[n]
            res["loop"][n + "_vs_compact_on"] = {
                "delta_ms_per_step": round(fl["median_ms_per_step"] - on["median_ms_per_step"], 4),
                "ratio": round(fl["median_ms_per_step"] / on["median_ms_per_step"], 4),
                "spread_ms": max(on["spread_ms"], fl["spread_ms"])}
    if all(n in legs for n in ("compact_on", "compact_off", "face_loop")):
        on, off, fl = (legs[n]["median_ms_per_step"] for n in ("compact_on", "compact_off", "face_loop"))
        res["loop"]["compact_on_vs_off"] = {
            "delta_ms_per_step": round(on - off, 4), "speedup": round(off / on, 4),
            "spread_ms": max(legs["compact_on"]["spread_ms"], legs["compact_off"]["spread_ms"])}
        res["loop"]["compact_on_vs_face_loop"] = {"delta_ms_per_step": round(on - fl, 4), "ratio": round(on / fl, 4)}
    del loop, multi, video
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
