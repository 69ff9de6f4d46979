#!/usr/bin/env python3
"""What automatic enrolment costs inside the multi-object loop, on the MI355X (GPU only: fails
without one).  The workload is tools/bench_multi_identity.py's: DeviceMultiTracker ("face",
"facemesh") at `--streams` x `--slots` (default 256 x 4) on tools/bench_multi_face.py's video, with
MobileFaceNet (tests/golden) and a gallery of `--gallery` random rows.

Steady state.  Enrolment on and no candidate (the default threshold of +inf against a gallery that is
not empty: every object is known).  A step then enqueues one launch more than without -- the enrol
kernel, which ends after its scan -- and the counted match in place of the plain one.  Each of the
three identify legs of tools/bench_multi_identity.py runs beside its twin with set_enrolment, the six
legs alternating in one process, `--pairs` rounds after two discarded warm-up rounds, a host clock
around `--steps` enqueued steps that ends in a stream synchronise.  A leg and its twin share one
tracker and one reserved gallery; enrolment is switched off and on between them, outside the clock
(trackers of their own differ by more than the quantity measured).  The bound: the twin's median is
no more than max(the two legs' spreads) + 10 us above its leg's (10 us: two launches at the 4-5 us
per call profiles/multi_identity_bench.json records under kernels_alone).  "within_bound" says
whether it held; the exit status is 1 if it did not for some pair.

Cold start.  zr_identity_enrol_async alone between device events at streams x slots rows, every row a
candidate with an embedding of its own and threshold 0: every object of every stream is new in one
step and becomes a row.  The kernel is serial in the candidates by design; the figure is per call and
per candidate.  Beside it the same call with no candidate (the steady state's scan) and with every row
a duplicate of the first (one row appended, streams x slots - 1 matches).

Writes one JSON document (default profiles/multi_enrol_bench.json)."""
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
BASE = {"identify_once": math.inf, "identify_1s": 1000.0, "identify_every_step": 0.0}
LAUNCH_ALLOWANCE_MS = 0.010


def enrol_alone(streams, slots, reps, headroom=64):
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, IdentityCfg, IdentityState
    lib = _lib.lib()
    n = streams * slots
    cap = n + headroom
    rng = np.random.default_rng(4)
    distinct = rng.standard_normal((n, 128)).astype(np.float32)
    same = np.tile(distinct[:1], (n, 1))
    fresh = np.zeros(n, np.dtype(IdentityState))
    fresh["row"], fresh["distance"], fresh["embeddings"] = -1, np.inf, 1
    known = fresh.copy()
    known["row"], known["flags"] = 0, 1
    b = DeviceBuffer.from_array
    d_state, d_of = DeviceBuffer(fresh.nbytes), b(np.arange(n, dtype=np.int32))
    d_rows, d_ids = DeviceBuffer(cap * 512), DeviceBuffer(cap * 8)
    d_count, d_next, d_counts = DeviceBuffer(4), b(np.zeros(1, np.uint64)), b(np.zeros(2, np.uint64))
    zero = np.zeros(1, np.int32)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))
    out = {"rows": n, "slots": slots, "capacity": cap, "reps": reps,
           "timing": "device events around one call; states and count restored on the stream before each"}
    for name, states, emb, thr, appended in (("cold_start_all_distinct", fresh, distinct, 0.0, n),
                                             ("all_duplicates_of_the_first", fresh, same, 0.0, 1),
                                             ("steady_state_no_candidate", known, distinct, math.inf, 0)):
        d_emb = b(emb)
        cfg = IdentityCfg(slots, 468, 1, 1, 0.4, thr, 1000.0)
        us = []
        for _ in range(reps + 2):
            _lib.check(lib.zr_memcpy_async(d_state.ptr, states.ctypes.data, states.nbytes, 0, stream))
            _lib.check(lib.zr_memcpy_async(d_count.ptr, zero.ctypes.data, 4, 0, stream))
            _lib.check(lib.zr_event_record(ev[0], stream))
            _lib.check(lib.zr_identity_enrol_async(C.byref(cfg), n, d_of.ptr, d_state.ptr, d_emb.ptr, d_rows.ptr,
                                                   d_ids.ptr, d_count.ptr, d_next.ptr, cap, 128, 1, d_counts.ptr,
                                                   d_counts.ptr + 8, stream))
            _lib.check(lib.zr_event_record(ev[1], stream))
            _lib.check(lib.zr_event_synchronize(ev[1]))
            ms = C.c_float()
            _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
            us.append(1e3 * ms.value)
        assert d_count.download((1,), np.int32)[0] == appended, name
        us = us[2:]   # the first calls warm the code object
        med = statistics.median(us)
        out[name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(min(us), 2),
                     "us_per_call_max": round(max(us), 2), "rows_appended": appended,
                     "us_per_row": round(med / n, 4)}
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_enrol_bench.json"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--headroom", type=int, default=1024, help="reserved rows past the gallery's")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("bench_multi_enrol: at least five rounds")
    import bench  # noqa: F401  (its environment first, then torch brings the device up, then the library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_enrol: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import bench_multi_face
    import make_golden_recognition as mg
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_enrol: no GPU")
    S, K = args.streams, args.slots
    res = {"tool": "tools/bench_multi_enrol.py", "enrol_kernel_alone": enrol_alone(S, K, args.reps)}
    print(json.dumps(res["enrol_kernel_alone"]), file=sys.stderr, flush=True)
    video, lists, frame = bench_multi_face.build_video(S, args.sets, args.device)
    model = mg.load_model_bytes()
    rng = np.random.default_rng(3)
    rows, ids = rng.standard_normal((args.gallery, 128)).astype(np.float32), list(range(args.gallery))
    # A leg and its twin share one tracker and one reserved gallery, enrolment switched off and on
    # between the legs (outside the clock): off, a step enqueues exactly what it does without
    # set_enrolment, and no difference between two trackers' buffers enters the comparison.
    legs_of, trackers, galleries, clocks = {}, {}, {}, {}
    for name, interval in BASE.items():
        g = H.Gallery(args.device)
        g.add(rows, ids)
        g.reserve(args.gallery + args.headroom)
        t = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
        t.set_recognition(model, g)
        t.set_identify_interval(interval)
        legs_of[name], legs_of[name + "+enrol"] = False, True
        for n in (name, name + "+enrol"):
            trackers[n], galleries[n] = t, g
        clocks[t] = 0

    def leg(name):
        t = trackers[name]
        t.set_enrolment(galleries[name] if legs_of[name] else None, 10 ** 6)
        name = t   # the clock is the tracker's
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

    for _ in range(2):  # warm-up, discarded: every path, every shape; the objects start and are first
        for n in legs_of:   # identified in the first round, and the second brings the device to its pace
            leg(n)
    runs = {n: [] for n in legs_of}
    for _ in range(args.pairs):
        for n in legs_of:
            runs[n].append(leg(n))
    legs = {}
    for n in legs_of:
        ms = [r["ms"] for r in runs[n]]
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(statistics.median(ms), 4),
                   "spread_ms": round(max(ms) - min(ms), 4),
                   "live_objects": statistics.median(r["live"] for r in runs[n]),
                   "embeddings_per_step": [round(r["embeddings"], 2) for r in runs[n]]}
    ok = True
    for n in BASE:
        a, e = legs[n], legs[n + "+enrol"]
        bound = max(a["spread_ms"], e["spread_ms"]) + LAUNCH_ALLOWANCE_MS
        delta = e["median_ms_per_step"] - a["median_ms_per_step"]
        t = trackers[n + "+enrol"]
        e["vs_" + n] = {"delta_ms_per_step": round(delta, 4), "bound_ms": round(bound, 4),
                        "within_bound": bool(delta <= bound)}
        e["enrolled_total"], e["enrol_dropped"] = t.enrolled_total(), t.enrol_dropped()
        ok = ok and delta <= bound and e["enrolled_total"] == 0
    res["steady_state"] = {
        "streams": S, "slots": K, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
        "rounds": args.pairs, "frame_clock_ms": FRAME_MS, "gallery_rows": args.gallery,
        "reserved_capacity": args.gallery + args.headroom,
        "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; the legs "
                  "alternate in one process after a warm-up leg of each, a leg and its +enrol twin on one tracker, enrolment switched between them",
        "bound": "median(leg+enrol) - median(leg) <= max(spread of either) + 0.010 ms",
        "legs": legs, "all_within_bound": bool(ok),
    }
    del trackers, video
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
