#!/usr/bin/env python3
"""What identities that learn cost inside the multi-object loop, on the MI355X (GPU only: fails
without one).  The workload is tools/bench_multi_enrol.py's: DeviceMultiTracker ("face", "facemesh")
at `--streams` x `--slots` (default 256 x 4) on tools/bench_multi_face.py's video, with MobileFaceNet
(tests/golden) and a gallery of `--gallery` random rows reserved to `--gallery` + `--headroom`.

The loop.  Each of the three identify legs of tools/bench_multi_identity.py runs beside its twin with
set_identity_smoothing(8) and set_gallery_refinement(gallery, 64) (the identity threshold is +inf: every
object is known and contributes whenever it is embedded).  A leg and its twin share one tracker and
one gallery, the two settings switched between them outside the clock; the six legs alternate in one
process, `--pairs` rounds after two discarded warm-up rounds, a host clock around `--steps` enqueued
steps that ends in a stream synchronise.  The twin enqueues two launches more per step (blend, refine).
The bound is tools/bench_multi_enrol.py's: the twin's median is no more than max(the two legs'
spreads) + 10 us per added launch above its leg's.  "within_bound" says whether it held; nothing is
tuned to make it hold, and the exit status is 1 if it did not for some pair.

The kernels alone.  zr_identity_blend_async and zr_identity_refine_async between device events,
`--calls` calls after `--warm` warm-ups, per call: nothing due; 256 due rows (refine: contributors on
256 distinct gallery rows); 1024 due rows (refine: all on one gallery row, one chain of 1024).

Writes one JSON document (default profiles/multi_template_bench.json)."""
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
ADDED_LAUNCHES = 2
TEMPLATE_CAP, MAX_SAMPLES = 8, 64


def kernels_alone(n, slots, calls, warm):
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, IdentityCfg, IdentityState
    lib = _lib.lib()
    rng = np.random.default_rng(4)
    b = DeviceBuffer.from_array
    dense, emb = rng.standard_normal((n, 128)).astype(np.float32), rng.standard_normal((n, 128)).astype(np.float32)
    d_dense, d_emb, d_query = b(dense), b(emb), DeviceBuffer(n * 512)
    d_rows, d_upd = b(rng.standard_normal((n, 128)).astype(np.float32)), b(np.zeros(n, np.uint32))
    d_count, d_total = b(np.array([n], np.int32)), b(np.zeros(1, np.uint64))
    cfg = IdentityCfg(slots, 468, 1, 1, 0.4, math.inf, 1000.0)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))

    def timed(call):
        for _ in range(warm):
            call()
        _lib.check(lib.zr_event_record(ev[0], stream))
        for _ in range(calls):
            call()
        _lib.check(lib.zr_event_record(ev[1], stream))
        _lib.check(lib.zr_event_synchronize(ev[1]))
        ms = C.c_float()
        _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
        return round(1e3 * ms.value / calls, 3)

    out = {"rows": n, "slots": slots, "calls": calls, "warm_ups": warm,
           "timing": "device events around `calls` back-to-back calls on one stream, per call"}
    for name, due, rows_of in (("nothing_due", 0, None), ("256_due_distinct_rows", 256, "distinct"),
                               ("1024_due_one_row", 1024, "one")):
        due = min(due, n)
        due_of = np.full(n, -1, np.int32)
        due_of[:due] = np.arange(due)
        st = np.zeros(n, np.dtype(IdentityState))
        st["row"], st["distance"], st["embeddings"] = -1, np.inf, 3
        st["row"][:due] = np.arange(due) if rows_of == "distinct" else 0
        st["distance"][:due] = 0.5
        d_of, d_st = b(due_of), b(st)
        out[name] = {
            "due_rows": due,
            "blend_us_per_call": timed(lambda: _lib.check(lib.zr_identity_blend_async(
                C.byref(cfg), n, d_of.ptr, d_st.ptr, d_emb.ptr, d_dense.ptr, TEMPLATE_CAP, d_query.ptr, stream))),
            "refine_us_per_call": timed(lambda: _lib.check(lib.zr_identity_refine_async(
                C.byref(cfg), n, d_of.ptr, d_st.ptr, d_dense.ptr, d_rows.ptr, d_upd.ptr, d_count.ptr, n, 128,
                MAX_SAMPLES, math.inf, d_total.ptr, stream)))}
    out["contributions_applied"] = int(d_total.download((1,), np.uint64)[0])
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_template_bench.json"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--headroom", type=int, default=1024, help="reserved rows past the gallery's")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("bench_multi_templates: at least five rounds")
    import bench  # noqa: F401  (its environment first, then torch brings the device up, then the library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_templates: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import bench_multi_face
    import make_golden_recognition as mg
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_templates: no GPU")
    S, K = args.streams, args.slots
    res = {"tool": "tools/bench_multi_templates.py", "kernels_alone": kernels_alone(S * K, K, args.calls, args.warm)}
    print(json.dumps(res["kernels_alone"]), file=sys.stderr, flush=True)
    video, lists, frame = bench_multi_face.build_video(S, args.sets, args.device)
    model = mg.load_model_bytes()
    rng = np.random.default_rng(3)
    rows, ids = rng.standard_normal((args.gallery, 128)).astype(np.float32), list(range(args.gallery))
    twin_of, trackers, galleries, clocks = {}, {}, {}, {}
    for name, interval in BASE.items():
        g = H.Gallery(args.device)
        g.add(rows, ids)
        g.reserve(args.gallery + args.headroom)
        t = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
        t.set_recognition(model, g)
        t.set_identify_interval(interval)
        twin_of[name], twin_of[name + "+templates"] = False, True
        for n in (name, name + "+templates"):
            trackers[n], galleries[n] = t, g
        clocks[t] = 0

    def leg(name):
        t = trackers[name]
        t.set_identity_smoothing(TEMPLATE_CAP if twin_of[name] else 1)
        t.set_gallery_refinement(galleries[name] if twin_of[name] else None, MAX_SAMPLES)
        t.synchronize()
        id0, r0 = t.identity_images(), t.refined_total()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            t.step(lists[clocks[t] % args.sets], FRAME_MS * clocks[t])
            clocks[t] += 1
        t.synchronize()
        el = time.perf_counter() - t0
        return {"ms": 1e3 * el / args.steps, "live": sum(t.object_counts()),
                "embeddings": (t.identity_images() - id0) / args.steps,
                "refined": (t.refined_total() - r0) / args.steps}

    for _ in range(2):  # warm-up, discarded: every path, every shape, the query buffer's allocation
        for n in twin_of:
            leg(n)
    runs = {n: [] for n in twin_of}
    for _ in range(args.pairs):
        for n in twin_of:
            runs[n].append(leg(n))
    legs = {}
    for n in twin_of:
        ms = [r["ms"] for r in runs[n]]
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(statistics.median(ms), 4),
                   "spread_ms": round(max(ms) - min(ms), 4),
                   "live_objects": statistics.median(r["live"] for r in runs[n]),
                   "embeddings_per_step": [round(r["embeddings"], 2) for r in runs[n]],
                   "contributions_per_step": [round(r["refined"], 2) for r in runs[n]]}
    ok = True
    for n in BASE:
        a, e = legs[n], legs[n + "+templates"]
        bound = max(a["spread_ms"], e["spread_ms"]) + ADDED_LAUNCHES * LAUNCH_ALLOWANCE_MS
        delta = e["median_ms_per_step"] - a["median_ms_per_step"]
        e["vs_" + n] = {"delta_ms_per_step": round(delta, 4), "bound_ms": round(bound, 4),
                        "within_bound": bool(delta <= bound)}
        e["refined_total"] = trackers[n].refined_total()
        # how the contributors spread over the gallery: few rows mean long same-row chains per step
        e["gallery_rows_refined"] = int(np.count_nonzero(galleries[n].row_updates()))
        ok = ok and delta <= bound
    res["loop"] = {
        "streams": S, "slots": K, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
        "rounds": args.pairs, "frame_clock_ms": FRAME_MS, "gallery_rows": args.gallery,
        "reserved_capacity": args.gallery + args.headroom, "template_cap": TEMPLATE_CAP, "max_samples": MAX_SAMPLES,
        "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; the legs alternate in "
                  "one process after two warm-up rounds, a leg and its +templates twin on one tracker and gallery, "
                  "smoothing and refinement switched between them",
        "bound": "median(leg+templates) - median(leg) <= max(spread of either) + 2 x 0.010 ms",
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
