#!/usr/bin/env python3
"""What merging duplicate gallery rows costs inside the multi-object loop, on the MI355X (GPU only:
fails without one): DeviceMultiTracker ("face", "facemesh") at `--streams` x `--slots` (default 256 x 4)
on tools/bench_multi_identity.py's video and leg discipline, recognition on with the identify interval at
0 (every live face embedded, matched and walked at every step) in every leg, and the loss threshold at -1
so an object stays tracked on whatever its stream shows.

Every leg has a tracker and a reserved gallery of its own with the same rows: `--gallery` random rows, and
behind them two looks of every live object, read from a seeding tracker at two successive steps -- the duplicates
an enrolment that knew no better would have made.  Four legs alternate in one process, `--pairs` rounds
after two warm-up legs of each (the order rotates by one leg each round), a host clock around `--steps`
enqueued steps that ends in a stream synchronise:
  merge_off     the path as it was: no set_identity_merging
  merge_scan    merging on with a link threshold of 0: no look is at distance 0 from a row, so nothing is
                evidence -- the walk's scan and the second launch alone
  merge_on      merging on at the identity threshold (+inf: every flip of an object's nearest row is
                evidence), three observations: the duplicates merge during the warm-up, and the timed
                rounds walk whatever evidence is left
  merge_off_twin  merge_off once more, a tracker and gallery of its own: what two equal legs differ by
Reports each leg's medians and spread, the observations, vetoes and merges per step, the ratios to
merge_off, and the stage alone between device events (back-to-back calls on one stream) at streams x slots
rows, every row tracked and due, none evidence: both launches, and the second launch alone
(min_observations = 0).

Writes one JSON document (default profiles/multi_merge_bench.json)."""
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
LEGS = ("merge_off", "merge_scan", "merge_on", "merge_off_twin")
MIN_OBSERVATIONS = 3


def kernels_alone(streams, slots, capacity, count, reps, warmup):
    """Every row tracked, due and carried from its own slot, on the row it was on: eligible, no evidence."""
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, GalleryLink, IdentityCfg, IdentityState, TrackState
    lib = _lib.lib()
    n = streams * slots
    st = np.zeros(n, np.dtype(TrackState))
    st["tracked"] = 1
    ident = np.zeros(n, np.dtype(IdentityState))
    ident["row"], ident["distance"] = np.arange(n) % count, 0.5
    links = np.zeros(capacity, np.dtype(GalleryLink))
    links["alias"], links["partner"] = np.arange(capacity), -1
    b = DeviceBuffer.from_array
    state, src, due_of = b(st), b((np.arange(n) % slots).astype(np.int32)), b(np.arange(n, dtype=np.int32))
    d_in, d_out, d_links, d_count = b(ident), b(ident), b(links), b(np.array([count], np.int32))
    flipped = ident.copy()   # every object's nearest row another one than before: every row is evidence
    flipped["row"] = (np.arange(n) + n) % count
    d_flipped = b(flipped)
    d_counts = b(np.zeros(3, np.uint64))
    cfg = IdentityCfg(slots, 468, 1, 1, 0.4, math.inf, 0.0)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))

    def call(min_obs, out_states=d_out):
        return lib.zr_identity_link_async(C.byref(cfg), state.ptr, n, src.ptr, due_of.ptr, d_in.ptr, out_states.ptr,
                                          d_links.ptr, d_count.ptr, capacity, min_obs, math.inf, d_counts.ptr, stream)

    out = {"rows": n, "slots": slots, "gallery_rows": count, "capacity": capacity, "reps": reps, "warmup": warmup,
           "what": "every row tracked, due and eligible, none evidence (the no-evidence scan)",
           "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)"}
    for name, min_obs in (("walk_and_canon", MIN_OBSERVATIONS), ("canon_alone", 0)):
        for _ in range(warmup):
            _lib.check(call(min_obs))
        _lib.check(lib.zr_event_record(ev[0], stream))
        for _ in range(reps):
            _lib.check(call(min_obs))
        _lib.check(lib.zr_event_record(ev[1], stream))
        _lib.check(lib.zr_event_synchronize(ev[1]))
        ms = C.c_float()
        _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
        out[name + "_us_per_call"] = round(1e3 * ms.value / reps, 3)
    out["walk_us_per_call"] = round(out["walk_and_canon_us_per_call"] - out["canon_alone_us_per_call"], 3)
    assert d_counts.download((3,), np.uint64).tolist() == [0, 0, 0]   # nothing was evidence
    # the other end: every row evidence, taken one after the other, 0xffffffff observations so nothing merges
    for _ in range(5):
        _lib.check(call(0xFFFFFFFF, d_flipped))
    _lib.check(lib.zr_stream_synchronize(stream))
    before = d_counts.download((3,), np.uint64)
    few = max(1, reps // 20)
    _lib.check(lib.zr_event_record(ev[0], stream))
    for _ in range(few):
        _lib.check(call(0xFFFFFFFF, d_flipped))
    _lib.check(lib.zr_event_record(ev[1], stream))
    _lib.check(lib.zr_event_synchronize(ev[1]))
    ms = C.c_float()
    _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
    walked = (d_counts.download((3,), np.uint64) - before) // few
    out["all_evidence"] = {"us_per_call": round(1e3 * ms.value / few, 3), "reps": few, "merged_per_call": int(walked[0]),
                           "vetoed_per_call": int(walked[1]), "observed_per_call": int(walked[2])}
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_merge_bench.json"))
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
        raise SystemExit("bench_multi_merge: at least five rounds")
    import bench  # noqa: F401  (its environment first, then torch brings the device up, then the library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_merge: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import bench_multi_face
    import make_golden_recognition as mg
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_merge: no GPU")
    S, K = args.streams, args.slots
    video, lists, frame = bench_multi_face.build_video(S, args.sets, args.device)
    model = mg.load_model_bytes()
    rng = np.random.default_rng(3)
    base_rows = rng.standard_normal((args.gallery, 128)).astype(np.float32)

    def tracker(gallery):
        t = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
        t.set_loss_threshold(-1.0)
        t.set_recognition(model, gallery)
        t.set_identify_interval(0.0)
        return t

    # the duplicates: two looks of every live object, at two successive steps
    seed_gallery = H.Gallery(args.device)
    seed_gallery.add(base_rows, list(range(args.gallery)))
    seeder, looks = tracker(seed_gallery), []
    for k in range(args.steps + 2):
        seeder.step(lists[k % args.sets], FRAME_MS * k)
        if k >= args.steps:
            seeder.synchronize()
            p = seeder.objects_packed()
            looks.append(np.array(p["embedding"][:p["count"]], np.float32))
    del seeder
    dup_rows = np.concatenate(looks)
    dup_rows = dup_rows[np.isfinite(dup_rows).all(axis=1)]
    rows = np.concatenate([base_rows, dup_rows])
    capacity = len(rows) + 1024
    res = {"tool": "tools/bench_multi_merge.py",
           "kernels_alone": kernels_alone(S, K, capacity, len(rows), args.reps, 50)}
    print(json.dumps(res["kernels_alone"]), file=sys.stderr, flush=True)

    galleries, trackers, clocks = {}, {}, {}
    for name in LEGS:
        g = H.Gallery(args.device)
        g.add(rows, list(range(len(rows))))
        g.reserve(capacity)
        t = tracker(g)
        if name == "merge_scan":
            t.set_identity_merging(g, MIN_OBSERVATIONS, 0.0)
        elif name == "merge_on":
            t.set_identity_merging(g, MIN_OBSERVATIONS)
        galleries[name], trackers[name], clocks[name] = g, t, 0

    def totals(t):
        return (t.identity_images(), t.merge_observed_total(), t.merge_vetoed_total(), t.merged_total())

    def leg(name):
        t = trackers[name]
        t.synchronize()
        before = totals(t)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            t.step(lists[clocks[name] % args.sets], FRAME_MS * clocks[name])
            clocks[name] += 1
        t.synchronize()
        el = time.perf_counter() - t0
        per = [(a - b) / args.steps for a, b in zip(totals(t), before)]
        return {"ms": 1e3 * el / args.steps, "live": sum(t.object_counts()), "embeddings": per[0], "observed": per[1],
                "vetoed": per[2], "merged": per[3]}

    warm = {n: [leg(n), leg(n)] for n in LEGS}
    runs = {n: [] for n in LEGS}
    for r in range(args.pairs):
        for n in LEGS[r % len(LEGS):] + LEGS[:r % len(LEGS)]:
            runs[n].append(leg(n))
    legs = {}
    for n in LEGS:
        ms = [r["ms"] for r in runs[n]]
        med = statistics.median(ms)
        aliases = galleries[n].aliases()
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(med, 4),
                   "spread_ms": round(max(ms) - min(ms), 4),
                   "live_objects": statistics.median(r["live"] for r in runs[n]),
                   "embeddings_per_step": [round(r["embeddings"], 2) for r in runs[n]],
                   "observed_per_step": [round(r["observed"], 2) for r in runs[n]],
                   "vetoed_per_step": [round(r["vetoed"], 2) for r in runs[n]],
                   "merged_per_step": [round(r["merged"], 3) for r in runs[n]],
                   "merged_during_warm_up": round(sum(r["merged"] for r in warm[n]) * args.steps),
                   "rows_merged_away": int((aliases != np.arange(len(aliases))).sum())}
    base = legs["merge_off"]["median_ms_per_step"]
    for n in LEGS[1:]:
        legs[n]["vs_merge_off"] = {"delta_ms_per_step": round(legs[n]["median_ms_per_step"] - base, 4),
                                   "ratio": round(legs[n]["median_ms_per_step"] / base, 4)}
    res["loop"] = {
        "streams": S, "slots": K, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
        "rounds": args.pairs, "warm_up_legs": 2, "frame_clock_ms": FRAME_MS, "gallery_rows": len(rows),
        "random_rows": args.gallery, "duplicate_rows": len(dup_rows), "reserved_capacity": capacity,
        "identify_interval_ms": 0.0, "identity_threshold": "+inf", "loss_threshold": -1.0,
        "min_observations": MIN_OBSERVATIONS,
        "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; the legs alternate in "
                  "one process after two warm-up legs of each, their order rotated by one each round, each leg a tracker "
                  "and a gallery of its own",
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
