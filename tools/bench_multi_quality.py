#!/usr/bin/env python3
"""What the face quality gate costs, and saves, inside the multi-object loop, on the MI355X (GPU only:
fails without one): DeviceMultiTracker ("face", "facemesh") at `--streams` x `--slots` (default 256 x 4)
on tools/bench_multi_identity.py's video and leg discipline, recognition on with the identify interval at
0 (one MobileFaceNet pass over the live faces per step) in every leg, and the loss threshold at -1 so an
object stays tracked on whatever its stream shows.

Four legs alternate in one process, `--pairs` rounds after a warm-up of each (on the plain video, where
the objects start), every leg a tracker of its own and a host clock around `--steps` enqueued steps that
ends in a stream synchronise:
  gate_off              the path as it was: no set_identity_quality
  gate_measure          both tiers all -inf: every due crop measured, nobody rejected -- the cost of measuring
  gate_measure_flat     the same on a video in which every second stream's frames are one flat colour
  gate_sharpness_flat   that video with min_sharpness between the two kinds of stream (`--min-sharpness`):
                        the flat streams' objects are measured and not embedded
Reports each leg's medians and spread, embeddings, measurements and rejections per step, the ratios to
gate_off, and the two kernels alone between device events (back-to-back calls on one stream) at
streams x slots rows with one due row per stream on the 112 x 112 grid.

Writes one JSON document (default profiles/multi_quality_bench.json)."""
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
LEGS = ("gate_off", "gate_measure", "gate_measure_flat", "gate_sharpness_flat")
FLAT = (120, 90, 60, 255)


def kernels_alone(streams, slots, frame_ptr, fw, fh, reps, warmup):
    """Slot 0 of every stream tracked and due, its crop a 300 px square of the given frame."""
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, FaceQuality, Frame, QualityCfg, QualityTier, TrackState
    lib = _lib.lib()
    n = streams * slots
    st = (TrackState * n)()
    for i in range(0, n, slots):
        st[i].tracked, st[i].active, st[i].frame_w, st[i].frame_h = 1, 1, fw, fh
    b = DeviceBuffer.from_array
    state = b(np.frombuffer(bytes(st), np.uint8))
    src = b(np.zeros(n, np.int32))
    view = (C.c_float * 5)(fw / 2.0, fh / 2.0, 300.0, 300.0, 0.0)
    desc = np.zeros(10, np.float32)
    _lib.check(lib.zr_view_describe(view, 1, 0, desc.ctypes.data))
    views = b(np.tile(desc, (n, 1)))
    due0 = np.zeros(n, np.int32)
    due0[::slots] = 1
    due, due_of = b(due0), b(np.where(due0 == 1, np.cumsum(due0) - 1, -1).astype(np.int32))
    recs = [b(np.zeros(n, np.dtype(FaceQuality))), b(np.zeros(n, np.dtype(FaceQuality)))]
    learn = DeviceBuffer(n * 4)
    skip = QualityTier(-math.inf, -math.inf, -math.inf, -math.inf)
    cfg = QualityCfg(slots, 112, 112, skip, skip)
    frames = (Frame * 1)(Frame(frame_ptr, fw, fh, fw * 4))
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))
    calls = {
        "measure": lambda: lib.zr_identity_quality_async(C.byref(cfg), frames, 1, state.ptr, n, src.ptr, views.ptr, None,
                                                         recs[0].ptr, recs[1].ptr, due.ptr, None, None, stream),
        "mask": lambda: lib.zr_identity_quality_mask_async(n, due_of.ptr, recs[1].ptr, learn.ptr, None, stream),
    }
    out = {"rows": n, "slots": slots, "due_rows": streams, "grid": "112x112", "crop_px": 300, "reps": reps,
           "warmup": warmup,
           "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)"}
    for name in ("measure", "mask"):
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
    assert int(due.download((n,), np.int32).sum()) == streams   # all -inf: nobody left the list
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_quality_bench.json"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4, help="video frames per stream (cycled)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--min-sharpness", type=float, default=1.0,
                    help="a flat frame measures exactly 0, the plain video's crops far above")
    ap.add_argument("--only", default=None, help="run this one leg alone (no kernels_alone, no file written)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.pairs < 5 and not args.only:
        raise SystemExit("bench_multi_quality: at least five rounds")
    import bench  # noqa: F401  (its environment first, then torch brings the device up, then the library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_quality: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    import bench_multi_face
    import make_golden_recognition as mg
    import zaru_amd.host as H
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_multi_quality: no GPU")
    S, K = args.streams, args.slots
    video, lists, frame = bench_multi_face.build_video(S, args.sets, args.device)
    fw, fh = (int(v) for v in frame.split("x"))
    res = {"tool": "tools/bench_multi_quality.py"}
    names = [args.only] if args.only else list(LEGS)
    if not args.only:
        res["kernels_alone"] = kernels_alone(S, K, video[0, 0].data_ptr(), fw, fh, args.reps, 50)
        print(json.dumps(res["kernels_alone"]), file=sys.stderr, flush=True)
    flat_video = flat_lists = None
    if any(n.endswith("_flat") for n in names):
        flat_video = video.clone()
        flat_video[:, 1::2] = torch.tensor(FLAT, dtype=torch.uint8, device=video.device)
        torch.cuda.synchronize(args.device)
        flat_lists = [[(flat_video[v, s].data_ptr(), fw, fh, fw * 4) for s in range(S)] for v in range(args.sets)]
    model = mg.load_model_bytes()
    gallery = H.Gallery(args.device)
    rng = np.random.default_rng(3)
    gallery.add(rng.standard_normal((args.gallery, 128)).astype(np.float32), list(range(args.gallery)))
    skip = H.FaceQualityGate()
    tiers = {"gate_off": None, "gate_measure": skip, "gate_measure_flat": skip,
             "gate_sharpness_flat": H.FaceQualityGate(min_sharpness=args.min_sharpness)}
    trackers, clocks = {}, {}
    for name in names:
        t = H.DeviceMultiTracker("face", "facemesh", S, K, args.device)
        t.set_loss_threshold(-1.0)
        t.set_recognition(model, gallery)
        t.set_identify_interval(0.0)
        if tiers[name] is not None:
            t.set_identity_quality(tiers[name])
        trackers[name], clocks[name] = t, 0

    def leg(name, frames):
        t = trackers[name]
        t.synchronize()
        before = (t.identity_images(), t.quality_measured_total(), t.quality_rejected_total())
        t0 = time.perf_counter()
        for _ in range(args.steps):
            t.step(frames[clocks[name] % args.sets], FRAME_MS * clocks[name])
            clocks[name] += 1
        t.synchronize()
        el = time.perf_counter() - t0
        after = (t.identity_images(), t.quality_measured_total(), t.quality_rejected_total())
        per = [(a - b) / args.steps for a, b in zip(after, before)]
        return {"ms": 1e3 * el / args.steps, "live": sum(t.object_counts()), "embeddings": per[0], "measured": per[1],
                "rejected": per[2]}

    def frames_of(name):
        return flat_lists if name.endswith("_flat") else lists

    for n in names:  # warm-up on the plain video: the objects start here; then once on the leg's own
        leg(n, lists)
        leg(n, frames_of(n))
    runs = {n: [] for n in names}
    for _ in range(args.pairs):
        for n in names:
            runs[n].append(leg(n, frames_of(n)))
    legs = {}
    for n in names:
        ms = [r["ms"] for r in runs[n]]
        med = statistics.median(ms)
        legs[n] = {"ms_per_step": [round(x, 4) for x in ms], "median_ms_per_step": round(med, 4),
                   "spread_ms": round(max(ms) - min(ms), 4),
                   "live_objects": statistics.median(r["live"] for r in runs[n]),
                   "embeddings_per_step": [round(r["embeddings"], 2) for r in runs[n]],
                   "measured_per_step": [round(r["measured"], 2) for r in runs[n]],
                   "rejected_per_step": [round(r["rejected"], 2) for r in runs[n]]}
    if "gate_off" in legs:
        base = legs["gate_off"]["median_ms_per_step"]
        for n in names:
            if n != "gate_off":
                legs[n]["vs_gate_off"] = {"delta_ms_per_step": round(legs[n]["median_ms_per_step"] - base, 4),
                                          "ratio": round(legs[n]["median_ms_per_step"] / base, 4)}
    res["loop"] = {
        "streams": S, "slots": K, "frame": frame, "video_frames": args.sets, "steps_per_leg": args.steps,
        "rounds": args.pairs, "frame_clock_ms": FRAME_MS, "gallery_rows": args.gallery, "identify_interval_ms": 0.0,
        "loss_threshold": -1.0, "min_sharpness": args.min_sharpness, "flat_colour": list(FLAT),
        "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; the legs alternate in "
                  "one process after a warm-up leg of each, each leg a tracker of its own",
        "legs": legs,
    }
    del trackers, video, flat_video
    if not args.only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
