#!/usr/bin/env python3
"""Cost of the landmark temporal filters on the MI355X (GPU only: fails without one).

(a) kernel alone: zr_lm_filter_async at 1024 streams x 478 landmarks (FaceMesh V2's extract) for
    each filter kind, timed with device events over `--reps` calls after a warm-up.  Bytes per
    call are computed here from the shapes and the state layout (kernels/lm_filter.hip): every
    value reads its input and writes its position (8 B); a filter adds its primed word (4 B
    read) and one (EMA) or two (alpha-beta, 1 euro) state floats read and written (8 / 16 B).
    The rate is those bytes over the event time; the share is against the HBM peak bench.py
    uses.  At this size the working set (~41 MB) stays in the 256 MiB Infinity Cache between
    calls, so the rate is not an HBM measurement; --streams scales it past the cache.
(b) whole loop: DeviceFaceLoop steps at the stream count, frame size and video of bench.py's
    "face_loop" side line, alternating "no filter" and "1 euro" legs in this one process
    (`--pairs` pairs after a warm-up of both), each leg a host clock around `--steps` steps that
    ends in a stream synchronise.  Reports both medians, each leg's spread, and the overhead per
    step beside the unfiltered run-to-run spread.

Writes one JSON document (default profiles/lm_filter_bench.json)."""
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

FILTERS = [("none", 0, ()), ("ema", 1, (0.6,)), ("alpha_beta", 2, (0.5, 0.1)), ("one_euro", 3, (1.0, 0.05, 1.0))]


def bytes_per_value(kind):
    """Algorithmic bytes per filtered value: input read + position write, the primed word read,
    and the state floats read and written."""
    state_floats = {0: 0, 1: 1, 2: 2, 3: 2}[kind]
    return 8 + (4 if kind else 0) + 8 * state_floats


def kernel_alone(streams, L, reps, warmup, peak_gbs):
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, LmFilter, TrackCfg
    lib = _lib.lib()
    rng = np.random.default_rng(1)
    lm = DeviceBuffer.from_array(rng.normal(128.0, 50.0, (streams, 3 * L)).astype(np.float32))
    flag = DeviceBuffer.from_array(np.ones((streams, 1), np.float32))
    pos = DeviceBuffer(streams * L * 3 * 4)
    cfg = TrackCfg(0, L, 256, 256, 1, 1, 0.5, 0.3, 0)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))
    out = []
    for name, kind, p in FILTERS:
        f = LmFilter.make(kind, *p)
        sb = _lib.lm_filter_state_size(f, L)
        st = DeviceBuffer(max(4, streams * sb))
        _lib.check(lib.zr_memset_async(st.ptr, 0, streams * sb, stream))

        def call():
            _lib.check(lib.zr_lm_filter_async(C.byref(f), C.byref(cfg), None, streams, lm.ptr, 3 * L, flag.ptr, 1,
                                              1.0 / 30.0, st.ptr if sb else None, pos.ptr, stream))
        for _ in range(warmup):  # the first call primes every value; the timed ones all filter
            call()
        _lib.check(lib.zr_event_record(ev[0], stream))
        for _ in range(reps):
            call()
        _lib.check(lib.zr_event_record(ev[1], stream))
        _lib.check(lib.zr_event_synchronize(ev[1]))
        ms = C.c_float()
        _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
        values = streams * L * 3
        nbytes = values * bytes_per_value(kind)
        us = 1e3 * ms.value / reps
        gbs = nbytes / (us * 1e-6) / 1e9
        out.append({"filter": name, "us_per_call": round(us, 3), "bytes_per_call": nbytes,
                    "state_bytes_per_stream": sb, "GB_per_s": round(gbs, 1),
                    "share_of_hbm_peak": round(gbs / peak_gbs, 4)})
        st.free()
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return {"streams": streams, "landmarks": L, "values_per_call": streams * L * 3, "reps": reps, "warmup": warmup,
            "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)",
            "working_set_MB": round(streams * L * 3 * 28 / 1e6, 1), "hbm_peak_GB_per_s": peak_gbs,
            "kinds": out}


def whole_loop(streams, sets, steps, pairs, device):
    """bench.py's face_loop_line video and loop, with and without a 1 euro filter."""
    import torch

    import bench
    import zaru_amd.host as H
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
            if s % 2 == 0 and (s // 2) % sets == v:
                continue
            y, x = fs.pos[s]
            y, x = min(fs.h - ph, y + 4 * v), min(fs.w - pw, x + 6 * v)
            video[v, s, y:y + ph, x:x + pw] = patch
    torch.cuda.synchronize(device)
    lists = [[(video[v, s].data_ptr(), fs.w, fs.h, fs.w * 4) for s in range(streams)] for v in range(sets)]
    loop = H.DeviceFaceLoop("face", "facemesh_v2", streams, device)
    one_euro = H.OneEuro(1.0, 0.05)

    def leg(filtered):
        loop.set_filter(one_euro if filtered else None, 1.0 / 30.0)
        loop.synchronize()
        d0 = loop.detections_run()
        t0 = time.perf_counter()
        for k in range(steps):
            loop.step(lists[k % sets])
        loop.synchronize()
        el = time.perf_counter() - t0
        return 1e3 * el / steps, loop.detections_run() - d0

    for filtered in (False, True):  # warm-up: both paths, every shape
        leg(filtered)
    ms = {False: [], True: []}
    dets = {False: [], True: []}
    for _ in range(pairs):
        for filtered in (False, True):
            m, d = leg(filtered)
            ms[filtered].append(m)
            dets[filtered].append(int(d))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    del loop, video
    return {"streams": streams, "frame": f"{fs.w}x{fs.h}", "video_frames": sets, "steps_per_leg": steps, "pairs": pairs,
            "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; legs alternate "
                      "no filter / 1 euro in one process after a warm-up leg of each",
            "no_filter_ms_per_step": [round(x, 4) for x in ms[False]],
            "one_euro_ms_per_step": [round(x, 4) for x in ms[True]],
            "no_filter_median_ms": round(med[False], 4), "one_euro_median_ms": round(med[True], 4),
            "no_filter_spread_ms": round(spread[False], 4), "one_euro_spread_ms": round(spread[True], 4),
            "overhead_ms_per_step": round(med[True] - med[False], 4),
            "overhead_fraction": round((med[True] - med[False]) / med[False], 5),
            "detections_per_leg": {"no_filter": dets[False], "one_euro": dets[True]}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lm_filter_bench.json"))
    ap.add_argument("--streams", type=int, default=1024, help="streams of the kernel-alone measurement")
    ap.add_argument("--landmarks", type=int, default=478)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--loop-streams", type=int, default=256)
    ap.add_argument("--loop-sets", type=int, default=8)
    ap.add_argument("--loop-steps", type=int, default=48)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-loop", action="store_true", help="kernel alone only")
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("bench_lm_filter: at least five pairs")
    # as bench.py orders it: its environment (hardware queues) first, then torch brings the
    # device up, then the library
    import bench
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_filter: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_lm_filter: no GPU")
    res = {"tool": "tools/bench_lm_filter.py",
           "kernel_alone": kernel_alone(args.streams, args.landmarks, args.reps, args.warmup, bench.HBM_PEAK_GBS)}
    print(json.dumps(res["kernel_alone"]), file=sys.stderr, flush=True)
    res["whole_loop"] = ("not measured" if args.no_loop else
                         whole_loop(args.loop_streams, args.loop_sets, args.loop_steps, args.pairs, args.device))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
