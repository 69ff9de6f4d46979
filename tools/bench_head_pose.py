#!/usr/bin/env python3
"""Cost of the head-pose (Procrustes) output on the MI355X (GPU only: fails without one).

(a) kernel alone: zr_procrustes_analyze_async over `--sets` (default 1024 and 8192) sets of the
    468-point canonical face mesh under seeded rotations, scales and translations, timed with
    device events over `--reps` back-to-back calls on one stream after a warm-up.  The kernel is
    latency-bound by design (its sums run in a defined order, kernels/procrustes.hip), so the
    figure is microseconds per call, with the bytes it moves (each set read once, one 84-byte
    record written) for scale.
(b) whole loop: DeviceFaceLoop steps at the stream count, frame size and video of bench.py's
    "face_loop" side line, alternating "pose off" and "pose on" legs in this one process
    (`--pairs` pairs after a warm-up of both), each leg a host clock around `--steps` steps that
    ends in a stream synchronise.  Reports both medians, each leg's spread, the step-time delta
    beside the pose-off run-to-run spread, and the kernel's time at the loop's stream count as a
    fraction of the pose-off step.

Writes one JSON document (default profiles/head_pose_bench.json)."""
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


def mesh_sets(mesh, n_sets, seed):
    """n_sets seeded similarity transforms of the mesh, (n_sets, len(mesh), 3) float32."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n_sets, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    i, j, k, w = q.T
    rot = np.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w),
                    2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w),
                    2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)], 1).reshape(n_sets, 3, 3)
    pts = np.einsum("nrc,pc->npr", rot, mesh.astype(np.float64)) * rng.uniform(5.0, 40.0, (n_sets, 1, 1))
    pts += rng.uniform(0.0, 1000.0, (n_sets, 1, 3))
    return pts.astype(np.float32)


def time_kernel(proc, n_sets, mesh, reps, warmup, stream, ev):
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, Pose
    lib = _lib.lib()
    pts = DeviceBuffer.from_array(mesh_sets(mesh, n_sets, 7))
    out = DeviceBuffer(n_sets * C.sizeof(Pose))

    def call():
        proc.analyze_async(pts.ptr, n_sets, out.ptr, flip_y=True, stream=stream)
    for _ in range(warmup):
        call()
    _lib.check(lib.zr_event_record(ev[0], stream))
    for _ in range(reps):
        call()
    _lib.check(lib.zr_event_record(ev[1], stream))
    _lib.check(lib.zr_event_synchronize(ev[1]))
    ms = C.c_float()
    _lib.check(lib.zr_event_elapsed(C.byref(ms), ev[0], ev[1]))
    rec = out.download((n_sets,), np.dtype(Pose))
    assert (rec["valid"] == 1).all() and np.isfinite(rec["quat"]).all()
    nbytes = n_sets * (len(mesh) * 12 + C.sizeof(Pose))
    return {"sets": n_sets, "us_per_call": round(1e3 * ms.value / reps, 3), "bytes_per_call": nbytes}


def kernel_alone(mesh, set_counts, reps, warmup):
    from zaru_amd import _lib
    lib = _lib.lib()
    proc = _lib.Procrustes(mesh)
    stream = C.c_void_p()
    _lib.check(lib.zr_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.zr_event_create_timing(C.byref(e)))
    out = [time_kernel(proc, n, mesh, reps, warmup, stream, ev) for n in set_counts]
    for e in ev:
        lib.zr_event_destroy(e)
    lib.zr_stream_destroy(stream)
    return {"points_per_set": len(mesh), "reps": reps, "warmup": warmup,
            "timing": "device events around `reps` back-to-back calls on one stream (launch gaps included)",
            "counts": out}


def whole_loop(mesh, streams, sets, steps, pairs, device):
    """bench.py's face_loop_line video and loop, with the pose output off and on."""
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
    valid = []

    def leg(pose):
        loop.set_pose_reference(mesh if pose else None, True)
        loop.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            loop.step(lists[k % sets])
        loop.synchronize()
        el = time.perf_counter() - t0
        if pose:
            valid.append(int(loop.poses().view(np.uint32)[:, 7].sum()))
        return 1e3 * el / steps

    for pose in (False, True):  # warm-up: both paths, every shape
        leg(pose)
    ms = {False: [], True: []}
    for _ in range(pairs):
        for pose in (False, True):
            ms[pose].append(leg(pose))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    del loop, video
    return {"streams": streams, "frame": f"{fs.w}x{fs.h}", "video_frames": sets, "steps_per_leg": steps, "pairs": pairs,
            "timing": "host clock around `steps` enqueued steps ending in a stream synchronise; legs alternate "
                      "pose off / pose on in one process after a warm-up leg of each",
            "pose_off_ms_per_step": [round(x, 4) for x in ms[False]],
            "pose_on_ms_per_step": [round(x, 4) for x in ms[True]],
            "pose_off_median_ms": round(med[False], 4), "pose_on_median_ms": round(med[True], 4),
            "pose_off_spread_ms": round(spread[False], 4), "pose_on_spread_ms": round(spread[True], 4),
            "delta_ms_per_step": round(med[True] - med[False], 4),
            "delta_fraction": round((med[True] - med[False]) / med[False], 5),
            "valid_poses_last_step_per_leg": valid}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_pose_bench.json"))
    ap.add_argument("--mesh", default=os.path.join(REPO, "tests", "golden", "canonical_face_mesh.npy"),
                    help="(n, 3) float32 reference points (.npy)")
    ap.add_argument("--sets", type=int, nargs="+", default=[1024, 8192])
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
        raise SystemExit("bench_head_pose: at least five pairs")
    mesh = np.ascontiguousarray(np.load(args.mesh), np.float32)
    # as bench.py orders it: its environment (hardware queues) first, then torch brings the
    # device up, then the library
    import bench  # noqa: F401
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_pose: no GPU")
    torch.cuda.set_device(args.device)
    torch.zeros(1, device=f"cuda:{args.device}")
    from zaru_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_head_pose: no GPU")
    counts = list(args.sets)
    if not args.no_loop and args.loop_streams not in counts:
        counts.append(args.loop_streams)
    res = {"tool": "tools/bench_head_pose.py", "kernel_alone": kernel_alone(mesh, counts, args.reps, args.warmup)}
    print(json.dumps(res["kernel_alone"]), file=sys.stderr, flush=True)
    if args.no_loop:
        res["whole_loop"] = "not measured"
    else:
        wl = whole_loop(mesh, args.loop_streams, args.loop_sets, args.loop_steps, args.pairs, args.device)
        k = next(c for c in res["kernel_alone"]["counts"] if c["sets"] == args.loop_streams)
        wl["kernel_us_at_loop_streams"] = k["us_per_call"]
        wl["kernel_fraction_of_pose_off_step"] = round(k["us_per_call"] * 1e-3 / wl["pose_off_median_ms"], 5)
        res["whole_loop"] = wl
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
