#!/usr/bin/env python3
"""Face recognition throughput: HBM-resident 1080p frames through FaceRecognizer (BlazeFace ->
device post-processing -> crop views -> MobileFaceNet -> gallery match), the embedder's
per-kernel table, the 64-channel stem against preprocessing + the same stem on the f32 tensor,
and embed_match_kernel alone against a large gallery.  Prints one JSON line.

    python tools/bench_recognition.py --steps 10 [--frames 1024] [--gallery 4096] [--out FILE]

Algorithmic bytes / flops: the stem reads 4 B per input pixel from the RGBA frame and
writes 64 x 56 x 56 f32 per image; gdc_kernel reads 512 x 49 f32 and writes 512; the match kernel
does 3 flops (subtract, multiply, add) per pair and dimension.  Roofline: 8 TB/s for the
memory-bound kernels, the 157.3 TFLOP/s f32 vector peak for the match kernel (it cannot use
fused multiply-adds, which that peak counts as two flops)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

HBM_BPS = 8e12
F32_VECTOR_FLOPS = 157.3e12


def profile_of(session, fn):
    from bench import parse_profile
    from zaru_amd._lib import check, lib
    check(lib().zr_profile_enable(session, 1))
    fn()
    need = C.c_size_t()
    buf = C.create_string_buffer(1 << 20)
    check(lib().zr_profile_read(session, buf, len(buf), C.byref(need)))
    check(lib().zr_profile_enable(session, 0))
    return parse_profile(buf.value.decode())


def timed(fn, sync, reps):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--gallery", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--match-queries", type=int, default=1024)
    ap.add_argument("--match-gallery", type=int, default=65536)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    from bench import FrameSet, load_patch
    import make_golden_recognition as mg
    from zaru_amd import _lib, host
    from zaru_amd._lib import DeviceBuffer, Frame, check, lib
    from zaru_amd.nn import Cnn, ColorMapper, NeuralNetwork, preprocess_views_device

    model = mg.load_model_bytes()
    rng = np.random.default_rng(0x5A52)
    n = args.frames
    frames = FrameSet(rng, n, patch=load_patch()).to_device("cuda:0")
    flist = [(frames[i].data_ptr(), 1920, 1080, 1920 * 4) for i in range(n)]
    rec = host.FaceRecognizer(model, "face", 0, args.chunk)
    gal = host.Gallery()
    rows = rng.normal(0, 14 / np.sqrt(128), size=(args.gallery, 128)).astype(np.float32)
    gal.add(rows, list(range(args.gallery)))

    found = rec.recognize(flist, gal)[0]
    for _ in range(args.warmup):
        rec.enqueue(flist, gal)
    rec.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        rec.enqueue(flist, gal)
    rec.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    res = {"workload": "face_recognition", "frames_per_step": n, "gallery": args.gallery, "steps": args.steps,
           "faces_found": int(found.sum()), "step_ms": dt * 1e3, "faces_per_s": float(found.sum()) / dt,
           "frames_per_s": n / dt}

    # the embedder's per-kernel table (one profiled step; the table is per launch, so per chunk)
    table = profile_of(rec.session(), lambda: (rec.enqueue(flist, gal), rec.synchronize()))
    res["embedder_kernels"] = table
    slow = max(table, key=lambda k: k["ms"])
    res["slowest_embedder_kernel"] = {"kernel": slow["kernel"], "ms": slow["ms"], "launches": slow["launches"]}
    imgs = n

    def per_image(sym):
        k = [t for t in table if t["kernel"].startswith(sym)]
        return sum(t["ms"] for t in k) * 1e-3 / imgs if k else None

    stem_bytes = 4.0 * 112 * 112 + 4.0 * 64 * 56 * 56
    gdc_bytes = 4.0 * 512 * 49 + 4.0 * 512
    t = per_image("stem_kernel<3,2,64,true>")
    if t:
        res["stem"] = {"us_per_image": t * 1e6, "bytes_per_image": stem_bytes, "GBps": stem_bytes / t / 1e9,
                       "roofline_fraction": stem_bytes / t / HBM_BPS}
    t = per_image("gdc_kernel")
    if t:
        res["gdc"] = {"us_per_image": t * 1e6, "bytes_per_image": gdc_bytes, "GBps": gdc_bytes / t / 1e9,
                      "roofline_fraction": gdc_bytes / t / HBM_BPS,
                      "projection": "unfused: the 512 -> 128 1x1 runs as the next GEMM launch"}
    # the unfused inverted-residual pairs (launch_ir / launch_irl decline every pair of this model)
    res["unfused_pairs_ms"] = {k["kernel"]: k["ms"] for k in table
                               if k["kernel"].startswith(("gemm", "dwpw"))}

    # 64-channel stem: fused sampling vs preprocessing + the stem on the f32 tensor, alternating pairs
    net = NeuralNetwork.from_onnx(model).load()
    cnn = Cnn(net, ColorMapper.linear(-1.0, 1.0))
    nb = min(args.chunk, n)
    views = [(960.0 + (i % 7), 540.0 + (i % 5), 400.0, 400.0, 0.0) for i in range(nb)]
    fr = [Frame(frames[i].data_ptr(), 1920, 1080, 1920 * 4) for i in range(nb)]
    vf = list(range(nb))
    d_x = DeviceBuffer(nb * 3 * 112 * 112 * 4)
    d_o = DeviceBuffer(nb * 128 * 4)
    fused = lambda: cnn.estimate_views_device(fr, views, vf, [d_o.ptr])
    split = lambda: (preprocess_views_device(fr, views, vf, 112, 112, -1.0, 1.0, d_x.ptr),
                     net.estimate_device(nb, d_x.ptr, [d_o.ptr]))
    pairs = []
    for _ in range(5):
        pairs.append((timed(fused, _lib.synchronize, 5), timed(split, _lib.synchronize, 5)))
    tf = profile_of(net._h, lambda: (fused(), _lib.synchronize()))
    ts = profile_of(net._h, lambda: (split(), _lib.synchronize()))
    stem_f = sum(k["ms"] for k in tf if k["kernel"].startswith("stem_kernel"))
    stem_s = sum(k["ms"] for k in ts if k["kernel"].startswith("stem_kernel"))
    res["stem_ab"] = {"batch": nb, "network_ms_fused": [p[0] * 1e3 for p in pairs],
                      "network_ms_preproc_plus_run": [p[1] * 1e3 for p in pairs],
                      "stem_kernel_ms_fused": stem_f, "stem_kernel_ms_on_tensor": stem_s,
                      "note": "the split path also runs preproc_kernel, which the session profile does not list"}

    # the match kernel alone
    Q, G = args.match_queries, args.match_gallery
    dq = DeviceBuffer.from_array(rng.normal(0, 1.2, size=(Q, 128)).astype(np.float32))
    dg = DeviceBuffer.from_array(rng.normal(0, 1.2, size=(G, 128)).astype(np.float32))
    di, dd = DeviceBuffer(Q * 4), DeviceBuffer(Q * 4)
    match = lambda: check(lib().zr_embed_match_async(dq.ptr, Q, dg.ptr, G, 128, None, di.ptr, dd.ptr, None, None))
    tm = timed(match, _lib.synchronize, 10)
    flops = 3.0 * Q * G * 128
    res["match"] = {"queries": Q, "gallery": G, "ms": tm * 1e3, "pair_dims_per_s": Q * G * 128 / tm,
                    "TFLOPs": flops / tm / 1e12, "roofline_fraction": flops / tm / F32_VECTOR_FLOPS}
    in_pipeline = timed(lambda: check(lib().zr_embed_match_async(dq.ptr, min(n, Q), dg.ptr, min(args.gallery, G), 128, None, di.ptr,
                                                                 dd.ptr, None, None)), _lib.synchronize, 20)
    res["match_in_pipeline_ms"] = in_pipeline * 1e3
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    del torch


if __name__ == "__main__":
    main()
