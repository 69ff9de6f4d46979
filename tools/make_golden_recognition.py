#!/usr/bin/env python3
"""Goldens for the face recognition network (tests/golden/mobilefacenet_f64.npz).

The CPU oracle does not know the `Constant` operator, so this file carries its own small ONNX
reader (protobuf varints, TensorProto raw/float/int64 data, the `value` attribute of Constant)
and a torch-CPU restatement of the six operators the graph uses: Conv (strides, pads, group),
Clip, Relu, Add, Reshape and Constant.  `run_model(graph, x, dtype)` evaluates the graph in
float64 (the golden) or float32 (the CPU chain the GPU tests compare against).

The model is kept under tests/golden/ as parts of at most 1 MiB (`mobilefacenet.onnx.part<k>`);
`load_model_bytes` joins them and checks length and SHA-256 against `mobilefacenet.onnx.json`.

    python tools/make_golden_recognition.py                 # rewrite mobilefacenet_f64.npz
    python tools/make_golden_recognition.py --split FILE    # (re)create the parts from FILE
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
PART = 1 << 20
SEED = 0x5A525600
SIZE = 112


# ------------------------------------------------------------------ model file
def load_model_bytes(golden_dir: str = GOLD) -> bytes:
    with open(os.path.join(golden_dir, "mobilefacenet.onnx.json")) as f:
        meta = json.load(f)
    data = b"".join(open(os.path.join(golden_dir, f"mobilefacenet.onnx.part{k}"), "rb").read()
                    for k in range(meta["parts"]))
    if len(data) != meta["bytes"] or hashlib.sha256(data).hexdigest() != meta["sha256"]:
        raise RuntimeError("tests/golden/mobilefacenet.onnx.part*: length or SHA-256 mismatch")
    return data


def split_model(src: str, golden_dir: str = GOLD) -> None:
    data = open(src, "rb").read()
    parts = [data[i:i + PART] for i in range(0, len(data), PART)]
    for k, p in enumerate(parts):
        with open(os.path.join(golden_dir, f"mobilefacenet.onnx.part{k}"), "wb") as f:
            f.write(p)
    with open(os.path.join(golden_dir, "mobilefacenet.onnx.json"), "w") as f:
        json.dump({"bytes": len(data), "parts": len(parts),
                   "sha256": hashlib.sha256(data).hexdigest()}, f, indent=1)
        f.write("\n")


# ------------------------------------------------------------------ protobuf
def _varint(b: bytes, i: int):
    v = 0
    s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, i


def _fields(b: bytes):
    i = 0
    while i < len(b):
        key, i = _varint(b, i)
        num, wire = key >> 3, key & 7
        if wire == 0:
            v, i = _varint(b, i)
        elif wire == 1:
            v, i = b[i:i + 8], i + 8
        elif wire == 2:
            n, i = _varint(b, i)
            v, i = b[i:i + n], i + n
        elif wire == 5:
            v, i = b[i:i + 4], i + 4
        else:
            raise ValueError(f"wire type {wire}")
        yield num, wire, v


def _s64(v: int) -> int:
    return v - (1 << 64) if v >= 1 << 63 else v


def _packed_varints(wire, v):
    if wire == 0:
        return [_s64(v)]
    out, i = [], 0
    while i < len(v):
        x, i = _varint(v, i)
        out.append(_s64(x))
    return out


def _tensor(b: bytes):
    dims, dtype, name, raw, fdata, idata = [], 0, "", None, [], []
    for num, wire, v in _fields(b):
        if num == 1:
            dims += _packed_varints(wire, v)
        elif num == 2:
            dtype = v
        elif num == 4:
            fdata += [struct.unpack("<f", v)[0]] if wire == 5 else list(np.frombuffer(v, "<f4"))
        elif num == 7:
            idata += _packed_varints(wire, v)
        elif num == 8:
            name = v.decode()
        elif num == 9:
            raw = v
    if dtype == 1:
        a = np.frombuffer(raw, "<f4") if raw is not None else np.array(fdata, np.float32)
    elif dtype == 7:
        a = np.frombuffer(raw, "<i8") if raw is not None else np.array(idata, np.int64)
    else:
        raise ValueError(f"tensor {name}: dtype {dtype}")
    return name, a.reshape(dims).copy()


def _attr(b: bytes):
    name, val = "", None
    for num, wire, v in _fields(b):
        if num == 1:
            name = v.decode()
        elif num == 2:
            val = struct.unpack("<f", v)[0]
        elif num == 3:
            val = _s64(v)
        elif num == 4:
            val = v.decode()
        elif num == 5:
            val = _tensor(v)[1]
        elif num == 8:
            val = (val if isinstance(val, list) else []) + _packed_varints(wire, v)
    return name, val


def parse_graph(model: bytes) -> dict:
    """{'nodes': [(op, name, inputs, outputs, attrs)], 'inits': {name: array}, 'inputs', 'outputs'}"""
    graph = next(v for num, wire, v in _fields(model) if num == 7 and wire == 2)
    g = {"nodes": [], "inits": {}, "inputs": [], "outputs": []}
    for num, wire, v in _fields(graph):
        if num == 1:
            op, name, ins, outs, attrs = "", "", [], [], {}
            for n2, _, v2 in _fields(v):
                if n2 == 1:
                    ins.append(v2.decode())
                elif n2 == 2:
                    outs.append(v2.decode())
                elif n2 == 3:
                    name = v2.decode()
                elif n2 == 4:
                    op = v2.decode()
                elif n2 == 5:
                    k, a = _attr(v2)
                    attrs[k] = a
            g["nodes"].append((op, name, ins, outs, attrs))
        elif num == 5:
            name, a = _tensor(v)
            g["inits"][name] = a
        elif num in (11, 12):
            name = next(v2.decode() for n2, _, v2 in _fields(v) if n2 == 1)
            g["inputs" if num == 11 else "outputs"].append(name)
    g["inputs"] = [n for n in g["inputs"] if n not in g["inits"]]
    return g


# ------------------------------------------------------------------ the six operators
def run_model(g: dict, x: np.ndarray, dtype=np.float64) -> np.ndarray:
    """x: [N,3,H,W] float32 -> the graph's first output, computed in `dtype` on the CPU.  The
    batch runs image by image: the Reshape target is the literal [1,-1]."""
    import torch
    import torch.nn.functional as F

    td = torch.float64 if dtype == np.float64 else torch.float32
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    consts = {k: torch.from_numpy(v).to(td) if v.dtype == np.float32 else v for k, v in g["inits"].items()}
    outs = []
    for n in range(x.shape[0]):
        env = dict(consts)
        env[g["inputs"][0]] = torch.from_numpy(np.ascontiguousarray(x[n:n + 1])).to(td)
        for op, name, ins, out, at in g["nodes"]:
            if op == "Constant":
                v = at["value"]
                env[out[0]] = torch.from_numpy(v).to(td) if v.dtype == np.float32 else v
            elif op == "Conv":
                pads = at.get("pads", [0, 0, 0, 0])
                xi = F.pad(env[ins[0]], (pads[1], pads[3], pads[0], pads[2]))
                env[out[0]] = F.conv2d(xi, env[ins[1]], env[ins[2]] if len(ins) > 2 else None,
                                       stride=tuple(at.get("strides", [1, 1])), groups=at.get("group", 1))
            elif op == "Clip":
                env[out[0]] = torch.clamp(env[ins[0]], min=float(env[ins[1]]), max=float(env[ins[2]]))
            elif op == "Relu":
                env[out[0]] = torch.relu(env[ins[0]])
            elif op == "Add":
                env[out[0]] = env[ins[0]] + env[ins[1]]
            elif op == "Reshape":
                env[out[0]] = env[ins[0]].reshape([int(d) for d in np.asarray(env[ins[1]])])
            else:
                raise ValueError(f"operator {op} ({name})")
        outs.append(env[g["outputs"][0]].numpy().reshape(-1))
    return np.stack(outs)


def codes_to_input(codes: np.ndarray) -> np.ndarray:
    """uint8 [..,3,H,W] -> codes * (2/255) - 1 in f32 (ColorMapper.linear(-1, 1))."""
    adj = np.float32((np.float32(1.0) - np.float32(-1.0)) / np.float32(255.0))
    return codes.astype(np.float32) * adj + np.float32(-1.0)


def random_codes(k: int) -> np.ndarray:
    return np.random.default_rng(SEED + k).integers(0, 256, size=(3, SIZE, SIZE), dtype=np.uint8)


def views_frames(golden_dir: str = GOLD) -> list:
    """The five `views` RGBA frames: the three 192x192 face views of sad_linus_mesh.npz (0, +10,
    -10 degrees), seeded noise, flat grey.  Each is sampled through its full-image view to 112^2."""
    mesh = np.load(os.path.join(golden_dir, "sad_linus_mesh.npz"))["codes"]  # [3,3,192,192]
    frames = []
    for v in range(3):
        f = np.full((192, 192, 4), 255, np.uint8)
        f[..., :3] = mesh[v].transpose(1, 2, 0)
        frames.append(f)
    noise = np.random.default_rng(SEED + 16).integers(0, 256, size=(192, 192, 4), dtype=np.uint8)
    noise[..., 3] = 255
    frames.append(noise)
    grey = np.full((192, 192, 4), 128, np.uint8)
    grey[..., 3] = 255
    frames.append(grey)
    return frames


def views_inputs(golden_dir: str = GOLD) -> np.ndarray:
    """[5,3,112,112] f32: views_frames() through the CPU oracle's preprocessing."""
    sys.path.insert(0, REPO)
    import oracle as O
    return np.stack([O.preproc(f, O.view_full(192, 192), SIZE, SIZE, -1.0, 1.0) for f in views_frames(golden_dir)])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--split", metavar="FILE", help="write the model parts from FILE first")
    args = ap.parse_args()
    if args.split:
        split_model(args.split)
    g = parse_graph(load_model_bytes())
    out = {}
    for k in range(2):
        codes = random_codes(k)
        out[f"{k}/codes"] = codes
        out[f"{k}/out"] = run_model(g, codes_to_input(codes)[None])[0].astype(np.float32)
    out["views/out"] = run_model(g, views_inputs()).astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, "mobilefacenet_f64.npz"), **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main()
