"""A minimal ONNX writer for synthetic test models (protobuf wire format by hand, no onnx
package): enough of ModelProto / GraphProto / NodeProto / AttributeProto / TensorProto to build
graphs of a few nodes."""
from __future__ import annotations

import struct

import numpy as np


def _varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _len(num: int, payload: bytes) -> bytes:
    return _varint((num << 3) | 2) + _varint(len(payload)) + payload


def _int(num: int, v: int) -> bytes:
    return _varint(num << 3) + _varint(v)


def tensor(name: str, a: np.ndarray) -> bytes:
    a = np.asarray(a)
    dtype = {np.dtype(np.float32): 1, np.dtype(np.int64): 7, np.dtype(np.float64): 11}[a.dtype]
    out = b"".join(_int(1, d) for d in a.shape) + _int(2, dtype)
    if name:
        out += _len(8, name.encode())
    return out + _len(9, a.tobytes())


def attr(name: str, v) -> bytes:
    out = _len(1, name.encode())
    if isinstance(v, float):
        return out + _varint((2 << 3) | 5) + struct.pack("<f", v) + _int(20, 1)
    if isinstance(v, int):
        return out + _int(3, v) + _int(20, 2)
    if isinstance(v, str):
        return out + _len(4, v.encode()) + _int(20, 3)
    if isinstance(v, np.ndarray):
        return out + _len(5, tensor("", v)) + _int(20, 4)
    if isinstance(v, (list, tuple)):
        return out + b"".join(_int(8, int(i)) for i in v) + _int(20, 7)
    raise TypeError(type(v))


def node(op: str, inputs, outputs, name: str = "", **attrs) -> bytes:
    out = b"".join(_len(1, i.encode()) for i in inputs) + b"".join(_len(2, o.encode()) for o in outputs)
    out += _len(3, (name or f"{op}_{outputs[0]}").encode()) + _len(4, op.encode())
    return out + b"".join(_len(5, attr(k, v)) for k, v in attrs.items())


def value_info(name: str, shape) -> bytes:
    dims = b"".join(_len(1, _int(1, d)) for d in shape)
    return _len(1, name.encode()) + _len(2, _len(1, _int(1, 1) + _len(2, dims)))


def model(nodes, inputs, outputs, initializers=None, opset: int = 13) -> bytes:
    """nodes: node() payloads; inputs / outputs: {name: shape}; initializers: {name: array}"""
    g = b"".join(_len(1, n) for n in nodes) + _len(2, b"test")
    g += b"".join(_len(5, tensor(k, v)) for k, v in (initializers or {}).items())
    g += b"".join(_len(11, value_info(k, s)) for k, s in inputs.items())
    g += b"".join(_len(12, value_info(k, s)) for k, s in outputs.items())
    return _int(1, 8) + _len(8, _int(2, opset)) + _len(7, g)
