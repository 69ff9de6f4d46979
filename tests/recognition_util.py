"""Shared by the recognition tests: the golden tool as a module, the model bytes, the goldens and
the numpy restatement of Embedding::difference."""
from __future__ import annotations

import functools
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def tool():
    path = os.path.join(REPO, "tools", "make_golden_recognition.py")
    spec = importlib.util.spec_from_file_location("make_golden_recognition", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def model_bytes(golden_dir: str) -> bytes:
    return tool().load_model_bytes(golden_dir)


@functools.lru_cache(maxsize=None)
def graph(golden_dir: str):
    return tool().parse_graph(model_bytes(golden_dir))


@functools.lru_cache(maxsize=None)
def golden(golden_dir: str):
    with np.load(os.path.join(golden_dir, "mobilefacenet_f64.npz")) as d:
        return {k: d[k] for k in d.files}


def difference_matrix(q: np.ndarray, g: np.ndarray) -> np.ndarray:
    """[Q][G] f32: s = s + d*d one k at a time in f32, then sqrt in f32 (vectorised over pairs,
    sequential over k -- every operation rounds to f32 on its own)."""
    q = np.asarray(q, np.float32)
    g = np.asarray(g, np.float32)
    s = np.zeros((q.shape[0], g.shape[0]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(q.shape[1]):
            d = q[:, k, None] - g[None, :, k]
            s = s + d * d
        return np.sqrt(s)
