"""The packed export of every stream's tracked objects (zr_multi_export_async), restated in numpy
from its contract and from DeviceMultiTracker::objects(s): which slots are exported, in which order,
and from which slot each part of a record is gathered.  Everything is moved as bits (uint32 words),
so any payload compares exactly.

Inputs (rows = S * K, stream-major):
    nobjects int32[S], src int32[rows], ids uint64[rows], roi u32[rows, 5], confidence u32[rows],
    lm u32[rows, 3 L]
    pose u32[rows, 21] or None
    ist {"row" i32, "distance" u32, "embeddings" u32, "flags" u32}[rows] and emb u32[rows, 128], or None
    eye_valid i32[2 rows], eye_diam u32[2 rows], eye_crop u32[2 rows, 5], eye_lm u32[2 rows, 228], or None
"""
import numpy as np

POSE, IDENTITY, EYE_LEFT, EYE_RIGHT = 1, 2, 4, 8

HEADER = np.dtype([("id", "<u8"), ("stream", "<i4"), ("slot", "<i4"), ("roi", "<u4", (5,)), ("confidence", "<u4"),
                   ("flags", "<u4"), ("reserved", "<u4")])
IDENT = np.dtype([("row", "<i4"), ("distance", "<u4"), ("embeddings", "<u4"), ("flags", "<u4")])
assert HEADER.itemsize == 48 and IDENT.itemsize == 16


def exported(nobjects, src, K):
    """[(stream, slot j, source slot r)] in stream-then-slot order."""
    out = []
    for s in range(len(nobjects)):
        no = min(max(int(nobjects[s]), 0), K)
        for j in range(no):
            r = int(src[s * K + j])
            if 0 <= r < K:
                out.append((s, j, r))
    return out


def export(K, nobjects, src, ids, roi, confidence, lm, pose=None, ist=None, emb=None, eye_valid=None, eye_diam=None,
           eye_crop=None, eye_lm=None):
    S = len(nobjects)
    recs = exported(nobjects, src, K)
    n = len(recs)
    offsets = np.zeros(S + 1, np.int32)
    for s, _, _ in recs:
        offsets[s + 1:] += 1
    out = {"count": n, "offsets": offsets, "header": np.zeros(n, HEADER), "lm": np.zeros((n, lm.shape[1]), np.uint32)}
    if pose is not None:
        out["pose"] = np.zeros((n, 21), np.uint32)
    if ist is not None:
        out["ident"] = np.zeros(n, IDENT)
        out["emb"] = np.zeros((n, 128), np.uint32)
    if eye_valid is not None:
        out["eye_valid"] = np.zeros(2 * n, np.int32)
        out["eye_diam"] = np.zeros(2 * n, np.uint32)
        out["eye_crop"] = np.zeros((2 * n, 5), np.uint32)
        out["eye_lm"] = np.zeros((2 * n, 228), np.uint32)
    for k, (s, j, r) in enumerate(recs):
        here, frm = s * K + j, s * K + r
        h = out["header"][k]
        h["id"], h["stream"], h["slot"] = ids[here], s, j
        h["roi"], h["confidence"] = roi[here], confidence[here]
        flags = 0
        out["lm"][k] = lm[frm]
        if pose is not None:
            flags |= POSE
            out["pose"][k] = pose[frm]
        if ist is not None and ist["embeddings"][frm] != 0:
            flags |= IDENTITY
            out["ident"][k] = ist[frm]
            out["emb"][k] = emb[frm]
        if eye_valid is not None:
            for side in range(2):
                e = 2 * frm + side
                if eye_valid[e] == 0:
                    continue
                flags |= EYE_RIGHT if side else EYE_LEFT
                out["eye_valid"][2 * k + side] = 1
                out["eye_diam"][2 * k + side] = eye_diam[e]
                out["eye_crop"][2 * k + side] = eye_crop[e]
                out["eye_lm"][2 * k + side] = eye_lm[e]
        h["flags"] = flags
    return out
