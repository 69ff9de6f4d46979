"""Plain numpy f32 restatements of tiled detection (host/detection.h: detection_tiles, TiledDetector;
kernels/track.hip: due_compact_tiles_kernel; kernels/detmerge.hip: det_merge_kernel), for
tests/test_tiled_cpu.py (these against the host classes the suite already pins) and
tests/test_gpu_tiled.py (each kernel alone, bit for bit).  No device call is made here.

A detection is a row of 20 f32: {conf, angle, cx, cy, w, h, 7 x (kx, ky)}, the device's record."""
import os

import numpy as np

f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the grid ---------------------------------------------------------------------------------------
def detection_tiles(W, H, cols, rows, overlap=0.25, include_full=True):
    """Rects as (cx, cy, w, h) f32: the full frame first when included, then row-major; the last
    column and row are placed against the frame's edge."""
    if cols < 1 or rows < 1:
        raise ValueError("cols and rows must be >= 1")
    if not (0.0 <= overlap < 1.0):
        raise ValueError("overlap must be in [0, 1)")
    if cols * rows + (1 if include_full else 0) > 16:
        raise ValueError("more than 16 rects")
    o, fw, fh, half = f32(overlap), f32(W), f32(H), f32(0.5)
    tw = fw / (f32(cols) - f32(cols - 1) * o)
    th = fh / (f32(rows) - f32(rows - 1) * o)
    sx, sy = tw * (f32(1) - o), th * (f32(1) - o)
    out = []
    if include_full:
        out.append((f32(0) + fw * half, f32(0) + fh * half, fw, fh))
    for r in range(rows):
        for c in range(cols):
            x0 = fw - tw if c + 1 == cols else f32(c) * sx
            y0 = fh - th if r + 1 == rows else f32(r) * sy
            out.append((x0 + tw * half, y0 + th * half, tw, th))
    return np.array(out, f32)


# ---- the tile compaction ----------------------------------------------------------------------------
def compact_tiles(pending, templates):
    """due_compact_tiles_kernel: the streams with a non-zero flag in order; T views per stream, tile
    t's template with the frame index set to the stream, and the slot s * T + t of each.  Returns
    (due, slots, views [ndue * T][10] u32, ndue, nviews)."""
    tm = np.asarray(templates, np.uint32).reshape(-1, 10)
    T = len(tm)
    due = np.flatnonzero(np.asarray(pending) != 0).astype(np.int32)
    slots = (due[:, None] * T + np.arange(T, dtype=np.int32)[None, :]).reshape(-1).astype(np.int32)
    views = np.tile(tm, (len(due), 1))
    views[:, 8] = np.repeat(due, T)
    return due, slots, views, len(due), len(due) * T


# ---- the merge --------------------------------------------------------------------------------------
def total_key(v):
    """f32::total_cmp's key: the bits, the magnitude flipped for negatives, as a signed int."""
    b = int(np.array(v, f32).view(np.int32))
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def iou(a, b):
    """Rect::iou (rect.rs:193-214) on (cx, cy, w, h) f32, operation for operation."""
    half = f32(0.5)
    ax, ay, bx, by = a[0] - a[2] * half, a[1] - a[3] * half, b[0] - b[2] * half, b[1] - b[3] * half
    mnx, mny = np.fmax(ax, bx), np.fmax(ay, by)
    mxx, mxy = np.fmin(ax + a[2], bx + b[2]), np.fmin(ay + a[3], by + b[3])
    inter = f32(0)
    if not (mnx > mxx or mny > mxy):
        x0, y0, x1, y1 = np.fmin(mnx, mxx), np.fmin(mny, mxy), np.fmax(mnx, mxx), np.fmax(mny, mxy)
        inter = (x1 - x0) * (y1 - y0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (a[2] * a[3] + b[2] * b[3] - inter)


def union(tile_count, tile_dets, tile_cap):
    """Tile order, within a tile its first min(count, tile_cap) rows (counts clamped to 0..tile_cap).
    Returns (rows [n][20], records past tile_cap summed)."""
    rows, dropped = [], 0
    for t, c in enumerate(np.asarray(tile_count).tolist()):
        rows.extend(np.asarray(tile_dets, f32)[t, :min(max(c, 0), tile_cap)])
        dropped += max(c - tile_cap, 0)
    return np.array(rows, f32).reshape(-1, 20), dropped


def nms(rows, keypoints, iou_thresh, remove):
    """NonMaxSuppression::process (nms.rs:59-145) on rows of 20 f32, as host/detection.cpp restates
    it.  Returns (rows out [m][20], (candidates, tied))."""
    rows = np.asarray(rows, f32).reshape(-1, 20)
    thr, nf = f32(iou_thresh), 6 + 2 * keypoints
    keys = [total_key(r[0]) for r in rows]
    order = sorted(range(len(rows)), key=lambda i: keys[i])  # stable: ties keep union order
    tied = sum(1 for i in range(len(rows)) if keys.count(keys[i]) > 1)
    out = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while order:
            seed = order.pop()
            group, keep = [seed], []
            for i in order:
                v = iou(rows[seed][2:6], rows[i][2:6])
                inside = (not (v < thr)) if remove else bool(v >= thr)
                (group if inside else keep).append(i)
            order = keep
            rec = np.zeros(20, f32)
            if remove:
                rec[:nf] = rows[seed][:nf]
            else:
                acc = np.zeros(20, f32)  # [0]: the divisor
                for i in group:
                    c = rows[i][0]
                    acc[0] = acc[0] + c
                    acc[1:nf] = acc[1:nf] + rows[i][1:nf] * c
                rec[0] = rows[seed][0]
                rec[1:nf] = acc[1:nf] / acc[0]
            out.append(rec)
    return np.array(out, f32).reshape(-1, 20), (len(rows), tied)


def merge(tile_count, tile_dets, tile_cap, keypoints, iou_thresh=0.3, remove=False):
    """One stream of zr_detect_merge_async.  Returns (rows [m][20], (candidates, tied), dropped)."""
    rows, dropped = union(tile_count, tile_dets, tile_cap)
    out, ties = nms(rows, keypoints, iou_thresh, remove)
    return out, ties, dropped


# ---- test inputs ------------------------------------------------------------------------------------------
def random_tiles(rng, T, cap, keypoints, clusters=6, counts=None):
    """[T][cap][20] rows around a few cluster centres, so that duplicates across tiles overlap, with
    distinct confidences; counts per tile."""
    dets = np.zeros((T, cap, 20), f32)
    centres = rng.uniform(100, 800, (clusters, 2))
    conf = rng.permutation(np.linspace(0.5, 0.99, T * cap)).astype(f32).reshape(T, cap)
    for t in range(T):
        for j in range(cap):
            c = centres[rng.integers(clusters)] + rng.uniform(-6, 6, 2)
            size = rng.uniform(60, 80, 2)
            dets[t, j, :6] = conf[t, j], rng.uniform(-0.5, 0.5), c[0], c[1], size[0], size[1]
            dets[t, j, 6:6 + 2 * keypoints] = rng.uniform(0, 900, 2 * keypoints)
        dets[t] = dets[t][np.argsort(-dets[t, :, 0], kind="stable")]  # a tile's own order: most confident first
    if counts is None:
        counts = rng.integers(cap // 2, cap + 1, T)
    return np.asarray(counts, np.int32), dets


def tie_case():
    """18 candidates in 3 tiles (at most 20: the reference's sort keeps their order), three of them
    sharing one confidence across tiles and overlapping, so that the order decides the sums."""
    rng = np.random.default_rng(9)
    counts, dets = random_tiles(rng, 3, 6, 6, clusters=2)
    counts[:] = 6
    for t, j in ((0, 2), (1, 2), (2, 3)):
        dets[t, j, 0] = f32(0.75)
        dets[t, j, 2:6] = 400 + 2 * t, 300 + t, 70, 70
    for t in range(3):
        dets[t] = dets[t][np.argsort(-dets[t, :, 0], kind="stable")]
    return counts, dets


# ---- rows <-> the host API's Detection ----------------------------------------------------------------
def to_detections(H, rows, keypoints):
    return [H.Detection(float(r[0]), H.Rect.from_center(float(r[2]), float(r[3]), float(r[4]), float(r[5])), float(r[1]),
                        [(float(r[6 + 2 * k]), float(r[7 + 2 * k])) for k in range(keypoints)]) for r in rows]


def from_detections(dets):
    out = np.zeros((len(dets), 20), f32)
    for i, d in enumerate(dets):
        out[i, :6] = d.confidence(), d.angle(), *d.bounding_rect().tuple()
        kp = d.keypoints()
        out[i, 6:6 + 2 * len(kp)] = np.array(kp, f32).reshape(-1)
    return out


def same_f32(a, b):
    """Equal as bits, any NaN equal to any NaN (the payload of an invalid operation is not pinned)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


# ---- the scene of the issue: two small faces on a gray 960 x 540 frame --------------------------------
SCENE_W, SCENE_H = 960, 540
FACES = ((144, 408, 200), (160, 700, 100))  # size, x0, y0


def face_patch(size):
    codes = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))["codes"][0]
    p = np.full((192, 192, 4), 255, np.uint8)
    p[..., :3] = codes.transpose(1, 2, 0)
    idx = np.arange(size) * 192 // size
    return p[idx][:, idx]


def gray_frame(bg=128):
    f = np.full((SCENE_H, SCENE_W, 4), bg, np.uint8)
    f[..., 3] = 255
    return f


def scene_frame(bg=128):
    f = gray_frame(bg)
    for size, x0, y0 in FACES:
        f[y0:y0 + size, x0:x0 + size] = face_patch(size)
    return f


def scene_tiles():
    return detection_tiles(SCENE_W, SCENE_H, 2, 1, 0.25, True)


def oracle_tiled(frame, tiles, tile_cap=64, side=128):
    """The CPU oracle's composition (oracle.Net f32, preproc, extract, nms, the detector's map with
    the tile's letterbox, nms of the union): (per-tile lists, merged list) of oracle Det."""
    import ctypes as C

    import oracle as O
    net = O.Net(os.path.join(REPO, "zaru_amd", "models", "face_detection_short_range.onnx"), f64=False)
    h, w = frame.shape[:2]
    per = []
    for cx, cy, tw, th in np.asarray(tiles, f32).tolist():
        rect = O.grow_to_fit_aspect(O.Rect(cx, cy, tw, th), side, side)
        view = O.view_compose(O.view_full(w, h), O.RRect(rect, 0.0))
        outs = net.run(O.preproc(frame, view, side, side, -1.0, 1.0)[None])
        dets = O.nms(O.extract(O.FACE, outs[0][0], outs[1][0], side, side), 0.3, 1)
        if dets:
            arr = (O.Det * len(dets))(*dets)
            O._lib().zo_detector_map(arr, len(dets), C.byref(rect), side)
            dets = [arr[i] for i in range(len(dets))]
        per.append(dets)
    merged = O.nms([d for p in per for d in p[:tile_cap]], 0.3, 1)
    return per, merged
