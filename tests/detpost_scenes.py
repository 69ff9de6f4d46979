"""Seeded crowded frames for the detector post-processing kernels (det_post_kernel,
kernels/detpost.hip; cand_kernel, kernels/misc.hip): raw `boxes [A][D]` / `logits [A]` tensors
with dozens to a thousand candidates in overlapping clusters, and edge frames at the kernels'
64-candidate chunk boundaries.  A plain helper module shared by tests/test_detpost_crowded_cpu.py
(which asserts the conditions the scenes are chosen for) and tests/test_gpu_detpost_crowded.py.

The three detector shapes (face/detection.rs:53, 86-88; hand/detection.rs:117):
    face       896 anchors, D = 16, 6 keypoints, 128 px input
    palm      2016 anchors, D = 18, 7 keypoints, 192 px input
    face_full 2304 anchors, D = 16, 6 keypoints, 192 px input
"""
import functools

import numpy as np

f32 = np.float32

#            anchors, D, keypoints, input side, oracle kind (oracle.FACE / PALM / FACE_FULL), cfg.face
SHAPES = {"face": (896, 16, 6, 128, 0, 1),
          "palm": (2016, 18, 7, 192, 1, 0),
          "face_full": (2304, 16, 6, 192, 2, 1)}

# (clusters, members); clusters None = one single-member cluster on every second anchor
CROWDS = [(12, 8), (40, 6), (100, 5), (5, 120), (None, 1)]

# The seed of each scene, per shape in CROWDS order: the first seed from 1 upwards for which
# H.nms_ties reports no tied candidate (tests/test_detpost_crowded_cpu.py asserts it).
SEEDS = {"face": [1, 1, 1, 2, 2], "palm": [1, 1, 1, 1, 1], "face_full": [1, 1, 1, 2, 4]}

# the image each frame was letterboxed from, cycled over a shape's frames (landscape, portrait, square)
IMAGES = [(640, 480), (480, 640), (1920, 1080), (256, 256), (1280, 720)]


def scene(anchors, D, side, clusters, members, seed):
    """One frame: background boxes uniform(-3, 3) with logits -9; `clusters` clusters with a centre in
    [0.1, 0.9] side and a size in [0.05, 0.3] side, each with `members` randomly chosen (distinct)
    anchors whose decoded centre is the cluster's + N(0, 0.1 size), whose size is the cluster's
    scaled by uniform(0.8, 1.25) and whose logit is uniform(0.05, 5.0).  The keypoint columns stay
    random.  Returns (boxes [A][D], logits [A]), float32."""
    anchors = np.asarray(anchors, np.float64)
    A = len(anchors)
    rng = np.random.default_rng(seed)
    boxes = rng.uniform(-3.0, 3.0, (A, D))
    logits = np.full(A, -9.0)
    chosen = rng.choice(A, clusters * members, replace=False).reshape(clusters, members)
    for c in range(clusters):
        cx, cy = rng.uniform(0.1, 0.9, 2) * side
        w, h = rng.uniform(0.05, 0.3, 2) * side
        a = chosen[c]
        boxes[a, 0] = cx + rng.normal(0.0, 0.1 * w, members) - anchors[a, 0] * side
        boxes[a, 1] = cy + rng.normal(0.0, 0.1 * h, members) - anchors[a, 1] * side
        boxes[a, 2] = w * rng.uniform(0.8, 1.25, members)
        boxes[a, 3] = h * rng.uniform(0.8, 1.25, members)
        logits[a] = rng.uniform(0.05, 5.0, members)
    return boxes.astype(f32), logits.astype(f32)


def _two_clusters(anchors, D, side, count, seed):
    """`count` candidates with distinct, evenly spread logits in (0.05, 5); the candidate of
    ascending-confidence rank r sits in cluster r % 2.  The two clusters are far apart and tight, so
    the first seed groups every second candidate of the order and retains the others, which the
    second seed then takes."""
    anchors = np.asarray(anchors, np.float64)
    A = len(anchors)
    rng = np.random.default_rng(seed)
    boxes = rng.uniform(-3.0, 3.0, (A, D))
    logits = np.full(A, -9.0)
    a = rng.permutation(A)[:count]  # rank r -> anchor a[r]: anchor order is not the sort order
    r = np.arange(count)
    size = 0.2 * side
    centre = np.where(r % 2 == 0, 0.25, 0.75) * side
    boxes[a, 0] = centre + rng.normal(0.0, 0.02 * size, count) - anchors[a, 0] * side
    boxes[a, 1] = centre + rng.normal(0.0, 0.02 * size, count) - anchors[a, 1] * side
    boxes[a, 2] = size * rng.uniform(0.95, 1.05, count)
    boxes[a, 3] = size * rng.uniform(0.95, 1.05, count)
    logits[a] = 0.05 + 4.9 * (r + 0.5) / max(count, 1)
    return boxes, logits


def _place(boxes, anchors, side, a, src):
    """Anchor a gets anchor src's row, its offset moved so that both decode to one centre."""
    boxes[a] = boxes[src]
    boxes[a, :2] += (np.asarray(anchors, np.float64)[src] - np.asarray(anchors, np.float64)[a]) * side


EDGE_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129)  # and A


def edge_frames(anchors, D, side):
    """Frames at the kernels' chunk boundaries, as a list of (name, boxes, logits, candidates):
    exactly 0, 1, 63, 64, 65, 127, 128, 129 and A candidates in two interleaved clusters; `thresh`,
    31 candidates of which one has a logit of exactly 0.0 (conf == thresh, kept) next to one of -1e-6
    (dropped); `nonfinite`, 40 candidates among which one logit each is +inf (conf 1.0), NaN and
    -NaN (a NaN confidence is kept: `conf < thresh` is false, face/detection.rs:111), and one -inf
    (conf 0, dropped) -- 43 candidates."""
    A = len(anchors)
    out = []
    for k, count in enumerate(EDGE_COUNTS + (A,)):
        boxes, logits = _two_clusters(anchors, D, side, count, 1000 + k)
        out.append((f"edge{count}", boxes.astype(f32), logits.astype(f32), count))
    boxes, logits = _two_clusters(anchors, D, side, 30, 2000)
    free = np.flatnonzero(logits < 0)
    _place(boxes, anchors, side, free[0], np.argmax(logits))  # the threshold candidate overlaps the top seed's cluster
    logits[free[0]] = 0.0
    logits[free[1]] = -1e-6
    out.append(("thresh", boxes.astype(f32), logits.astype(f32), 31))
    boxes, logits = _two_clusters(anchors, D, side, 40, 2001)
    free = np.flatnonzero(logits < 0)
    order = np.argsort(logits)
    top, second = order[-1], order[-2]  # one in each cluster
    _place(boxes, anchors, side, free[0], top)     # +inf: conf 1.0, the first seed
    _place(boxes, anchors, side, free[1], second)  # the NaNs: one in each cluster
    _place(boxes, anchors, side, free[2], top)
    _place(boxes, anchors, side, free[3], top)
    logits = logits.astype(f32)
    logits[free[0]] = np.inf
    logits[free[1]] = np.nan
    logits[free[2]] = -f32(np.nan)
    logits[free[3]] = -np.inf
    out.append(("nonfinite", boxes.astype(f32), logits, 43))
    return out


class Frames:
    """Every frame of a shape -- the crowded scenes in CROWDS order, then the edge frames: names [n],
    boxes [n][A][D], logits [n][A] (read-only), images [n] of (w, h), candidates [n], crowded [n]."""

    def __init__(self, shape):
        import zaru_amd.host as H
        self.shape = shape
        self.A, self.D, self.nkp, self.side, self.kind, self.face = SHAPES[shape]
        self.anchors = np.ascontiguousarray(H.anchors(shape), f32)
        self.names, boxes, logits, self.candidates, crowded = [], [], [], [], []
        for (clusters, members), seed in zip(CROWDS, SEEDS[shape]):
            clusters = self.A // 2 if clusters is None else clusters
            b, l = scene(self.anchors, self.D, self.side, clusters, members, seed)
            self.names.append(f"crowd{clusters}x{members}")
            boxes.append(b)
            logits.append(l)
            self.candidates.append(clusters * members)
            crowded.append(True)
        for name, b, l, c in edge_frames(self.anchors, self.D, self.side):
            self.names.append(name)
            boxes.append(b)
            logits.append(l)
            self.candidates.append(c)
            crowded.append(False)
        self.n = len(self.names)
        self.images = [IMAGES[i % len(IMAGES)] for i in range(self.n)]
        self.boxes, self.logits, self.crowded = np.stack(boxes), np.stack(logits), np.array(crowded)
        self.boxes.setflags(write=False)
        self.logits.setflags(write=False)
        self.letterbox = np.array([H.letterbox_view(w, h, self.side, self.side)[1].tuple() for w, h in self.images], f32)
        self._rows = {}

    def host(self, i, remove):
        """The host restatement's detections of frame i (H.detect_post), computed once."""
        import zaru_amd.host as H
        if ("h", i, remove) not in self._rows:
            self._rows["h", i, remove] = H.detect_post(self.shape, self.boxes[i], self.logits[i], *self.images[i],
                                                       remove=remove)
        return self._rows["h", i, remove]

    def oracle(self, i, remove):
        """The oracle's detections of frame i (O.detect_post), computed once."""
        import oracle as O
        if ("o", i, remove) not in self._rows:
            self._rows["o", i, remove] = O.detect_post(self.kind, self.boxes[i], self.logits[i], *self.images[i],
                                                       self.side, self.side, remove=remove)
        return self._rows["o", i, remove]


@functools.lru_cache(maxsize=None)
def frames(shape):
    return Frames(shape)


def same_words(a, b):
    """Bit equality of two float32 arrays, except that a NaN equals a NaN at the same position."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
