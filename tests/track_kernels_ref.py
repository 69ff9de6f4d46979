"""Plain restatements of the device loops' bookkeeping kernels (kernels/track.hip: next_view,
hand_manage_kernel, due_compact_kernel, reseed_kernel, seed_kernel), f32 values throughout, for
tests/test_gpu_track_kernels.py (each kernel alone, bit for bit) and tests/test_track_kernels_cpu.py
(these restatements against the pieces the suite already pins).  No device call is made here.

Geometry is the oracle's (oracle/geom.c: iou, grow_rel, grow_to_fit_aspect, view_compose, view_full);
the 40-byte view descriptor is zr_view_describe's.  Comparisons are written as the reference writes
them (crates/zaru/src/hand/tracking.rs:115-219): a detection is discarded, and a hand swept, on
``iou >= thresh``, so a NaN IoU (two zero-area rects: 0 / 0; two infinite ones) does neither.

Arrays are laid out as the entry points take them: stream s owns slots [s * K, s * K + K)."""
import numpy as np

import oracle as O
from zaru_amd import _lib

f32 = np.float32
STATE = np.dtype(_lib.TrackState)       # 92 bytes
MANAGE_ARRAYS = ("state", "ids", "hroi", "src", "nhands", "next_id", "next_det", "det_pending")
BRANCHES = ("compact", "untracked", "ignored", "count_clamped", "count_negative", "filtered", "newcomer",
            "dropped", "sweep_last", "sweep_move", "none_left", "due", "not_due", "nan_zero", "nan_inf",
            "nan_sweep", "nhands_over", "nhands_under")


def _rect(v):
    return O.Rect(float(v[0]), float(v[1]), float(v[2]), float(v[3]))


def describe(view5, frame):
    v = np.ascontiguousarray(view5, f32).reshape(1, 5)
    out = np.zeros((1, 10), np.uint32)
    _lib.check(_lib.lib().zr_view_describe(v.ctypes.data, 1, int(frame), out.ctypes.data))
    return out[0]


def next_view(roi5, frame_w, frame_h, aw, ah, frame):
    """track.hip next_view: view_rect = roi.grow_to_fit_aspect (landmark.rs:465), the view of it in the
    full frame, the aspect-fit local rect of that view (landmark.rs:320-323) and the view of that."""
    vr = O.RRect(O.grow_to_fit_aspect(_rect(roi5), aw, ah), float(roi5[4]))
    view = O.view_compose(O.view_full(int(frame_w), int(frame_h)), vr)
    local = O.grow_to_fit_aspect(O.rect_from_top_left(0.0, 0.0, view.rect.w, view.rect.h), aw, ah)
    net = O.view_compose(view, local)
    tl = local.top_left()
    view_rect = np.array([vr.rect.cx, vr.rect.cy, vr.rect.w, vr.rect.h, vr.rad], f32)
    loc = np.array([tl[0], tl[1], local.w], f32)
    return view_rect, loc, describe([net.rect.cx, net.rect.cy, net.rect.w, net.rect.h, net.rad], frame)


def _with_view(st, aw, ah, frame):
    st = st.copy()
    st["view_rect"], st["local"], desc = next_view(st["roi"], st["frame_w"], st["frame_h"], aw, ah, frame)
    return st, desc


def idle_state(frame_w, frame_h):
    st = np.zeros((), STATE)
    st["roi"][2:4] = 1.0
    st["frame_w"], st["frame_h"] = frame_w, frame_h
    return st


def manage(A, cfg, now, init_clock):
    """HandTracker::track's bookkeeping as hand_manage_kernel documents it.  `A` holds the arrays of
    MANAGE_ARRAYS plus count, dets [S][dcap][20] and fsize [S][2]; cfg = {K, dcap, iou, grow,
    use_angle, interval, aw, ah}.  Returns (outputs, trace): the arrays of MANAGE_ARRAYS after the
    step, `views` [S * K][10] and `dropped` [S]; ids / hroi past a stream's count are left as they
    came (the kernel does not define them).  trace[s] = {tags, rois, dets, keep, survivors}."""
    K, dcap, thr, grow = cfg["K"], cfg["dcap"], float(f32(cfg["iou"])), float(f32(cfg["grow"]))
    S = len(A["nhands"])
    out = {k: np.array(A[k], copy=True) for k in MANAGE_ARRAYS}
    out["views"] = np.zeros((S * K, 10), np.uint32)
    out["dropped"] = np.zeros(S, np.int32)
    trace = []
    for s in range(S):
        tags, base = set(), s * K
        fw, fh = A["fsize"][s]
        next_det = float(now) if init_clock else float(A["next_det"][s])
        n = int(A["nhands"][s])
        if n > K:
            tags.add("nhands_over")
        if n < 0:
            tags.add("nhands_under")
        n = min(max(n, 0), K)
        # retain_mut (116-127): a lost hand leaves; the others' RoI is their updated_roi
        hands = []
        for h in range(n):
            st = A["state"][base + h]
            if not st["active"]:
                continue
            if not st["tracked"]:
                tags.add("untracked")
            roi = np.array(st["updated"] if st["tracked"] else A["hroi"][base + h], f32)
            if h != len(hands):
                tags.add("compact")
            hands.append({"state": st.copy(), "id": int(A["ids"][base + h]), "roi": roi, "src": h})
        # retain (140-156) against the hands that existed before this step's new ones, then extend
        # (158-194); the device's slots are bounded and count the overflow
        existing = [h["roi"] for h in hands]
        dropped, next_id, keep, visited = 0, int(A["next_id"][s]), [], []
        count = int(A["count"][s])
        if not A["det_pending"][s]:
            if count != 0:
                tags.add("ignored")
        else:
            if count > dcap:
                tags.add("count_clamped")
            if count < 0:
                tags.add("count_negative")
            for d in range(min(count, dcap)):
                dd = A["dets"][s, d]
                g = O.grow_rel(_rect(dd[2:6]), grow)
                ious = [O.iou(_rect(r), g) for r in existing]
                visited.append(dd.copy())
                if any(v >= thr for v in ious):
                    tags.add("filtered")
                    keep.append(False)
                    continue
                keep.append(True)
                if any(np.isnan(v) for v in ious):
                    tags.add("nan_inf" if np.isinf(dd[4]) else "nan_zero")
                if len(hands) >= K:
                    dropped += 1
                    tags.add("dropped")
                    continue
                st = np.zeros((), STATE)
                st["roi"] = (g.cx, g.cy, g.w, g.h, dd[1] if cfg["use_angle"] else 0.0)
                st["active"], st["frame_w"], st["frame_h"] = 1, fw, fh
                hands.append({"state": st, "id": next_id, "roi": np.array(st["roi"], f32), "src": -1})
                next_id += 1
                tags.add("newcomer")
        # the swap_remove sweep (196-208): the range is fixed before the loop
        pre = [h["roi"].copy() for h in hands]
        idx = list(range(len(hands)))
        for i in reversed(range(len(hands))):
            for j in range(i):
                v = O.iou(_rect(hands[i]["roi"]), _rect(hands[j]["roi"]))
                if np.isnan(v):
                    tags.add("nan_sweep")
                if v >= thr:
                    tags.add("sweep_last" if i == len(hands) - 1 else "sweep_move")
                    hands[i], idx[i] = hands[-1], idx[-1]
                    hands.pop()
                    idx.pop()
                    break
        # the schedule (210-218)
        req = len(hands) == 0 or now >= next_det
        tags.add("none_left" if len(hands) == 0 else "due" if req else "not_due")
        if req:
            next_det += cfg["interval"]
        out["next_det"][s], out["det_pending"][s] = next_det, 1 if req else 0
        out["nhands"][s], out["next_id"][s], out["dropped"][s] = len(hands), next_id, dropped
        for h in range(K):
            i = base + h
            if h < len(hands):
                st = hands[h]["state"]
                out["ids"][i], out["hroi"][i], out["src"][i] = hands[h]["id"], hands[h]["roi"], hands[h]["src"]
            else:
                st = idle_state(fw, fh)
                out["src"][i] = -1
            out["state"][i], out["views"][i] = _with_view(st, cfg["aw"], cfg["ah"], s)
        trace.append({"tags": tags, "rois": existing, "dets": visited, "keep": keep, "pre_sweep": pre,
                      "survivors": idx})
    return out, trace


def compact(flags, template):
    """due_compact_kernel: the streams with a non-zero flag in order, each with the template view
    whose frame index is the stream."""
    due = np.flatnonzero(np.asarray(flags) != 0).astype(np.int32)
    views = np.tile(np.asarray(template, np.uint32).reshape(1, 10), (len(due), 1))
    views[:, 8] = due
    return due, views, len(due)


def total_key(v):
    """f32::total_cmp's key (num.rs): the bits, the magnitude flipped for negatives, as a signed int."""
    b = int(np.array(v, f32).view(np.int32))
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def reseed(states, counts, dets, dcap, fsize, aw, ah):
    """reseed_kernel: a stream without RoI whose detection found something takes the rect of
    max_by_key(TotalF32(confidence)) -- the last of equal maxima -- unrotated.  Returns (states,
    {stream: view descriptor}) of the re-seeded streams; the others are untouched."""
    out, views = np.array(states, copy=True), {}
    for s in range(len(out)):
        cnt = min(int(counts[s]), dcap)
        if out[s]["active"] or cnt <= 0:
            continue
        best = 0
        for k in range(1, cnt):
            if total_key(dets[s, k, 0]) >= total_key(dets[s, best, 0]):
                best = k
        st = out[s].copy()
        st["roi"][:4], st["roi"][4] = dets[s, best, 2:6], 0.0
        st["active"], st["frame_w"], st["frame_h"] = 1, fsize[s, 0], fsize[s, 1]
        out[s], views[s] = _with_view(st, aw, ah, s)
    return out, views


def seed(counts, dets, dcap, forced, nforced, fsize, R, grow, use_angle, aw, ah):
    """seed_kernel: slot k of frame f is detection k's rect (grown when grow > 0, at its angle when
    use_angle), else -- a frame without detections -- its forced RoI k, else idle."""
    N = len(counts)
    states, views = np.zeros(N * R, STATE), np.zeros((N * R, 10), np.uint32)
    for f in range(N):
        for k in range(R):
            st = np.zeros((), STATE)
            st["frame_w"], st["frame_h"] = fsize[f]
            cnt = int(counts[f])
            if k < cnt and k < dcap:
                d = dets[f, k]
                r = _rect(d[2:6])
                if grow > 0:
                    r = O.grow_rel(r, float(f32(grow)))
                st["roi"] = (r.cx, r.cy, r.w, r.h, d[1] if use_angle else 0.0)
                st["active"] = 1
            elif cnt == 0 and nforced is not None and k < int(nforced[f]):
                st["roi"], st["active"] = forced[f, k], 1
            else:
                st["roi"][2:4] = 1.0
            states[f * R + k], views[f * R + k] = _with_view(st, aw, ah, f)
    return states, views


# ---- the scenario table of the manage tests -----------------------------------------------------------
KINDS = ("compact", "untracked", "ignored", "count_clamped", "count_negative", "filtered", "dropped",
         "pair", "move", "none_left", "nan_zero", "nan_inf", "plain")
NHANDS_OVER_AT, NHANDS_UNDER_AT = 40, 91   # in the middle: even an unclamped read stays inside the arrays


def _det(conf, angle, cx, cy, w, h):
    d = np.zeros(20, f32)
    d[:6] = conf, angle, cx, cy, w, h
    d[6:] = np.arange(14) + 0.5   # keypoints: never read by the bookkeeping
    return d


def scenarios(cfg, S=150, seed_=2024):
    """S streams of K slots, each of one KINDS scenario (s % len(KINDS)) with seeded jitter; objects sit
    in columns 110 px apart and are 60..80 px wide, so only the overlaps a scenario builds exist."""
    K, dcap, grow = cfg["K"], cfg["dcap"], cfg["grow"]
    rng = np.random.default_rng(seed_)
    A = {"state": np.zeros(S * K, STATE), "ids": np.zeros(S * K, np.uint64), "hroi": np.zeros((S * K, 5), f32),
         "src": np.full(S * K, 7, np.int32), "nhands": np.zeros(S, np.int32), "next_id": np.zeros(S, np.uint64),
         "next_det": rng.uniform(-1e6, 1e6, S), "det_pending": np.ones(S, np.int32),
         "count": np.zeros(S, np.int32), "dets": rng.uniform(-9, 9, (S, dcap, 20)).astype(f32),
         "fsize": np.c_[640 + np.arange(S), 480 + np.arange(S) % 7].astype(np.uint32)}
    A["hroi"][:] = rng.uniform(1, 500, (S * K, 5))      # stale: a tracked hand's is replaced
    A["ids"][:] = rng.integers(0, 2 ** 62, S * K, dtype=np.int64).astype(np.uint64)
    A["next_id"][:] = (np.arange(S) * 1000 + 2 ** 33).astype(np.uint64)

    def col(c, dy=0.0, size=None):
        w = f32(rng.uniform(60, 80)) if size is None else size
        return np.array([60 + 110 * c + rng.uniform(-5, 5), 200 + dy + rng.uniform(-5, 5), w, w * f32(1.125)], f32)

    def hand(s, h, rect, tracked=True, active=True, angle=None):
        st = A["state"][s * K + h]
        a = f32(rng.uniform(-1, 1)) if angle is None else angle
        st["updated"] = (*rect, a)
        st["roi"] = (rect[0], rect[1], rect[2] * f32(1.5), rect[3] * f32(1.5), a)   # the tracker's padded RoI
        st["view_rect"], st["local"] = rng.uniform(0, 9, 5), rng.uniform(0, 9, 3)   # rewritten by the step
        st["active"], st["tracked"] = int(active), int(tracked and active)
        st["frame_w"], st["frame_h"] = A["fsize"][s]
        st["confidence"] = rng.uniform(0.5, 1)
        if not st["tracked"]:
            A["hroi"][s * K + h] = (*rect, a)
        A["nhands"][s] = max(A["nhands"][s], h + 1)

    def dets(s, *rects, count=None):
        for k, r in enumerate(rects):
            A["dets"][s, k] = _det(rng.uniform(0.5, 1), rng.uniform(-1, 1), *r)
        A["count"][s] = len(rects) if count is None else count

    def shrunk(rect):   # the detection whose grown box is (about) rect
        g = f32(1 + 2 * grow)
        return np.array([rect[0], rect[1], rect[2] / g, rect[3] / g], f32)

    for s in range(S):
        kind = KINDS[s % len(KINDS)]
        if kind == "compact":          # lost hands between live ones
            for h in range(4):
                hand(s, h, col(h), active=h in (0, 2) if s % 2 else h in (1, 3))
            dets(s)
        elif kind == "untracked":      # an active slot without an estimate keeps its hroi
            for h in range(3):
                hand(s, h, col(h), tracked=h != 1)
            dets(s, shrunk(col(3)))
        elif kind == "ignored":        # det_pending = 0: the count is not looked at
            hand(s, 0, col(0))
            hand(s, 1, col(1))
            dets(s, shrunk(col(2)), shrunk(col(3)), shrunk(col(4)))
            A["det_pending"][s] = 0
        elif kind == "count_clamped":  # dcap detections are there, the count says more
            r0 = col(0)
            hand(s, 0, r0)
            dets(s, shrunk(col(1)), shrunk(r0), shrunk(col(2)), *(shrunk(col(c, 120)) for c in range(dcap - 3)),
                 count=dcap + 3)
        elif kind == "count_negative":
            hand(s, 0, col(0))
            dets(s, shrunk(col(1)), count=-3)
        elif kind == "filtered":       # on top of an existing RoI, then a newcomer
            r1 = col(1)
            hand(s, 0, col(0))
            hand(s, 1, r1, tracked=bool(s & 1))
            dets(s, shrunk(r1), shrunk(col(2)))
        elif kind == "dropped":        # more kept detections than free slots
            for h in range(K - 1):
                hand(s, h, col(h))
            dets(s, shrunk(col(0, 120)), shrunk(col(1, 120)), shrunk(col(2, 120)))
        elif kind == "pair":           # two newcomers on each other: the sweep removes the last
            hand(s, 0, col(0))
            r = col(2)
            dets(s, shrunk(r), shrunk(r + np.array([3, 2, 0, 0], f32)))
        elif kind == "move":           # the removed one is not the last: the last moves into its slot
            hand(s, 0, col(0))
            r = col(1)
            dets(s, shrunk(r), shrunk(r + np.array([2, 3, 0, 0], f32)), shrunk(col(3)))
        elif kind == "none_left":
            hand(s, 0, col(0), active=False)
            hand(s, 1, col(1), active=False)
            dets(s)
        elif kind == "nan_zero":       # a RoI collapsed to a point and zero-size detections: IoU = 0 / 0
            p = col(1)
            hand(s, 0, col(0))
            hand(s, 1, np.array([p[0], p[1], 0, 0], f32))
            dets(s, np.array([p[0], p[1], 0, 0], f32), np.array([p[0] + 50, p[1] + 9, 0, 0], f32))
        elif kind == "nan_inf":        # infinite sizes: inf / inf
            p = col(0)
            hand(s, 0, np.array([p[0], p[1], np.inf, np.inf], f32), angle=f32(0))
            dets(s, np.array([p[0], p[1], np.inf, np.inf], f32))
        else:                          # plain: live hands and a newcomer
            for h in range(int(rng.integers(1, 4))):
                hand(s, h, col(h))
            dets(s, shrunk(col(4)))
    for s, n in ((NHANDS_OVER_AT, K + 3), (NHANDS_UNDER_AT, -2)):   # counts the kernel clamps to K and 0
        for h in range(K):
            hand(s, h, col(h, -120))   # a row of their own: the next stream's hands, read as theirs, would stay
        dets(s)
        A["nhands"][s] = n
    return A


def second_step(out1, cfg, seed_=77):
    """The inputs of a second step on the first one's outputs, with what happens in between made up:
    an update that loses some hands and moves others (one onto its neighbour), new detections, and
    clocks that differ between streams (some not yet due, one due exactly now)."""
    K, dcap = cfg["K"], cfg["dcap"]
    S = len(out1["nhands"])
    rng = np.random.default_rng(seed_)
    A = {k: np.array(out1[k], copy=True) for k in MANAGE_ARRAYS}
    now = float(A["next_det"].max()) - cfg["interval"] + 15.0
    for s in range(S):
        n = int(A["nhands"][s])
        finite = bool(np.isfinite(A["hroi"][s * K:s * K + n]).all())
        for h in range(n):
            st = A["state"][s * K + h]
            r = rng.random()
            if r < 0.2:
                st["active"] = st["tracked"] = 0                      # lost
            elif r < 0.8:
                st["tracked"], st["confidence"] = 1, rng.uniform(0.5, 1)
                st["updated"] = A["hroi"][s * K + h] + (rng.uniform(-4, 4, 5) * (1, 1, 0, 0, 0.01)).astype(f32)
                st["roi"] = st["updated"]
            else:
                st["tracked"] = 0                                     # no estimate yet: keeps its hroi
        if n >= 2 and finite and s % 4 == 0:                          # drifted onto the first: swept
            st = A["state"][s * K + n - 1]
            st["active"] = st["tracked"] = 1
            st["updated"] = A["state"][s * K]["updated"] if A["state"][s * K]["tracked"] else A["hroi"][s * K]
        A["next_det"][s] = now + (-30.0, 0.0, 25.0)[s % 3]
    A["count"] = rng.integers(-1, dcap + 2, S).astype(np.int32)
    d = rng.uniform(0, 1, (S, dcap, 20)).astype(f32)
    d[..., 2], d[..., 3] = rng.uniform(40, 600, (S, dcap)), rng.uniform(40, 440, (S, dcap))
    d[..., 4:6] = rng.uniform(20, 50, (S, dcap, 2))
    A["dets"], A["fsize"] = d, np.c_[640 + np.arange(S), 480 + np.arange(S) % 7].astype(np.uint32)
    return A, now


def coverage(*traces):
    """Branch -> the number of streams it occurred in, over the given steps' traces."""
    n = dict.fromkeys(BRANCHES, 0)
    for tr in traces:
        for t in tr:
            for tag in t["tags"]:
                n[tag] += 1
    return n


def same_f32(a, b):
    """Bit equality of two f32 arrays, any NaN equal to any NaN: the sign and payload of a NaN an
    operation makes (inf - inf: x86 gives 0xffc00000, gfx950 0x7fc00000, in the view_rect of an
    infinite RoI) are the processor's choice, which neither IEEE 754 nor the reference pins.  Every
    other value, the sign of a zero and infinities included, is compared
    by its bits."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


FLOAT_FIELDS = ("roi", "view_rect", "local", "confidence", "updated")
INT_FIELDS = ("active", "frame_w", "frame_h", "tracked")


def same_states(a, b):
    """same_f32 over the float fields of two TrackState arrays, equality over the others."""
    return all(same_f32(a[k], b[k]) for k in FLOAT_FIELDS) and all(np.array_equal(a[k], b[k]) for k in INT_FIELDS)


def same_views(a, b):
    """View descriptors: eight floats (same_f32), the frame index and the padding word."""
    a, b = np.ascontiguousarray(a, np.uint32).reshape(-1, 10), np.ascontiguousarray(b, np.uint32).reshape(-1, 10)
    return same_f32(a[:, :8].view(f32), b[:, :8].view(f32)) and np.array_equal(a[:, 8:], b[:, 8:])


# ---- NaN IoU in NMS: one BlazeFace-shaped frame ----------------------------------------------------------
def nms_nan_frame(anchors):
    """896 anchors, D = 16, every logit -20 but seven with distinct confidences: three zero-size boxes
    (two at one centre, one elsewhere; the IoU of any two of them is 0 / 0), two overlapping
    ordinary boxes and two disjoint ones.  SuppressionMode::Remove retains a candidate only while
    iou < thresh, so the first zero-size box removes the other two; Average groups on iou >= thresh,
    so each stays alone.  Returns (boxes [896][16], logits [896], image size)."""
    A, D = 896, 16
    rng = np.random.default_rng(12)
    boxes = rng.uniform(-2, 2, (A, D)).astype(f32)
    boxes[:, 2:4] = 10.0
    logits = np.full(A, -20.0, f32)
    an = np.asarray(anchors, f32) * f32(128)
    #       anchor, confidence, (dx, dy, w, h)
    seven = [(40, 0.97, (0.0, 0.0, 0.0, 0.0)),                                        # zero-size, top of the order
             (300, 0.95, (0.0, 0.0, 24.0, 20.0)),                                     # ordinary, overlapped by 301
             (700, 0.90, (0.0, 0.0, 18.0, 18.0)),                                     # disjoint
             (120, 0.85, (an[40, 0] - an[120, 0], an[40, 1] - an[120, 1], 0.0, 0.0)),  # zero-size at 40's centre
             (301, 0.80, (3.0, 2.0, 24.0, 20.0)),
             (500, 0.75, (1.0, -1.0, 0.0, 0.0)),                                      # zero-size elsewhere
             (860, 0.70, (0.0, 0.0, 12.0, 16.0))]                                     # disjoint
    for a, conf, b in seven:
        boxes[a, :4] = b
        logits[a] = np.log(conf / (1 - conf))
    return boxes, logits, (640, 480)


def det_rows(dets, host):
    """Detections of the host API (host) or the oracle as the device's rows of 20 floats: {conf, angle,
    cx, cy, w, h, 7 x (kx, ky)}, keypoints past the network's zero."""
    out = np.zeros((len(dets), 20), f32)
    for i, d in enumerate(dets):
        if host:
            out[i, :6] = d.confidence(), d.angle(), *d.bounding_rect().tuple()
            kp = d.keypoints()
        else:
            out[i, :6] = d.conf, d.angle, *d.rect.tuple()
            kp = [(d.kp[k][0], d.kp[k][1]) for k in range(d.nkp)]
        out[i, 6:6 + 2 * len(kp)] = np.array(kp, f32).reshape(-1)
    return out
