"""The bookkeeping kernels the device loops stand on, each alone on synthetic data and past one
wavefront, workgroup and 1024-stream chunk, against tests/track_kernels_ref.py (pinned without a GPU
by tests/test_track_kernels_cpu.py):

  * hand_manage_kernel (zr_multi_manage_async, zr_hand_manage_async): 150 streams of 5 slots;
  * due_compact_kernel (zr_due_compact_async, zr_track_lost_compact_async): up to 2500 streams;
  * reseed_kernel (zr_track_reseed_best_async): 300 streams;
  * seed_kernel (zr_track_seed_detections_async): 70 frames of 4 slots;
  * det_post_kernel with a frame map (zr_detect_post_mapped_async) against the plain call.

Every comparison is of bits.  The one exception is a NaN the arithmetic itself makes (the views of an
infinite RoI: inf - inf): any NaN equals any NaN there, its sign and payload being the processor's
choice (track_kernels_ref.same_f32).  Output buffers start as 0xA5 bytes, and what a contract leaves
unwritten must still hold them."""
import ctypes as C
import os

import numpy as np
import pytest

import track_kernels_ref as R
from zaru_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32
A5 = 0xA5A5A5A5
CONFIGS = {"faces": dict(K=5, dcap=6, iou=0.3, grow=0.0, use_angle=0, interval=40.0, aw=1, ah=1),
           "hands": dict(K=5, dcap=6, iou=0.3, grow=1.5, use_angle=1, interval=40.0, aw=1, ah=1)}
S_MANAGE, NOW = 150, 1000.0


class HandCfg(C.Structure):
    _fields_ = [("slots", C.c_int), ("iou_thresh", C.c_float), ("palm_grow", C.c_float),
                ("interval_ms", C.c_double), ("aspect_w", C.c_int), ("aspect_h", C.c_int)]


class DetCfg(C.Structure):
    _fields_ = [("face", C.c_int), ("anchors", C.c_int), ("params", C.c_int), ("keypoints", C.c_int),
                ("in_w", C.c_int), ("in_h", C.c_int), ("thresh", C.c_float), ("iou", C.c_float), ("mode", C.c_int)]


def _up(a):
    return _lib.DeviceBuffer.from_array(a)


def _sentinel(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xA5, np.uint8).view(dtype).reshape(shape)


# ---- manage -----------------------------------------------------------------------------------------------
_FIRST = {}


def _first_step(name):
    """The scenario table and the restatement's first step of a configuration, computed once."""
    if name not in _FIRST:
        a = R.scenarios(CONFIGS[name], S_MANAGE)
        _FIRST[name] = (a, *R.manage(a, CONFIGS[name], NOW, 1))
    return _FIRST[name]


def _device_manage(entry, cfg, A, now, init_clock):
    """One call over S streams whose arrays carry one more stream of 0xA5 bytes, which must come back
    untouched.  Returns the outputs in the restatement's layout."""
    lib = _lib.lib()
    S, K, dcap = len(A["nhands"]), cfg["K"], cfg["dcap"]
    host = dict(A)
    host["views"], host["dropped"] = _sentinel((S * K, 10), np.uint32), _sentinel((S,), np.int32)
    rows, dev = {}, {}
    for k, a in host.items():
        b = np.ascontiguousarray(a).view(np.uint8).reshape(S, -1)
        rows[k] = b.shape[1]
        dev[k] = _up(np.vstack([b, np.full((1, b.shape[1]), 0xA5, np.uint8)]))
    if entry == "multi":
        c = _lib.MultiCfg(slots=K, iou_thresh=cfg["iou"], det_grow=cfg["grow"], use_angle=cfg["use_angle"],
                          interval_ms=cfg["interval"], aspect_w=cfg["aw"], aspect_h=cfg["ah"])
        fn = lib.zr_multi_manage_async
    else:
        assert cfg["use_angle"] == 1   # the hand tracker always takes the detection's angle
        c = HandCfg(K, cfg["iou"], cfg["grow"], cfg["interval"], cfg["aw"], cfg["ah"])
        fn = lib.zr_hand_manage_async
    _lib.check(fn(dev["state"].ptr, dev["ids"].ptr, dev["hroi"].ptr, dev["src"].ptr, dev["nhands"].ptr,
                  dev["next_id"].ptr, dev["next_det"].ptr, dev["det_pending"].ptr, dev["count"].ptr, dev["dets"].ptr,
                  dcap, dev["fsize"].ptr, S, C.byref(c), now, init_clock, dev["views"].ptr, dev["dropped"].ptr, None))
    _lib.synchronize()
    out = {}
    for k, a in host.items():
        got = dev[k].download((S + 1, rows[k]), np.uint8)
        assert (got[S] == 0xA5).all(), ("the stream past n was touched", k)
        out[k] = got[:S].reshape(-1).view(np.asarray(a).dtype).reshape(np.asarray(a).shape)
    for k in ("count", "dets", "fsize"):
        assert out[k].tobytes() == np.ascontiguousarray(A[k]).tobytes(), ("an input was written", k)
    return out


def _check_manage(got, want, K, step):
    S = len(want["nhands"])
    for k in ("nhands", "det_pending", "next_det", "next_id", "dropped", "src"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (step, k, "streams" if k != "src" else "slots", bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    for i in range(S * K):
        assert R.same_states(got["state"][i:i + 1], want["state"][i:i + 1]), (step, "state", divmod(i, K))
        assert R.same_views(got["views"][i], want["views"][i]), (step, "view", divmod(i, K))
    for s in range(S):
        live = slice(s * K, s * K + int(want["nhands"][s]))
        assert np.array_equal(got["ids"][live], want["ids"][live]), (step, "ids", s)
        assert R.same_f32(got["hroi"][live], want["hroi"][live]), (step, "hroi", s)


@pytest.mark.parametrize("entry,name", [("multi", "faces"), ("multi", "hands"), ("hand", "hands")])
def test_manage_alone(entry, name):
    """150 streams (three workgroups of 64 threads, the last partial) x 5 slots, two steps: the clock
    starts in the first, and the second runs on the first one's outputs after a made-up update.  The
    table (track_kernels_ref.scenarios) holds every branch of the bookkeeping in at least three
    streams, the NaN-IoU rows (zero-area and infinite RoI / detection pairs: the reference starts an
    object, and the sweep keeps it) and two streams whose count is outside 0..K."""
    cfg = CONFIGS[name]
    a1, want1, _ = _first_step(name)
    got1 = _device_manage(entry, cfg, a1, NOW, 1)
    _check_manage(got1, want1, cfg["K"], "first")
    for s in (R.NHANDS_OVER_AT, R.NHANDS_UNDER_AT):   # counts K + 3 and -2 behave as K and 0
        assert got1["nhands"][s] == (cfg["K"] if s == R.NHANDS_OVER_AT else 0)
    a2, now2 = R.second_step(got1, cfg)
    want2, _ = R.manage(a2, cfg, now2, 0)
    got2 = _device_manage(entry, cfg, a2, now2, 0)
    _check_manage(got2, want2, cfg["K"], "second")
    assert 0 < got2["det_pending"].sum() < S_MANAGE   # clocks due and not due


# ---- due / lost compact -----------------------------------------------------------------------------------
def _flags(case):
    rng = np.random.default_rng(31)
    n = {"one": 1, "none": 130, "all": 70, "mixed": 2500}[case]   # mixed: past two 1024-stream chunks, no multiple of 64
    if case == "none":
        return np.zeros(n, np.int32)
    if case in ("one", "all"):
        return np.ones(n, np.int32)
    due = (rng.random(n) < 0.55).astype(np.int32)
    due[0] = due[-1] = 1
    due[100:300] = 0          # runs of zeros and ones across wave and chunk borders
    due[1000:1100] = 1
    due[2040:2060] = 5        # any non-zero flag counts
    due[2060:2070] = -1
    return due


@pytest.mark.parametrize("which", ["due", "lost"])
@pytest.mark.parametrize("case", ["one", "none", "all", "mixed"])
def test_due_compact_alone(case, which):
    lib = _lib.lib()
    flags = _flags(case)
    n = len(flags)
    rng = np.random.default_rng(n)
    tmpl = rng.integers(1, 2 ** 31, 10, dtype=np.int64).astype(np.uint32)
    if which == "due":
        d_in, fn = _up(flags), lib.zr_due_compact_async
    else:   # a stream is due when its tracker holds no RoI; any non-zero `active` is a RoI
        st = np.frombuffer(rng.integers(0, 256, n * R.STATE.itemsize, dtype=np.uint8).tobytes(), R.STATE).copy()
        st["active"] = np.where(flags != 0, 0, rng.integers(1, 2 ** 32, n, dtype=np.uint64)).astype(np.uint32)
        d_in, fn = _up(st), lib.zr_track_lost_compact_async
    d_due, d_views = _up(_sentinel((n + 1,), np.int32)), _up(_sentinel((n + 1, 10), np.uint32))
    d_n, d_total = _up(np.array([-5], np.int32)), _up(np.array([1000, A5], np.uint64))
    want_due, want_views, m = R.compact(flags, tmpl)
    for total, want_total in ((d_total.ptr, 1000 + m), (None, 1000 + m)):   # with and without the running total
        d_n.upload(np.array([-5], np.int32))
        _lib.check(fn(d_in.ptr, n, tmpl.ctypes.data, d_due.ptr, d_n.ptr, d_views.ptr, total, None))
        _lib.synchronize()
        assert d_n.download((1,), np.int32)[0] == m
        assert d_total.download((2,), np.uint64).tolist() == [want_total, A5]
        due, views = d_due.download((n + 1,), np.int32), d_views.download((n + 1, 10), np.uint32)
        assert np.array_equal(due[:m], want_due) and np.array_equal(views[:m], want_views)
        assert (due[m:].view(np.uint32) == A5).all() and (views[m:] == A5).all(), "written at or past *ndue"
    if case == "mixed":
        assert m > 1024 and n > 2048 and n % 64


# ---- reseed -----------------------------------------------------------------------------------------------
def _bits(u):
    return np.array(u, np.uint32).view(f32)


def _reseed_case():
    N, dcap = 300, 8   # two workgroups of 256 threads, the last partial
    rng = np.random.default_rng(5)
    st = np.frombuffer(rng.integers(0, 256, N * R.STATE.itemsize, dtype=np.uint8).tobytes(), R.STATE).copy()
    for k in R.FLOAT_FIELDS:   # ordinary floats (a random NaN would only blur the comparison)
        st[k] = rng.uniform(-500, 500, st[k].shape)
    st["active"] = 0
    counts = rng.integers(1, dcap + 1, N).astype(np.int32)
    dets = rng.uniform(0, 1, (N, dcap, 20)).astype(f32)
    dets[..., 2:4] = rng.uniform(0, 600, (N, dcap, 2))
    dets[..., 4:6] = rng.uniform(10, 300, (N, dcap, 2))
    pnan, nnan = _bits(0x7FC00000), _bits(0xFFC00000)
    best = {}
    for s in range(N):
        kind = s % 12
        if kind == 0:
            st["active"][s] = (1, 7, 2 ** 31)[s // 12 % 3]          # tracked this frame: untouched
        elif kind == 1:
            counts[s] = 0
        elif kind == 2:
            counts[s] = -4
        elif kind == 3:
            counts[s], dets[s, dcap - 1, 0] = dcap + 3, 2.0          # the count is clamped; the last slot wins
            best[s] = dcap - 1
        elif kind == 4:
            counts[s], dets[s, 1, 0], dets[s, 5, 0], dets[s, 6, 0] = 7, 0.999, 0.999, 0.5
            dets[s, 0, 0] = 0.999 if s & 1 else 0.1                  # equal maxima: the last wins
            best[s] = 5
        elif kind == 5:
            counts[s], dets[s, 2, 0], dets[s, 4, 0] = 6, pnan, np.inf  # +NaN is the greatest key
            best[s] = 2
        elif kind == 6:
            counts[s] = 4
            dets[s, :4, 0] = (-1e30, nnan, -np.inf, -2e30)            # -NaN is the lowest, below -inf
            best[s] = 0
        elif kind == 7:
            counts[s] = 3
            dets[s, :3, 0] = (-0.0, 0.0, -0.0) if s & 1 else (0.0, -0.0, -0.0)   # -0.0 < +0.0
            best[s] = 1 if s & 1 else 0
        elif kind == 8:
            counts[s] = 5
            dets[s, :5, 0] = -rng.uniform(1, 2, 5)                   # all negative: the least negative
            dets[s, 3, 0] = -0.5
            best[s] = 3
        elif kind == 9:
            counts[s], dets[s, 1, 0], dets[s, 6, 0] = dcap, np.inf, 3e38
            best[s] = 1
        elif kind == 10:
            counts[s], dets[s, 0, 0] = 1, nnan                        # alone: taken whatever it is
            best[s] = 0
    fsize = np.c_[320 + np.arange(N), 240 + np.arange(N) % 11].astype(np.uint32)
    return N, dcap, st, counts, dets, fsize, best


def test_reseed_alone():
    lib = _lib.lib()
    N, dcap, st, counts, dets, fsize, best = _reseed_case()
    aw, ah = 4, 3
    want, want_views = R.reseed(st, counts, dets, dcap, fsize, aw, ah)
    for s, k in best.items():   # the restatement picks what the case was built to make it pick
        assert s in want_views and want["roi"][s].tobytes() == np.array([*dets[s, k, 2:6], 0], f32).tobytes(), s
    m = len(want_views)
    assert 0 < m < N and sum(1 for s in range(N) if s not in want_views) >= 3 * (N // 12)
    cfg = _lib.TrackCfg(kind=0, num_landmarks=468, in_w=192, in_h=192, aspect_w=aw, aspect_h=ah, loss_thresh=0.5,
                        padding=0.3, rois_per_frame=1)
    d_counts, d_dets, d_fsize = _up(counts), _up(dets), _up(fsize)
    d_n = _up(np.array([500, A5], np.uint64))
    for counter in (d_n.ptr, None):   # with and without the running count
        d_st, d_views = _up(np.concatenate([st, _sentinel((1,), R.STATE)])), _up(_sentinel((N + 1, 10), np.uint32))
        _lib.check(lib.zr_track_reseed_best_async(d_counts.ptr, d_dets.ptr, dcap, d_fsize.ptr, N, C.byref(cfg),
                                                  d_st.ptr, d_views.ptr, counter, None))
        _lib.synchronize()
        got, views = d_st.download((N + 1,), R.STATE), d_views.download((N + 1, 10), np.uint32)
        assert d_n.download((2,), np.uint64).tolist() == [500 + m, A5]
        assert got[N:].tobytes() == _sentinel((1,), R.STATE).tobytes() and (views[N] == A5).all()
        for s in range(N):
            if s in want_views:
                assert R.same_states(got[s:s + 1], want[s:s + 1]), ("state", s, s % 12)
                assert R.same_views(views[s], want_views[s]), ("view", s, s % 12)
            else:
                assert got[s:s + 1].tobytes() == st[s:s + 1].tobytes() and (views[s] == A5).all(), ("touched", s)


# ---- seed from detections ---------------------------------------------------------------------------------
@pytest.mark.parametrize("grow,use_angle", [(0.0, 0), (1.5, 1), (0.0, 1), (1.5, 0)])
@pytest.mark.parametrize("dcap", [3, 8])
def test_seed_detections_alone(dcap, grow, use_angle):
    lib = _lib.lib()
    N, Rr, aw, ah = 70, 4, 3, 4   # 280 slots: two workgroups of 256 threads
    rng = np.random.default_rng(100 + dcap)
    counts = (np.arange(N) % (Rr + 4) - 1).astype(np.int32)   # -1, 0 .. R + 2
    dets = rng.uniform(-1, 1, (N, dcap, 20)).astype(f32)
    dets[..., 2:4] = rng.uniform(0, 600, (N, dcap, 2))
    dets[..., 4:6] = rng.uniform(10, 300, (N, dcap, 2))
    forced = rng.uniform(5, 400, (N, Rr, 5)).astype(f32)
    nforced = np.array([(0, Rr - 2, Rr, Rr + 3)[f // (Rr + 4) % 4] for f in range(N)], np.int32)
    assert {int(v) for v in nforced[counts == 0]} == {0, Rr - 2, Rr, Rr + 3}
    fsize = np.c_[640 + np.arange(N), 480 - np.arange(N)].astype(np.uint32)
    cfg = _lib.TrackCfg(kind=0, num_landmarks=468, in_w=192, in_h=192, aspect_w=aw, aspect_h=ah, loss_thresh=0.5,
                        padding=0.3, rois_per_frame=Rr)
    d_counts, d_dets, d_forced, d_nforced, d_fsize = _up(counts), _up(dets), _up(forced), _up(nforced), _up(fsize)
    n = N * Rr
    for with_forced, with_copy in ((True, True), (False, True), (True, False)):
        want, want_views = R.seed(counts, dets, dcap, forced if with_forced else None,
                                  nforced if with_forced else None, fsize, Rr, grow, use_angle, aw, ah)
        d_st, d_copy = _up(_sentinel((n + 1,), R.STATE)), _up(_sentinel((n + 1,), R.STATE))
        d_views = _up(_sentinel((n + 1, 10), np.uint32))
        _lib.check(lib.zr_track_seed_detections_async(
            d_counts.ptr, d_dets.ptr, dcap, d_forced.ptr if with_forced else None,
            d_nforced.ptr if with_forced else None, d_fsize.ptr, N, C.byref(cfg), grow, use_angle, d_st.ptr,
            d_copy.ptr if with_copy else None, d_views.ptr, None))
        _lib.synchronize()
        got, copy = d_st.download((n + 1,), R.STATE), d_copy.download((n + 1,), R.STATE)
        views = d_views.download((n + 1, 10), np.uint32)
        for i in range(n):
            assert got[i:i + 1].tobytes() == want[i:i + 1].tobytes(), ("state", divmod(i, Rr), with_forced)
            assert views[i].tobytes() == want_views[i].tobytes(), ("view", divmod(i, Rr), with_forced)
        tail = _sentinel((1,), R.STATE).tobytes()
        assert got[n:].tobytes() == tail and (views[n] == A5).all()
        assert copy.tobytes() == (got.tobytes() if with_copy else tail * (n + 1))
        active = want["active"].reshape(N, Rr).sum(1)
        assert {int(v) for v in active} == set(range(Rr + 1)) if with_forced else active.max() == min(Rr, dcap)


# ---- mapped post-processing -------------------------------------------------------------------------------
def test_detect_post_mapped_alone():
    """The face frames of tests/golden/decode_cases.npz through a permutation map with two frames
    fewer than there are: slot map[f] is row f of the plain call, the skipped slots keep 0xA5."""
    import zaru_amd.host as H
    lib = _lib.lib()
    g = np.load(os.path.join(GOLDEN, "decode_cases.npz"))
    keys = sorted({k.split("/")[0] for k in g.files if k.startswith("face")})
    A, D, side, dcap = 896, 16, 128, 32
    n = len(keys)
    boxes = np.stack([g[f"{k}/boxes"].reshape(A, D) for k in keys]).astype(f32)
    logits = np.stack([g[f"{k}/confs"].reshape(A) for k in keys]).astype(f32)
    lbox = np.array([H.letterbox_view(*(int(v) for v in g[f"{k}/img"]), side, side)[1].tuple() for k in keys], f32)
    fmap = np.array([3, 0, 4, 1, 2], np.int32)
    assert n == 5 and sorted(fmap) == list(range(n))
    cfg = DetCfg(1, A, D, 6, side, side, 0.5, 0.3, 0)
    d_logits, d_boxes, d_anchors = _up(logits), _up(boxes), _up(H.anchors("face").astype(f32))
    # the plain call
    d_lbox = _up(lbox)
    d_count, d_dets, d_ties = (_up(_sentinel(s, np.uint32)) for s in ((n,), (n, dcap, 20), (n, 2)))
    _lib.check(lib.zr_detect_post_async(d_logits.ptr, d_boxes.ptr, d_anchors.ptr, d_lbox.ptr, n, C.byref(cfg),
                                        d_count.ptr, d_dets.ptr, dcap, None, 0, 0, 1, d_ties.ptr, None))
    _lib.synchronize()
    count = d_count.download((n,), np.int32)
    dets, ties = d_dets.download((n, dcap, 20), np.uint32), d_ties.download((n, 2), np.int32)
    for i, k in enumerate(keys):   # (the plain call is the fixture's)
        want = g[f"{k}/want"]
        assert count[i] == len(want) and np.array_equal(dets[i, :len(want)], want.view(np.uint32)), k
    # the mapped call: the letterbox is the output slot's
    lbox_m = np.zeros_like(lbox)
    lbox_m[fmap] = lbox
    d_lbox_m, d_map, d_nf = _up(lbox_m), _up(fmap), _up(np.array([n - 2], np.int32))
    m_count, m_dets, m_ties = (_up(_sentinel(s, np.uint32)) for s in ((n,), (n, dcap, 20), (n, 2)))
    _lib.check(lib.zr_detect_post_mapped_async(d_logits.ptr, d_boxes.ptr, d_anchors.ptr, d_lbox_m.ptr, n, d_map.ptr,
                                               d_nf.ptr, C.byref(cfg), m_count.ptr, m_dets.ptr, dcap, m_ties.ptr, None))
    _lib.synchronize()
    got_count = m_count.download((n,), np.int32)
    got_dets, got_ties = m_dets.download((n, dcap, 20), np.uint32), m_ties.download((n, 2), np.int32)
    for f in range(n - 2):
        slot = fmap[f]
        assert got_count[slot] == count[f] and np.array_equal(got_ties[slot], ties[f]), f
        assert np.array_equal(got_dets[slot], dets[f]), f   # the detections, and 0xA5 past them
    for f in range(n - 2, n):
        slot = fmap[f]
        assert got_count[slot:slot + 1].view(np.uint32)[0] == A5 and (got_dets[slot] == A5).all(), ("skipped", f)
        assert (got_ties[slot].view(np.uint32) == A5).all()
