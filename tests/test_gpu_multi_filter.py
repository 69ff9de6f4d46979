"""Landmark filters in the multi-object loop (DeviceMultiTracker.set_filter): a filter's state
belongs to an object and follows it from slot to slot.

A. zr_lm_filter_indexed_async alone on the scripted moves of tests/multi_filter_ref.py, against
   that model (pinned on the CPU by tests/test_multi_filter_cpu.py), bit for bit;
B. zr_track_update_positions_indexed_async fed by filter kind none against
   zr_track_update_indexed_async;
C. the loop on a script of injected detections against tests/multi_tracker_ref.py, whose trackers
   carry the filter (bit for bit: ids, RoIs, landmarks, confidence), with compaction on and off;
D. real detections: a face leaves, the survivor moves to slot 0 and keeps its state, a newcomer
   takes the vacated slot and starts from the default state;
E. set_filter during a run resets every object, set_filter(None) returns to the unfiltered path,
   the pose is taken from the filtered landmarks, a bad elapsed is refused before anything runs.

Time: the loop consumes an estimate one step after it is made, so what the device filters at step
t + 1 the oracle's trackers filtered at the end of step t.  A set_filter on the device between
steps t and t + 1 is therefore a set_filter on the oracle's trackers before its step t, and the
elapsed handed to the device's step t is the one the oracle's trackers take on frame t."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_ref as R
import multi_filter_ref as M
import multi_tracker_ref as MR

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FILTERS = {0: None, 1: ("ema", 0.6), 2: ("alpha_beta", 0.5, 0.1), 3: ("one_euro", 1.0, 0.05)}
KINDS = {0: (468, 1404, 1, 192), 1: (21, 63, 1, 224)}  # landmarks, floats per image of outputs 0 / 1, input side


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


def _lm_filter(spec):
    from zaru_amd._lib import LmFilter
    if spec is None:
        return LmFilter.make(0)
    return LmFilter.make({"ema": 1, "alpha_beta": 2, "one_euro": 3}[spec[0]], *spec[1:],
                         *((1.0,) if spec[0] == "one_euro" and len(spec) == 3 else ()))


# ---- A: the kernel alone ------------------------------------------------------------------------
@pytest.mark.parametrize("fkind", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", [0, 1])
def test_indexed_kernel_follows_the_object(kind, fkind):
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, TrackCfg, TrackState
    lib = _lib.lib()
    L, ls, fs, side = KINDS[kind]
    S, K = 3, 4
    n = S * K
    spec = FILTERS[fkind]
    flt, cfg = _lm_filter(spec), TrackCfg(kind, L, side, side, 1, 1, 0.5, 0.3, K)
    sb = _lib.lm_filter_state_size(flt, L)
    tracks = M.object_tracks(M.GPU_SCRIPT, L, seed=100 + fkind + L)  # the seed the CPU test confirmed
    model = M.SlotFilters(S, K, lambda: M.numpy_filter(spec))
    rng = np.random.default_rng(kind * 10 + fkind)
    # nothing of either buffer is default at the start: every row of step 0 is new or idle
    d_in = DeviceBuffer.from_array(np.full(max(n * sb, 4), 0xFF, np.uint8))
    d_out = DeviceBuffer.from_array(np.full(max(n * sb, 4), 0xA5, np.uint8))
    d_pos = DeviceBuffer(n * L * 3 * 4)
    compared = primed_seen = 0
    for t in range(len(M.GPU_SCRIPT)):
        ids, src, active, live = M.tables(M.GPU_SCRIPT, t, K, M.GPU_NO_ESTIMATE, M.GPU_BAD_SRC)
        index = None
        if t in M.GPU_SHUFFLED:  # the estimates stored in a shuffled dense order
            rows = [i for i in range(n) if live[i]]
            index = np.full(n, -1, np.int32)
            index[rows] = rng.permutation(len(rows)).astype(np.int32)
            for (tt, i), v in M.GPU_NO_ESTIMATE.items():
                if tt == t:
                    index[i] = v
        else:
            assert all(tt != t for tt, _ in M.GPU_NO_ESTIMATE)
        lm = rng.uniform(-1e6, 1e6, (n, ls)).astype(F)
        fl = rng.uniform(-4.0, 4.0, (n, fs)).astype(F)
        for i in range(n):
            if live[i]:
                lm[i if index is None else index[i]] = tracks[(t, ids[i])].reshape(-1)
        st = (TrackState * n)()
        for i in range(n):
            st[i].active = int(active[i])
        # rows of the input buffer that no object brings its state from hold 0xFF: an idle slot's, a
        # slot whose occupant left, the slot a new object starts in
        if sb:
            used = {(i // K) * K + src[i] for i in range(n) if live[i] and 0 <= src[i] < K}
            before = d_in.download((n, sb), np.uint8)
            for r in range(n):
                if r not in used:
                    before[r] = 0xFF
            d_in.upload(before)
        d_st, d_lm, d_fl = (DeviceBuffer.from_array(np.frombuffer(bytes(st), np.uint8)), DeviceBuffer.from_array(lm),
                            DeviceBuffer.from_array(fl))
        d_src = DeviceBuffer.from_array(np.array(src, np.int32))
        d_idx = None if index is None else DeviceBuffer.from_array(index)
        _lib.check(lib.zr_lm_filter_indexed_async(C.byref(flt), C.byref(cfg), d_st.ptr, n, K, d_lm.ptr, ls, d_fl.ptr,
                                                  fs, None if d_idx is None else d_idx.ptr, d_src.ptr, M.ELAPSED[t],
                                                  d_in.ptr if sb else None, d_out.ptr if sb else None, d_pos.ptr,
                                                  None))
        _lib.synchronize()
        pos = d_pos.download((n, L, 3), F)
        want = model.step(src, live, [tracks[(t, o)] if o is not None else None for o in ids], M.ELAPSED[t])
        if sb:
            assert np.array_equal(d_in.download((n, sb), np.uint8), before), t  # only read
            after = d_out.download((n, sb), np.uint8)
        for i in range(n):
            if not live[i]:  # not active, or active without an estimate
                assert np.isnan(pos[i]).all(), (t, i)
                if sb:
                    assert not after[i].any(), (t, i)
                continue
            assert not np.isnan(pos[i]).any(), (t, i)
            assert np.array_equal(pos[i].view(np.uint32), want[i].view(np.uint32)), (kind, fkind, t, i, ids[i])
            compared += 1
            if model.primed[i]:
                primed_seen += 1
                if fkind:
                    assert not np.array_equal(pos[i], tracks[(t, ids[i])]), (t, i)  # not a pass-through value
            if sb:
                assert after[i].view(np.uint32)[:3 * L].tolist() == [1] * (3 * L), (t, i)
        d_in, d_out = d_out, d_in
    assert compared == 50 and primed_seen == 33, (compared, primed_seen)  # every live slot-step of the script


# ---- B: the update on indexed positions -----------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_positions_indexed_update_matches_indexed_update(kind):
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, TrackCfg, TrackState
    lib = _lib.lib()
    L, ls, fs, side = KINDS[kind]
    n, K = 8, 4
    cfg, none = TrackCfg(kind, L, side, side, 1, 1, 0.5, 0.3, K), _lm_filter(None)
    rng = np.random.default_rng(31 + kind)
    lm = rng.normal(side / 2, side / 5, (n, ls)).astype(F)
    fl = rng.uniform(1.0, 4.0, (n, fs)).astype(F)
    # where each RoI's estimate is stored: RoI 2 is inactive, RoI 5 active with none (lost)
    index = np.array([3, 0, -1, 5, 2, -1, 1, 4], np.int32)
    fl[index[6], 0] = -3.0 if kind == 0 else 0.1  # RoI 6 is below the loss threshold
    st = (TrackState * n)()
    for i in range(n):
        st[i].roi[:] = [200.0 + 30 * i, 180.0 + 10 * i, 120.0 + 5 * i, 130.0, 0.1 * i - 0.3]
        st[i].active = 0 if i == 2 else 1
        st[i].frame_w, st[i].frame_h = 640, 480
    seed = np.frombuffer(bytes(st), np.uint8)
    d_lm, d_fl, d_idx = DeviceBuffer.from_array(lm), DeviceBuffer.from_array(fl), DeviceBuffer.from_array(index)
    d_src = DeviceBuffer.from_array(np.full(n, -1, np.int32))
    got = []
    for positions in (False, True):
        d_st, d_views = DeviceBuffer.from_array(seed), DeviceBuffer.from_array(np.zeros(n * 40, np.uint8))
        d_out = DeviceBuffer.from_array(np.zeros(n * L * 3, F))
        _lib.check(lib.zr_track_seed_async(d_st.ptr, n, C.byref(cfg), d_views.ptr, None))
        if positions:
            d_pos = DeviceBuffer(n * L * 3 * 4)
            _lib.check(lib.zr_lm_filter_indexed_async(C.byref(none), C.byref(cfg), d_st.ptr, n, K, d_lm.ptr, ls,
                                                      d_fl.ptr, fs, d_idx.ptr, d_src.ptr, 0.03, None, None, d_pos.ptr,
                                                      None))
            _lib.check(lib.zr_track_update_positions_indexed_async(d_st.ptr, n, C.byref(cfg), d_pos.ptr, d_fl.ptr, fs,
                                                                   d_idx.ptr, d_out.ptr, d_views.ptr, None))
        else:
            _lib.check(lib.zr_track_update_indexed_async(d_st.ptr, n, C.byref(cfg), d_lm.ptr, ls, d_fl.ptr, fs,
                                                         d_idx.ptr, d_out.ptr, d_views.ptr, None))
        _lib.synchronize()
        got.append((d_st.download((n, C.sizeof(TrackState)), np.uint8), d_views.download((n, 40), np.uint8),
                    d_out.download((n, L, 3), np.uint32)))
    for a, b, what in zip(got[0], got[1], ("states", "views", "lm_out")):
        assert np.array_equal(a, b), (kind, what)
    states = np.frombuffer(got[1][0].tobytes(), np.dtype(TrackState))
    assert [i for i in range(n) if not states["tracked"][i]] == [2, 5, 6]
    assert not np.array_equal(got[1][0], seed.reshape(n, -1))  # the update did something


# ---- the loop: shared helpers -----------------------------------------------------------------------
FW, FH = 480, 360


def _noise(n, seed, h=FH, w=FW):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8) for _ in range(n)]


def _det(H, d):
    conf, (cx, cy, w, h), angle = d
    return H.Detection(conf, H.Rect.from_center(cx, cy, w, h), angle)


def _record(objs, count, pending):
    """One stream's step as comparable values: the floats as their bits."""
    return (int(count), bool(pending),
            [(int(o["id"]), np.asarray(o["rect"], F).tobytes(), F(o["angle"]).tobytes(),
              np.ascontiguousarray(o["landmarks"], F).tobytes(), F(o["confidence"]).tobytes()) for o in objs])


def _ref_objects(ref):
    return [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
             "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in ref.objects()]


def _dev_objects(dev, s):
    return [{"id": o["id"], "rect": o["view_rect"].rect().tuple(), "angle": o["view_rect"].rotation_radians(),
             "landmarks": o["landmarks"], "confidence": o["confidence"]} for o in dev.objects(s)]


class _Timed:
    """A host LandmarkTracker whose track(frame) passes the elapsed time of the step in progress
    (clock["elapsed"]; None: the filter's dt), as the multi-object oracle calls track(frame) only."""

    def __init__(self, tracker, clock):
        self.t, self.clock = tracker, clock

    def __getattr__(self, name):
        return getattr(self.t, name)

    def track(self, frame):
        e = self.clock["elapsed"]
        return self.t.track(frame) if e is None else self.t.track(frame, e)


class _Factory:
    """make_tracker of the oracle: every object owns a fresh copy of the current filter.
    set_filter reaches the trackers of the live objects too, and resets them."""

    def __init__(self, H, spec, dt=None):
        self.H, self.spec, self.dt, self.clock = H, spec, dt, {"elapsed": None}

    def _apply(self, tr):
        f = None if self.spec is None else R.host_filter(self.H, self.spec)
        if self.dt is None:
            tr.set_filter(f)
        else:
            tr.set_filter(f, self.dt)

    def __call__(self):
        tr = self.H.LandmarkTracker("facemesh")
        if self.spec is not None:
            self._apply(tr)
        return _Timed(tr, self.clock)

    def set_filter(self, refs, spec, dt=None):
        self.spec, self.dt = spec, dt
        for ref in refs:
            for o in ref.objs:
                self._apply(o.tracker.t)


def _set_device_filter(H, dev, spec, dt=None):
    f = None if spec is None else R.host_filter(H, spec)
    if dt is None:
        dev.set_filter(f)
    else:
        dev.set_filter(f, dt)


# ---- C: scripted parity with the oracle -----------------------------------------------------------
S, K, STEPS = 3, 4, 7
# per step, per stream: (confidence, (cx, cy, w, h), angle) handed to both sides
FACE_SCRIPT = {
    0: {0: [(0.9, (200.0, 180.0, 80.0, 88.0), 0.3)],
        1: [(0.9, (100.0, 100.0, 60.0, 60.0), 0.0), (0.8, (104.0, 101.0, 60.0, 60.0), 0.1)],  # a pair: the sweep
        2: [(0.9, (300.0, 200.0, 100.0, 80.0), -0.2), (0.7, (120.0, 260.0, 72.0, 72.0), 0.5)]},
    2: {1: [(0.6, (330.0, 250.0, 88.0, 88.0), 1.0)]},        # a late newcomer
    4: {2: [(0.9, (300.0, 60.0, 60.0, 60.0), 0.0)]},
}
# (step, stream): a detection placed exactly on the RoI that stream's first object holds when the
# step's IoU filter runs (known to the oracle one step ahead), followed by a newcomer
ON_TOP = {(2, 0): (0.9, (420.0, 60.0, 50.0, 50.0), 0.0), (4, 2): None}
CASES = {"ema": (("ema", 0.6), [None] * STEPS),
         "one_euro": (("one_euro", 1.0, 0.05), [0.033, 0.05, 0.016, 0.033, 0.1, 0.02, 0.04])}


@pytest.fixture(scope="module")
def face_frames():
    return [_noise(STEPS, 10 + s) for s in range(S)]


def _run_face_oracle(H, frames, spec, elapsed):
    factory = _Factory(H, spec)
    refs = []
    for s in range(S):
        r = MR.MultiTrackerRef(H, "face", "facemesh", K, make_tracker=factory)
        r.loss = -1.0
        r.interval = 40.0
        refs.append(r)
    records, injected, object_steps = [], [], 0
    for k in range(STEPS):
        row, inj = [], {}
        factory.clock["elapsed"] = elapsed[k]
        for s in range(S):
            dets = list(FACE_SCRIPT.get(k, {}).get(s, []))
            if (k, s) in ON_TOP:
                first = refs[s].objs[0]
                assert first.pending is not None  # loss threshold -1: never lost
                dets.insert(0, (0.9, tuple(first.pending["updated_roi"].rect().tuple()), 0.0))
                if ON_TOP[(k, s)] is not None:
                    dets.append(ON_TOP[(k, s)])
            inj[s] = dets
            refs[s].step(frames[s][k], 15.0 * k, [_det(H, d) for d in dets])
            row.append(_record(_ref_objects(refs[s]), len(refs[s].objs), refs[s].pending))
            object_steps += len(refs[s].objects())
        records.append(row)
        injected.append(inj)
    return {"records": records, "injected": injected, "object_steps": object_steps,
            "filtered": sum(r.filtered for r in refs), "swept": sum(r.swept for r in refs)}


def _run_face_device(H, frames, injected, spec, elapsed, compact=True):
    from zaru_amd._lib import DeviceBuffer
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    dev.set_compact(compact)
    if spec is not None:
        _set_device_filter(H, dev, spec)
    bufs = [DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)])) for k in range(STEPS)]
    fb = FH * FW * 4
    records = []
    for k in range(STEPS):
        for s in range(S):
            if injected[k][s]:
                dev.inject_detections(s, [_det(H, d) for d in injected[k][s]])
        fr = [(bufs[k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)]
        if elapsed[k] is None:
            dev.step(fr, 15.0 * k)
        else:
            dev.step(fr, 15.0 * k, elapsed[k])
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        records.append([_record(_dev_objects(dev, s), counts[s], pend[s]) for s in range(S)])
    return records


@pytest.mark.parametrize("case", ["ema", "one_euro"])
def test_scripted_parity_with_filtered_oracle(H, face_frames, case):
    """Counts, pending flags, ids, RoIs, landmarks and confidence equal the oracle's, bit for bit, at
    every step and stream; compaction off changes no bit; an unfiltered run differs."""
    spec, elapsed = CASES[case]
    oracle = _run_face_oracle(H, face_frames, spec, elapsed)
    got = _run_face_device(H, face_frames, oracle["injected"], spec, elapsed)
    compared = 0
    for k in range(STEPS):
        for s in range(S):
            want, have = oracle["records"][k][s], got[k][s]
            assert have[0] == want[0], ("count", k, s, have[0], want[0])
            assert have[1] == want[1], ("pending", k, s)
            assert [o[0] for o in have[2]] == [o[0] for o in want[2]], ("ids", k, s)
            for g, w in zip(have[2], want[2]):
                assert g[1] == w[1], ("rect", k, s, g[0])
                assert g[2] == w[2], ("angle", k, s, g[0])
                assert g[3] == w[3], ("landmarks", k, s, g[0])
                assert g[4] == w[4], ("confidence", k, s, g[0])
                compared += 1
    print("object-steps compared:", compared, "filtered:", oracle["filtered"], "swept:", oracle["swept"])
    assert compared == oracle["object_steps"] and compared >= 10, (compared, oracle["object_steps"])
    assert oracle["filtered"] >= 1 and oracle["swept"] >= 1, oracle
    assert _run_face_device(H, face_frames, oracle["injected"], spec, elapsed, compact=False) == got
    plain = _run_face_device(H, face_frames, oracle["injected"], None, [None] * STEPS)
    assert any(g[3] != p[3] for k in range(STEPS) for s in range(S)
               for g, p in zip(got[k][s][2], plain[k][s][2]) if g[0] == p[0])  # the filter really is applied


# ---- D: the state follows a real object -----------------------------------------------------------
RW, RH, RT, BLANK_FROM, BACK_FROM = 960, 480, 11, 4, 8
LEFT, RIGHT, TOP = 40, 536, 48  # the two patches of test_gpu_multi_tracker.py's two-face frame


def _patch():
    codes = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))["codes"][0]
    p = np.full((192, 192, 4), 255, np.uint8)
    p[..., :3] = codes.transpose(1, 2, 0)
    return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)  # 384 x 384


def _shift(t):
    return 3 * t, 2 * t if t < 6 else 24 - 2 * t  # (dx, dy): right all along, down then up


def _moving_faces(blank=None):
    """Both patches shifted a few pixels per frame; `blank` ("left" / "right") shows the background in
    that patch's place on frames BLANK_FROM .. BACK_FROM - 1."""
    rng = np.random.default_rng(3)
    patch = _patch()
    bg = rng.integers(0, 256, size=(RH, RW, 4), dtype=np.uint8)
    frames = np.empty((RT, RH, RW, 4), np.uint8)
    for t in range(RT):
        dx, dy = _shift(t)
        frames[t] = bg
        for name, x0 in (("left", LEFT), ("right", RIGHT)):
            if name == blank and BLANK_FROM <= t < BACK_FROM:
                continue
            frames[t, TOP + dy:TOP + dy + 384, x0 + dx:x0 + dx + 384] = patch
    return frames


def test_state_follows_a_real_object(H):
    from zaru_amd._lib import DeviceBuffer
    spec = ("one_euro", 1.0, 0.05)
    found = H.Detector("face").detect(_moving_faces()[0])
    print("faces on frame 0:", [(d.confidence(), d.bounding_rect().tuple()) for d in found])
    assert len(found) == 2, ("precondition: two detections on frame 0", len(found))
    cx = found[0].bounding_rect().center[0]
    first = "left" if abs(cx - (LEFT + 192)) < abs(cx - (RIGHT + 192)) else "right"
    frames = _moving_faces(blank=first)  # the first detection is id 0 in slot 0: it leaves
    factory = _Factory(H, spec)
    ref = MR.MultiTrackerRef(H, "face", "facemesh", 4, make_tracker=factory)
    ref.interval = 33.0
    dev, plain = H.DeviceMultiTracker("face", "facemesh", 1, 4), H.DeviceMultiTracker("face", "facemesh", 1, 4)
    _set_device_filter(H, dev, spec)
    for d in (dev, plain):
        d.set_redetect_interval(33.0)
    buf = DeviceBuffer.from_array(frames)
    fb = RH * RW * 4
    ids_seen, compared, oracle_results, differs_after_move = [], 0, 0, 0
    moved_at = None
    for t in range(RT):
        now = 33.0 * t
        fr = [(buf.ptr + t * fb, RW, RH, RW * 4)]
        dev.step(fr, now)
        plain.step(fr, now)
        dev.synchronize()
        plain.synchronize()
        ref.step(frames[t], now)
        want = _record(_ref_objects(ref), len(ref.objs), ref.pending)
        oracle_results += len(want[2])
        got = _record(_dev_objects(dev, 0), dev.object_counts()[0], dev.detection_pending()[0])
        assert got[:2] == want[:2], (t, got[:2], want[:2])
        assert [o[0] for o in got[2]] == [o[0] for o in want[2]], (t, "ids")
        for g, w in zip(got[2], want[2]):
            assert g == w, (t, g[0], [a == b for a, b in zip(g, w)])
            compared += 1
        objs = dev.objects(0)
        ids_seen.append([o["id"] for o in objs])
        if moved_at is None and ids_seen[-1][:1] == [1]:
            moved_at = t
        if moved_at is not None:  # the survivor, in slot 0 now, against the unfiltered loop's
            mine = [o for o in objs if o["id"] == 1]
            theirs = [o for o in plain.objects(0) if o["id"] == 1]
            if mine and theirs:
                differs_after_move += int(not np.array_equal(mine[0]["landmarks"], theirs[0]["landmarks"]))
    print("ids:", ids_seen, "moved at:", moved_at, "compared:", compared)
    # preconditions: properties of the loop as it was before filters, reported when they fail
    assert ids_seen[2] == [0, 1], ("precondition: both faces tracked from step 2", ids_seen)
    assert any(0 not in ids for ids in ids_seen[BLANK_FROM:BLANK_FROM + 3]), \
        ("precondition: id 0 is lost within two steps of the blanking", ids_seen)
    assert moved_at is not None and moved_at <= BLANK_FROM + 2 and all(ids[:1] == [1] for ids in ids_seen[moved_at:]), \
        ("precondition: the survivor has id 1 and is the first entry afterwards: it moved to slot 0", ids_seen)
    new = [i for ids in ids_seen[BACK_FROM:] for i in ids if i >= 2]
    assert new and ids_seen[-1][0] == 1 and ids_seen[-1][1] == new[-1], \
        ("precondition: a new id appears after the face is back, in the slot the survivor vacated", ids_seen)
    assert compared == oracle_results and compared >= 12, (compared, oracle_results)
    assert differs_after_move >= 3, differs_after_move


# ---- E: set_filter during a run, the pose, refusals -------------------------------------------------
E_SCRIPT = {0: [(0.9, (120.0, 120.0, 90.0, 90.0), 0.0), (0.9, (340.0, 200.0, 120.0, 110.0), 0.0)]}


def _one_stream_run(H, frames, steps, schedule, device_only=False, pose=None):
    """1 stream x 2 slots on noise frames.  schedule: {t: (spec, dt)} -- the device's set_filter
    after its step t, the oracle's before its step t (the module docstring says why).  Returns the
    device's and the oracle's records per step (and the device's objects)."""
    from zaru_amd._lib import DeviceBuffer
    factory = _Factory(H, None)
    ref = MR.MultiTrackerRef(H, "face", "facemesh", 2, make_tracker=factory)
    ref.loss = -1.0
    ref.interval = 1e9
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(1e9)
    if pose is not None:
        dev.set_pose_reference(pose)
    if -1 in schedule:  # before the first step, on both sides
        factory.set_filter([ref], *schedule[-1])
        _set_device_filter(H, dev, *schedule[-1])
    out = []
    for t in range(steps):
        dets = [_det(H, d) for d in E_SCRIPT.get(t, [])]
        if dets:
            dev.inject_detections(0, dets)
        b = DeviceBuffer.from_array(frames[t])
        dev.step([(b.ptr, FW, FH, FW * 4)], 10.0 * t)
        dev.synchronize()
        got = _record(_dev_objects(dev, 0), dev.object_counts()[0], dev.detection_pending()[0])
        want = None
        if not device_only:
            if t in schedule:
                factory.set_filter([ref], *schedule[t])
            ref.step(frames[t], 10.0 * t, dets)
            want = _record(_ref_objects(ref), len(ref.objs), ref.pending)
        out.append((got, want, dev.objects(0)))
        if t in schedule:
            _set_device_filter(H, dev, *schedule[t])
    return out


def test_set_filter_resets_every_object_and_none_restores_the_unfiltered_path(H):
    frames = _noise(8, 77)
    ema = ("ema", 0.6)
    # a filter from the start, the same filter again after step 3 (a reset), none after step 5
    run = _one_stream_run(H, frames, 8, {-1: (ema, None), 3: (ema, None), 5: (None, None)})
    results = 0
    for t, (got, want, _) in enumerate(run):
        assert got == want, (t, [a == b for a, b in zip(got, want)])
        results += len(got[2])
    assert results == 14  # two objects with a result from step 1 on
    # without the reset the old state still weighs in: the first estimate filtered after it differs
    keep = _one_stream_run(H, frames, 5, {-1: (ema, None)}, device_only=True)
    assert keep[3][0] == run[3][0] and keep[4][0] != run[4][0]
    # set_filter(None) leaves nothing behind: a filter set and taken away before anything was
    # filtered is a tracker that never had one, bit for bit
    never = _one_stream_run(H, frames, 4, {}, device_only=True)
    undone = _one_stream_run(H, frames, 4, {-1: (("one_euro", 1.0, 0.05), None), 0: (None, None)}, device_only=True)
    assert [r[0] for r in never] == [r[0] for r in undone]
    assert never[3][0] != run[3][0]  # and the filtered run is not that


def test_pose_is_of_the_filtered_landmarks(H):
    import procrustes_ref as P
    mesh = P.canonical_mesh()
    analyzer = H.ProcrustesAnalyzer(mesh)
    frames = _noise(4, 78)
    spec = ("one_euro", 1.0, 0.05)
    run = _one_stream_run(H, frames, 4, {-1: (spec, None)}, pose=mesh)
    plain = _one_stream_run(H, frames, 4, {}, device_only=True)
    posed = 0
    for t, (got, want, objs) in enumerate(run):
        assert got == want, t
        for o in objs:
            w = analyzer.analyze(o["landmarks"][:len(mesh)], flip_y=True).pose().view(np.uint32)
            assert np.array_equal(o["pose"].view(np.uint32), w), (t, o["id"])
            posed += 1
    assert posed == 6  # two objects, steps 1 to 3
    assert run[3][0][2][0][3] != plain[3][0][2][0][3]  # step 3's landmarks are filtered ones


def test_bad_elapsed_is_refused_before_anything_is_enqueued(H):
    from zaru_amd._lib import DeviceBuffer
    frames = _noise(3, 79)
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    dev.set_loss_threshold(-1.0)
    dev.set_filter(H.OneEuro(1.0, 0.05))
    bufs = [DeviceBuffer.from_array(f) for f in frames]
    dev.inject_detections(0, [_det(H, d) for d in E_SCRIPT[0]])
    dev.step([(bufs[0].ptr, FW, FH, FW * 4)], 0.0, 0.02)
    dev.step([(bufs[1].ptr, FW, FH, FW * 4)], 10.0)
    dev.synchronize()

    def snapshot():
        return (dev.object_counts(), dev.detection_pending(), dev.landmark_images(), dev.detector_frames())

    before = snapshot()
    for bad in (0.0, -0.033, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            dev.step([(bufs[2].ptr, FW, FH, FW * 4)], 1e12, bad)  # whatever now_ms says
    with pytest.raises(RuntimeError):
        dev.set_filter(H.OneEuro(1.0, 0.05), -1.0)
    assert snapshot() == before
    dev.step([(bufs[2].ptr, FW, FH, FW * 4)], 20.0, 0.05)
    dev.synchronize()
    assert [o["id"] for o in dev.objects(0)] == [0, 1]
