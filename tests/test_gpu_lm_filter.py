"""Landmark temporal filters on the device (kernels/lm_filter.hip, zr_lm_filter_async,
zr_track_update_positions_async) and in the device loops (DeviceTracker / DeviceFaceLoop
set_filter), bit for bit against the host restatement (zaru_amd.host LandmarkFilter /
LandmarkTracker.set_filter; crates/zaru/src/filter, landmark.rs:142-202,293-302,330-333):

A. the kernel on synthetic network outputs, every track kind x every filter kind, with inactive
   streams (state bytes untouched, NaN rows) and a stream that pauses and resumes;
B. zr_track_update_positions_async fed by filter kind 0 against zr_track_update_async;
C. DeviceFaceLoop with a 1 euro filter against the host loop, frame by frame, through loss and
   re-seeding, and against an unfiltered loop (the filter really is applied);
D. DeviceTracker against per-stream host LandmarkTrackers (EMA; alpha-beta with varying elapsed);
E. set_filter resets the state, set_filter(None) returns to the unfiltered path."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = 640, 480
FILTERS = {0: None, 1: ("ema", 0.6), 2: ("alpha_beta", 0.5, 0.1), 3: ("one_euro", 1.0, 0.05)}
# track kind: landmarks, floats per image of output 0 / output 1, network input side
KINDS = {0: (468, 1404, 1, 192), 1: (21, 63, 1, 224), 2: (76, 213, 15, 64), 3: (68, 143, 0, 112)}
ELAPSED = (0.033, 0.05, 0.016, 0.033, 0.1, 0.02)


def _lm_filter(spec):
    from zaru_amd._lib import LmFilter
    if spec is None:
        return LmFilter.make(0)
    return LmFilter.make({"ema": 1, "alpha_beta": 2, "one_euro": 3}[spec[0]], *spec[1:],
                         *((1.0,) if spec[0] == "one_euro" and len(spec) == 3 else ()))


def _cfg(kind, loss=0.5):
    from zaru_amd._lib import TrackCfg
    L, _, _, side = KINDS[kind]
    return TrackCfg(kind, L, side, side, 1, 1, loss, 0.3, 0)


def _outputs(rng, kind, n, prev=None):
    """Seeded network outputs of landmark-like magnitude; a step moves them a little."""
    L, ls, fs, side = KINDS[kind]
    if prev is None:
        lm = rng.normal(0.5, 0.2, (n, ls)) if kind == 3 else rng.normal(side / 2, side / 5, (n, ls))
        fl = rng.normal(side / 2, side / 5, (n, max(fs, 1)))
    else:
        lm = prev[0] + rng.normal(0.0, 0.01 if kind == 3 else 2.0, prev[0].shape)
        fl = prev[1] + rng.normal(0.0, 2.0, prev[1].shape)
    return lm.astype(F), fl.astype(F)


@pytest.mark.parametrize("fkind", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_kernel_matches_host_filter(kind, fkind):
    import zaru_amd.host as Hm
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, TrackState
    L, ls, fs, side = KINDS[kind]
    n, T = 5, 6
    lib = _lib.lib()
    flt, cfg = _lm_filter(FILTERS[fkind]), _cfg(kind)
    sb = _lib.lm_filter_state_size(flt, L)
    assert (sb == 0) == (fkind == 0)
    d_fs = DeviceBuffer.from_array(np.zeros(max(n * sb, 4), np.uint8))  # all-zero: the default state
    d_pos = DeviceBuffer(n * L * 3 * 4)
    host = [Hm.LandmarkFilter(R.host_filter(Hm, FILTERS[fkind]), L) if fkind else None for _ in range(n)]
    rng = np.random.default_rng(100 + 10 * kind + fkind)
    outs, after_step1, moved = None, None, 0
    for t in range(T):
        outs = _outputs(rng, kind, n, outs)
        active = [i != 1 and not (i == 3 and t in (2, 3)) for i in range(n)]
        st = (TrackState * n)()
        for i in range(n):
            st[i].active = int(active[i])
        d_st = DeviceBuffer.from_array(np.frombuffer(bytes(st), np.uint8))
        d_lm, d_fl = DeviceBuffer.from_array(outs[0]), DeviceBuffer.from_array(outs[1])
        before = d_fs.download((n, sb), np.uint8) if sb else None
        _lib.check(lib.zr_lm_filter_async(C.byref(flt), C.byref(cfg), d_st.ptr, n, d_lm.ptr, ls,
                                          d_fl.ptr if fs else None, fs, ELAPSED[t], d_fs.ptr if sb else None,
                                          d_pos.ptr, None))
        _lib.synchronize()
        pos = d_pos.download((n, L, 3), F)
        after = d_fs.download((n, sb), np.uint8) if sb else None
        for i in range(n):
            if not active[i]:
                assert np.isnan(pos[i]).all(), (t, i)
                if sb:
                    assert np.array_equal(before[i], after[i]), (t, i)
                continue
            want = R.extract(kind, L, outs[0][i], outs[1][i], side, side)
            raw = want
            if fkind:
                want = host[i].filter(want, ELAPSED[t])
                moved += int(t > 0 and not np.array_equal(want, raw))
            assert np.array_equal(pos[i].view(np.uint32), want.view(np.uint32)), (kind, fkind, t, i)
        if sb and t == 1:
            after_step1 = after[3].copy()
        if sb and t == 3:  # stream 3 paused at steps 2-3: it resumes from its step-1 state
            assert np.array_equal(after[3], after_step1)
            assert not np.array_equal(after[0], before[0])  # while an active stream's state moves
    if fkind:
        assert moved >= 3 * (T - 1)  # the comparison was not of pass-through values
    # d_state == NULL: every stream counts as active
    _lib.check(lib.zr_lm_filter_async(C.byref(flt), C.byref(cfg), None, n, d_lm.ptr, ls, d_fl.ptr if fs else None,
                                      fs, 0.03, d_fs.ptr if sb else None, d_pos.ptr, None))
    _lib.synchronize()
    assert not np.isnan(d_pos.download((n, L, 3), F)).any()


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_positions_update_matches_update(kind):
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer, TrackState
    L, ls, fs, side = KINDS[kind]
    n = 4
    lib = _lib.lib()
    cfg, none = _cfg(kind), _lm_filter(None)
    rng = np.random.default_rng(7 + kind)
    lm, fl = _outputs(rng, kind, n)
    if kind == 0:
        fl[:, 0] = [3.0, -2.0, 1.5, 0.7]   # face_flag logits: stream 1 is below the loss threshold
    elif kind == 1:
        fl[:, 0] = [0.9, 0.8, 0.1, 0.95]   # presence: stream 2 is below it
    st = (TrackState * n)()
    for i in range(n):
        st[i].roi[:] = [300.0 + 10 * i, 240.0 - 5 * i, 200.0 + 7 * i, 180.0 + 3 * i, 0.1 * i - 0.15]
        st[i].active, st[i].frame_w, st[i].frame_h = 1, W, H
    seed = np.frombuffer(bytes(st), np.uint8)
    d_lm, d_fl = DeviceBuffer.from_array(lm), DeviceBuffer.from_array(fl)
    flag = d_fl.ptr if fs else None
    got = []
    for positions in (False, True):
        d_st, d_views = DeviceBuffer.from_array(seed), DeviceBuffer.from_array(np.zeros(n * 40, np.uint8))
        d_out = DeviceBuffer.from_array(np.zeros(n * L * 3, F))
        _lib.check(lib.zr_track_seed_async(d_st.ptr, n, C.byref(cfg), d_views.ptr, None))
        if positions:
            d_pos = DeviceBuffer(n * L * 3 * 4)
            _lib.check(lib.zr_lm_filter_async(C.byref(none), C.byref(cfg), d_st.ptr, n, d_lm.ptr, ls, flag, fs,
                                              0.03, None, d_pos.ptr, None))
            _lib.check(lib.zr_track_update_positions_async(d_st.ptr, n, C.byref(cfg), d_pos.ptr,
                                                           flag if kind <= 1 else None, fs if kind <= 1 else 0,
                                                           d_out.ptr, d_views.ptr, None))
        else:
            _lib.check(lib.zr_track_update_async(d_st.ptr, n, C.byref(cfg), d_lm.ptr, ls, flag, fs, d_out.ptr,
                                                 d_views.ptr, None))
        _lib.synchronize()
        got.append((d_st.download((n, C.sizeof(TrackState)), np.uint8), d_views.download((n, 40), np.uint8),
                    d_out.download((n, L, 3), np.uint32)))
    for a, b, what in zip(got[0], got[1], ("states", "views", "lm_out")):
        assert np.array_equal(a, b), (kind, what)
    states = np.frombuffer(got[0][0].tobytes(), np.dtype(TrackState))
    lost = {0: [1], 1: [2]}.get(kind, [])
    assert [i for i in range(n) if not states["tracked"][i]] == lost
    assert all(np.isnan(got[0][2][i].view(F)).all() for i in lost)
    assert not np.array_equal(got[0][0], seed.reshape(n, -1))  # the update did something


# ---- C: the face loop -------------------------------------------------------------------------
S_FACE, T_FACE = 6, 10


def _patch():
    codes = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))["codes"][0]
    p = np.full((192, 192, 4), 255, np.uint8)
    p[..., :3] = codes.transpose(1, 2, 0)
    return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)  # 384 x 384


def _face_video(seed=5):
    """The six synthetic streams of test_gpu_face_loop.py: tracked throughout, disappears and
    returns, noise only, jumps, appears late, seeded with set_roi."""
    rng = np.random.default_rng(seed)
    patch = _patch()
    S, T = S_FACE, T_FACE
    frames = np.empty((T, S, H, W, 4), np.uint8)
    where = {}
    for s in range(S):
        bg = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        y0, x0 = int(rng.integers(0, 60)), int(rng.integers(0, 200))
        for t in range(T):
            frames[t, s] = bg
            y, x = y0 + 2 * t, x0 + 3 * t
            if s == 1 and t in (3, 4):
                continue
            if s == 2:
                continue
            if s == 3 and t >= 5:
                y, x = min(H - 384, y + 80), max(0, x - 180)
            if s == 4 and t < 2:
                continue
            frames[t, s, y:y + 384, x:x + 384] = patch
            where[(t, s)] = (y, x)
    return frames, where


def _best(dets):
    best = None
    for d in dets:
        if best is None or d.confidence() >= best.confidence():
            best = d
    return best


def _same_rrect(a, b):
    return a.rect() == b.rect() and a.rotation_radians() == b.rotation_radians()


def test_filtered_face_loop_matches_host_loop():
    import zaru_amd.host as Hm
    from zaru_amd._lib import DeviceBuffer
    S, T = S_FACE, T_FACE
    frames, where = _face_video()
    buf = DeviceBuffer.from_array(frames)
    fb = H * W * 4
    spec = ("one_euro", 1.0, 0.05)
    loop = Hm.DeviceFaceLoop("face", "facemesh_v2", S, 0)
    plain = Hm.DeviceFaceLoop("face", "facemesh_v2", S, 0)
    loop.set_filter(R.host_filter(Hm, spec), 1.0 / 30.0)
    trackers = [Hm.LandmarkTracker("facemesh_v2", 0) for _ in range(S)]
    for tr in trackers:
        tr.set_filter(R.host_filter(Hm, spec), 1.0 / 30.0)
    detector = Hm.Detector("face", 0)
    seed = Hm.RotatedRect(Hm.Rect.from_center(where[(0, 5)][1] + 192.0, where[(0, 5)][0] + 200.0, 330.0, 330.0), 0.05)
    trackers[5].set_roi(seed)
    loop.set_roi(5, seed)
    plain.set_roi(5, seed)
    stats = {"tracked": 0, "detect_runs": 0, "reseeds": 0, "lost": 0, "differs": 0}
    first = {}
    for t in range(T):
        fr = [(buf.ptr + (t * S + s) * fb, W, H, W * 4) for s in range(S)]
        loop.step(fr)
        plain.step(fr)
        loop.synchronize()
        plain.synchronize()
        st, lms = loop.states(), loop.landmarks()
        pst, plm = plain.states(), plain.landmarks()
        ran, counts = loop.detected(), loop.detection_counts()
        for s in range(S):
            had_roi = trackers[s].roi() is not None
            r = trackers[s].track(frames[t, s])
            assert st[s]["tracked"] == (r is not None), (t, s)
            if r is not None:
                stats["tracked"] += 1
                first.setdefault(s, t)
                assert np.array_equal(lms[s].view(np.uint32), r["landmarks"].view(np.uint32)), (t, s)
                assert _same_rrect(st[s]["updated_roi"], r["updated_roi"]), (t, s)
                assert not ran[s] and counts[s] == -1
                if pst[s]["tracked"] and t > first[s]:
                    stats["differs"] += int(not np.array_equal(lms[s], plm[s]))
            else:
                stats["lost"] += int(had_roi)
                assert np.isnan(lms[s]).all(), (t, s)
                dets = detector.detect(frames[t, s])
                stats["detect_runs"] += 1
                assert ran[s] == 1 and counts[s] == len(dets), (t, s, ran[s], counts[s], len(dets))
                best = _best(dets)
                if best is not None:
                    trackers[s].set_roi_rect(best.bounding_rect())
                    stats["reseeds"] += 1
            want = trackers[s].roi()
            assert st[s]["active"] == (want is not None), (t, s)
            if want is not None:
                assert _same_rrect(st[s]["roi"], want), (t, s, st[s]["roi"], want)
    print(stats)
    assert loop.detections_run() == stats["detect_runs"]
    assert loop.reacquisitions() == stats["reseeds"]
    assert stats["tracked"] >= S * T // 3, stats
    # loss and re-seeding happened with the filter state kept across both
    assert stats["lost"] >= 2 and stats["reseeds"] >= 4, stats
    # the filter was applied: filtered landmarks differ from the unfiltered loop's
    assert stats["differs"] >= 1, stats


# ---- D / E: DeviceTracker ---------------------------------------------------------------------
def _track_video(S, T, seed):
    """Per stream a noise background with the face patch drifting; the last stream is noise only."""
    rng = np.random.default_rng(seed)
    patch = _patch()
    frames = np.empty((T, S, H, W, 4), np.uint8)
    rois = []
    for s in range(S):
        bg = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        y0, x0 = int(rng.integers(0, H - 384 - 2 * T)), int(rng.integers(0, W - 384 - 4 * T))
        for t in range(T):
            frames[t, s] = bg
            if s < S - 1:
                frames[t, s, y0 + 2 * t:y0 + 2 * t + 384, x0 + 4 * t:x0 + 4 * t + 384] = patch
        side = float(rng.uniform(300, 380))
        rois.append((x0 + 192.0 + float(rng.uniform(-10, 10)), y0 + 192.0 + float(rng.uniform(-10, 10)),
                     side, side, float(rng.uniform(-0.15, 0.15))))
    return frames, rois


_VIDEO = {}


def _shared_video():
    """Built and uploaded once for D and E (read only)."""
    if not _VIDEO:
        from zaru_amd._lib import DeviceBuffer
        frames, rois = _track_video(4, 4, 43)
        _VIDEO["v"] = (frames, rois, DeviceBuffer.from_array(frames))
    return _VIDEO["v"]


def _frames_at(buf, t, S):
    fb = H * W * 4
    return [(buf.ptr + (t * S + s) * fb, W, H, W * 4) for s in range(S)]


@pytest.mark.parametrize("spec", [("ema", 0.6), ("alpha_beta", 0.5, 0.1)], ids=["ema", "alpha_beta"])
@pytest.mark.parametrize("network", ["facemesh", "eye", "face68_pfld"])
def test_filtered_device_tracker_matches_host_trackers(network, spec):
    import zaru_amd.host as Hm
    S, T = 4, 4
    frames, rois, buf = _shared_video()
    elapsed = [None] * T if spec[0] == "ema" else [0.033, 0.05, 0.016, 0.1]
    dev = Hm.DeviceTracker(network, 0)
    dev.set_filter(R.host_filter(Hm, spec))
    dev.set_rois(rois, [(W, H)] * S)
    host = [Hm.LandmarkTracker(network, 0) for _ in range(S)]
    for s in range(S):
        host[s].set_filter(R.host_filter(Hm, spec))
        host[s].set_roi(Hm.RotatedRect(Hm.Rect.from_center(*rois[s][:4]), rois[s][4]))
    tracked = 0
    for t in range(T):
        if elapsed[t] is None:
            dev.step(_frames_at(buf, t, S))
        else:
            dev.step(_frames_at(buf, t, S), elapsed[t])
        dev.synchronize()
        st, lms = dev.states(), dev.landmarks()
        for s in range(S):
            r = host[s].track(frames[t, s]) if elapsed[t] is None else host[s].track(frames[t, s], elapsed[t])
            assert st[s]["tracked"] == (r is not None), (network, t, s)
            want = host[s].roi()
            assert st[s]["active"] == (want is not None), (network, t, s)
            if r is None:
                assert np.isnan(lms[s]).all(), (network, t, s)
                continue
            tracked += 1
            assert np.array_equal(lms[s].view(np.uint32), r["landmarks"].view(np.uint32)), (network, spec, t, s)
            assert _same_rrect(st[s]["updated_roi"], r["updated_roi"]), (network, t, s)
            assert _same_rrect(st[s]["roi"], want), (network, t, s)
    assert tracked >= (S - 1) * T // 2


def _rois_of(states):
    return [(*st["roi"].rect().tuple(), st["roi"].rotation_radians()) for st in states]


def test_set_filter_resets_and_none_restores_unfiltered_path():
    import zaru_amd.host as Hm
    frames, rois, buf = _shared_video()
    S = 3  # the face streams: they stay tracked
    sizes = [(W, H)] * S

    def fr(t):
        return _frames_at(buf, t, 4)[:S]

    def result(tr):
        tr.synchronize()
        st = tr.states()
        assert all(x["tracked"] for x in st)
        return tr.landmarks().view(np.uint32), _rois_of(st), tr.views().view(np.uint32)

    ema = lambda: Hm.Ema(0.6)  # noqa: E731
    a, keep = Hm.DeviceTracker("facemesh", 0), Hm.DeviceTracker("facemesh", 0)
    for tr in (a, keep):
        tr.set_filter(ema())
        tr.set_rois(rois[:S], sizes)
        for t in (0, 1):
            tr.step(fr(t))
    _, rois1, _ = result(a)
    a.set_filter(ema())  # the same filter again: a reset
    a.step(fr(2))
    keep.step(fr(2))
    fresh = Hm.DeviceTracker("facemesh", 0)
    fresh.set_filter(ema())
    fresh.set_rois(rois1, sizes)
    fresh.step(fr(2))
    lm_a, rois2, views_a = result(a)
    lm_f, rois_f, views_f = result(fresh)
    assert np.array_equal(lm_a, lm_f) and rois2 == rois_f and np.array_equal(views_a, views_f)
    assert not np.array_equal(lm_a, result(keep)[0])  # without the reset the old state still weighs in
    # set_filter(None): byte-identical to a tracker that never had a filter, given the same ROIs
    a.set_filter(None)
    a.step(fr(3))
    never = Hm.DeviceTracker("facemesh", 0)
    never.set_rois(rois2, sizes)
    never.step(fr(3))
    lm_a, rois_a, views_a = result(a)
    lm_n, rois_n, views_n = result(never)
    assert np.array_equal(lm_a, lm_n) and rois_a == rois_n and np.array_equal(views_a, views_n)
