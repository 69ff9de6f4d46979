"""Procrustes analysis on the device (kernels/procrustes.hip, zr_procrustes_analyze_async) and as
the head-pose output of the device loops (DeviceTracker / DeviceFaceLoop set_pose_reference,
poses), against the host mirror (zaru_amd.host ProcrustesAnalyzer: the same header on the CPU)
byte for byte, and against a numpy f64 Kabsch:

A. the kernel against the host, every byte of every record: reference sizes around the wavefront
   width, several set counts, a stride larger than the reference, flip_y, a validity mask;
B. the kernel against f64 on 67 seeded transforms of the canonical face mesh (the reference's
   MAX_DELTA on the rotation angle);
C. the collapsed set and the NaN set return the host's bits; what the C ABI refuses;
D. DeviceTracker (FaceMesh V1): poses equal the host analyzer on the loop's own landmarks, a lost
   stream has valid 0, and the loop's states / landmarks / views are those of a loop without pose;
E. DeviceFaceLoop (FaceMesh V2, 1 euro filter): the same on the filtered landmarks, through loss
   and re-seeding;
F. end to end: FaceMesh V1 on the golden views, pose on the device, the reference's 5 degree bars."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import procrustes_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = 640, 480
WORDS = 21  # a zr_pose in 32-bit words; word 7 is `valid`
POINTS = np.array(R.cases()["points"], F)


def _reference(n_ref):
    return POINTS if n_ref == 8 else np.ascontiguousarray(R.canonical_mesh()[:n_ref])


def _sets(rng, ref, n_sets, m=None):
    """Seeded rigid transforms of `ref` plus small noise, as (n_sets, m, 3) with m >= len(ref)
    points per set; the points past the reference are unrelated values the kernel must ignore."""
    m = m or len(ref)
    out = rng.normal(0.0, 50.0, (n_sets, m, 3))
    for i in range(n_sets):
        rot = R.random_rotation(rng)
        out[i, :len(ref)] = ((ref.astype(np.float64) @ rot.T) * rng.uniform(0.5, 300.0) + rng.uniform(-200, 200, 3) +
                             rng.normal(0, 0.01, ref.shape))
    return out.astype(F)


def _host_records(Hm, ref, sets, flip, valid=None):
    a = Hm.ProcrustesAnalyzer(ref)
    out = np.empty((len(sets), WORDS), np.uint32)
    for i, pts in enumerate(sets):
        if valid is not None and not valid[i]:
            out[i] = 0x7FC00000
            out[i, 7] = 0
        else:
            out[i] = a.analyze(pts[:len(ref)], flip_y=flip).pose().view(np.uint32)
    return out


def _device_records(ref, sets, flip, valid=None):
    from zaru_amd import _lib
    rec = _lib.Procrustes(ref).analyze(sets, flip_y=flip, valid=valid)
    return np.frombuffer(rec.tobytes(), np.uint32).reshape(len(sets), WORDS)


@pytest.mark.parametrize("n_ref", [2, 8, 63, 64, 65, 468])
def test_kernel_matches_host_every_byte(n_ref):
    import zaru_amd.host as Hm
    ref = _reference(n_ref)
    rng = np.random.default_rng(300 + n_ref)
    for n_sets in (1, 3, 67):
        for flip in (False, True):
            sets = _sets(rng, ref, n_sets)
            want = _host_records(Hm, ref, sets, flip)
            got = _device_records(ref, sets, flip)
            assert np.array_equal(got, want), (n_ref, n_sets, flip, np.argwhere(got != want)[:5])
            assert (got[:, 7] == 1).all()
            if n_ref > 2:  # (two points leave the rotation about their line open)
                assert np.isfinite(got.view(F)[:, [i for i in range(WORDS) if i != 7]]).all()


def test_kernel_stride_and_validity_mask():
    """478 landmarks per set against the 468-point mesh (stride 1434), and a mask with zeros: those
    records are valid 0 / NaN, their neighbours what they are without a mask."""
    import zaru_amd.host as Hm
    ref = R.canonical_mesh()
    rng = np.random.default_rng(9)
    sets = _sets(rng, ref, 67, m=478)
    valid = np.ones(67, np.int32)
    valid[[0, 5, 6, 40, 66]] = 0
    sets[5] = np.nan  # never read
    want = _host_records(Hm, ref, sets, True, valid)
    got = _device_records(ref, sets, True, valid)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    nomask = _device_records(ref, sets, True)
    keep = valid != 0
    assert np.array_equal(nomask[keep], got[keep])
    assert (got[~keep, 7] == 0).all() and np.isnan(got[~keep].view(F)[:, :7]).all()


def test_kernel_against_f64_kabsch():
    ref = R.canonical_mesh()
    rng = np.random.default_rng(67)
    sets = _sets(rng, ref, 67)
    got = _device_records(ref, sets, False).view(F)
    worst = worst_scale = worst_t = 0.0
    for i in range(67):
        scale, rot, trans, _ = R.kabsch_f64(ref, sets[i])
        worst = max(worst, R.rotation_angle(R.quat_to_matrix(got[i, 8:12]), rot))
        worst_scale = max(worst_scale, abs(got[i, 3] - scale) / scale)
        worst_t = max(worst_t, float(np.abs(got[i, 4:7] - trans).max()))
    print(f"device quaternion vs f64 Kabsch over 67 sets: max angle {worst:.3e} rad, "
          f"max relative scale error {worst_scale:.3e}, max translation error {worst_t:.3e}")
    assert worst <= 1e-5


def test_collapsed_and_nan_sets_return_the_host_bits():
    import zaru_amd.host as Hm
    sets = np.stack([np.tile(np.array([[3.0, -2.0, 0.5]], F), (8, 1)), POINTS.copy(), POINTS.copy(), POINTS * 2])
    sets[1, 1, 1] = np.nan
    sets[2, 4, 0] = np.inf
    for flip in (False, True):
        want = _host_records(Hm, POINTS, sets, flip)
        got = _device_records(POINTS, sets, flip)
        assert np.array_equal(got, want), (flip, np.argwhere(got != want)[:5])
    assert got.view(F)[0, 3] == 0.0 and np.array_equal(got.view(F)[0, 8:12], np.array([0, 0, 0, 1], F))
    assert np.isnan(got.view(F)[1, 3]) and got.view(F)[3, 3] == 2.0


def test_analyze_argument_errors():
    from zaru_amd import _lib
    from zaru_amd._lib import DeviceBuffer
    lib = _lib.lib()
    p = _lib.Procrustes(POINTS)
    d_pts, d_out = DeviceBuffer.from_array(_sets(np.random.default_rng(1), POINTS, 2)), DeviceBuffer(2 * 84)
    ok = (p.ptr, d_pts.ptr, 2, 24, 0, None, d_out.ptr, None)
    for i, v in ((0, None), (1, None), (6, None), (2, 0), (3, 23), (2, 1 << 31), (3, 1 << 31)):
        args = list(ok)
        args[i] = v
        assert lib.zr_procrustes_analyze_async(*args) == -1, (i, v)
    assert lib.zr_procrustes_analyze_tracked_async(p.ptr, d_pts.ptr, 2, 24, 0, None, d_out.ptr, None) == -1
    _lib.check(lib.zr_procrustes_analyze_async(*ok))
    _lib.synchronize()
    assert (d_out.download((2, WORDS), np.uint32)[:, 7] == 1).all()


# ---- D / E / F: the loops -----------------------------------------------------------------------
def _patch(view=0, zoom=2):
    codes = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))["codes"][view]
    p = np.full((192, 192, 4), 255, np.uint8)
    p[..., :3] = codes.transpose(1, 2, 0)
    return np.repeat(np.repeat(p, zoom, axis=0), zoom, axis=1)


def _frames_at(buf, t, S):
    fb = H * W * 4
    return [(buf.ptr + (t * S + s) * fb, W, H, W * 4) for s in range(S)]


def _check_poses(Hm, analyzer, poses, landmarks, tracked, n_ref=468):
    poses = poses.view(np.uint32)
    for s in range(len(poses)):
        if tracked[s]:
            want = analyzer.analyze(landmarks[s][:n_ref], flip_y=True).pose().view(np.uint32)
            assert np.array_equal(poses[s], want), s
            assert poses[s, 7] == 1 and np.isfinite(poses[s].view(F)[8:]).all()
        else:
            assert poses[s, 7] == 0 and np.isnan(np.delete(poses[s].view(F), 7)).all(), s


def test_device_tracker_poses():
    """FaceMesh V1, 3 streams, 4 steps; stream 1's face disappears after step 1."""
    import zaru_amd.host as Hm
    from zaru_amd._lib import DeviceBuffer
    S, T = 3, 4
    rng = np.random.default_rng(43)
    patch = _patch()
    frames = np.empty((T, S, H, W, 4), np.uint8)
    rois = []
    for s in range(S):
        bg = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        y0, x0 = int(rng.integers(0, H - 384 - 2 * T)), int(rng.integers(0, W - 384 - 4 * T))
        for t in range(T):
            frames[t, s] = bg
            if not (s == 1 and t >= 2):
                frames[t, s, y0 + 2 * t:y0 + 2 * t + 384, x0 + 4 * t:x0 + 4 * t + 384] = patch
        rois.append((x0 + 192.0, y0 + 192.0, 340.0, 340.0, 0.05 * (s - 1)))
    buf = DeviceBuffer.from_array(frames)
    mesh = R.canonical_mesh()
    analyzer = Hm.ProcrustesAnalyzer(mesh)
    on, off = Hm.DeviceTracker("facemesh", 0), Hm.DeviceTracker("facemesh", 0)
    on.set_pose_reference(mesh)  # flip_y defaults to True
    with pytest.raises(RuntimeError):
        off.poses()
    for tr in (on, off):
        tr.set_rois(rois, [(W, H)] * S)
    seen = []
    for t in range(T):
        for tr in (on, off):
            tr.step(_frames_at(buf, t, S))
            tr.synchronize()
        st, lm = on.states(), on.landmarks()
        st_off = off.states()
        tracked = [x["tracked"] for x in st]
        seen.append(tracked)
        _check_poses(Hm, analyzer, on.poses(), lm, tracked)
        # pose is an output only: the loop itself is what it is without it
        assert np.array_equal(lm.view(np.uint32), off.landmarks().view(np.uint32)), t
        assert np.array_equal(on.views().view(np.uint32), off.views().view(np.uint32)), t
        for a, b in zip(st, st_off):
            assert a["tracked"] == b["tracked"] and a["active"] == b["active"] and a["confidence"] == b["confidence"]
            for k in ("roi", "updated_roi", "view_rect"):
                assert a[k].rect() == b[k].rect() and a[k].rotation_radians() == b[k].rotation_radians(), (t, k)
    assert all(seen[t][0] and seen[t][2] for t in range(T))
    assert seen[0][1] and seen[1][1] and not seen[3][1]  # stream 1 was tracked, then lost
    # off again: no record is produced, and a smaller reference than the network is fine
    on.set_pose_reference(None)
    on.step(_frames_at(buf, 0, S))
    with pytest.raises(RuntimeError):
        on.poses()
    with pytest.raises(RuntimeError):
        Hm.DeviceTracker("hand", 0).set_pose_reference(mesh)  # 21 landmarks < 468 reference points


def test_device_face_loop_poses_filtered_and_reseeded():
    """FaceMesh V2 (478 landmarks against the 468-point mesh) with a 1 euro filter; stream 1's face
    disappears for two frames and is re-acquired by the detector, stream 2 is noise only."""
    import zaru_amd.host as Hm
    from zaru_amd._lib import DeviceBuffer
    S, T = 3, 7
    rng = np.random.default_rng(5)
    patch = _patch()
    frames = np.empty((T, S, H, W, 4), np.uint8)
    for s in range(S):
        bg = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        y0, x0 = int(rng.integers(0, 60)), int(rng.integers(0, 200))
        for t in range(T):
            frames[t, s] = bg
            if s == 2 or (s == 1 and t in (3, 4)):
                continue
            frames[t, s, y0 + 2 * t:y0 + 2 * t + 384, x0 + 3 * t:x0 + 3 * t + 384] = patch
    buf = DeviceBuffer.from_array(frames)
    mesh = R.canonical_mesh()
    analyzer = Hm.ProcrustesAnalyzer(mesh)
    on, off = Hm.DeviceFaceLoop("face", "facemesh_v2", S, 0), Hm.DeviceFaceLoop("face", "facemesh_v2", S, 0)
    for loop in (on, off):
        loop.set_filter(Hm.OneEuro(1.0, 0.05), 1.0 / 30.0)
    on.set_pose_reference(mesh, True)
    seen = []
    for t in range(T):
        for loop in (on, off):
            loop.step(_frames_at(buf, t, S))
            loop.synchronize()
        st, lm = on.states(), on.landmarks()
        tracked = [x["tracked"] for x in st]
        seen.append(tracked)
        _check_poses(Hm, analyzer, on.poses(), lm, tracked)
        assert np.array_equal(lm.view(np.uint32), off.landmarks().view(np.uint32)), t
        for a, b in zip(st, off.states()):
            assert a["tracked"] == b["tracked"] and a["active"] == b["active"]
            assert a["roi"].rect() == b["roi"].rect() and a["roi"].rotation_radians() == b["roi"].rotation_radians()
    assert on.reacquisitions() == off.reacquisitions() >= 3  # both faces at the start, stream 1 again
    assert on.detections_run() == off.detections_run()
    col = [[seen[t][s] for t in range(T)] for s in range(S)]
    assert sum(col[0]) >= T - 1 and not any(col[2])
    assert any(col[1][:3]) and not col[1][4] and col[1][T - 1]  # tracked, lost, tracked again


def test_facemesh_views_head_pose_end_to_end():
    """FaceMesh V1 on the golden views' pixels, the pose on the device: the reference's acceptance
    test (mediapipe.rs:589-600), |roll|, |pitch| and |yaw - view| below 5 degrees."""
    import zaru_amd.host as Hm
    from zaru_amd._lib import DeviceBuffer
    view_deg = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))["view_deg"]
    frames = np.stack([_patch(v, 1) for v in range(3)])
    buf = DeviceBuffer.from_array(frames)
    tr = Hm.DeviceTracker("facemesh", 0)
    tr.set_pose_reference(R.canonical_mesh(), True)
    tr.set_rois([(96.0, 96.0, 192.0, 192.0, 0.0)] * 3, [(192, 192)] * 3)
    tr.step([(buf.ptr + v * 192 * 192 * 4, 192, 192, 192 * 4) for v in range(3)])
    tr.synchronize()
    poses = tr.poses()
    assert (poses.view(np.uint32)[:, 7] == 1).all()
    for v in range(3):
        rot = poses[v, 12:21].reshape(3, 3).astype(np.float64)
        roll = math.degrees(math.atan2(rot[2, 1], rot[2, 2]))
        pitch = math.degrees(-math.asin(max(-1.0, min(1.0, rot[2, 0]))))
        yaw = math.degrees(math.atan2(rot[1, 0], rot[0, 0]))
        print(f"view {view_deg[v]}: roll {roll:.2f} pitch {pitch:.2f} yaw {yaw:.2f}")
        assert abs(roll) < 5.0 and abs(pitch) < 5.0 and abs(yaw - float(view_deg[v])) < 5.0
