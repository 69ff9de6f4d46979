"""ProcrustesAnalyzer on the host (zaru_amd.host, host/procrustes.cpp over
kernels/procrustes_math.h): the reference's own suite with its own bars
(crates/zaru/src/procrustes.rs:275-276, 348-483), the FaceMesh head-pose acceptance test
(face/landmark/mediapipe.rs:589-600) on the golden views, degenerate and non-finite inputs,
centroid and scale bit for bit against the numpy restatement, argument errors of the host mirror
and the C ABI, and the stand-alone sanitizer build of the shared header.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import procrustes_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MAX_DELTA = 0.00001
MAX_TRANSLATION_DELTA = 0.001
CASES = R.cases()
POINTS = np.array(CASES["points"], F)


@pytest.fixture(scope="module")
def Hm():
    import zaru_amd.host as Hm
    return Hm


@pytest.fixture(scope="module")
def analyzer(Hm):
    return Hm.ProcrustesAnalyzer(POINTS)


def _analyze(analyzer, matrix):
    return analyzer.analyze(R.apply(matrix, POINTS))


@pytest.mark.parametrize("case", CASES["transforms"], ids=[c["name"] for c in CASES["transforms"]])
def test_recover_transform(analyzer, case):
    """test_identity / test_translate / test_uniform_scaling / test_rotation / test_combinations."""
    want = np.array(case["matrix"], F).reshape(4, 4)
    got = _analyze(analyzer, want).transform()
    assert not np.isnan(want).any() and not np.isnan(got).any()
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= MAX_DELTA, (want, got)


def test_transform_list_is_the_reference_suite():
    names = [c["name"] for c in CASES["transforms"]]
    assert len(names) == 15 and names[0] == "identity"
    assert sum(n.startswith("translate") for n in names) == 3
    assert {"scale_4", "scale_0.2", "scale_0"} <= set(names)
    assert sum(n.startswith("rot_") for n in names) == 4 and sum(n.startswith("combination") for n in names) == 4


def test_identity_rotation_angle(analyzer):
    res = _analyze(analyzer, np.eye(4))
    assert R.rotation_angle(R.quat_to_matrix(res.rotation), np.eye(3)) <= MAX_DELTA


@pytest.mark.parametrize("s", CASES["exact_scales"])
def test_power_of_two_scale_is_exact(analyzer, s):
    res = _analyze(analyzer, np.diag([s, s, s, 1.0]))
    assert res.scale == s
    q = res.rotation.astype(np.float64)
    assert np.abs(q - [0, 0, 0, 1]).max() <= MAX_DELTA
    assert np.abs(res.translation).max() <= MAX_DELTA


def _clamp_degrees(d):
    return ((d + 180) % 360) - 180


@pytest.mark.parametrize("zr", CASES["z_rotation"], ids=[f"s{c['scale']}_t{c['translation']}" for c in CASES["z_rotation"]])
def test_rot_around_z(analyzer, zr):
    """test_rot_around_z and large_scale_and_move: every degree from -180 to 360."""
    scaling, t = zr["scale"], np.array(zr["translation"], F)
    lo, hi = CASES["z_rotation_degrees"]
    expected, recovered = [], []
    for deg in range(lo, hi + 1):
        angle = float(F(math.radians(F(deg))))
        m = np.eye(4)
        m[:3, :3] = scaling * np.array([[math.cos(angle), -math.sin(angle), 0],
                                        [math.sin(angle), math.cos(angle), 0], [0, 0, 1]])
        m[:3, 3] = t
        res = _analyze(analyzer, m.astype(F))
        assert abs(res.scale - scaling) <= MAX_DELTA * max(abs(res.scale), abs(scaling)), (deg, res.scale)
        assert np.abs(res.translation.astype(np.float64) - t).max() <= MAX_TRANSLATION_DELTA, (deg, res.translation)
        roll, pitch, yaw = res.euler_angles()
        assert abs(roll) <= MAX_DELTA and abs(pitch) <= MAX_DELTA, (deg, roll, pitch)
        expected.append(_clamp_degrees(deg))
        recovered.append(_clamp_degrees(int(round(math.degrees(yaw)))))
    assert recovered == expected


def test_jitter(analyzer):
    j = CASES["jitter"]
    rot = R.euler_matrix(*j["euler"])
    noise = np.random.default_rng(0).random((8, 3)) - 0.5
    pts = (POINTS.astype(np.float64) @ rot.T) * j["factor"] + np.array(j["offset"]) + noise
    res = analyzer.analyze(pts.astype(F))
    print("jitter: scale", res.scale, "translation", res.translation, "euler deg",
          [math.degrees(a) for a in res.euler_angles()])
    assert abs(res.scale - j["factor"]) <= 0.1
    assert np.abs(res.translation.astype(np.float64) - j["offset"]).max() <= 0.5
    for got, want in zip(res.euler_angles(), j["euler"]):
        assert abs(math.degrees(got) - math.degrees(want)) <= 0.2


@pytest.fixture(scope="module")
def mesh_views():
    z = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))
    return z["landmarks"], z["view_deg"]


def test_facemesh_views_head_pose(Hm, mesh_views):
    """The reference's FaceMesh acceptance test on the golden landmarks of its three views."""
    landmarks, view_deg = mesh_views
    a = Hm.ProcrustesAnalyzer(R.canonical_mesh())
    for lm, deg in zip(landmarks, view_deg):
        roll, pitch, yaw = (math.degrees(v) for v in a.analyze(lm, flip_y=True).euler_angles())
        print(f"view {deg}: roll {roll:.2f} pitch {pitch:.2f} yaw {yaw:.2f}")
        assert abs(roll) < 5.0 and abs(pitch) < 5.0 and abs(yaw - float(deg)) < 5.0, (deg, roll, pitch, yaw)


def test_collapsed_set(analyzer):
    res = analyzer.analyze(np.tile(np.array([[3.0, -2.0, 0.5]], F), (8, 1)))
    assert res.scale == 0.0
    assert np.array_equal(res.rotation, np.array([0, 0, 0, 1], F))
    assert np.isfinite(res.translation).all()


def test_nan_point_returns_nan(analyzer):
    pts = POINTS.copy()
    pts[1, 1] = np.nan
    res = analyzer.analyze(pts)  # returns: every loop has a fixed trip count
    assert np.isnan(res.scale) and np.isnan(res.rotation).all() and np.isnan(res.rotation_matrix).all()
    # one canonical quiet NaN, so that host and device records are the same bytes; only the x and
    # z of the centroid (words 0 and 2) never meet the NaN
    pose = res.pose().view(np.uint32)
    assert pose[7] == 1 and all(v == 0x7FC00000 for i, v in enumerate(pose) if i not in (0, 2, 7))
    assert np.isfinite(res.centroid[[0, 2]]).all()


def test_mirrored_set_gives_a_proper_rotation(analyzer):
    pts = POINTS.copy()
    pts[:, 0] = -pts[:, 0]
    m = analyzer.analyze(pts).rotation_matrix.astype(np.float64)
    assert np.abs(m @ m.T - np.eye(3)).max() <= 1e-3 and abs(np.linalg.det(m) - 1.0) <= 1e-3


def _seeded_set(rng, ref):
    rot = R.random_rotation(rng)
    return ((ref.astype(np.float64) @ rot.T) * rng.uniform(0.5, 300.0) + rng.uniform(-200, 200, 3) +
            rng.normal(0, 0.01, ref.shape)).astype(F)


@pytest.mark.parametrize("n_ref", [2, 8, 65])
def test_centroid_and_scale_match_numpy_restatement(Hm, n_ref):
    rng = np.random.default_rng(20 + n_ref)
    ref = np.resize(R.canonical_mesh(), (n_ref, 3)) if n_ref != 8 else POINTS
    a = Hm.ProcrustesAnalyzer(ref)
    rc, rs = R.centroid_scale_f32(ref)
    assert np.array_equal(a.reference_centroid.view(np.uint32), rc.view(np.uint32))
    assert F(a.reference_scale).view(np.uint32) == rs.view(np.uint32)
    for flip in (False, True):
        pts = _seeded_set(rng, ref)
        res = a.analyze(pts, flip_y=flip)
        c, s = R.centroid_scale_f32(pts, flip)
        assert np.array_equal(res.centroid.view(np.uint32), c.view(np.uint32)), (n_ref, flip)
        assert F(res.scale).view(np.uint32) == F(s / rs).view(np.uint32), (n_ref, flip)


def test_centroid_and_scale_match_on_golden_views(Hm, mesh_views):
    landmarks, _ = mesh_views
    a = Hm.ProcrustesAnalyzer(R.canonical_mesh())
    _, rs = R.centroid_scale_f32(R.canonical_mesh())
    for lm in landmarks:
        res = a.analyze(lm, flip_y=True)
        c, s = R.centroid_scale_f32(lm, True)
        assert np.array_equal(res.centroid.view(np.uint32), c.view(np.uint32))
        assert F(res.scale).view(np.uint32) == F(s / rs).view(np.uint32)


def test_host_agrees_with_f64_kabsch(Hm):
    """The f32 Jacobi against numpy's f64 SVD on seeded transforms of the canonical mesh: the
    angle between the rotations stays within the reference's MAX_DELTA."""
    rng = np.random.default_rng(5)
    ref = R.canonical_mesh()
    a = Hm.ProcrustesAnalyzer(ref)
    worst = 0.0
    for _ in range(16):
        pts = _seeded_set(rng, ref)
        res = a.analyze(pts)
        scale, rot, trans, _ = R.kabsch_f64(ref, pts)
        worst = max(worst, R.rotation_angle(R.quat_to_matrix(res.rotation), rot))
        assert abs(res.scale - scale) <= 1e-5 * scale
    print("worst angle to f64 Kabsch:", worst)
    assert worst <= MAX_DELTA


def test_host_argument_errors(Hm, analyzer):
    MATCH = "at least 2 points|different length|must be"
    with pytest.raises(RuntimeError, match=MATCH):
        Hm.ProcrustesAnalyzer(POINTS[:1])
    with pytest.raises(RuntimeError, match=MATCH):
        Hm.ProcrustesAnalyzer(np.zeros((0, 3), F))
    with pytest.raises(RuntimeError, match=MATCH):
        Hm.ProcrustesAnalyzer(np.zeros((4, 2), F))
    with pytest.raises(RuntimeError, match=MATCH):
        analyzer.analyze(POINTS[:7])
    with pytest.raises(RuntimeError, match=MATCH):
        analyzer.analyze(np.zeros((9, 3), F))
    assert len(analyzer) == 8


def test_c_abi_argument_errors():
    """What the C ABI refuses before it touches a device."""
    from zaru_amd import _lib
    lib = _lib.lib()
    out = C.c_void_p()
    pts = np.ascontiguousarray(POINTS)
    bad = pts.copy()
    bad[3, 2] = np.inf
    nan = pts.copy()
    nan[0, 0] = np.nan
    big = np.zeros((2049, 3), F)
    for ref, n in ((None, 8), (pts, 1), (pts, 0), (bad, 8), (nan, 8), (big, 2049)):
        rc = lib.zr_procrustes_create(None if ref is None else ref.ctypes.data, n, C.byref(out))
        assert rc == -1 and out.value is None, (n, rc)
    assert lib.zr_procrustes_create(pts.ctypes.data, 8, None) == -1
    assert lib.zr_procrustes_analyze_async(None, 1, 1, 24, 0, None, 1, None) == -1
    assert lib.zr_procrustes_analyze_tracked_async(None, 1, 1, 24, 0, 1, 1, None) == -1
    assert b"null" in lib.zr_last_error()
    lib.zr_procrustes_destroy(None)  # a no-op
    assert C.sizeof(_lib.Pose) == 84
    with pytest.raises(_lib.ZaruError):
        _lib.Procrustes(np.zeros((5, 2), F))
    with pytest.raises(_lib.ZaruError):
        _lib.Procrustes(POINTS[:1])


def test_sanitized_native_check(tmp_path):
    """tests/native/procrustes_check.cpp: the shared header over the JSON cases and the degenerate
    sets, built with AddressSanitizer and UBSan by the host compiler and run directly."""
    exe = str(tmp_path / "procrustes_check")
    src = os.path.join(REPO, "tests", "native", "procrustes_check.cpp")
    cxx = os.environ.get("CXX", "g++")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                        "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(REPO, "tests", "golden", "procrustes_cases.json")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1].startswith("ok ")
