"""The aligned identity crop, the parts that need no GPU:

  * zaru_amd.host.aligned_crop_view and zr_face_align_host against tests/align_ref.py's numpy f32
    restatement, bit for bit (the view's ten words and the record), on the three fixture meshes and on
    random point sets: P = 2 and P = 8, groups of 1 and of 4, strides 2 and 3, L = 6 with an index of L - 1,
    coordinates around 1e4, and -0.0;
  * the fallbacks (coincident face points, coordinates of 3e38, a max_residual between two cases'
    residuals), each leaving the view passed in untouched;
  * every refusal of the two entry points that needs no device buffer;
  * conditions on the fixture itself: the eye order, the residual, the fitted roll against view_deg;
  * consistency: the template points, mapped through the fitted transform and back through the returned
    view's sampling map inverted, land where they started -- which a sign or centre error shared by the
    code and its restatement would not survive.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import zaru_amd.host as H
from zaru_amd import _lib

import align_ref as AR

f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture():
    g = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))
    return g["landmarks"].astype(f32), g["view_deg"].astype(np.float64), g["codes"]


def five_point(max_residual=math.inf):
    a = H.FaceAlignment.facemesh_five_point()
    a.max_residual = max_residual
    return a


# ---- the cases, shared with tests/test_gpu_align.py --------------------------------------------------
def random_cases():
    """name -> (template, groups, landmarks [L][stride], ow, oh, frame_w, frame_h)."""
    rng = np.random.default_rng(2024)
    out = {}

    def points(P, ow, oh):
        return [(float(f32(x)), float(f32(y))) for x, y in rng.uniform(0.1, 0.9, (P, 2)) * (ow, oh)]

    def face(L, stride, centre, spread):
        lm = rng.normal(0.0, spread, (L, stride)).astype(f32)
        lm[:, 0] += f32(centre[0])
        lm[:, 1] += f32(centre[1])
        return lm

    out["p2_single"] = (points(2, 112, 112), [[3], [0]], face(6, 3, (200, 150), 40), 112, 112, 480, 360)
    out["p8_groups_of_4"] = (points(8, 112, 112), [list(rng.choice(40, 4, replace=False)) for _ in range(8)],
                             face(40, 3, (300, 200), 60), 112, 112, 640, 480)
    out["p8_mixed_groups"] = (points(8, 96, 128), [[0], [1, 2], [3, 4, 5], [6, 7, 8, 9], [10], [11, 12], [13], [14, 15]],
                              face(16, 3, (100, 300), 30), 96, 128, 333, 517)
    out["stride2"] = (points(5, 112, 112), [[0, 1], [2], [3], [4], [5]], face(6, 2, (50, 60), 20), 112, 112, 192, 192)
    out["last_index"] = (points(3, 112, 112), [[5], [0, 5], [2]], face(6, 3, (90, 90), 25), 112, 112, 192, 192)
    out["around_1e4"] = (points(5, 112, 112), [[0], [1], [2], [3], [4]], face(6, 3, (10000, 9000), 80), 112, 112,
                         16000, 12000)
    lm = face(6, 3, (0, 0), 30)
    lm[0, :2], lm[1, 0], lm[2, 1] = -0.0, -0.0, -0.0
    out["negative_zero"] = (points(4, 112, 112), [[0], [1], [2], [3]], lm, 112, 112, 64, 64)
    # the template rotated by 90 degrees, scaled and moved: an exact similarity, |rad| near pi / 2
    t = points(5, 112, 112)
    lm = np.zeros((6, 3), f32)
    lm[:5, 0] = [150.0 - 1.5 * y for _, y in t]
    lm[:5, 1] = [40.0 + 1.5 * x for x, _ in t]
    out["quarter_turn"] = (t, [[0], [1], [2], [3], [4]], lm, 112, 112, 320, 240)
    return out


def fallback_cases():
    """name -> (case as above, the FAIL bit)."""
    base = AR.TEMPLATE, [[0], [1], [2], [3], [4]]
    same = np.zeros((6, 3), f32)
    same[:, 0], same[:, 1] = 77.5, 31.25
    huge = np.zeros((6, 3), f32)
    huge[:, :2] = [[3e38, 1.0], [-3e38, 2.0], [3e38, 3e38], [1.0, -3e38], [2.0, 5.0], [0.0, 0.0]]
    inf = same.copy()
    inf[2, 0] = math.inf
    nan = same.copy()
    nan[4, 1] = math.nan
    return {"coincident": ((*base, same, 112, 112, 192, 192), AR.FAIL_DEGENERATE),
            "huge": ((*base, huge, 112, 112, 192, 192), AR.FAIL_DEGENERATE),
            "infinite": ((*base, inf, 112, 112, 192, 192), AR.FAIL_DEGENERATE),
            "nan": ((*base, nan, 112, 112, 192, 192), AR.FAIL_DEGENERATE)}


def c_align(case, max_residual=math.inf, frame=0, view=None):
    """zr_face_align_host on a case -> (rc, view row, record row); `view` is the row passed in."""
    t, g, lm, ow, oh, fw, fh = case
    cfg = _lib.AlignCfg.make(t, g, ow, oh, max_residual)
    lm = np.ascontiguousarray(lm, f32)
    v = np.zeros(1, AR.VIEW_DESC) if view is None else view
    r = np.zeros(1, AR.RECORD)
    rc = _lib.lib().zr_face_align_host(C.byref(cfg), lm.ctypes.data, lm.shape[0], lm.shape[1], fw, fh, frame,
                                       v.ctypes.data, r.ctypes.data)
    return rc, v[0], r[0]


def describe(view, frame=0):
    z = (C.c_float * 5)(*view.zr_view())
    d = np.zeros(1, AR.VIEW_DESC)
    _lib.check(_lib.lib().zr_view_describe(z, 1, frame, d.ctypes.data))
    return d[0]


def check_case(name, case, max_residual=math.inf):
    t, g, lm, ow, oh, fw, fh = case
    want = AR.fit(t, g, lm, ow, oh, max_residual)
    sentinel = np.zeros(1, AR.VIEW_DESC)
    sentinel.view(np.uint32)[:] = 0xA5A5A5A5
    rc, v, r = c_align(case, max_residual, frame=7, view=sentinel.copy())
    assert rc == 0, (name, _lib.lib().zr_last_error())
    assert r.tobytes() == AR.record(want).tobytes(), (name, r, AR.record(want))
    hv, hr = H.aligned_crop_view(lm, fw, fh, H.FaceAlignment(t, [list(map(int, x)) for x in g], ow, oh, max_residual))
    got = np.zeros(1, AR.RECORD)
    got["scale"], got["rad"], got["residual"], got["flags"] = hr["scale"], hr["angle"], hr["residual"], hr["flags"]
    assert got.tobytes() == r.tobytes(), (name, hr, r)
    if want["crop"] is None:
        assert want["flags"] & AR.FALLBACK and not want["flags"] & AR.ALIGNED
        assert hv is None and v.tobytes() == sentinel.tobytes(), (name, "a fallback writes no view")
    else:
        assert want["flags"] == AR.ALIGNED
        wv = AR.view_desc(want["crop"], fw, fh, 7)
        assert v.tobytes() == wv.tobytes(), (name, v, wv)
        assert describe(hv, 7).tobytes() == wv.tobytes(), (name, describe(hv, 7), wv)
    return want


@pytest.mark.parametrize("view", [0, 1, 2])
def test_fixture_meshes_bit_for_bit(view):
    lm, _, _ = fixture()
    want = check_case(f"mesh{view}", (AR.TEMPLATE, AR.GROUPS, lm[view], 112, 112, 192, 192))
    assert want["flags"] == AR.ALIGNED
    # the default settings are the restatement's
    hv, hr = H.aligned_crop_view(lm[view], 192, 192, five_point())
    assert f32(hr["scale"]).tobytes() == want["scale"].tobytes() and hr["flags"] == AR.ALIGNED
    assert describe(hv).tobytes() == AR.view_desc(want["crop"], 192, 192).tobytes()


@pytest.mark.parametrize("name", list(random_cases()))
def test_random_point_sets_bit_for_bit(name):
    want = check_case(name, random_cases()[name])
    assert want["flags"] == AR.ALIGNED, "the random sets are well conditioned"
    if name == "quarter_turn":
        assert abs(abs(float(want["rad"])) - math.pi / 2) < 1e-3 and float(want["residual"]) < 1e-3


def test_default_settings():
    a = H.FaceAlignment.facemesh_five_point()
    assert np.array_equal(a.template, np.array(AR.TEMPLATE, f32)) and a.groups == AR.GROUPS
    assert (a.ow, a.oh, a.num_points) == (112, 112, 5) and a.max_residual == math.inf
    assert a.cfg_bytes() == bytes(_lib.AlignCfg.make(AR.TEMPLATE, AR.GROUPS))
    assert C.sizeof(_lib.AlignCfg) == 208 and C.sizeof(_lib.FaceAlignment) == 16


@pytest.mark.parametrize("name", list(fallback_cases()))
def test_degenerate_fallbacks(name):
    case, bit = fallback_cases()[name]
    want = check_case(name, case)
    assert want["flags"] == AR.FALLBACK | bit, (name, want)
    if name == "coincident":
        assert float(want["scale"]) == 0.0
    if name == "huge":
        assert not np.isfinite(want["scale"])


def test_max_residual_separates_two_cases():
    lm, _, _ = fixture()
    res = [float(AR.fit(AR.TEMPLATE, AR.GROUPS, lm[v])["residual"]) for v in range(3)]
    lo, hi = int(np.argmin(res)), int(np.argmax(res))
    limit = float(f32((res[lo] + res[hi]) / 2))
    assert res[lo] < limit < res[hi]
    ok = check_case("below", (AR.TEMPLATE, AR.GROUPS, lm[lo], 112, 112, 192, 192), limit)
    bad = check_case("above", (AR.TEMPLATE, AR.GROUPS, lm[hi], 112, 112, 192, 192), limit)
    assert ok["flags"] == AR.ALIGNED and bad["flags"] == AR.FALLBACK | AR.FAIL_RESIDUAL
    # the limit itself passes (residual <= max_residual), and -inf / 0 reject everything
    edge = check_case("edge", (AR.TEMPLATE, AR.GROUPS, lm[hi], 112, 112, 192, 192), res[hi])
    assert edge["flags"] == AR.ALIGNED
    none = check_case("none", (AR.TEMPLATE, AR.GROUPS, lm[lo], 112, 112, 192, 192), 0.0)
    assert none["flags"] == AR.FALLBACK | AR.FAIL_RESIDUAL


def test_refusals():
    lm, _, _ = fixture()
    good = (AR.TEMPLATE, AR.GROUPS, lm[0], 112, 112, 192, 192)
    assert c_align(good)[0] == 0
    t5, g5 = list(AR.TEMPLATE), [list(g) for g in AR.GROUPS]

    def rc(template=t5, groups=g5, landmarks=lm[0], ow=112, oh=112, max_residual=math.inf, num_points=None,
           raw_group=None):
        cfg = _lib.AlignCfg.make(template, groups, ow, oh, max_residual)
        if num_points is not None:
            cfg.num_points = num_points
        if raw_group is not None:
            p, j, idx = raw_group
            cfg.group[p][j] = idx
        a = np.ascontiguousarray(landmarks, f32)
        v, r = np.zeros(1, AR.VIEW_DESC), np.zeros(1, AR.RECORD)
        return _lib.lib().zr_face_align_host(C.byref(cfg), a.ctypes.data, a.shape[0], a.shape[1], 192, 192, 0,
                                             v.ctypes.data, r.ctypes.data)

    nine = [(float(i), float(i * i)) for i in range(9)]
    bad = [rc(num_points=1), rc(num_points=9), rc(num_points=0), rc(template=nine[:1], groups=[[0]]),
           rc(ow=0), rc(oh=0), rc(ow=-3),
           rc(raw_group=(2, 0, -1)),                      # an empty group
           rc(raw_group=(0, 1, 468)), rc(raw_group=(4, 0, 468)), rc(raw_group=(1, 1, -2)),   # >= L, < -1
           rc(landmarks=lm[0][:6]),                       # the default groups on L = 6
           rc(template=[(math.inf, 1.0)] + t5[1:]), rc(template=t5[:4] + [(2.0, math.nan)]),
           rc(template=[(5.0, 6.0)] * 5),                 # den == 0
           rc(template=[(5.0, 6.0)] * 2, groups=[[0], [1]]),
           rc(max_residual=math.nan)]
    assert bad == [-1] * len(bad), bad
    # NULL pointers and the stride
    cfg = _lib.AlignCfg.make(t5, g5)
    a = np.ascontiguousarray(lm[0], f32)
    v, r = np.zeros(1, AR.VIEW_DESC), np.zeros(1, AR.RECORD)
    f = _lib.lib().zr_face_align_host
    bad = [f(None, a.ctypes.data, 468, 3, 192, 192, 0, v.ctypes.data, r.ctypes.data),
           f(C.byref(cfg), None, 468, 3, 192, 192, 0, v.ctypes.data, r.ctypes.data),
           f(C.byref(cfg), a.ctypes.data, 468, 3, 192, 192, 0, None, r.ctypes.data),
           f(C.byref(cfg), a.ctypes.data, 468, 3, 192, 192, 0, v.ctypes.data, None),
           f(C.byref(cfg), a.ctypes.data, 0, 3, 192, 192, 0, v.ctypes.data, r.ctypes.data),
           f(C.byref(cfg), a.ctypes.data, 468, 1, 192, 192, 0, v.ctypes.data, r.ctypes.data)]
    assert bad == [-1] * len(bad), bad
    assert not v.tobytes().strip(b"\0") and not r.tobytes().strip(b"\0"), "a refusal writes nothing"
    # the host module refuses the same, and what its constructor can see
    for make in (lambda: H.FaceAlignment(t5[:1], [[0]]), lambda: H.FaceAlignment(nine, [[0]] * 9),
                 lambda: H.FaceAlignment(t5, g5[:4]), lambda: H.FaceAlignment(t5, [[]] + g5[1:]),
                 lambda: H.FaceAlignment(t5, [[1, 2, 3, 4, 5]] + g5[1:]), lambda: H.FaceAlignment(t5, [[-1]] + g5[1:])):
        with pytest.raises(Exception):
            make()
    for al in (H.FaceAlignment([(5.0, 6.0)] * 5, g5), H.FaceAlignment(t5, g5, 0, 112),
               H.FaceAlignment(t5, g5, 112, 112, math.nan), H.FaceAlignment(t5, [[468]] + g5[1:])):
        with pytest.raises(Exception):
            H.aligned_crop_view(lm[0], 192, 192, al)


# ---- conditions on the reference data ----------------------------------------------------------------
def test_fixture_sanity():
    lm, view_deg, _ = fixture()
    fits = [AR.fit(AR.TEMPLATE, AR.GROUPS, lm[v]) for v in range(3)]
    for v, r in enumerate(fits):
        assert r["q"][0][0] < r["q"][1][0], ("the image-left eye comes first", v)
        assert float(r["residual"]) <= 3.0, (v, r["residual"])
    assert view_deg[0] == 0.0
    for v in (1, 2):
        roll = math.degrees(float(fits[v]["rad"]) - float(fits[0]["rad"]))
        print(f"view {v}: view_deg {view_deg[v]:+.1f}, fitted roll relative to view 0 {roll:+.3f} deg")
        assert abs(roll - -view_deg[v]) <= 2.0, (v, roll, view_deg[v])


# ---- consistency -------------------------------------------------------------------------------------
def _consistency(name, case):
    t, g, lm, ow, oh, fw, fh = case
    r = AR.fit(t, g, lm, ow, oh)
    assert r["crop"] is not None
    _, v, _ = c_align(case)
    a, b = float(r["a"]), float(r["b"])
    (mtx, mty), (mqx, mqy) = (float(x) for x in r["mean_t"]), (float(x) for x in r["mean_q"])
    scale_px = max(1.0, abs(mqx), abs(mqy)) / 1e4   # 1e-3 px at the fixture's size, f32 resolution beyond
    for x, y in t:
        x, y = float(f32(x)), float(f32(y))
        px = mqx + a * (x - mtx) - b * (y - mty)       # q = M t + T
        py = mqy + b * (x - mtx) + a * (y - mty)
        bx, by = AR.unsample_point(v, px, py, ow, oh)
        assert abs(bx - x) <= 1e-3 * max(1.0, scale_px) and abs(by - y) <= 1e-3 * max(1.0, scale_px), (name, x, y, bx, by)
        # and forwards: the view samples the template point from where the fit puts it
        fx, fy = AR.sample_point(v, x, y, ow, oh)
        tol = 1e-3 * max(1.0, scale_px) * max(1.0, float(r["scale"]))
        assert abs(fx - px) <= tol and abs(fy - py) <= tol, (name, fx, fy, px, py)


@pytest.mark.parametrize("view", [0, 1, 2])
def test_consistency_on_the_fixture(view):
    lm, _, _ = fixture()
    _consistency(f"mesh{view}", (AR.TEMPLATE, AR.GROUPS, lm[view], 112, 112, 192, 192))


@pytest.mark.parametrize("name", ["p2_single", "p8_groups_of_4", "p8_mixed_groups", "stride2", "quarter_turn"])
def test_consistency_on_random_sets(name):
    _consistency(name, random_cases()[name])


def test_face_points_land_near_the_template():
    """What alignment is for: through the aligned view, the fixture's own face points sit within the
    residual's few grid pixels of the template points (the bounding crop puts them elsewhere)."""
    lm, _, _ = fixture()
    for v in range(3):
        case = (AR.TEMPLATE, AR.GROUPS, lm[v], 112, 112, 192, 192)
        r = AR.fit(*case[:3])
        _, d, _ = c_align(case)
        worst = 0.0
        for (tx, ty), (qx, qy) in zip(AR.TEMPLATE, r["q"]):
            gx, gy = AR.unsample_point(d, float(qx), float(qy), 112, 112)
            worst = max(worst, math.hypot(gx - tx, gy - ty))
        assert worst <= 3.0 * math.sqrt(5.0), (v, worst)   # one point cannot exceed sqrt(P) x the rms bound
