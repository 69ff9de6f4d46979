"""The face quality gate, the parts that need no GPU:

  * zaru_amd.host.face_quality (zr_face_quality_host) against tests/quality_ref.py's numpy restatement over
    the CPU oracle's view lookup, bit for bit, on every grid and view the GPU file runs too;
  * the tiers: -inf skips, a NaN value fails, LEARN implies EMBED;
  * the schedule of MultiQualityRef with a fake embed / match: a rejected object stays due, `rejected`
    counts up and resets, a held-back object is neither enrolled nor refined;
  * the frontal measure on the golden mesh views;
  * the argument refusals of the three entries.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import zaru_amd.host as H
from zaru_amd import _lib

import multi_enrol_ref as ER
import procrustes_ref as PR
import quality_ref as QR

f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS2_5 = math.cos(math.radians(5.0)) ** 2


# ---- frames and views, shared with tests/test_gpu_quality.py -----------------------------------------
def frames():
    """name -> HxWx4 uint8, alpha 255.  Two sizes, each a few hundred pixels a side at most."""
    rng = np.random.default_rng(91)
    noise = rng.integers(0, 256, (150, 200, 4), dtype=np.uint8)
    flat = np.empty((120, 160, 4), np.uint8)
    flat[...] = (90, 140, 33, 255)
    yy, xx = np.mgrid[0:112, 0:112]
    checker = np.zeros((112, 112, 4), np.uint8)
    checker[..., :3] = (((xx + yy) & 1) * 255)[..., None]
    out = {"noise": noise, "flat": flat, "checker": checker}
    for f in out.values():
        f[..., 3] = 255
    return out


def views():
    """name -> (frame name, RotatedRect in frame px)."""
    def rr(cx, cy, w, h, rad=0.0):
        return H.RotatedRect(H.Rect.from_center(cx, cy, w, h), rad)
    return {
        "inside": ("noise", rr(100.0, 75.0, 80.0, 80.0)),
        "downsampled": ("noise", rr(100.0, 75.0, 190.0, 140.0)),
        "half_outside": ("noise", rr(0.0, 75.0, 90.0, 90.0)),
        "mostly_inside": ("noise", rr(30.0, 75.0, 80.0, 80.0)),
        "corner": ("noise", rr(195.0, 146.0, 60.0, 60.0)),
        "wholly_outside": ("noise", rr(-300.0, -300.0, 50.0, 50.0)),
        "rotated": ("noise", rr(110.0, 70.0, 70.0, 50.0, 0.6)),
        "flat": ("flat", rr(80.0, 60.0, 64.0, 64.0)),
        "flat_rotated_out": ("flat", rr(150.0, 20.0, 80.0, 80.0, -1.1)),
        "checker": ("checker", rr(56.0, 56.0, 112.0, 112.0)),
    }


GRIDS = [(2, 2), (3, 3), (7, 5), (112, 112)]


def host_view(name):
    fname, r = views()[name]
    f = frames()[fname]
    return f, H.ViewData.full(f.shape[1], f.shape[0]).view(r)


def _same(got, want, ctx):
    assert QR.bits(got) == QR.bits(want), (ctx, got, want)


@pytest.mark.parametrize("grid", GRIDS + [(128, 128)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_face_quality_bits(grid):
    ow, oh = grid
    names = list(views()) if ow * oh <= 49 or grid == (112, 112) else ["inside", "rotated", "half_outside"]
    for name in names:
        frame, view = host_view(name)
        _same(H.face_quality(frame, view, ow, oh), QR.record(frame, QR.oracle_view(H, view), ow, oh), (name, grid))


def test_small_grids_have_no_or_one_interior_pixel():
    frame, view = host_view("inside")
    q = H.face_quality(frame, view, 2, 2)
    assert q["samples"] == 0 and q["sharpness"] == 0.0 and not np.signbit(f32(q["sharpness"])) and q["inside"] == 1.0
    q = H.face_quality(frame, view, 3, 3)
    assert q["samples"] == 1 and q["sharpness"] == 0.0   # one sample has no variance


def test_checkerboard_needs_64_bit_sums():
    """Every Lap = +-1020, so s2 = 12100 * 1040400 > 2^32: a 32-bit final sum fails."""
    frame, view = host_view("checker")
    g = QR.luma_grid(frame, QR.oracle_view(H, view), 112, 112)
    assert set(np.unique(g)) == {0, 255}
    n_in, n, s1, s2 = QR.sums(g)
    assert (n_in, n) == (12544, 12100) and s2 == 12100 * 1040400 > 2 ** 32 and s1 == 0
    q = H.face_quality(frame, view, 112, 112)
    assert q["samples"] == 12100 and q["sharpness"] == 1040400.0


def test_flat_and_outside():
    frame, view = host_view("flat")
    q = H.face_quality(frame, view, 112, 112)
    assert q["sharpness"] == 0.0 and q["samples"] == 12100 and q["inside"] == 1.0 and q["size"] == 64.0
    frame, view = host_view("wholly_outside")
    q = H.face_quality(frame, view, 112, 112)
    assert q["inside"] == 0.0 and q["samples"] == 0 and q["sharpness"] == 0.0
    frame, view = host_view("half_outside")
    q = H.face_quality(frame, view, 112, 112)
    assert 0.4 < q["inside"] < 0.6 and 0 < q["samples"] < 12100
    assert math.isnan(q["frontal"])


# ---- the tiers -----------------------------------------------------------------------------------
def test_tier_logic():
    m = {"size": f32(40), "inside": f32(0.75), "sharpness": f32(100), "frontal": f32(math.nan), "samples": 9}
    assert QR.judge(m)["flags"] == QR.MEASURED | QR.EMBED | QR.LEARN          # -inf skips, even a NaN value
    assert QR.judge(m, (40.0, 0.75, 100.0, -math.inf))["flags"] == 7            # >= passes at equality
    assert QR.judge(m, (40.5, -math.inf, -math.inf, -math.inf))["flags"] == QR.MEASURED | QR.FAIL_SIZE
    r = QR.judge(m, (41.0, 0.8, 101.0, 0.5), rejected_before=6)                   # a NaN value fails
    assert r["flags"] == QR.MEASURED | QR.FAIL_SIZE | QR.FAIL_INSIDE | QR.FAIL_SHARPNESS | QR.FAIL_FRONTAL
    assert r["rejected"] == 7 and QR.judge(m, (41.0,) + QR.SKIP[1:], rejected_before=QR.U32_MAX)["rejected"] == QR.U32_MAX
    held = QR.judge(m, QR.SKIP, (-math.inf, 0.8, -math.inf, -math.inf), rejected_before=3)
    assert held["flags"] == QR.MEASURED | QR.EMBED and held["rejected"] == 0
    # LEARN implies EMBED: a learn tier that passes cannot rescue an embed tier that fails
    assert QR.judge(m, (50.0,) + QR.SKIP[1:], QR.SKIP)["flags"] == QR.MEASURED | QR.FAIL_SIZE


def test_host_tiers_are_the_refs():
    frame, view = host_view("half_outside")
    ov = QR.oracle_view(H, view)
    m = QR.measure(frame, ov, 7, 5)
    pose = np.full(21, 0.25, f32)
    pose.view(np.uint32)[7] = 1
    pose[20] = 0.9
    invalid = pose.copy()
    invalid.view(np.uint32)[7] = 0
    tiers = [QR.SKIP, (float(m["size"]), float(m["inside"]), float(m["sharpness"]), -math.inf),
             (float(m["size"]) + 1, -math.inf, -math.inf, -math.inf), (-math.inf, 0.99, -math.inf, -math.inf),
             (-math.inf, -math.inf, 1e9, -math.inf), (-math.inf, -math.inf, -math.inf, 0.9),
             (-math.inf, -math.inf, -math.inf, 0.95)]
    for p in (None, pose, invalid):
        for e in tiers:
            for l in (None, tiers[3], tiers[6]):
                got = H.face_quality(frame, view, 7, 5, pose=p, embed_tier=H.FaceQualityGate(*e),
                                     learn_tier=None if l is None else H.FaceQualityGate(*l))
                _same(got, QR.record(frame, ov, 7, 5, p, e, l), (e, l))
    assert H.face_quality(frame, view, 7, 5, pose=pose)["frontal"] == f32(0.9)
    assert math.isnan(H.face_quality(frame, view, 7, 5, pose=invalid)["frontal"])
    g = H.FaceQualityGate()
    assert (g.min_size, g.min_inside, g.min_sharpness, g.min_frontal) == QR.SKIP


# ---- the schedule --------------------------------------------------------------------------------
class _Obj:
    def __init__(self, oid):
        self.id, self.pending, self.lm = oid, None, None


class _Timeline:
    """Stands for MultiTrackerRef: objects appear at scripted steps and have landmarks from the step after."""

    def __init__(self, starts):
        self.starts, self.objs, self.k = starts, [], 0

    def step(self, frame, now_ms, injected=()):
        for o in self.objs:
            o.lm = o.pending
        for oid in self.starts.get(self.k, []):
            self.objs.append(_Obj(oid))
        for o in self.objs:
            o.pending = {"landmarks": [(1.0 + o.id, 2.0, 0.0), (3.0 + o.id, 5.0, 0.0)]}
        self.k += 1

    def objects(self):
        return [o for o in self.objs if o.lm is not None]


def test_schedule_with_the_gate():
    """One stream, clock 15 ms a step, identify interval 0.  The "frame" is the step number and the fake
    measure reads an object's sharpness from a script: object 0 is sharp from step 3 on, learn-grade from
    step 5; object 1 (tracked from step 3) is always learn-grade."""
    tl = _Timeline({0: [0], 2: [1]})
    sharp = {0: {1: 5, 2: 5, 3: 50, 4: 50, 5: 500, 6: 5, 7: 500}}
    embedded = []

    def measure(frame, view, pose):
        oid = view
        return {"size": f32(10), "inside": f32(1), "sharpness": f32(sharp.get(oid, {}).get(frame, 500)),
                "frontal": f32(math.nan), "samples": 4}

    def embed(frame, rect):
        e = np.zeros(128, f32)
        e[0] = 100.0 * (rect.tuple()[0] > 2.5) + 0.001 * frame   # the objects are far apart, their looks close
        embedded.append(frame)
        return e

    def make_match(rows, ids):
        def match(e):
            if not rows:
                return QR.IR.NO_MATCH, math.inf
            d = ER.distances(e, rows)
            j = int(np.argmin(d))
            return ids[j], d[j]
        return match

    gal = ER.GalleryRef(8, [], [], 100)
    ref = QR.MultiQualityRef(H, [tl], embed, make_match, gal, embed_tier=(-math.inf, -math.inf, 10.0, -math.inf),
                             learn_tier=(-math.inf, -math.inf, 100.0, -math.inf), measure=measure,
                             crop=lambda lm, frame: int(lm[0][0] - 1.0), interval=0.0, threshold=1.0, refine=True,
                             max_samples=64, enrol=True)
    log = []
    for k in range(8):
        ref.step([k], 15.0 * k, [()])
        log.append({o.id: (q and (q["flags"], q["rejected"]), i and i["embeddings"], i and i["flags"])
                    for o, i, q in ref.objects(0)})
    rej, held, learn = QR.MEASURED | QR.FAIL_SHARPNESS, QR.MEASURED | QR.EMBED, QR.MEASURED | QR.EMBED | QR.LEARN
    # object 0: rejected at steps 1 and 2 (stays due, not embedded: no identity), held back at 3 and 4
    # (embedded, matched against an empty gallery, not enrolled), enrolled at 5, rejected again at 6
    assert [l.get(0) for l in log[1:]] == [
        ((rej, 1), None, None), ((rej, 2), None, None), ((held, 0), 1, 0), ((held, 0), 2, 0),
        ((learn, 0), 3, ER.EVER_KNOWN | ER.ENROLLED), ((rej, 1), 3, ER.EVER_KNOWN | ER.ENROLLED),
        ((learn, 0), 4, ER.EVER_KNOWN | ER.ENROLLED)]
    # object 1: enrolled at its first look, known and refining from then on
    assert log[3][1] == ((learn, 0), 1, ER.EVER_KNOWN | ER.ENROLLED)
    assert [e[1:] for e in ref.events if e[3] == "enrol"] == [(0, 1, "enrol", 0), (0, 0, "enrol", 1)]
    assert [e[0] for e in ref.events if e[3] == "enrol"] == [3, 5]
    assert (ref.measured, ref.rejected, ref.held_back) == (12, 3, 2) and ref.images == 9 == len(embedded)
    # the held-back looks left no trace in the gallery: object 0's row is its step-5 embedding, refined by
    # its step-7 look alone (the rejected step 6 made none)
    assert [r[:3] for r in ref.refined if r[2] == 0] == [(7, 0, 0)]
    assert ref.updates[1] == 1 and gal.ids == [100, 101]
    assert sorted(c[3] for c in ref.cases if c[2] == 0) == ["held"] * 2 + ["learn"] * 2 + ["reject"] * 3


# ---- frontal -------------------------------------------------------------------------------------
def test_frontal_on_the_golden_mesh_views():
    z = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))
    a = H.ProcrustesAnalyzer(PR.canonical_mesh())
    frame, view = host_view("inside")
    for lm, deg in zip(z["landmarks"], z["view_deg"]):
        pose = a.analyze(lm, flip_y=True).pose()
        q = H.face_quality(frame, view, 7, 5, pose=pose)
        print(f"view {deg}: frontal {q['frontal']:.5f}")
        assert q["frontal"] == pose[20] and q["frontal"] >= COS2_5, (deg, q["frontal"])
        gate = H.FaceQualityGate(min_frontal=COS2_5)
        assert H.face_quality(frame, view, 7, 5, pose=pose, embed_tier=gate)["flags"] & QR.LEARN


# ---- refusals ------------------------------------------------------------------------------------
def _qcfg(slots=4, ow=112, oh=112, embed=QR.SKIP, learn=QR.SKIP):
    return _lib.QualityCfg(slots, ow, oh, _lib.QualityTier(*embed), _lib.QualityTier(*learn))


def test_quality_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    assert C.sizeof(_lib.FaceQuality) == 32 and C.sizeof(_lib.QualityCfg) == 44 and _lib.FaceQuality.flags.offset == 16
    assert _lib.EXPORT_QUALITY == 16 and C.sizeof(_lib.MultiExportArgs) == 24 * C.sizeof(C.c_void_p)   # as it was
    p, q = 4096, 8192   # stand for device pointers: none of these calls gets as far as using them
    frame = (_lib.Frame * 1)(_lib.Frame(p, 64, 64, 256))

    def gate(c=_qcfg(), n=8, frames=frame, nf=1, **kw):
        a = dict(state=p, src=p, views=p, pose=None, rin=p, rout=q, due=p, m=None, r=None)
        a.update(kw)
        return lib.zr_identity_quality_async(None if c is None else C.byref(c), frames, nf, a["state"], n, a["src"],
                                             a["views"], a["pose"], a["rin"], a["rout"], a["due"], a["m"], a["r"], None)

    assert gate(c=None) == -1 and gate(frames=None) == -1
    for name in ("state", "src", "views", "rin", "rout", "due"):
        assert gate(**{name: None}) == -1, name
    assert gate(n=0) == -1 and gate(n=(1 << 24) + 4) == -1
    for n, slots in ((8, 0), (8, 65), (8, -1), (8, 3), (9, 4), (130, 64)):
        assert gate(c=_qcfg(slots=slots), n=n) == -1, (n, slots)
    for ow, oh in ((0, 112), (112, 0), (-1, 5), (129, 128), (16385, 1), (1 << 16, 1 << 16)):
        assert gate(c=_qcfg(ow=ow, oh=oh)) == -1, (ow, oh)
    for k in range(4):
        t = list(QR.SKIP)
        t[k] = math.nan
        assert gate(c=_qcfg(embed=t)) == -1 and gate(c=_qcfg(learn=t)) == -1, k
    assert gate(rin=p, rout=p) == -1
    frontal = (-math.inf, -math.inf, -math.inf, 0.5)
    assert gate(c=_qcfg(embed=frontal)) == -1 and gate(c=_qcfg(learn=frontal)) == -1   # no pose records
    assert gate(nf=0) == -1
    assert gate(frames=(_lib.Frame * 1)(_lib.Frame(None, 64, 64, 256))) == -1
    assert gate(frames=(_lib.Frame * 1)(_lib.Frame(p, 0, 64, 256))) == -1

    def mask(n=8, **kw):
        a = dict(of=p, q=p, out=q, held=None)
        a.update(kw)
        return lib.zr_identity_quality_mask_async(n, a["of"], a["q"], a["out"], a["held"], None)

    for name in ("of", "q", "out"):
        assert mask(**{name: None}) == -1, name
    assert mask(n=0) == -1 and mask(n=(1 << 24) + 1) == -1

    img = np.zeros((4, 4, 4), np.uint8)
    hf = _lib.Frame(img.ctypes.data, 4, 4, 16)
    view = (C.c_float * 10)()
    out = _lib.FaceQuality()

    def host(c=_qcfg(ow=3, oh=3), f=hf, v=view, o=out):
        return lib.zr_face_quality_host(None if c is None else C.byref(c), None if f is None else C.byref(f), v,
                                        None, None if o is None else C.byref(o))

    assert host() == 0
    assert host(c=None) == -1 and host(f=None) == -1 and host(v=None) == -1 and host(o=None) == -1
    assert host(c=_qcfg(ow=0, oh=3)) == -1 and host(c=_qcfg(ow=129, oh=128)) == -1
    assert host(c=_qcfg(ow=3, oh=3, embed=(math.nan,) + QR.SKIP[1:])) == -1
    assert host(f=_lib.Frame(None, 4, 4, 16)) == -1
    with pytest.raises(RuntimeError):
        H.face_quality(img, H.ViewData.full(4, 4), 3, 3, pose=np.zeros(20, f32))
