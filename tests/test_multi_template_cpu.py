"""Identities that learn, the parts that need no GPU:

  * the argument refusals of zr_identity_blend_async and zr_identity_refine_async (nothing is
    launched: the pointers are made up), and the ABI sizes they leave as they were;
  * tests/multi_template_ref.py's blend and refine on hand-written timelines.
"""
import ctypes as C
import math

import numpy as np

from zaru_amd import _lib

import multi_template_ref as TR

f32 = np.float32


def _icfg(**kw):
    v = dict(slots=4, num_landmarks=468, aspect_w=1, aspect_h=1, crop_grow=0.4, threshold=math.inf, interval_ms=1000.0)
    v.update(kw)
    return _lib.IdentityCfg(**v)


def test_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    assert C.sizeof(_lib.IdentityState) == 24 and _lib.IdentityState.flags.offset == 12
    assert C.sizeof(_lib.ExportIdentity) == 16 and C.sizeof(_lib.IdentityCfg) == 32
    p, q, r = 4096, 8192, 16384  # stand for device pointers: none of these calls gets as far as using them

    def blend(c=_icfg(), n=8, cap=8, **kw):
        a = dict(of=p, sout=p, eout=p, dense=q, query=r)
        a.update(kw)
        return lib.zr_identity_blend_async(None if c is None else C.byref(c), n, a["of"], a["sout"], a["eout"],
                                           a["dense"], cap, a["query"], None)

    assert blend(c=None) == -1 and blend(n=0) == -1 and blend(n=(1 << 24) + 4) == -1
    for name in ("of", "sout", "eout", "dense", "query"):
        assert blend(**{name: None}) == -1, name
    for n, slots in ((8, 0), (8, 65), (9, 4)):
        assert blend(c=_icfg(slots=slots), n=n) == -1, (n, slots)
    assert blend(c=_icfg(interval_ms=-5.0)) == -1 and blend(c=_icfg(num_landmarks=0)) == -1
    assert blend(c=_icfg(crop_grow=math.nan)) == -1 and blend(c=_icfg(aspect_w=0)) == -1
    assert blend(cap=0) == -1
    assert blend(query=q) == -1                       # in place: the raw samples would be lost
    assert blend(eout=p + 4) == -1 and blend(dense=q + 4) == -1 and blend(query=r + 4) == -1

    def refine(c=_icfg(), n=8, cap=16, dim=128, max_samples=64, thr=0.5, **kw):
        a = dict(of=p, sout=p, dense=q, rows=r, upd=p, count=p, total=p)
        a.update(kw)
        return lib.zr_identity_refine_async(None if c is None else C.byref(c), n, a["of"], a["sout"], a["dense"],
                                            a["rows"], a["upd"], a["count"], cap, dim, max_samples, thr, a["total"], None)

    assert refine(c=None) == -1 and refine(n=0) == -1 and refine(n=(1 << 24) + 4) == -1
    for name in ("of", "sout", "dense", "rows", "upd", "count"):
        assert refine(**{name: None}) == -1, name
    for n, slots in ((8, 0), (8, 65), (9, 4)):
        assert refine(c=_icfg(slots=slots), n=n) == -1, (n, slots)
    assert refine(c=_icfg(interval_ms=-5.0)) == -1 and refine(c=_icfg(num_landmarks=0)) == -1
    assert refine(cap=0) == -1 and refine(cap=2 ** 31) == -1
    assert refine(dim=64) == -1 and refine(dim=0) == -1 and refine(dim=256) == -1
    assert refine(max_samples=0) == -1 and refine(max_samples=1) == -1
    assert refine(dense=q + 4) == -1 and refine(rows=r + 8) == -1
    # thresholds (NaN, +-inf) and a NULL total are settings, not errors: checked on the GPU, where they run


# ---- the reference on timelines -------------------------------------------------------------------
def _item(sample, row=0, distance=0.25, due=True):
    return {"due": due, "row": row, "distance": f32(distance), "sample": np.asarray(sample, f32)}


def test_update_rounds_every_operation_on_its_own():
    rng = np.random.default_rng(3)
    m, e = rng.standard_normal(128).astype(f32), rng.standard_normal(128).astype(f32)
    got = TR.update(m, e, 3)
    for k in range(128):
        d = f32(e[k] - m[k])
        assert got[k].tobytes() == f32(m[k] + f32(d / f32(3))).tobytes()
    assert got.dtype == f32
    # a fused or a double-precision evaluation differs somewhere on 128 random floats
    wide = (m.astype(np.float64) + (e.astype(np.float64) - m.astype(np.float64)) / 3.0).astype(f32)
    assert wide.tobytes() != got.tobytes()


def test_blend_timeline():
    rng = np.random.default_rng(5)
    looks = rng.standard_normal((7, 128)).astype(f32)
    cap = 4
    # the first look is taken verbatim, -0 and a NaN's payload included
    first = looks[0].copy()
    first[3] = f32(-0.0)
    odd = first.copy()
    odd.view(np.uint32)[9] = 0x7FC12345
    assert TR.blend(np.zeros(128, f32), first, 0, cap).tobytes() == first.tobytes()
    assert TR.blend(np.zeros(128, f32), odd, 0, cap).tobytes() == odd.tobytes()
    assert TR.blend(first, odd, 3, cap).tobytes() == odd.tobytes()        # e not finite, c > 0: verbatim
    assert TR.blend(odd, first, 3, cap).tobytes() == first.tobytes()      # t not finite: the template restarts
    inf = looks[1].copy()
    inf[100] = -math.inf
    assert TR.blend(inf, first, 2, cap).tobytes() == first.tobytes()
    # -0 survives only the verbatim path: 0 + (-0 - 0) / w is +0
    assert TR.blend(np.zeros(128, f32), first, 1, cap)[3].tobytes() == f32(0.0).tobytes()
    # below the cap the template is the mean of the looks so far; at the cap the weight stays 1 / cap
    t = looks[0]
    for c in range(1, 7):
        nxt = TR.blend(t, looks[c], c, cap)
        if c + 1 <= cap:
            mean = looks[:c + 1].astype(np.float64).mean(axis=0)
            assert np.abs(nxt - mean).max() < 1e-6, c
        assert nxt.tobytes() == TR.update(t, looks[c], min(c + 1, cap)).tobytes()
        t = nxt
    assert TR.blend(t, looks[0], 0xFFFFFFFF, cap).tobytes() == TR.update(t, looks[0], cap).tobytes()
    assert TR.blend(t, looks[0], 0xFFFFFFFF, 0xFFFFFFFF).tobytes() == TR.update(t, looks[0], 0xFFFFFFFF).tobytes()
    # cap 1 is the formula with w = 1, not a copy
    assert TR.blend(t, looks[0], 5, 1).tobytes() == TR.update(t, looks[0], 1).tobytes()


def test_refine_timeline():
    rng = np.random.default_rng(6)
    first = rng.standard_normal(128).astype(f32)
    samples = rng.standard_normal((9, 128)).astype(f32)
    # below the cap: the f64 mean of the first value and the samples, within 1e-6
    rows, upd = [first.copy(), first.copy()], [0, 0]
    for j in range(5):
        done = TR.refine([_item(samples[j])], rows, upd, 2, 64, 0.5)
        assert done == [(0, 0, j + 2)] and upd == [j + 1, 0]
        mean = np.concatenate([first[None], samples[:j + 1]]).astype(np.float64).mean(axis=0)
        assert np.abs(rows[0] - mean).max() < 1e-6, j
    assert rows[1].tobytes() == first.tobytes()
    # at the cap the weight stays 1 / max_samples, and the count goes on
    rows, upd = [first.copy()], [0]
    for j in range(6):
        before = rows[0].copy()
        (_, _, w), = TR.refine([_item(samples[j])], rows, upd, 1, 3, 0.5)
        assert w == min(j + 2, 3) and upd[0] == j + 1
        assert rows[0].tobytes() == TR.update(before, samples[j], w).tobytes()
    # the count saturates, the weight is max_samples' whatever the count
    rows, upd = [first.copy(), first.copy()], [0xFFFFFFFE, 0xFFFFFFFF]
    done = TR.refine([_item(samples[0], 0), _item(samples[1], 1), _item(samples[2], 0)], rows, upd, 2, 2 ** 32 - 1, 0.5)
    assert [w for _, _, w in done] == [2 ** 32 - 1] * 3 and upd == [0xFFFFFFFF, 0xFFFFFFFF]
    # who contributes
    rows, upd = [first.copy() for _ in range(4)], [0] * 4
    bad = samples[3].copy()
    bad[7] = math.nan
    items = [_item(samples[0], due=False), _item(samples[0], row=-1), _item(samples[0], row=3),   # past the count
             _item(samples[0], row=4), _item(samples[0], distance=0.75), _item(samples[1], distance=0.5),
             _item(samples[2], distance=math.nan), _item(bad), _item(samples[4], row=2, distance=0.0)]
    assert TR.refine(items, rows, upd, 3, 64, 0.5) == [(5, 0, 2), (8, 2, 2)] and upd == [1, 0, 1, 0]
    assert rows[1].tobytes() == first.tobytes() and rows[3].tobytes() == first.tobytes()
    keep = [r.copy() for r in rows]
    assert TR.refine(items, rows, upd, 3, 64, math.nan) == []                  # NaN: nobody
    assert [i for i, _, _ in TR.refine(items, rows, upd, 3, 64, math.inf)] == [4, 5, 8]   # +inf: every known, a NaN distance never
    rows = keep
    assert [i for i, _, _ in TR.refine(items, rows, upd, 3, 64, 0.0)] == [8]   # distance 0 at threshold 0 contributes
    assert TR.refine(items, rows, upd, -5, 64, math.inf) == [] and TR.refine(items, rows, upd, 0, 64, math.inf) == []


def test_order_of_the_last_two_contributors_shows():
    """70 contributors on one row: the chain with its last two swapped differs in bits at every cap, so
    a test built on such a chain fails on a wrong order -- while a swap in the middle may not show."""
    rng = np.random.default_rng(7)
    first = rng.standard_normal(128).astype(f32)
    samples = rng.standard_normal((70, 128)).astype(f32)

    def chain(order, max_samples):
        rows, upd = [first.copy()], [0]
        TR.refine([_item(samples[j]) for j in order], rows, upd, 1, max_samples, 0.5)
        assert upd == [70]
        return rows[0]

    straight, swapped = list(range(70)), list(range(68)) + [69, 68]
    for max_samples in (2, 3, 32, 2 ** 20):
        a, b = chain(straight, max_samples), chain(swapped, max_samples)
        differing = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        print("max_samples", max_samples, "floats that differ", differing)
        assert differing > 0, max_samples
