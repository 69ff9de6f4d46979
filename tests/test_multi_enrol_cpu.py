"""Automatic enrolment, the parts that need no GPU:

  * the argument refusals of zr_embed_match_count_async and zr_identity_enrol_async (nothing is
    launched: the pointers are made up);
  * the sequential rule of tests/multi_enrol_ref.py on a hand-written timeline of synthetic embeddings.
"""
import ctypes as C
import math

import numpy as np

from zaru_amd import _lib

import multi_enrol_ref as ER

f32 = np.float32


def _icfg(**kw):
    v = dict(slots=4, num_landmarks=468, aspect_w=1, aspect_h=1, crop_grow=0.4, threshold=math.inf, interval_ms=1000.0)
    v.update(kw)
    return _lib.IdentityCfg(**v)


def test_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    assert C.sizeof(_lib.IdentityState) == 24 and _lib.IdentityState.flags.offset == 12
    p, q = 4096, 8192  # stand for device pointers: none of these calls gets as far as using them

    def match(nq=70, cap=130, dim=128, **kw):
        a = dict(query=p, gallery=q, g=p, valid=p, idx=p, dist=p)
        a.update(kw)
        return lib.zr_embed_match_count_async(a["query"], nq, a["gallery"], cap, a["g"], dim, a["valid"], a["idx"],
                                              a["dist"], None)

    for name in ("query", "gallery", "g", "idx", "dist"):
        assert match(**{name: None}) == -1, name
    assert match(nq=0) == -1 and match(dim=0) == -1 and match(cap=0) == -1
    assert match(nq=2 ** 31) == -1 and match(cap=2 ** 31) == -1 and match(nq=2 ** 25, cap=2 ** 25) == -1

    def enrol(c=_icfg(), n=8, cap=16, dim=128, min_emb=1, **kw):
        a = dict(of=p, sout=q, eout=q, rows=p, ids=p, count=p, next=p, total=p, dropped=p)
        a.update(kw)
        return lib.zr_identity_enrol_async(None if c is None else C.byref(c), n, a["of"], a["sout"], a["eout"],
                                           a["rows"], a["ids"], a["count"], a["next"], cap, dim, min_emb, a["total"],
                                           a["dropped"], None)

    assert enrol(c=None) == -1 and enrol(n=0) == -1 and enrol(n=(1 << 24) + 4) == -1
    for name in ("of", "sout", "eout", "rows", "ids", "count", "next", "total", "dropped"):
        assert enrol(**{name: None}) == -1, name
    for n, slots in ((8, 0), (8, 65), (9, 4)):
        assert enrol(c=_icfg(slots=slots), n=n) == -1, (n, slots)
    assert enrol(c=_icfg(interval_ms=-5.0)) == -1 and enrol(c=_icfg(num_landmarks=0)) == -1
    assert enrol(cap=0) == -1 and enrol(cap=2 ** 31) == -1
    assert enrol(dim=64) == -1 and enrol(dim=0) == -1 and enrol(dim=256) == -1
    assert enrol(min_emb=0) == -1
    assert enrol(eout=q + 4) == -1 and enrol(rows=p + 8) == -1
    # thresholds (NaN, +inf) are settings, not errors: checked on the GPU, where they run


# ---- the rule on a timeline ---------------------------------------------------------------------
def _unit(k, scale=1.0):
    e = np.zeros(128, f32)
    e[k] = scale
    return e


def _item(emb, due=True, row=-1, distance=math.inf, embeddings=1, flags=0):
    return {"due": due, "row": row, "distance": f32(distance), "embeddings": embeddings, "flags": flags,
            "embedding": np.asarray(emb, f32)}


def test_distance_is_the_references_difference():
    """s = s + d * d in order, each operation rounded on its own: against a scalar f32 loop."""
    rng = np.random.default_rng(4)
    a, rows = rng.standard_normal(128).astype(f32), rng.standard_normal((5, 128)).astype(f32)
    got = ER.distances(a, rows)
    for j in range(5):
        s = f32(0)
        for k in range(128):
            d = f32(a[k] - rows[j, k])
            s = f32(s + f32(d * d))
        assert got[j].tobytes() == np.sqrt(s).tobytes()
    assert ER.nearest(np.array([2.0, math.nan, 1.0, 1.0], f32), 10) == (12, f32(1.0))
    assert ER.nearest(np.array([math.nan], f32)) is None and ER.nearest(np.zeros(0, f32)) is None


def test_rule_on_a_timeline():
    p1, p2 = _unit(0), _unit(2, 3.0)
    near_p1 = p1 + _unit(1, 0.25)   # 0.25 from p1
    g = ER.GalleryRef(4, rows=[_unit(9)], ids=[100], next_id=500)
    # step 1: a first-seen face, its duplicate in the same step, a row that was not due, a known row
    a, b, idle, known = _item(p1), _item(near_p1), _item(p2, due=False), _item(_unit(9), row=0, distance=0.0)
    ev = ER.enrol_step([a, b, idle, known], g, 0.5)
    assert ev == [(0, "enrol", 1), (1, "match", 1), (3, "known", 0)]
    assert (a["row"], a["distance"], a["flags"]) == (1, 0.0, ER.EVER_KNOWN | ER.ENROLLED)
    assert (b["row"], b["distance"], b["flags"]) == (1, f32(0.25), ER.EVER_KNOWN)
    assert (idle["row"], idle["flags"]) == (-1, 0) and known["flags"] == ER.EVER_KNOWN
    assert g.ids == [100, 500] and g.next_id == 501 and g.rows[1].tobytes() == p1.tobytes()
    # step 2: the enrolled face drifted past the threshold at its next embedding (the commit left row -1):
    # ever known, so no second person; the duplicate is matched against this call's rows only, and there
    # are none: it stays what the commit made it
    a.update(row=-1, distance=f32(2.0), embeddings=2, embedding=p1 + _unit(5, 2.0))
    assert ER.enrol_step([a, idle], g, 0.5) == [] and len(g.rows) == 2 and a["row"] == -1
    assert a["flags"] == ER.EVER_KNOWN | ER.ENROLLED
    # min_embeddings = 2: not at the first embedding, at the second
    c = _item(p2, embeddings=1)
    assert ER.enrol_step([c], g, 0.5, min_embeddings=2) == [] and c["flags"] == 0
    c["embeddings"] = 2
    assert ER.enrol_step([c], g, 0.5, min_embeddings=2) == [(0, "enrol", 2)] and g.ids[2] == 501
    # a NaN (or inf) in the embedding: no candidate, not counted as dropped
    bad, worse = _item(_unit(3, math.nan)), _item(_unit(3, math.inf))
    assert ER.enrol_step([bad, worse], g, 0.5) == [] and g.dropped == 0
    # capacity 4: one more row, then the next candidate is dropped and stays unknown; a later duplicate of
    # the row appended in this call still matches it
    d, e, d2 = _item(_unit(20)), _item(_unit(21)), _item(_unit(20))
    assert ER.enrol_step([d, e, d2], g, 0.5) == [(0, "enrol", 3), (1, "dropped", -1), (2, "match", 3)]
    assert (e["row"], e["flags"]) == (-1, 0) and g.dropped == 1 and g.enrolled_total == 3 and len(g.rows) == 4
    assert ER.enrol_step([e], g, 0.5) == [(0, "dropped", -1)] and g.dropped == 2


def test_nan_and_infinite_thresholds():
    # NaN: nothing is ever within the threshold, so every eligible object is enrolled, twins included
    g = ER.GalleryRef(8)
    twins = [_item(_unit(1)), _item(_unit(1)), _item(_unit(2))]
    assert [k for _, k, _ in ER.enrol_step(twins, g, math.nan)] == ["enrol"] * 3 and g.ids == [0, 1, 2]
    # +inf with an empty gallery: the first candidate is enrolled, every later one is that person; and the
    # lowest row wins among equal distances
    g = ER.GalleryRef(8, next_id=7)
    items = [_item(_unit(1)), _item(_unit(2)), _item(_unit(3, 100.0))]
    assert ER.enrol_step(items, g, math.inf) == [(0, "enrol", 0), (1, "match", 0), (2, "match", 0)]
    assert items[1]["distance"] == np.sqrt(f32(2.0)) and g.ids == [7]
    g = ER.GalleryRef(8)
    items = [_item(_unit(1)), _item(_unit(2)), _item(_unit(3))]
    ev = ER.enrol_step(items[:2], g, 0.0) + ER.enrol_step(items[2:], g, math.inf)
    assert ev == [(0, "enrol", 0), (1, "enrol", 1), (0, "enrol", 2)]   # rows of earlier calls are the match's business
    g = ER.GalleryRef(8)
    items = [_item(_unit(1)), _item(_unit(2)), _item(_unit(3))]
    ER.enrol_step(items[:2], g, 0.0)
    third = [_item(_unit(4)), _item(_unit(1, 0.0))]   # the zero vector: 1.0 from row 2 only (this call's)
    assert ER.enrol_step(third, g, 1.0) == [(0, "enrol", 2), (1, "match", 2)]
    # equal distances: the lowest row
    g = ER.GalleryRef(8)
    items = [_item(_unit(1)), _item(_unit(2)), _item(_unit(1, 0.0))]
    assert ER.enrol_step(items, g, 1.0) == [(0, "enrol", 0), (1, "enrol", 1), (2, "match", 0)]
    assert items[2]["distance"] == f32(1.0)
