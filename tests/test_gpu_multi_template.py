"""Identities that learn on the device: zr_identity_blend_async, zr_identity_refine_async, Gallery's update
counts, DeviceMultiTracker.set_identity_smoothing / set_gallery_refinement, every comparison bit for bit
against tests/multi_template_ref.py:

  * the two kernels alone, on synthetic states;
  * the loop against MultiTemplateRef at every step, stream and object: smoothing alone, refinement
    alone, both with enrolment;
  * itself with the setters never called, or set and cleared (no bit may move).

The loop runs tests/test_gpu_multi_enrol.py's script: streams 0 and 1 see the same frames and the same
injected detections, so their objects embed to the same bits and are same-step contributors to one row.
"""
import ctypes as C
import math

import numpy as np
import pytest

import multi_enrol_ref as ER
import multi_identity_ref as IR
import multi_template_ref as TR
import multi_tracker_ref as MR
import test_gpu_multi_enrol as TE
import test_gpu_multi_identity as TI
from test_gpu_multi_enrol import H, embed, frames, model, setup  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
S, K, CLOCK, STEPS, FW, FH = TE.S, TE.K, TE.CLOCK, TE.STEPS, TE.FW, TE.FH
GALLERY_IDS, FIRST_ID, INTERVAL = TE.GALLERY_IDS, TE.FIRST_ID, TE.INTERVAL
CAP, MAX_SAMPLES, MIN_EMB = 2, 3, 2
SENTINEL = np.array([0xA5A5A5A5], np.uint32).view(f32)[0]   # a NaN with a payload: no arithmetic makes it


def _cfg(threshold=math.inf, slots=4):
    from zaru_amd import _lib
    return _lib.IdentityCfg(slots, 468, 1, 1, 0.4, threshold, 1000.0)


# ---- the blend kernel alone ------------------------------------------------------------------------
def _blend(st, emb, due_of, dense, cap):
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    n = len(st)
    sentinel = np.full((n, 128), SENTINEL, f32)
    d_st, d_emb, d_of, d_dense, d_q = b(st), b(emb), b(due_of), b(dense), b(sentinel)
    cfg = _cfg()
    _lib.check(lib.zr_identity_blend_async(C.byref(cfg), n, d_of.ptr, d_st.ptr, d_emb.ptr, d_dense.ptr, cap, d_q.ptr,
                                           None))
    _lib.synchronize()
    want = sentinel.copy()
    for i in range(n):
        k = int(due_of[i])
        if 0 <= k < n:
            want[k] = TR.blend(emb[i], dense[k], int(st["embeddings"][i]), cap)
    got = d_q.download((n, 128), f32)
    for k in range(n):
        assert got[k].tobytes() == want[k].tobytes(), ("query row", k)
    assert d_dense.download((n, 128), f32).tobytes() == dense.tobytes(), "the raw samples are only read"
    assert d_emb.download((n, 128), f32).tobytes() == emb.tobytes() and d_st.download((n,), st.dtype).tobytes() == st.tobytes()
    return got, want, sentinel


@pytest.mark.parametrize("cap", [1, 2, 8])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_blend_small(variant, cap):
    """n = 8 (2 x 4), d_due_of not the identity map.
    a: not due; c = 0 with a -0 in e; c = 0 with a NaN in e; t with an inf; e with a NaN and c > 0; c = 1, 2,
       0xffffffff.
    b: c = cap - 1, cap, cap + 5; an out-of-range d_due_of (n: not due); c = 0xfffffffe; both t and e not finite;
       c = 3; c = 0 with finite floats."""
    rng = np.random.default_rng(20 + cap)
    n = 8
    emb, dense = rng.standard_normal((n, 128)).astype(f32), rng.standard_normal((n, 128)).astype(f32)
    st = TE._states(n)
    if variant == "a":
        due_of = np.array([-1, 3, 0, 6, 1, 7, 2, 5], np.int32)
        st["embeddings"] = [4, 0, 0, 2, 3, 1, 2, 0xFFFFFFFF]
        dense[3, 17] = f32(-0.0)
        dense[0].view(np.uint32)[40] = 0xFFC00123   # a NaN with a sign and a payload
        emb[3, 127] = math.inf
        dense[1, 0] = math.nan
    else:
        due_of = np.array([5, 4, 7, n, 0, 2, 6, 1], np.int32)
        st["embeddings"] = [cap - 1, cap, cap + 5, 2, 0xFFFFFFFE, 2, 3, 0]
        emb[5, 64], dense[2, 65] = -math.inf, math.nan
        dense[5, 1] = f32(-0.0)   # c = cap - 1 (0 when cap = 1: verbatim, -0 kept)
    got, want, sentinel = _blend(st, emb, due_of, dense, cap)
    free = sorted(set(range(n)) - {int(k) for k in due_of if 0 <= k < n})
    assert free and all(got[k].tobytes() == sentinel[k].tobytes() for k in free)
    if variant == "a":
        assert got[3].tobytes() == dense[3].tobytes() and np.signbit(got[3, 17])       # c = 0: verbatim
        assert got[0].tobytes() == dense[0].tobytes() and got[6].tobytes() == dense[6].tobytes()
        assert got[1].tobytes() == dense[1].tobytes()                                   # e not finite, c > 0
        assert np.isfinite(got[7]).all() and (cap == 1 or got[7].tobytes() != dense[7].tobytes())   # c = 1: blended
        assert got[5].tobytes() == TR.update(emb[7], dense[5], cap).tobytes()           # c = 0xffffffff: w = cap


def test_blend_past_a_wavefront_of_rows():
    """n = 132 (33 x 4), 70 due rows scattered, their packed images a permutation."""
    rng = np.random.default_rng(23)
    n, nd = 132, 70
    emb, dense = rng.standard_normal((n, 128)).astype(f32), rng.standard_normal((n, 128)).astype(f32)
    st = TE._states(n)
    st["embeddings"] = rng.integers(0, 12, n)
    due_of = np.full(n, -1, np.int32)
    due_of[rng.choice(n, nd, replace=False)] = rng.permutation(n)[:nd]   # packed images anywhere in [0, n)
    assert (due_of[due_of >= 0] != np.nonzero(due_of >= 0)[0]).any()
    got, want, sentinel = _blend(st, emb, due_of, dense, 8)
    used = set(int(k) for k in due_of if k >= 0)
    assert len(used) == nd and all(got[k].tobytes() == sentinel[k].tobytes() for k in range(n) if k not in used)


# ---- the refine kernel alone -----------------------------------------------------------------------
def _items(st, due_of, dense):
    n = len(st)
    return [{"due": bool(0 <= due_of[i] < n), "row": int(st["row"][i]), "distance": st["distance"][i],
             "sample": dense[due_of[i]] if 0 <= due_of[i] < n else None} for i in range(n)]


def _refine(st, due_of, dense, grows, upd, count, max_samples, threshold, total=True):
    """The kernel on device copies, and the oracle on the same data: the whole gallery allocation, the counts
    and the total compared as bytes.  Returns the oracle's contributions and rows."""
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    n, capacity = len(st), len(grows)
    upd = np.asarray(upd, np.uint32)
    d_st, d_of, d_dense, d_rows, d_upd = b(st), b(due_of), b(dense), b(grows), b(upd)
    d_count = b(np.array([count], np.int32))
    d_total = b(np.array([1000], np.uint64)) if total else None
    cfg = _cfg()
    _lib.check(lib.zr_identity_refine_async(C.byref(cfg), n, d_of.ptr, d_st.ptr, d_dense.ptr, d_rows.ptr, d_upd.ptr,
                                            d_count.ptr, capacity, 128, max_samples, threshold,
                                            d_total.ptr if total else None, None))
    _lib.synchronize()
    want_rows, want_upd = grows.copy(), [int(u) for u in upd]
    done = TR.refine(_items(st, due_of, dense), want_rows, want_upd, count, max_samples, threshold)
    got_rows = d_rows.download((capacity, 128), f32)
    for r in range(capacity):
        assert got_rows[r].tobytes() == want_rows[r].tobytes(), ("gallery row", r)
    assert d_upd.download((capacity,), np.uint32).tolist() == want_upd, "update counts"
    if total:
        assert d_total.download((1,), np.uint64)[0] == 1000 + len(done)
    assert d_st.download((n,), st.dtype).tobytes() == st.tobytes(), "the states are only read"
    assert d_dense.download((n, 128), f32).tobytes() == dense.tobytes() and d_count.download((1,), np.int32)[0] == count
    return done, want_rows, want_upd


def _gallery_alloc(rng, capacity):
    return rng.standard_normal((capacity, 128)).astype(f32)


@pytest.mark.parametrize("threshold", [0.5, math.nan, math.inf, 0.0])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_refine_small(variant, threshold):
    """n = 8 (2 x 4), capacity 6, count 4.
    a: not due; row -1; row >= count; row >= capacity; distance above, equal to and below 0.5; a NaN distance.
    b: a non-finite sample (leading its row), a second contributor to that row; distance exactly 0; an
       out-of-range d_due_of; row < -1; a third contributor; a row of its own; an inf sample."""
    rng = np.random.default_rng(31)
    n = 8
    dense, grows = rng.standard_normal((n, 128)).astype(f32), _gallery_alloc(rng, 6)
    st = TE._states(n, row=0, distance=0.25)
    if variant == "a":
        due_of = np.array([-1, 2, 0, 5, 1, 7, 3, 6], np.int32)
        st["row"] = [0, -1, 4, 6, 1, 1, 2, 2]
        st["distance"][4:] = [0.75, 0.5, 0.25, math.nan]
        want = {0.5: [5, 6], math.inf: [4, 5, 6], 0.0: []}
    else:
        due_of = np.array([4, 2, 0, n, 1, 7, 3, 6], np.int32)
        st["row"] = [3, 3, 1, 0, -2, 3, 2, 2]
        st["distance"][2] = 0.0
        dense[4, 5], dense[6, 99] = math.nan, math.inf
        want = {0.5: [1, 2, 5, 6], math.inf: [1, 2, 5, 6], 0.0: [2]}
    done, rows, upd = _refine(st, due_of, dense, grows, [0, 5, 1, 2, 9, 9], 4, 64, threshold)
    assert [i for i, _, _ in done] == ([] if math.isnan(threshold) else want[threshold])


@pytest.mark.parametrize("total", [True, False])
def test_refine_nothing_eligible_writes_nothing(total):
    """Every row due, none eligible: the gallery allocation and the counts keep their bytes (compared in
    _refine, rows past the count included)."""
    rng = np.random.default_rng(32)
    n = 8
    dense, grows = rng.standard_normal((n, 128)).astype(f32), _gallery_alloc(rng, 6)
    grows[4:] = SENTINEL
    st = TE._states(n, row=1, distance=0.75)
    st["row"][:3] = [-1, 4, 7]
    dense[2, 3] = math.nan
    st["distance"][5] = 0.25   # row 5 (packed image 2): eligible but for its sample
    done, _, _ = _refine(st, np.arange(n, dtype=np.int32)[::-1].copy(), dense, grows, [3, 0xFFFFFFFF, 0, 0, 7, 7], 4, 2,
                         0.5, total)
    assert done == []


def test_refine_a_chain_longer_than_a_wavefront():
    """n = 132, capacity 130, count 65, max_samples 2^20: 70 contributors to row 7 interleaved with
    contributors to rows 0, 13, 31, 63 and 64, d_due_of a permutation.  The reference with row 7's last two
    contributors swapped differs, so a kernel that applied them in another order fails."""
    rng = np.random.default_rng(33)
    n, capacity, count, big = 132, 130, 65, 2 ** 20
    dense, grows = rng.standard_normal((n, 128)).astype(f32), _gallery_alloc(rng, capacity)
    due_of = rng.permutation(n).astype(np.int32)
    st = TE._states(n, row=-1, distance=0.25)
    where = np.sort(rng.choice(n, 70, replace=False))
    st["row"][where] = 7
    others = np.setdiff1d(np.arange(n), where)
    st["row"][others] = np.resize(np.array([0, 13, 31, 63, 64, 65, -1]), len(others))   # 65: past the count
    assert where[-1] - where[0] > 64 and (np.diff(where) > 1).any()
    upd = np.zeros(capacity, np.uint32)
    items = _items(st, due_of, dense)
    a, b = int(where[-2]), int(where[-1])
    swapped = [dict(it) for it in items]
    swapped[a]["sample"], swapped[b]["sample"] = items[b]["sample"], items[a]["sample"]
    straight_rows, swapped_rows = grows.copy(), grows.copy()
    TR.refine(items, straight_rows, [0] * capacity, count, big, 0.5)
    TR.refine(swapped, swapped_rows, [0] * capacity, count, big, 0.5)
    differing = int((straight_rows[7].view(np.uint32) != swapped_rows[7].view(np.uint32)).sum())
    print("floats of row 7 that differ with the last two contributors swapped:", differing)
    assert differing > 0
    done, rows, got_upd = _refine(st, due_of, dense, grows, upd, count, big, 0.5)
    assert got_upd[7] == 70 and sum(1 for _, r, _ in done if r == 7) == 70
    assert {r for _, r, _ in done} == {0, 7, 13, 31, 63, 64} and got_upd[65] == 0


@pytest.mark.parametrize("max_samples", [2, 3, 64])
def test_refine_update_counts(max_samples):
    """Six rows whose counts start at 0, 1, max_samples - 2, max_samples, 0xfffffffe and 0xffffffff, two
    contributors each (n = 12)."""
    rng = np.random.default_rng(34)
    n = 12
    dense, grows = rng.standard_normal((n, 128)).astype(f32), _gallery_alloc(rng, 8)
    st = TE._states(n, distance=0.25)
    st["row"] = np.arange(n) % 6
    start = [0, 1, max_samples - 2, max_samples, 0xFFFFFFFE, 0xFFFFFFFF, 11, 12]
    done, rows, upd = _refine(st, rng.permutation(n).astype(np.int32), dense, grows, start, 6, max_samples, 0.5)
    assert upd == [2, 3, max_samples, max_samples + 2, 0xFFFFFFFF, 0xFFFFFFFF, 11, 12]
    assert [w for _, _, w in done] == [min(u + 2, max_samples) for u in start[:6]] + \
        [min(min(u + 1, 0xFFFFFFFF) + 2, max_samples) for u in start[:6]]


@pytest.mark.parametrize("distinct", [False, True])
def test_refine_1024_rows(distinct):
    """n = 1024: all on one gallery row (one chain of 1024), or on 1,024 rows of their own."""
    rng = np.random.default_rng(35)
    n = 1024
    dense, grows = rng.standard_normal((n, 128)).astype(f32), _gallery_alloc(rng, n)
    st = TE._states(n, row=517, distance=0.25)
    if distinct:
        st["row"] = rng.permutation(n)
    done, rows, upd = _refine(st, rng.permutation(n).astype(np.int32), dense, grows, np.zeros(n, np.uint32), n, 64, 0.5)
    assert len(done) == n and (upd == [1] * n if distinct else upd[517] == n and sum(upd) == n)


# ---- the loop against the oracle -------------------------------------------------------------------
def _make_match(H):
    return lambda rows, ids: IR.host_match(TI._gallery(H, rows, ids))


def _oracle_run(H, frames, embed, rows, ids, threshold, capacity, cap=1, refine=None, enrol=False, steps=STEPS):
    """refine: None or (max_samples, update_threshold)."""
    trackers = []
    for s in range(S):
        t = MR.MultiTrackerRef(H, "face", "facemesh", K)
        t.loss, t.interval = -1.0, 40.0
        trackers.append(t)
    gal = ER.GalleryRef(capacity, rows, ids, FIRST_ID)
    ref = TR.MultiTemplateRef(H, trackers, embed, _make_match(H), gal, interval=INTERVAL, threshold=threshold,
                              template_cap=cap, refine=refine is not None, max_samples=refine[0] if refine else 64,
                              update_threshold=refine[1] if refine else math.nan, enrol=enrol, min_embeddings=MIN_EMB)
    out = {"track": [], "identity": [], "gallery": gal, "ref": ref}
    for k in range(steps):
        ref.step([frames[s][k] for s in range(S)], CLOCK * k,
                 [[TI._det(H, d) for d in dets] for dets in TE._injected(k)])
        out["track"].append([TI._track_record(
            [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
              "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in trackers[s].objects()],
            len(trackers[s].objs), trackers[s].pending) for s in range(S)])
        out["identity"].append([[(o.id, TE._record(i, i and i["flags"] & ER.ENROLLED)) for o, i in ref.objects(s)]
                                for s in range(S)])
    return out


def _tracker(H, model, gallery, threshold, cap=None, refine=None, enrol=False, first_id=FIRST_ID):
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    _settings(dev, model, gallery, threshold, cap, refine, enrol, first_id)
    return dev


def _settings(dev, model, gallery, threshold, cap, refine, enrol, first_id=FIRST_ID):
    dev.set_recognition(model, gallery)
    dev.set_identify_interval(INTERVAL)
    dev.set_identity_threshold(threshold)
    if cap is not None:
        dev.set_identity_smoothing(cap)
    if refine is not None:
        dev.set_gallery_refinement(gallery, refine[0], refine[1])
    if enrol:
        dev.set_enrolment(gallery, first_id, MIN_EMB)


def _steps(H, dev, frames, first, last, out=None, bufs=None):
    from zaru_amd._lib import DeviceBuffer
    out = out or {"track": [], "identity": [], "dev": dev, "bufs": {}}
    fb = FH * FW * 4
    for k in range(first, last):
        out["bufs"][k] = DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)]))
        for s, dets in enumerate(TE._injected(k)):
            if dets:
                dev.inject_detections(s, [TI._det(H, d) for d in dets])
        dev.step([(out["bufs"][k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)], CLOCK * k)
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        objs = [dev.objects(s) for s in range(S)]
        out["track"].append([TI._track_record(
            [{"id": o["id"], "rect": o["view_rect"].rect().tuple(), "angle": o["view_rect"].rotation_radians(),
              "landmarks": o["landmarks"], "confidence": o["confidence"]} for o in objs[s]], counts[s], pend[s])
            for s in range(S)])
        out["identity"].append([[(o["id"], TE._record(o["identity"], o["identity"] and o["identity"]["enrolled"]))
                                 for o in objs[s]] for s in range(S)])
    return out


def _reserved(H, rows, capacity):
    g = TI._gallery(H, rows, GALLERY_IDS)
    g.reserve(capacity)
    return g


def _gate(refined):
    """An update threshold that gates out the contributions with the largest distance of the last step that
    has any, and keeps every smaller distance: half way between that distance and the next one below it."""
    last = max(k for k, *_ in refined)
    top = max(d for k, *_, d in refined if k == last)
    below = max(d for *_, d in refined if d < top)
    return float(f32(0.5 * (top + below)))


@pytest.fixture(scope="module")
def plan(H, frames, embed):
    """Thresholds from plain oracle runs, as test_gpu_multi_enrol's setup chooses its own.  Every distance
    between two different raw embeddings of the script (or the gallery's rows) lies in [lo, hi].  A template
    of two looks is within hi / 2 of either; the identity threshold sits half way between hi / 2 and lo, so
    a first look is a stranger to every row and a template stays with its own.  The update thresholds come
    from trial runs with the update threshold at the identity threshold."""
    plain = _oracle_run(H, frames, embed, [], [], math.inf, 64)
    embs = {}
    for k in range(STEPS):
        for s in range(S):
            for _, rec in plain["identity"][k][s]:
                if rec is not None:
                    embs.setdefault(rec[3], (k, s))
    rng = np.random.default_rng(79)
    first = next(rec for _, rec in plain["identity"][1][2] if rec is not None)
    rows = np.stack([np.frombuffer(first[3], f32), rng.standard_normal(128).astype(f32),
                     rng.standard_normal(128).astype(f32)])
    pts = np.concatenate([np.stack([np.frombuffer(e, f32) for e in embs]), rows[1:]])
    dist = [np.delete(ER.distances(pts[i], pts), i) for i in range(len(pts) - 2)]
    lo, hi = min(float(d.min()) for d in dist), max(float(d[:len(embs) - 1].max()) for d in dist)
    print("raw embeddings", len(embs), "smallest distance", lo, "largest", hi)
    assert lo > 0 and len(embs) >= 12 and hi / 2 < lo, (lo, hi, len(embs))
    threshold = float(f32(0.5 * (hi / 2 + lo)))
    both = dict(rows=rows, ids=GALLERY_IDS, threshold=threshold, capacity=16, cap=CAP, enrol=True)
    trial = _oracle_run(H, frames, embed, refine=(MAX_SAMPLES, math.nan), **both)
    alone = dict(rows=rows, ids=GALLERY_IDS, threshold=math.inf, capacity=16)   # every object known: all contribute
    trial_alone = _oracle_run(H, frames, embed, refine=(MAX_SAMPLES, math.inf), **alone)
    return {"smooth": dict(rows=rows, ids=GALLERY_IDS, threshold=threshold, capacity=16, cap=CAP),
            "refine": dict(alone, refine=(MAX_SAMPLES, _gate(trial_alone["ref"].refined))),
            "both": dict(both, refine=(MAX_SAMPLES, _gate(trial["ref"].refined)))}


@pytest.fixture(scope="module")
def oracles(H, frames, embed, plan):
    return {mode: _oracle_run(H, frames, embed, **kw) for mode, kw in plan.items()}


def _device_run(H, frames, model, kw, steps=STEPS):
    g = _reserved(H, kw["rows"], kw["capacity"])
    dev = _tracker(H, model, g, kw["threshold"], kw.get("cap"), kw.get("refine"), kw.get("enrol", False))
    out = _steps(H, dev, frames, 0, steps)
    out["gallery"] = g
    return out


@pytest.fixture(scope="module")
def devices(H, frames, model, plan):
    return {mode: _device_run(H, frames, model, kw) for mode, kw in plan.items()}


def test_script_contains_the_events(oracles, plan):
    for mode in ("smooth", "refine", "both"):
        ref = oracles[mode]["ref"]
        print(mode, {k: v for k, v in plan[mode].items() if k != "rows"})
        print(" refined", ref.refined, "\n gated", ref.gated, "\n blended", ref.blended, "\n events", ref.events)
    for mode in ("refine", "both"):
        ref = oracles[mode]["ref"]
        assert ref.refined and ref.refined_total == len(ref.refined)
        # a same-step pair on one row: streams 0 and 1, one after the other
        steps_rows = [(k, r) for k, s, _, r, _, _ in ref.refined]
        pairs = [(k, r) for k, s, _, r, _, _ in ref.refined if s == 1 and (k, r) in
                 {(k2, r2) for k2, s2, _, r2, _, _ in ref.refined if s2 == 0}]
        assert pairs, steps_rows
        # known, but gated out by the update threshold
        assert ref.gated
        # a row that reaches max_samples, and goes on at that weight
        ws = [w for _, _, _, r, w, _ in ref.refined if r == pairs[0][1]] if mode == "both" else \
            [w for *_, w, _ in ref.refined]
        assert MAX_SAMPLES in ws and max(ref.updates) >= MAX_SAMPLES - 1
    for mode in ("smooth", "both"):
        ref = oracles[mode]["ref"]
        assert any(c >= CAP and w == CAP for *_, c, w in ref.blended), ref.blended   # the cap caps: c + 1 > cap
    ref = oracles["both"]["ref"]
    enrolled = [(k, s, oid) for k, s, oid, kind, _ in ref.events if kind == "enrol"]
    assert enrolled and all((k, s, oid, MIN_EMB - 1, 2) in ref.blended for k, s, oid in enrolled)   # a template of two looks
    assert any(kind == "match" and s == 1 for _, s, _, kind, _ in ref.events)
    assert not oracles["smooth"]["ref"].refined and not oracles["refine"]["ref"].blended


@pytest.mark.parametrize("mode", ["smooth", "refine", "both"])
def test_loop_against_the_oracle(mode, oracles, devices):
    oracle, device = oracles[mode], devices[mode]
    compared = 0
    for k in range(STEPS):
        for s in range(S):
            assert device["track"][k][s] == oracle["track"][k][s], ("tracking", k, s)
            w, g = oracle["identity"][k][s], device["identity"][k][s]
            assert [i for i, _ in g] == [i for i, _ in w], ("ids", k, s)
            for (oid, wr), (_, gr) in zip(w, g):
                assert (gr is None) == (wr is None), ("identified", k, s, oid)
                if wr is None:
                    continue
                for field, name in enumerate(("id", "distance", "embeddings", "embedding", "enrolled")):
                    assert gr[field] == wr[field], (name, k, s, oid, gr[:3], wr[:3], gr[4], wr[4])
                compared += 1
    assert compared >= 30, compared
    gal, dev, want = device["gallery"], device["dev"], oracle["gallery"]
    rows, ids = gal.rows()
    assert len(gal) == len(want.rows) and list(ids) == want.ids
    for r in range(len(want.rows)):
        assert rows[r].tobytes() == want.rows[r].tobytes(), ("gallery row", r)
    assert gal.row_updates().tolist() == oracle["ref"].updates
    assert dev.refined_total() == oracle["ref"].refined_total
    assert dev.enrolled_total() == want.enrolled_total and dev.enrol_dropped() == want.dropped


def test_templates_off_moves_no_bit(H, frames, model, setup):
    """Never set, set and cleared, and test_gpu_multi_enrol's own device run: the same bits."""
    runs = []
    for mode in ("never", "cleared", "enrol"):
        g = TE._reserved(H, setup)
        if mode == "enrol":
            run = TE._device_run(H, frames, model, g, setup["threshold"], "on")
        else:
            dev = H.DeviceMultiTracker("face", "facemesh", S, K)
            dev.set_loss_threshold(-1.0)
            dev.set_redetect_interval(40.0)
            dev.set_recognition(model, g)
            dev.set_identify_interval(INTERVAL)
            dev.set_identity_threshold(setup["threshold"])
            dev.set_enrolment(g, FIRST_ID)
            if mode == "cleared":
                dev.set_identity_smoothing(8)
                dev.set_gallery_refinement(g)
                assert dev.identity_smoothing() == 8 and dev.gallery_refinement()
                dev.set_identity_smoothing(1)
                dev.set_gallery_refinement(None)
            assert dev.identity_smoothing() == 1 and not dev.gallery_refinement()
            run = _steps(H, dev, frames, 0, STEPS)
        rows, ids = g.rows()
        runs.append((run["identity"], run["track"], rows.tobytes(), list(ids)))
        assert not any(g.row_updates()) and run["dev"].refined_total() == 0
    assert runs[0] == runs[1] == runs[2]
    assert len(runs[0][3]) > 3


def test_a_second_tracker_matches_the_refined_rows(H, frames, model, plan, devices):
    """Created after the first synchronised, recognition only: its first embeddings (raw: no smoothing) are
    measured against the rows as the first tracker left them."""
    gal = devices["both"]["gallery"]
    rows, ids = gal.rows()
    before = rows.tobytes()
    assert rows[:3].tobytes() != plan["both"]["rows"].tobytes()   # refined
    dev = _tracker(H, model, gal, plan["both"]["threshold"])
    run = _steps(H, dev, frames, 0, 3)
    seen = 0
    for s in range(S):
        for _, rec in run["identity"][2][s]:
            if rec is None or rec[2] != 1:
                continue
            e = np.frombuffer(rec[3], f32)
            row, d = ER.nearest(ER.distances(e, rows))
            assert rec[1] == f32(d).tobytes(), (s, rec[:3])
            assert rec[0] == (int(ids[row]) if d <= f32(plan["both"]["threshold"]) else IR.NO_MATCH)
            seen += 1
    assert seen >= 4 and gal.rows()[0].tobytes() == before and dev.refined_total() == 0


def test_saved_and_reloaded_gallery_continues_its_means(H, frames, model, plan):
    """Two runs of five steps; then set_recognition again (every object starts over, in both) -- on the same
    gallery in one run, on a fresh gallery loaded from rows() + row_updates() in the other -- and three more
    steps: the same bits.  Without the counts the loaded rows would restart their means."""
    kw, cut = plan["both"], 5
    outs = []
    for reload in (False, True):
        first = _device_run(H, frames, model, kw, steps=cut)
        g, dev = first["gallery"], first["dev"]
        counts = g.row_updates()
        assert counts.any()
        if reload:
            rows, ids = g.rows()
            enrolled = g.enrolled()
            g = H.Gallery()
            g.reserve(kw["capacity"])
            g.add(rows, list(ids))
            assert not g.row_updates().any()
            g.set_row_updates(counts.tolist())
            assert g.row_updates().tolist() == counts.tolist()
            with pytest.raises(RuntimeError):
                g.set_row_updates(counts.tolist()[:-1])
        # from here on every object is known to its nearest row and contributes to it
        after = (model, g, math.inf, kw["cap"], (MAX_SAMPLES, math.inf), True)
        _settings(dev, *after, FIRST_ID + enrolled if reload else FIRST_ID)
        more = _steps(H, dev, frames, cut, STEPS)
        rows, ids = g.rows()
        outs.append((more["identity"], more["track"], rows.tobytes(), list(ids), g.row_updates().tolist()))
        assert dev.refined_total() > sum(counts)   # the means went on after the cut
    assert outs[0] == outs[1]


def test_objects_packed_carries_the_template(devices, oracles):
    dev = devices["smooth"]["dev"]
    p = dev.objects_packed()
    want = {(s, oid): rec for s in range(S) for oid, rec in oracles["smooth"]["identity"][STEPS - 1][s]}
    seen = 0
    for k in range(p["count"]):
        rec = want[(int(p["stream"][k]), int(p["id"][k]))]
        if rec is None:
            continue
        assert p["identity_present"][k] and p["embedding"][k].tobytes() == rec[3]
        seen += rec[2] >= 2
    assert seen >= 4


def test_setter_refusals(H, model, plan):
    rows = plan["both"]["rows"]
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    g, other, loose = _reserved(H, rows, 8), _reserved(H, rows, 8), TI._gallery(H, rows, GALLERY_IDS)
    with pytest.raises(RuntimeError):
        dev.set_identity_smoothing(8)          # no recognition yet
    with pytest.raises(RuntimeError):
        dev.set_gallery_refinement(g)
    dev.set_recognition(model, g)
    for bad in (lambda: dev.set_identity_smoothing(0), lambda: dev.set_gallery_refinement(other),
                lambda: dev.set_gallery_refinement(g, 1), lambda: dev.set_gallery_refinement(g, 0)):
        with pytest.raises(RuntimeError):
            bad()
    dev.set_recognition(model, loose)
    with pytest.raises(RuntimeError):
        dev.set_gallery_refinement(loose)      # not reserved
    with pytest.raises(RuntimeError):
        loose.row_updates()
    with pytest.raises(RuntimeError):
        loose.set_row_updates([0, 0, 0])
    dev.set_recognition(model, g)
    dev.set_identity_smoothing(8)
    dev.set_gallery_refinement(g, 2, math.inf)
    assert dev.identity_smoothing() == 8 and dev.gallery_refinement()
    dev.set_recognition(model, g)              # every set_recognition turns both off
    assert dev.identity_smoothing() == 1 and not dev.gallery_refinement()
    # one writer at a time: a refining tracker that has stepped and not synchronised keeps others out
    dev.set_gallery_refinement(g)
    second = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    second.set_recognition(model, g)
    second.set_gallery_refinement(g)
    from zaru_amd._lib import DeviceBuffer
    buf = DeviceBuffer.from_array(np.zeros((FH, FW, 4), np.uint8))
    view = [(buf.ptr, FW, FH, FW * 4)]
    dev.step(view, 0.0)
    with pytest.raises(RuntimeError):
        second.step(view, 0.0)
    dev.synchronize()
    second.step(view, 0.0)
    second.synchronize()
    g.clear()
    assert len(g) == 0 and g.row_updates().tolist() == []
