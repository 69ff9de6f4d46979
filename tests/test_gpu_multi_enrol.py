"""Automatic enrolment on the device: zr_embed_match_count_async, zr_identity_enrol_async, Gallery.reserve
and DeviceMultiTracker.set_enrolment, against

  * zr_embed_match_async at the same gallery size (the counted match, bit for bit);
  * tests/multi_enrol_ref.py's numpy restatement of the rule on synthetic states (the kernel alone);
  * tests/multi_enrol_ref.py's loop oracle, bit for bit at every step, stream and object;
  * itself with enrolment off (no bit of the recognition or the tracking may move).

The loop's script: streams 0 and 1 see the same frames and the same injected detections, so their
objects embed to the same bits and stream 1's are the same-step duplicates of stream 0's; stream 2's
first object is a row of the gallery from the start.  Every object is embedded again after 40 ms, from
another frame: its embedding drifts past the threshold, and it must not become a second person.
"""
import ctypes as C
import math

import numpy as np
import pytest

import multi_enrol_ref as ER
import multi_identity_ref as IR
import multi_tracker_ref as MR
import test_gpu_multi_identity as TI

pytestmark = pytest.mark.gpu

f32 = np.float32
FW, FH, S, K, CLOCK = TI.FW, TI.FH, TI.S, TI.K, TI.CLOCK
STEPS = 8
A = (0.9, (200.0, 180.0, 80.0, 88.0), 0.3)
B = (0.7, (120.0, 260.0, 72.0, 72.0), 0.5)
Cc = (0.9, (300.0, 200.0, 100.0, 80.0), -0.2)
D = (0.9, (100.0, 100.0, 60.0, 60.0), 0.0)
E = (0.6, (380.0, 80.0, 64.0, 64.0), 1.0)
F = (0.8, (400.0, 300.0, 56.0, 56.0), 0.0)
SCRIPT = {0: {0: [A, B], 1: [A, B], 2: [Cc, D]}, 3: {0: [E], 1: [E], 2: [F]}}
GALLERY_IDS = [7, 1000, 2 ** 40 + 3]
FIRST_ID = 5000
INTERVAL = 40.0


@pytest.fixture(scope="module")
def H():
    import zaru_amd.host as H
    return H


# ---- the counted match --------------------------------------------------------------------------
def _match_inputs(g):
    rng = np.random.default_rng(50 + g)
    q, cap = 70, 130
    queries = rng.standard_normal((q, 128)).astype(f32)
    gallery = rng.standard_normal((cap, 128)).astype(f32)
    gallery[g:] = queries[np.arange(cap - g) % q]   # a kernel that read them would win at distance 0
    valid = np.ones(q, np.int32)
    valid[[3, 17, 64, 69]] = 0
    return queries, gallery, valid


def _match(queries, gallery, valid, g, counted):
    from zaru_amd import _lib
    lib = _lib.lib()
    b = _lib.DeviceBuffer.from_array
    q, cap = len(queries), len(gallery)
    dq, dg, dv = b(queries), b(gallery), b(valid)
    di, dd = b(np.full(q, 77, np.int32)), b(np.full(q, 7.0, f32))
    if counted:
        dn = b(np.array([g], np.int32))
        _lib.check(lib.zr_embed_match_count_async(dq.ptr, q, dg.ptr, cap, dn.ptr, 128, dv.ptr, di.ptr, dd.ptr, None))
    else:
        _lib.check(lib.zr_embed_match_async(dq.ptr, q, dg.ptr, g, 128, dv.ptr, di.ptr, dd.ptr, None, None))
    _lib.synchronize()
    return di.download((q,), np.int32), dd.download((q,), f32)


@pytest.mark.parametrize("g", [0, 1, 63, 64, 65, 130])
def test_counted_match_is_the_plain_match_at_the_device_count(g):
    queries, gallery, valid = _match_inputs(g)
    want_i, want_d = _match(queries, gallery, valid, g, False)
    got_i, got_d = _match(queries, gallery, valid, g, True)
    assert got_i.tobytes() == want_i.tobytes() and got_d.tobytes() == want_d.tobytes()
    assert (got_i < g).all() and (got_i[valid == 0] == -1).all() and np.isinf(got_d[valid == 0]).all()
    if g:
        assert (got_i[valid != 0] >= 0).all() and (got_d[valid != 0] > 0).all()   # no row past the count was read


def test_counted_match_clamps_the_count():
    queries, gallery, valid = _match_inputs(65)
    for g, clamped in ((-5, 0), (1000, 130), (131, 130)):
        want_i, want_d = _match(queries, gallery, valid, clamped, False)
        got_i, got_d = _match(queries, gallery, valid, g, True)
        assert got_i.tobytes() == want_i.tobytes() and got_d.tobytes() == want_d.tobytes(), g


# ---- the enrol kernel alone, on synthetic states ------------------------------------------------------
def _states(n, row=-1, distance=math.inf, embeddings=2, flags=0):
    from zaru_amd import _lib
    st = np.zeros(n, np.dtype(_lib.IdentityState))
    st["row"], st["distance"], st["embeddings"], st["flags"] = row, distance, embeddings, flags
    st["next_ms"] = 1000.0 + np.arange(n)
    return st


def _enrol(st, emb, due_of, rows, ids, capacity, next_id, threshold, min_embeddings, slots=4):
    """The kernel on device copies, and the oracle on the same data: everything compared as bytes.
    Returns the oracle's events and gallery."""
    from zaru_amd import _lib
    lib = _lib.lib()
    b = _lib.DeviceBuffer.from_array
    n, have = len(st), len(ids)
    grows = np.full((capacity, 128), 7.0, f32)
    gids = np.full(capacity, 0xA5A5A5A5A5A5A5A5, np.uint64)
    grows[:have], gids[:have] = rows, ids
    d_st, d_emb, d_of, d_rows, d_ids = b(st), b(emb), b(due_of), b(grows), b(gids)
    d_count, d_next = b(np.array([have], np.int32)), b(np.array([next_id], np.uint64))
    d_total, d_drop = b(np.array([1000], np.uint64)), b(np.array([10], np.uint64))
    cfg = _lib.IdentityCfg(slots, 468, 1, 1, 0.4, threshold, 1000.0)
    _lib.check(lib.zr_identity_enrol_async(C.byref(cfg), n, d_of.ptr, d_st.ptr, d_emb.ptr, d_rows.ptr, d_ids.ptr,
                                           d_count.ptr, d_next.ptr, capacity, 128, min_embeddings, d_total.ptr,
                                           d_drop.ptr, None))
    _lib.synchronize()
    items = [{"due": bool(due_of[i] >= 0), "row": int(st["row"][i]), "distance": st["distance"][i],
              "embeddings": int(st["embeddings"][i]), "flags": int(st["flags"][i]), "embedding": emb[i]}
             for i in range(n)]
    g = ER.GalleryRef(capacity, rows, ids, next_id)
    events = ER.enrol_step(items, g, threshold, min_embeddings)
    want = st.copy()
    for i, it in enumerate(items):
        want["row"][i], want["distance"][i], want["flags"][i] = it["row"], it["distance"], it["flags"]
    now = len(g.rows)
    grows[:now], gids[:now] = np.stack(g.rows) if now else grows[:0], np.array(g.ids, np.uint64)
    assert d_st.download((n,), st.dtype).tobytes() == want.tobytes(), "states"
    assert d_emb.download((n, 128), f32).tobytes() == emb.tobytes(), "the objects' embeddings are only read"
    assert d_rows.download((capacity, 128), f32).tobytes() == grows.tobytes(), "gallery rows"
    assert d_ids.download((capacity,), np.uint64).tobytes() == gids.tobytes(), "ids"
    assert d_count.download((1,), np.int32)[0] == now and d_next.download((1,), np.uint64)[0] == g.next_id
    assert d_total.download((1,), np.uint64)[0] == 1000 + g.enrolled_total
    assert d_drop.download((1,), np.uint64)[0] == 10 + g.dropped
    return events, g, want


@pytest.mark.parametrize("variant", ["a", "b"])
def test_enrol_small(variant):
    """n = 8 (2 x 4), two rows present, capacity 5, min_embeddings 2, threshold 0.5.
    a: enrol, its duplicate, a row that was not due, enrol, a NaN embedding, enrol, an EVER_KNOWN row, dropped.
    b: below min_embeddings, enrol, a known row, enrol, a duplicate, enrol, dropped, a duplicate after the
       gallery is full."""
    rng = np.random.default_rng(12)
    n = 8
    emb = (4.0 * rng.standard_normal((n, 128))).astype(f32)   # far apart
    rows, ids = (4.0 * rng.standard_normal((2, 128))).astype(f32), [100, 101]
    st, due_of = _states(n), np.arange(n, dtype=np.int32)
    if variant == "a":
        emb[0, 5] = 1.0
        emb[1] = emb[0]
        emb[1, 5] = 1.25              # 0.25 from row 0's embedding: within the threshold
        due_of[2] = -1
        emb[4, 127] = np.nan
        st["flags"][6] = ER.EVER_KNOWN
        want_kinds = {0: "enrol", 1: "match", 3: "enrol", 5: "enrol", 7: "dropped"}
    else:
        st["embeddings"][0] = 1
        st["row"][2], st["distance"][2] = 1, 0.125
        emb[4] = emb[1]
        emb[7] = emb[5]
        want_kinds = {1: "enrol", 2: "known", 3: "enrol", 4: "match", 5: "enrol", 6: "dropped", 7: "match"}
    events, g, want = _enrol(st, emb, due_of, rows, ids, 5, 500, 0.5, 2)
    assert {i: k for i, k, _ in events} == want_kinds
    assert g.ids == [100, 101, 500, 501, 502] and g.dropped == 1
    if variant == "a":
        assert want["row"][1] == 2 and want["distance"][1] == f32(0.25) and want["flags"][1] == ER.EVER_KNOWN
        assert want[2:3].tobytes() == st[2:3].tobytes() and want[4:5].tobytes() == st[4:5].tobytes()
        assert want[6:7].tobytes() == st[6:7].tobytes() and want[7:8].tobytes() == st[7:8].tobytes()
    else:
        assert want[0:1].tobytes() == st[0:1].tobytes() and want["flags"][2] == ER.EVER_KNOWN
        assert want["row"][7] == 4 and want["distance"][7] == 0.0 and want["flags"][7] == ER.EVER_KNOWN


def test_enrol_past_the_workgroup_width():
    """n = 320, all distinct, threshold 0: every row is appended; the appended rows pass 256."""
    rng = np.random.default_rng(13)
    n = 320
    emb = rng.standard_normal((n, 128)).astype(f32)
    rows, ids = rng.standard_normal((10, 128)).astype(f32), list(range(900, 910))
    events, g, want = _enrol(_states(n, embeddings=1), emb, np.arange(n, dtype=np.int32)[::-1].copy(), rows, ids,
                             384, 2 ** 33, 0.0, 1)
    assert [k for _, k, _ in events] == ["enrol"] * n and len(g.rows) == 330
    assert (want["row"] == 10 + np.arange(n)).all() and g.ids[-1] == 2 ** 33 + n - 1


def test_enrol_clusters():
    """n = 320 drawn as 40 tight clusters: 40 rows, each member on its cluster's first row."""
    rng = np.random.default_rng(14)
    n, nc = 320, 40
    centres = rng.standard_normal((nc, 128)).astype(f32)
    cluster = rng.permutation(np.repeat(np.arange(nc), n // nc))
    emb = (centres[cluster] + f32(0.01) * rng.standard_normal((n, 128)).astype(f32)).astype(f32)
    intra, inter = 0.0, math.inf
    for i in range(n):
        d = ER.distances(emb[i], emb)
        same = cluster == cluster[i]
        intra, inter = max(intra, float(d[same].max())), min(inter, float(d[~same].min()))
    threshold = float(f32(0.5 * (intra + inter)))
    print("largest intra-cluster", intra, "smallest inter-cluster", inter, "threshold", threshold)
    assert intra < 0.5 and inter > 5.0 and intra < threshold < inter   # no distance sits at the threshold
    events, g, want = _enrol(_states(n, embeddings=1), emb, np.arange(n, dtype=np.int32), np.zeros((0, 128), f32), [],
                             384, 0, threshold, 1)
    assert len(g.rows) == nc and g.dropped == 0
    first = {}
    for i in range(n):
        first.setdefault(cluster[i], len(first))
        assert want["row"][i] == first[cluster[i]], i
    assert sum(k == "match" for _, k, _ in events) == n - nc


# ---- the loop against the oracle -------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    same = TI._noise(STEPS, 20)
    return [same, same, TI._noise(STEPS, 22)]   # streams 0 and 1: the same frames


@pytest.fixture(scope="module")
def model():
    return TI.RU.model_bytes(TI.GOLDEN)


@pytest.fixture(scope="module")
def embed(H, model):
    raw = IR.host_embed(H.FaceEmbedder(model))
    cache = {}

    def fn(frame, rect):
        key = (id(frame), rect.tuple())
        if key not in cache:
            cache[key] = raw(frame, rect)
        return cache[key]
    return fn


def _injected(k):
    return [list(SCRIPT.get(k, {}).get(s, [])) for s in range(S)]


def _record(i, enrolled):
    if i is None:
        return None
    return (int(i["id"]), f32(i["distance"]).tobytes(), int(i["embeddings"]),
            np.ascontiguousarray(i["embedding"], f32).tobytes(), bool(enrolled))


def _oracle_run(H, frames, embed, rows, ids, threshold, capacity, enrol=True):
    trackers = []
    for s in range(S):
        t = MR.MultiTrackerRef(H, "face", "facemesh", K)
        t.loss, t.interval = -1.0, 40.0
        trackers.append(t)
    host = TI._gallery(H, rows, ids)   # what the matches of a step see: the rows before that step
    gal = ER.GalleryRef(capacity, rows, ids, FIRST_ID)
    ref = ER.MultiEnrolRef(H, trackers, embed, IR.host_match(host), gal,
                           on_append=lambda r, i: host.add(np.ascontiguousarray(r, f32), list(i)),
                           interval=INTERVAL, threshold=threshold, enrol=enrol)
    out = {"track": [], "identity": [], "gallery": gal, "ref": ref}
    for k in range(STEPS):
        ref.step([frames[s][k] for s in range(S)], CLOCK * k, [[TI._det(H, d) for d in dets] for dets in _injected(k)])
        out["track"].append([TI._track_record(
            [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
              "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in trackers[s].objects()],
            len(trackers[s].objs), trackers[s].pending) for s in range(S)])
        out["identity"].append([[(o.id, _record(i, i and i["flags"] & ER.ENROLLED)) for o, i in ref.objects(s)]
                                for s in range(S)])
    return out


def _device_run(H, frames, model, gallery, threshold, enrol, steps=STEPS, recognition=True):
    """enrol: None (never called), "off" (set, then set_enrolment(None)) or "on"."""
    from zaru_amd._lib import DeviceBuffer
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    if recognition:
        dev.set_recognition(model, gallery)
        dev.set_identify_interval(INTERVAL)
        dev.set_identity_threshold(threshold)
    if enrol is not None:
        dev.set_enrolment(gallery, FIRST_ID)
        if enrol == "off":
            dev.set_enrolment(None)
    bufs = [DeviceBuffer.from_array(np.stack([frames[s][k] for s in range(S)])) for k in range(steps)]
    fb = FH * FW * 4
    out = {"track": [], "identity": [], "dev": dev, "bufs": bufs}
    for k in range(steps):
        for s, dets in enumerate(_injected(k)):
            if dets:
                dev.inject_detections(s, [TI._det(H, d) for d in dets])
        dev.step([(bufs[k].ptr + s * fb, FW, FH, FW * 4) for s in range(S)], CLOCK * k)
        dev.synchronize()
        counts, pend = dev.object_counts(), dev.detection_pending()
        objs = [dev.objects(s) for s in range(S)]
        out["track"].append([TI._track_record(
            [{"id": o["id"], "rect": o["view_rect"].rect().tuple(), "angle": o["view_rect"].rotation_radians(),
              "landmarks": o["landmarks"], "confidence": o["confidence"]} for o in objs[s]], counts[s], pend[s])
            for s in range(S)])
        out["identity"].append([[(o["id"], _record(o["identity"], o["identity"] and o["identity"]["enrolled"]))
                                 for o in objs[s]] for s in range(S)])
    return out


@pytest.fixture(scope="module")
def setup(H, frames, embed):
    """A run without a gallery gives every embedding the script makes.  The gallery's first row is stream
    2's first object at its first embedding; the threshold is half the smallest distance between any two
    different embeddings or rows, so only equal bits match."""
    plain = _oracle_run(H, frames, embed, [], [], math.inf, 64, enrol=False)
    embs = {}
    for k in range(STEPS):
        for s in range(S):
            for _, rec in plain["identity"][k][s]:
                if rec is not None:
                    embs.setdefault(rec[3], (k, s))
    rng = np.random.default_rng(78)
    first = next(rec for _, rec in plain["identity"][1][2] if rec is not None)
    rows = np.stack([np.frombuffer(first[3], f32), rng.standard_normal(128).astype(f32),
                     rng.standard_normal(128).astype(f32)])
    pts = np.concatenate([np.stack([np.frombuffer(e, f32) for e in embs]), rows[1:]])
    smallest = min(float(np.delete(ER.distances(pts[i], pts), i).min()) for i in range(len(pts)))
    assert smallest > 0 and len(embs) >= 12, (smallest, len(embs))
    threshold = float(f32(0.5 * smallest))
    unbounded = _oracle_run(H, frames, embed, rows, GALLERY_IDS, threshold, 64)
    appended = unbounded["gallery"].enrolled_total
    assert appended >= 4 and unbounded["gallery"].dropped == 0
    return {"rows": rows, "threshold": threshold, "capacity": 3 + appended - 1}


@pytest.fixture(scope="module")
def oracle(H, frames, embed, setup):
    return _oracle_run(H, frames, embed, setup["rows"], GALLERY_IDS, setup["threshold"], setup["capacity"])


def _reserved(H, setup, capacity=None):
    g = TI._gallery(H, setup["rows"], GALLERY_IDS)
    g.reserve(capacity or setup["capacity"])
    return g


@pytest.fixture(scope="module")
def device(H, frames, model, setup):
    g = _reserved(H, setup)
    out = _device_run(H, frames, model, g, setup["threshold"], "on")
    out["gallery"] = g
    return out


def test_script_contains_the_events(oracle, setup):
    ev = oracle["ref"].events
    print("threshold", setup["threshold"], "capacity", setup["capacity"], "events", ev)
    kinds = [e[3] for e in ev]
    assert "known" in kinds and "enrol" in kinds and "match" in kinds and "dropped" in kinds
    # stream 1's object matches the row stream 0's object appended in that very step, at distance 0
    dup = [(k, row) for k, s, _, kind, row in ev if kind == "match" and s == 1]
    assert dup and all((k, 0, row) in {(k2, s2, r2) for k2, s2, _, kind2, r2 in ev if kind2 == "enrol"} for k, row in dup)
    matched = [rec for k in range(STEPS) for _, rec in oracle["identity"][k][1] if rec and rec[0] >= FIRST_ID]
    assert matched and all(rec[1] == f32(0.0).tobytes() and not rec[4] for rec in matched if rec[2] == 1)
    # stream 2's first object is the gallery's first row from its first embedding on: known, never enrolled
    _, rec = oracle["identity"][1][2][0]
    assert rec[0] == GALLERY_IDS[0] and rec[1] == f32(0.0).tobytes() and not rec[4]
    # an enrolled object drifted at its next embedding: unknown again, still the enrolled one, no new row
    drifted = [rec for k in range(STEPS) for s in range(S) for _, rec in oracle["identity"][k][s]
               if rec and rec[4] and rec[2] >= 2 and rec[0] == IR.NO_MATCH]
    assert drifted
    g = oracle["gallery"]
    assert len(g.rows) == g.capacity and g.dropped >= 1 and g.ids[3:] == list(range(FIRST_ID, FIRST_ID + len(g.ids) - 3))


def test_loop_against_the_oracle(oracle, device):
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
    assert len(gal) == len(want.rows) == gal.capacity() and gal.enrolled() == want.enrolled_total
    assert rows.tobytes() == np.stack(want.rows).tobytes() and list(ids) == want.ids
    assert dev.enrolled_total() == want.enrolled_total and dev.enrol_dropped() == want.dropped
    assert [gal.id_of(r) for r in (-1, 0, 3, len(gal))] == [H_NO_MATCH, GALLERY_IDS[0], FIRST_ID, H_NO_MATCH]


H_NO_MATCH = IR.NO_MATCH


def test_reidentification_by_a_second_tracker(H, frames, model, setup, oracle, device):
    """Created after the first synchronised, on the same gallery and frames: its own track ids, the same
    persons at distance 0, nobody enrolled."""
    gal, first = device["gallery"], device["dev"]
    size, total, dropped = len(gal), first.enrolled_total(), first.enrol_dropped()
    again = _device_run(H, frames, model, gal, setup["threshold"], "on")
    assert again["track"] == device["track"]
    seen = 0
    for k in range(STEPS):
        for s in range(S):
            for (oid, was), (_, now) in zip(device["identity"][k][s], again["identity"][k][s]):
                assert (was is None) == (now is None)
                if was is None or was[2] != 1 or was[0] == IR.NO_MATCH:
                    continue
                assert now[0] == was[0] and now[1] == f32(0.0).tobytes() and now[2] == 1 and now[3] == was[3], (k, s, oid)
                assert not now[4]
                seen += was[0] >= FIRST_ID
    assert seen >= 8, seen
    assert len(gal) == size and gal.enrolled() == total
    assert first.enrolled_total() == total and first.enrol_dropped() == dropped
    assert again["dev"].enrolled_total() == 0 and again["dev"].enrol_dropped() >= 1
    # two trackers enrolling at once: refused where it can be seen -- the first has stepped and not synchronised
    second, fb = again["dev"], FH * FW * 4
    views = [(device["bufs"][0].ptr + s * fb, FW, FH, FW * 4) for s in range(S)]
    first.step(views, CLOCK * STEPS)
    with pytest.raises(RuntimeError):
        second.step(views, CLOCK * STEPS)
    first.synchronize()
    second.step(views, CLOCK * STEPS)
    second.synchronize()


def test_enrolment_off_moves_no_bit(H, frames, model, setup, device):
    plain = _device_run(H, frames, model, TI._gallery(H, setup["rows"], GALLERY_IDS), setup["threshold"], None)
    assert any(rec is not None and rec[0] == GALLERY_IDS[0] for _, rec in plain["identity"][1][2])
    for mode in (None, "off"):
        g = _reserved(H, setup)
        run = _device_run(H, frames, model, g, setup["threshold"], mode)
        assert run["identity"] == plain["identity"] and run["track"] == plain["track"], mode
        assert len(g) == 3 and g.enrolled() == 0 and run["dev"].enrolled_total() == 0 and not run["dev"].enrolment()
    # and with enrolment on the tracking is that of the loop without it
    assert device["track"] == plain["track"]
    assert device["identity"] != plain["identity"]


def test_set_enrolment_refusals(H, model, setup):
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    g, other, loose = _reserved(H, setup), _reserved(H, setup), TI._gallery(H, setup["rows"], GALLERY_IDS)
    with pytest.raises(RuntimeError):
        dev.set_enrolment(g, 1)            # no recognition yet
    dev.set_recognition(model, g)
    for bad in (lambda: dev.set_enrolment(other, 1), lambda: dev.set_enrolment(g, 1, 0)):
        with pytest.raises(RuntimeError):
            bad()
    dev.set_recognition(model, loose)
    with pytest.raises(RuntimeError):
        dev.set_enrolment(loose, 1)        # not reserved
    dev.set_recognition(model, g)
    dev.set_enrolment(g, 1, 3)
    assert dev.enrolment()
    dev.set_recognition(model, g)          # every set_recognition turns it off
    assert not dev.enrolment()
    with pytest.raises(RuntimeError):
        g.reserve(100)                     # once


def test_gallery_add_rows_and_capacity(H, frames, model, setup):
    g = _reserved(H, setup, 12)
    run = _device_run(H, frames, model, g, setup["threshold"], "on", steps=3)
    enrolled = len(g) - 3
    assert enrolled >= 3 and g.enrolled() == enrolled == run["dev"].enrolled_total()
    rng = np.random.default_rng(5)
    extra = rng.standard_normal((2, 128)).astype(f32)
    g.add(extra, [77, 78])                 # behind the rows the device appended
    rows, ids = g.rows()
    assert len(g) == 5 + enrolled and list(ids) == GALLERY_IDS + list(range(FIRST_ID, FIRST_ID + enrolled)) + [77, 78]
    assert rows[-2:].tobytes() == extra.tobytes() and rows[:3].tobytes() == setup["rows"].tobytes()
    assert g.enrolled() == enrolled       # add is not an enrolment
    # saved and loaded: a fresh gallery of these rows gives the same ids at distance 0
    fresh = H.Gallery()
    fresh.add(rows, list(ids))
    got_ids, got_d = fresh.match(rows)
    assert list(got_ids) == list(ids) and (got_d == 0).all()
    got_ids, got_d = g.match(rows)
    assert list(got_ids) == list(ids) and (got_d == 0).all()
    # past the capacity: refused, nothing changes
    room = g.capacity() - len(g)
    with pytest.raises(RuntimeError):
        g.add(rng.standard_normal((room + 1, 128)).astype(f32), list(range(room + 1)))
    assert len(g) == 5 + enrolled
    g.add(rng.standard_normal((room, 128)).astype(f32), list(range(room)))
    assert len(g) == g.capacity() == 12
    with pytest.raises(RuntimeError):
        g.add(extra[:1], [1])
    # clear resets both sides; the next enrolment numbers from its first_id again
    g.clear()
    assert len(g) == 0 and g.enrolled() == 0 and g.rows()[0].shape == (0, 128)
    g.add(extra, [77, 78])
    assert len(g) == 2 and list(g.match(extra)[0]) == [77, 78]
