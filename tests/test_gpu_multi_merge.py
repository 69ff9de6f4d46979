"""Merging duplicate gallery rows on the device: zr_identity_link_async, Gallery's link table and
DeviceMultiTracker.set_identity_merging, every comparison bit for bit against tests/multi_merge_ref.py:

  * the kernel alone, on synthetic states;
  * the loop against MultiMergeRef at every step, stream and object;
  * itself with merging off, and with merging that can never merge (no bit may move);
  * the read-only mode, a saved and reloaded table, the host's own merge and the refusals.

The loop runs tests/test_gpu_multi_enrol.py's script on its frames (one more of them), embedding every
object again after 25 ms -- every second step -- so that the objects injected at step 3 are due at other
steps than those injected at step 0.  The gallery is made of raw embeddings of a plain oracle run, so the
events are forced: see ``setup``.
"""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import multi_enrol_ref as ER
import multi_identity_ref as IR
import multi_merge_ref as MG
import multi_tracker_ref as MR
import test_gpu_multi_enrol as TE
import test_gpu_multi_identity as TI
import test_gpu_multi_template as TT
from test_gpu_multi_enrol import H, embed, model  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
S, K, CLOCK, FW, FH = TE.S, TE.K, TE.CLOCK, TE.FW, TE.FH
STEPS = TE.STEPS + 1     # the objects injected at step 3 get their third look at step 8
INTERVAL = 25.0
FIRST_ID = TE.FIRST_ID
CAPACITY = 12
MIN_OBS = 2


# ---- the kernel alone, on synthetic states ----------------------------------------------------------
def _links(capacity):
    from zaru_amd import _lib
    l = np.zeros(capacity, np.dtype(_lib.GalleryLink))
    l["alias"], l["partner"] = np.arange(capacity), -1
    return l


def _link(tracked, src, due_of, st_in, st_out, links, count, slots, min_obs, threshold, counts=True):
    """The two launches on device copies, and the oracle on the same data: the states, the whole table and
    the counters compared as bytes; everything that is only read checked unchanged.  Returns the oracle's
    events and what it left."""
    from zaru_amd import _lib
    lib, b = _lib.lib(), _lib.DeviceBuffer.from_array
    n, capacity = len(st_out), len(links)
    rng = np.random.default_rng(n)
    state = np.frombuffer(rng.integers(0, 256, n * C.sizeof(_lib.TrackState), dtype=np.uint8).tobytes(),
                          np.dtype(_lib.TrackState)).copy()   # only `tracked` is read
    state["tracked"] = tracked
    src, due_of = np.asarray(src, np.int32), np.asarray(due_of, np.int32)
    start = np.array([1000, 10, 7], np.uint64)
    d_state, d_src, d_of, d_in, d_out, d_links = b(state), b(src), b(due_of), b(st_in), b(st_out), b(links)
    d_count, d_counts = b(np.array([count], np.int32)), b(start)
    cfg = _lib.IdentityCfg(slots, 468, 1, 1, 0.4, math.nan, 1000.0)   # only `slots` is read
    _lib.check(lib.zr_identity_link_async(C.byref(cfg), d_state.ptr, n, d_src.ptr, d_of.ptr, d_in.ptr, d_out.ptr,
                                          d_links.ptr, d_count.ptr, capacity, min_obs, threshold,
                                          d_counts.ptr if counts else None, None))
    _lib.synchronize()
    as_dicts = lambda st: [{"row": int(r), "distance": d} for r, d in zip(st["row"], st["distance"])]
    ref_links = [{k: int(l[k]) for k in ("alias", "partner", "seen", "reserved")} for l in links]
    ref_out, tally = as_dicts(st_out), {"merged": 0, "vetoed": 0, "observed": 0}
    events = MG.link_step([int(t) for t in tracked], src.tolist(), due_of.tolist(), as_dicts(st_in), ref_out, ref_links,
                          count, slots, min_obs, threshold, tally)
    want_out, want_links = st_out.copy(), links.copy()
    want_out["row"] = [o["row"] for o in ref_out]
    for k in ("alias", "partner", "seen", "reserved"):
        want_links[k] = [l[k] for l in ref_links]
    got_links = d_links.download((capacity,), links.dtype)
    assert got_links.tobytes() == want_links.tobytes(), ("links", got_links, want_links)
    got_out = d_out.download((n,), st_out.dtype)
    assert got_out.tobytes() == want_out.tobytes(), ("states", np.nonzero(got_out["row"] != want_out["row"]))
    want_counts = start + np.array([tally["merged"], tally["vetoed"], tally["observed"]], np.uint64)
    assert d_counts.download((3,), np.uint64).tolist() == (want_counts if counts else start).tolist()
    assert d_in.download((n,), st_in.dtype).tobytes() == st_in.tobytes(), "the carried states are only read"
    assert d_count.download((1,), np.int32)[0] == count
    assert d_state.download((n,), state.dtype).tobytes() == state.tobytes()
    assert d_src.download((n,), np.int32).tobytes() == src.tobytes() and d_of.download((n,), np.int32).tobytes() == due_of.tobytes()
    return events, want_links, want_out, tally


def _small(variant):
    """slots = 4, n = 8, capacity 16; the objects' distances are 0.25 except where said.
    a: stream 0: row 0 flips 0 -> 1, the second sighting of (0, 1) (merge); row 1 flips 2 -> 3 while row 2 holds
       2 (veto); row 3 is not tracked.  Stream 1: row 4 flips 5 -> 6 (pending); row 5 holds 1 and is not due
       (canonicalised to 0); row 6 is a new object (src -1); row 7 is due and stays on 4.
    b: the objects have moved between slots.  Person {2, 3} is merged already, and {7, 8}; row 1 (from slot 3)
       flips 3 -> 8: (2, 7), its second sighting: merge, rows 7 and 8 relabelled; row 0 flips 0 -> 4 at
       distance 0.75; row 2 is due with an out-of-range d_due_of.  Stream 1: row 6 (from slot 0) flips 5 -> 6,
       but row 4 holds 5 (veto, resetting a pending record of row 6); row 7 flips 0 -> 1 (pending, replacing
       another partner); row 5 holds 8 and is not due (canonicalised to 2)."""
    n, capacity = 8, 16
    st_in, st_out = TE._states(n, distance=0.25), TE._states(n, distance=0.25)
    st_out["next_ms"] += 40.0
    st_out["embeddings"] += 1
    links = _links(capacity)
    tracked, src = np.ones(n, np.uint32), np.arange(n, dtype=np.int32) % 4
    due_of = np.full(n, -1, np.int32)
    if variant == "a":
        st_in["row"] = [0, 2, 2, 4, 5, 1, 7, 4]
        st_out["row"] = [1, 3, 2, 4, 6, 1, 8, 4]
        due_of[[0, 1, 4, 6, 7]] = [3, 0, 1, 2, 4]
        tracked[3], src[6] = 0, -1
        links[1] = (1, 0, 1, 0)
        want = [("observe", 0, 0, 1, 2), ("merge", 0, 0, 1), ("veto", 1, 2, 3, 2), ("observe", 4, 5, 6, 1),
                ("canonicalise", 0, 1, 0), ("canonicalise", 5, 1, 0)]
    else:
        src[:] = [1, 3, 2, 0, 1, 2, 0, 3]
        #               slot: 0  1  2  3 | 0  1  2  3
        st_in["row"] = [-1, 0, 9, 3, 5, 5, 8, 0]
        st_out["row"] = [4, 8, 4, -1, 5, 8, 6, 1]
        st_out["distance"][0] = 0.75
        due_of[[0, 1, 2, 6, 7]] = [0, 1, 8, 2, 3]
        tracked[3] = 0
        links[3], links[8] = (2, -1, 0, 0), (7, -1, 0, 0)
        links[7], links[6], links[1] = (7, 2, 1, 0), (6, 5, 1, 0), (1, 9, 1, 0)
        want = [("observe", 1, 2, 7, 2), ("merge", 1, 2, 7), ("veto", 6, 5, 6, 4), ("observe", 7, 0, 1, 1),
                ("canonicalise", 1, 8, 2), ("canonicalise", 5, 8, 2)]
    return dict(tracked=tracked, src=src, due_of=due_of, st_in=st_in, st_out=st_out, links=links, slots=4), want


@pytest.mark.parametrize("variant", ["a", "b"])
def test_link_small(variant):
    case, want = _small(variant)
    events, links, out, tally = _link(count=9, min_obs=2, threshold=0.5, **case)
    assert events == want
    assert tally == {"merged": 1, "vetoed": 1, "observed": 2}
    if variant == "b":
        assert links["alias"][:9].tolist() == [0, 1, 2, 2, 4, 5, 6, 2, 2] and tuple(links[6]) == (6, -1, 0, 0)
        assert tuple(links[1]) == (1, 0, 1, 0)


@pytest.mark.parametrize("count", [-5, 0, 16 + 7, 3, 7])
def test_link_clamps_the_count(count):
    """G = clamp(count, 0, capacity): below it nothing is evidence, and no row at or past it is read, relabelled
    or canonicalised (the table past the count holds sentinels that a kernel reading it would act on)."""
    case, _ = _small("b")
    G = min(max(count, 0), 16)
    for r in range(G, 16):
        case["links"][r] = (0, 0, 0xA5A5A5A5, 0xA5A5A5A5) if count <= 7 else case["links"][r]
    events, links, out, tally = _link(count=count, min_obs=1, threshold=0.5, **case)
    assert all(max(ev[2], ev[3]) < G for ev in events)
    if G == 0:
        assert events == []
    if count == 23:
        assert tally["merged"] >= 1


@pytest.mark.parametrize("threshold", [0.5, math.nan, math.inf, 0.0])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_link_thresholds(variant, threshold):
    case, _ = _small(variant)
    case["st_in"]["distance"][4], case["st_out"]["distance"][7] = 0.0, 0.0
    if variant == "b":
        case["st_in"]["distance"][3], case["st_out"]["distance"][1] = 0.0, 0.0   # row 1 carries slot 3's state
    events, *_ = _link(count=9, min_obs=2, threshold=threshold, **case)
    walked = [ev for ev in events if ev[0] != "canonicalise"]
    if math.isnan(threshold):
        assert walked == []
    elif threshold == 0.0:
        assert [ev[1] for ev in walked] == ([] if variant == "a" else [1, 1])
    elif math.isinf(threshold) and variant == "b":
        assert walked[0] == ("veto", 0, 0, 4, 2)   # row 0's 0.75 is within +inf, and row 2 holds 4
    if variant == "b":
        assert [ev for ev in events if ev[0] == "canonicalise" and ev[1] == 5]   # pass 2 runs whatever the threshold


@pytest.mark.parametrize("counts", [True, False])
def test_link_nothing_eligible_writes_nothing(counts):
    """Every row due and tracked, none evidence, every reported row canonical: the table, the states and the
    counters keep their bytes (compared in _link); and so with a NULL d_counts."""
    case, _ = _small("a")
    case["st_in"]["row"] = [0, 2, 2, 4, 5, 0, 7, 4]
    case["st_out"]["row"] = [0, 2, 2, 4, 5, 0, 8, -1]
    case["links"][12] = (2 ** 31 - 1, 3, 9, 0)   # past the count: never read
    case["links"][9] = (-7, -1, 0, 0)
    events, links, *_ = _link(count=9, min_obs=2, threshold=0.5, counts=counts, **case)
    assert events == [] and links["alias"][12] == 2 ** 31 - 1 and links["alias"][9] == -7


def test_link_read_only_mode():
    """min_observations = 0: pass 1 is skipped, pass 2 runs."""
    case, _ = _small("a")
    case["links"][1] = (0, -1, 0, 0)
    events, links, out, tally = _link(count=9, min_obs=0, threshold=0.5, **case)
    assert events == [("canonicalise", 0, 1, 0), ("canonicalise", 5, 1, 0)] and tally["observed"] == 0


def test_link_without_counters():
    case, want = _small("a")
    events, *_ = _link(count=9, min_obs=2, threshold=0.5, counts=False, **case)
    assert events == want


def _random(n, slots, capacity, used, seed):
    """Random states whose rows lie in [-1, used)."""
    rng = np.random.default_rng(seed)
    st_in, st_out = TE._states(n), TE._states(n)
    st_in["row"], st_out["row"] = rng.integers(-1, used, n), rng.integers(-1, used, n)
    st_in["distance"], st_out["distance"] = rng.choice([0.125, 0.75], n, p=[0.8, 0.2]), rng.choice([0.125, 0.75], n, p=[0.8, 0.2])
    keep = rng.random(n) < 0.5
    st_out["row"][keep], st_out["distance"][keep] = st_in["row"][keep], st_in["distance"][keep]
    tracked = (rng.random(n) < 0.6).astype(np.uint32)
    src = rng.integers(-1, slots + 1, n).astype(np.int32)
    due_of = np.where(rng.random(n) < 0.5, rng.permutation(n), -1).astype(np.int32)
    return dict(tracked=tracked, src=src, due_of=due_of, st_in=st_in, st_out=st_out, links=_links(capacity), slots=slots)


def test_link_a_stream_that_straddles_two_chunks():
    """slots = 3, n = 768: stream 85 is rows 255..257.  Row 255 flips 20 -> 21 while row 256 holds 20 (veto: the
    neighbour is in the next chunk); row 256 itself flips 22 -> 20, and nobody holds 22 (an observation).
    The other 255 streams are random over rows 0..7, so rows 20..22 are three people when stream 85 is reached."""
    n, slots = 768, 3
    case = _random(n, slots, 64, 8, 41)
    for i, (p, b) in ((255, (20, 21)), (256, (22, 20)), (257, (-1, -1))):
        case["st_in"]["row"][i], case["st_out"]["row"][i] = p, b
        case["st_in"]["distance"][i] = case["st_out"]["distance"][i] = 0.125
        case["tracked"][i], case["src"][i], case["due_of"][i] = 1, i - 255, i
    case["tracked"][257] = 0
    events, links, out, tally = _link(count=40, min_obs=2, threshold=0.5, **case)
    mine = [ev for ev in events if ev[1] in (255, 256, 257) and ev[0] in ("veto", "observe")]
    assert mine == [("veto", 255, 20, 21, 256), ("observe", 256, 20, 22, 1)]
    assert tally["merged"] >= 1 and tally["vetoed"] >= 5 and tally["observed"] >= 20, tally


def test_link_a_veto_in_slot_63():
    """slots = 64, n = 128: the ballot is a full wavefront wide.  Row 64 (stream 1, slot 0) flips 3 -> 4 and row
    127 (slot 63) holds 4; row 0 (stream 0) does the same with nobody else on 3 or 4."""
    n, slots = 128, 64
    case = _random(n, slots, 32, 20, 42)
    case["st_in"]["row"][:], case["st_out"]["row"][:] = -1, -1
    case["tracked"][:], case["due_of"][:] = 1, -1
    for i in (0, 64):
        case["st_in"]["row"][i], case["st_out"]["row"][i], case["src"][i], case["due_of"][i] = 3, 4, 0, i
        case["st_in"]["distance"][i] = case["st_out"]["distance"][i] = 0.125
    case["st_in"]["row"][127] = case["st_out"]["row"][127] = 4
    case["st_out"]["row"][63] = 25   # slot 63 of stream 0: a row past the count vetoes nothing
    events, *_ = _link(count=20, min_obs=2, threshold=0.5, **case)
    assert events == [("observe", 0, 3, 4, 1), ("veto", 64, 3, 4, 127)]


def test_link_relabel_past_the_workgroup_width():
    """Capacity 320, count 300: person 10 owns rows 10, 100, 255, 256, 260 and 299, and merges into row 5."""
    n, slots, capacity = 8, 4, 320
    case, _ = _small("a")
    case["links"] = _links(capacity)
    members = [10, 100, 255, 256, 260, 299]
    case["links"]["alias"][members] = 10
    case["links"]["alias"][301] = 10     # past the count: not a member
    case["st_in"]["row"][:] = case["st_out"]["row"][:] = -1
    case["st_in"]["row"][0], case["st_out"]["row"][0] = 5, 260
    case["st_out"]["row"][5] = 299       # not due: canonicalised to 5
    events, links, out, tally = _link(count=300, min_obs=1, threshold=0.5, **case)
    assert events == [("observe", 0, 5, 10, 1), ("merge", 0, 5, 10), ("canonicalise", 0, 260, 5),
                      ("canonicalise", 5, 299, 5)]
    assert links["alias"][members].tolist() == [5] * 6 and links["alias"][301] == 10
    assert (links["alias"][:300] == np.arange(300)).sum() == 300 - 6


# ---- the loop against the oracle -------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    same = TI._noise(STEPS, 20)   # (test_gpu_multi_enrol's frames, and one more)
    return [same, same, TI._noise(STEPS, 22)]   # streams 0 and 1: the same frames


def _oracle_run(H, frames, embed, rows, ids, threshold, aliases=None, min_obs=MIN_OBS, links=None, steps=STEPS):
    trackers = []
    for s in range(S):
        t = MR.MultiTrackerRef(H, "face", "facemesh", K)
        t.loss, t.interval = -1.0, 40.0
        trackers.append(t)
    gal = ER.GalleryRef(CAPACITY, rows, ids, FIRST_ID)
    if links is None:
        links = MG.default_links(CAPACITY)
        for r, a in enumerate(aliases or []):
            links[r]["alias"] = a
    ref = MG.MultiMergeRef(H, trackers, embed, TT._make_match(H), gal, interval=INTERVAL, threshold=threshold,
                           slots=K, merge_capacity=CAPACITY, min_observations=min_obs, links=links)
    out = {"track": [], "identity": [], "gallery": gal, "ref": ref}
    for k in range(steps):
        ref.step([frames[s][k] for s in range(S)], CLOCK * k,
                 [[TI._det(H, d) for d in dets] for dets in TE._injected(k)])
        out["track"].append([TI._track_record(
            [{"id": o.id, "rect": o.roi.rect().tuple(), "angle": o.roi.rotation_radians(),
              "landmarks": o.lm["landmarks"], "confidence": o.lm["confidence"]} for o in trackers[s].objects()],
            len(trackers[s].objs), trackers[s].pending) for s in range(S)])
        out["identity"].append([[(o.id, TE._record(i, False)) for o, i in ref.objects(s)] for s in range(S)])
        assert MG.is_flat(ref.links, len(gal.rows))
    return out


def _looks(run):
    """(stream, object id) -> [(step, embedding bytes)], one entry per embedding the object made."""
    looks = {}
    for k, per_stream in enumerate(run["identity"]):
        for s, objs in enumerate(per_stream):
            for oid, rec in objs:
                if rec is not None and rec[2] > len(looks.setdefault((s, oid), [])):
                    looks[(s, oid)].append((k, rec[3]))
    return looks


@pytest.fixture(scope="module")
def setup(H, frames, embed):
    """A run without a gallery gives every embedding the script makes (the raw ones: no smoothing), and the
    step of each.  A and B are two objects of stream 0 (and, bit for bit, of stream 1) that are embedded at
    the same steps; Cc and F objects of stream 2, F a later one that is first embedded between two looks of
    A, say looks m and m + 1, and not at look m + 1's step.  The rows, with their aliases:
        0  A's look m                    A is on row 0 at look m and on row 1 at look m + 1, at distance 0, in
        1  A's look m + 1                streams 0 and 1: two observations in one step, the merge (0, 1)
        2  F's first look, alias 1       F reports row 1, and row 0 from the merge on: while it is not due
        3  B's look m + 2
        4  A's look m + 2, alias 3       A seems to be B's person while B is in the frame on row 3: a veto
        5  Cc's first look
        6  Cc's second look              one observation of (5, 6) in stream 2 only: pending for good
    The threshold is half the smallest distance between two different embeddings, so only equal bits match."""
    plain = _oracle_run(H, frames, embed, [], [], math.inf, min_obs=0)
    looks = _looks(plain)
    print("looks (stream, object): steps", {k: [t for t, _ in v] for k, v in looks.items()})
    steps_of = lambda key: [t for t, _ in looks[key]]
    zero = sorted(k for k in looks if k[0] == 0)
    A = max(zero, key=lambda k: (len(looks[k]), -k[1]))
    B = next(k for k in zero if k != A and steps_of(k) == steps_of(A))
    assert [e for _, e in looks[A]] == [e for _, e in looks[(1, A[1])]], "streams 0 and 1 are duplicates"
    two = sorted(k for k in looks if k[0] == 2)
    Cc = next(k for k in two if steps_of(k)[:1] == steps_of(A)[:1] and len(looks[k]) >= 3)
    pick = None
    for F in two:
        fs = steps_of(F) + [10 ** 6]
        for m in range(len(looks[A]) - 2):
            if steps_of(A)[m] < fs[0] < steps_of(A)[m + 1] < fs[1]:
                pick = pick or (F, m)
    assert pick, "no object of stream 2 is first embedded between two looks of A"
    F, m = pick
    emb = lambda key, i: np.frombuffer(looks[key][i][1], f32)
    rows = np.stack([emb(A, m), emb(A, m + 1), emb(F, 0), emb(B, m + 2), emb(A, m + 2), emb(Cc, 0), emb(Cc, 1)])
    pts = np.stack([np.frombuffer(e, f32) for e in {e for v in looks.values() for _, e in v}])
    smallest = min(float(np.delete(ER.distances(pts[i], pts), i).min()) for i in range(len(pts)))
    assert smallest > 0 and len(pts) >= 12, (smallest, len(pts))
    return {"rows": rows, "ids": [100 + r for r in range(len(rows))], "aliases": [0, 1, 1, 3, 3, 5, 6],
            "threshold": float(f32(0.5 * smallest)), "merge_step": steps_of(A)[m + 1], "veto_step": steps_of(A)[m + 2],
            "A": A, "B": B, "Cc": Cc, "F": F}


@pytest.fixture(scope="module")
def oracle(H, frames, embed, setup):
    return _oracle_run(H, frames, embed, setup["rows"], setup["ids"], setup["threshold"], setup["aliases"])


def _gallery(H, setup, aliases=True):
    g = TI._gallery(H, setup["rows"], setup["ids"])
    g.reserve(CAPACITY)
    if aliases:
        g.set_aliases(setup["aliases"])
    return g


def _tracker(H, model, gallery, threshold, min_obs):
    """min_obs None: set_identity_merging is never called."""
    dev = H.DeviceMultiTracker("face", "facemesh", S, K)
    dev.set_loss_threshold(-1.0)
    dev.set_redetect_interval(40.0)
    dev.set_recognition(model, gallery)
    dev.set_identify_interval(INTERVAL)
    dev.set_identity_threshold(threshold)
    if min_obs is not None:
        dev.set_identity_merging(gallery, min_obs)
    return dev


def _device_run(H, frames, model, gallery, threshold, min_obs, steps=STEPS):
    out = TT._steps(H, _tracker(H, model, gallery, threshold, min_obs), frames, 0, steps)
    for per_stream in out["identity"]:   # (nothing is enrolled here: the oracle's records say False)
        assert not any(rec[4] for objs in per_stream for _, rec in objs if rec is not None)
    out["gallery"] = gallery
    return out


@pytest.fixture(scope="module")
def device(H, frames, model, setup):
    return _device_run(H, frames, model, _gallery(H, setup), setup["threshold"], MIN_OBS)


def test_script_contains_the_events(oracle, setup):
    ref = oracle["ref"]
    print({k: v for k, v in setup.items() if k != "rows"})
    print("events", ref.link_events, "\nlinks", ref.links, "\ncounts", ref.counts)
    kinds = lambda kind: [(k, s, oid, due, ev) for k, s, oid, due, ev in ref.link_events if ev[0] == kind]
    # the merge (0, 1): stream 0's observation and stream 1's in one step
    merges = kinds("merge")
    assert [(k, s, ev[2:]) for k, s, _, _, ev in merges] == [(setup["merge_step"], 1, (0, 1))]
    assert [(k, s, ev[2:]) for k, s, _, _, ev in kinds("observe") if k == setup["merge_step"] and s < 2] == \
        [(setup["merge_step"], 0, (0, 1, 1)), (setup["merge_step"], 1, (0, 1, 2))]
    # the vetoes: A against B's person, once per stream
    assert [(k, s, ev[2:4]) for k, s, _, _, ev in kinds("veto")] == [(setup["veto_step"], 0, (0, 3)), (setup["veto_step"], 1, (0, 3))]
    # an observation that never completed
    assert (ref.links[6]["alias"], ref.links[6]["partner"], ref.links[6]["seen"]) == (6, 5, 1)
    # a reported row changed by canonicalisation in a step where its object was not due
    late = [(k, s, oid, ev) for k, s, oid, due, ev in kinds("canonicalise") if not due]
    assert late and (late[0][0], late[0][1], late[0][2], late[0][3][2:]) == (setup["merge_step"], 2, setup["F"][1], (1, 0))
    assert ref.counts == {"merged": 1, "vetoed": 2, "observed": 3}
    assert [l["alias"] for l in ref.links[:7]] == [0, 0, 0, 3, 3, 5, 6]
    # what the objects report: F is person 101 (row 1) before the merge and person 100 from the merge on
    ids = {k: dict(oracle["identity"][k][2]).get(setup["F"][1]) for k in range(STEPS)}
    assert ids[setup["merge_step"] - 1][0] == 101 and ids[setup["merge_step"]][0] == 100
    assert ids[setup["merge_step"]][2] == ids[setup["merge_step"] - 1][2]   # no new embedding in between


def _compare(oracle, device, steps=STEPS):
    compared = 0
    for k in range(steps):
        for s in range(S):
            assert device["track"][k][s] == oracle["track"][k][s], ("tracking", k, s)
            w, g = oracle["identity"][k][s], device["identity"][k][s]
            assert [i for i, _ in g] == [i for i, _ in w], ("ids", k, s)
            for (oid, wr), (_, gr) in zip(w, g):
                assert (gr is None) == (wr is None), ("identified", k, s, oid)
                if wr is None:
                    continue
                for field, name in enumerate(("id", "distance", "embeddings", "embedding", "enrolled")):
                    assert gr[field] == wr[field], (name, k, s, oid, gr[:3], wr[:3])
                compared += 1
    return compared


def _table(ref, count):
    return ([l["alias"] for l in ref.links[:count]], [l["partner"] for l in ref.links[:count]],
            [l["seen"] for l in ref.links[:count]])


def test_loop_against_the_oracle(oracle, device, setup):
    assert _compare(oracle, device) >= 30
    gal, dev, ref = device["gallery"], device["dev"], oracle["ref"]
    alias, partner, seen = _table(ref, len(gal))
    got_partner, got_seen = gal.pending_links()
    assert gal.aliases().tolist() == alias and got_partner.tolist() == partner and got_seen.tolist() == seen
    assert (dev.merged_total(), dev.merge_vetoed_total(), dev.merge_observed_total()) == \
        (ref.counts["merged"], ref.counts["vetoed"], ref.counts["observed"])
    rows, ids = gal.rows()
    assert rows.tobytes() == setup["rows"].tobytes() and list(ids) == setup["ids"] and not gal.row_updates().any()
    assert gal.person_ids().tolist() == [100, 100, 100, 103, 103, 105, 106]
    # the packed export derives the person from the row it is handed, like objects(): the canonical one
    p = dev.objects_packed()
    want = {(s, oid): rec for s in range(S) for oid, rec in oracle["identity"][STEPS - 1][s]}
    packed = {(int(p["stream"][k]), int(p["id"][k])): int(p["identity_id"][k]) for k in range(p["count"])
              if p["identity_present"][k]}
    assert packed == {key: rec[0] for key, rec in want.items() if rec is not None} and 103 in packed.values()
    assert dev.identity_merging()["min_observations"] == MIN_OBS and math.isnan(dev.identity_merging()["link_threshold"])


def test_merging_that_cannot_merge_moves_no_bit(H, frames, model, setup):
    """0xffffffff observations are never reached: against the loop with merging never set, on galleries whose
    tables start at their defaults."""
    runs = []
    for min_obs in (None, 0xFFFFFFFF):
        g = _gallery(H, setup, aliases=False)
        run = _device_run(H, frames, model, g, setup["threshold"], min_obs)
        rows, ids = g.rows()
        runs.append((run["identity"], run["track"], rows.tobytes(), list(ids), g.row_updates().tolist()))
        assert g.aliases().tolist() == list(range(len(g)))
        dev = run["dev"]
        assert dev.merged_total() == 0 and (dev.identity_merging() is None) == (min_obs is None)
        assert (dev.merge_observed_total() > 0) == (min_obs is not None)   # it did look
    assert runs[0] == runs[1]


def test_read_only_mode(H, frames, embed, model, setup, oracle, device):
    """A second tracker with min_observations = 0 on the merged gallery: canonical rows, no record written."""
    gal = device["gallery"]
    before = (gal.aliases().tolist(), [a.tolist() for a in gal.pending_links()])
    want = _oracle_run(H, frames, embed, setup["rows"], setup["ids"], setup["threshold"], min_obs=0,
                       links=copy.deepcopy(oracle["ref"].links))
    run = _device_run(H, frames, model, gal, setup["threshold"], 0)
    assert _compare(want, run) >= 30
    assert (gal.aliases().tolist(), [a.tolist() for a in gal.pending_links()]) == before
    dev = run["dev"]
    assert (dev.merged_total(), dev.merge_vetoed_total(), dev.merge_observed_total()) == (0, 0, 0)
    seen = {rec[0] for per_stream in run["identity"] for objs in per_stream for _, rec in objs if rec is not None}
    assert 100 in seen and 103 in seen and not seen & {101, 102, 104}


def test_saved_and_reloaded_table(H, frames, model, setup):
    """A run, then the script again on the gallery it left (its pending records reset, as a load does) and on
    a fresh gallery loaded from rows() + aliases(): the same bits."""
    first = _device_run(H, frames, model, _gallery(H, setup), setup["threshold"], MIN_OBS)
    g = first["gallery"]
    rows, ids = g.rows()
    aliases = g.aliases().tolist()
    assert aliases == [0, 0, 0, 3, 3, 5, 6] and g.pending_links()[1].any()
    g.set_aliases(aliases)
    assert not g.pending_links()[1].any() and g.pending_links()[0].tolist() == [-1] * len(g)
    fresh = H.Gallery()
    fresh.reserve(CAPACITY)
    fresh.add(rows, list(ids))
    assert fresh.aliases().tolist() == list(range(len(ids)))
    fresh.set_aliases(aliases)
    outs = []
    for gal in (g, fresh):
        run = _device_run(H, frames, model, gal, setup["threshold"], MIN_OBS)
        outs.append((run["identity"], run["track"], gal.aliases().tolist(), [a.tolist() for a in gal.pending_links()],
                     run["dev"].merge_vetoed_total(), run["dev"].merge_observed_total()))
    assert outs[0] == outs[1] and outs[0][4] == 2 and outs[0][2] == aliases
    people = {rec[0] for per_stream in outs[0][0] for objs in per_stream for _, rec in objs if rec is not None}
    assert 100 in people and 101 not in people
    # a plain multi-template gallery of the merged people: the higher row answers with the person's id
    loose = H.Gallery()
    loose.add(rows, g.person_ids().tolist())
    got_ids, got_d = loose.match(rows)
    assert got_ids.tolist() == [100, 100, 100, 103, 103, 105, 106] and (got_d == 0).all()


def test_merge_rows_and_set_aliases(H, setup):
    g = _gallery(H, setup, aliases=False)
    n = len(g)
    assert g.aliases().tolist() == list(range(n)) and g.pending_links()[0].tolist() == [-1] * n
    assert g.merge_rows(4, 2) == 2 and g.merge_rows(6, 4) == 2 and g.merge_rows(2, 6) == 2
    assert g.aliases().tolist() == [0, 1, 2, 3, 2, 5, 2]
    assert g.merge_rows(6, 1) == 1 and g.aliases().tolist() == [0, 1, 1, 3, 1, 5, 1]   # the lower canonical row wins
    assert g.person_ids().tolist() == [100, 101, 101, 103, 101, 105, 101] and g.id_of(1) == 101
    for a, b in ((-1, 0), (0, n), (n, n), (0, -2)):
        with pytest.raises(RuntimeError):
            g.merge_rows(a, b)
    for bad in ([0, 1, 1, 3, 1, 5], [0, 1, 1, 3, 1, 5, 1, 1], [0, 1, 3, 3, 4, 5, 6], [0, 0, 1, 3, 4, 5, 6],
                [0, -1, 2, 3, 4, 5, 6], [1, 1, 2, 3, 4, 5, 6]):
        with pytest.raises(RuntimeError):
            g.set_aliases(bad)
    assert g.aliases().tolist() == [0, 1, 1, 3, 1, 5, 1]   # a refused table changes nothing
    g.set_aliases(list(range(n)))
    assert g.aliases().tolist() == list(range(n))
    g.merge_rows(0, 1)
    g.clear()
    g.add(setup["rows"][:3], [1, 2, 3])
    assert g.aliases().tolist() == [0, 1, 2]   # clear() wrote the defaults
    loose = TI._gallery(H, setup["rows"], setup["ids"])
    for call in (loose.aliases, loose.person_ids, loose.pending_links, lambda: loose.set_aliases(list(range(n))),
                 lambda: loose.merge_rows(0, 1)):
        with pytest.raises(RuntimeError):
            call()


def test_setter_refusals(H, model, setup):
    dev = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    g, other, loose = _gallery(H, setup), _gallery(H, setup), TI._gallery(H, setup["rows"], setup["ids"])
    with pytest.raises(RuntimeError):
        dev.set_identity_merging(g)            # no recognition yet
    dev.set_recognition(model, g)
    with pytest.raises(RuntimeError):
        dev.set_identity_merging(other)        # not the recognition gallery
    dev.set_recognition(model, loose)
    with pytest.raises(RuntimeError):
        dev.set_identity_merging(loose)        # not reserved
    dev.set_recognition(model, g)
    assert dev.identity_merging() is None and dev.merged_total() == 0
    dev.set_identity_merging(g, 5, 0.75)
    assert dev.identity_merging() == {"min_observations": 5, "link_threshold": 0.75}
    dev.set_identity_merging(None)
    assert dev.identity_merging() is None
    dev.set_identity_merging(g)
    assert dev.identity_merging()["min_observations"] == 3
    dev.set_recognition(model, g)              # every set_recognition turns it off
    assert dev.identity_merging() is None
    # one writer at a time: a merging tracker that has stepped and not synchronised keeps others out
    dev.set_identity_merging(g)
    second = H.DeviceMultiTracker("face", "facemesh", 1, 2)
    second.set_recognition(model, g)
    second.set_identity_merging(g, 1)
    from zaru_amd._lib import DeviceBuffer
    buf = DeviceBuffer.from_array(np.zeros((FH, FW, 4), np.uint8))
    view = [(buf.ptr, FW, FH, FW * 4)]
    dev.step(view, 0.0)
    with pytest.raises(RuntimeError):
        second.step(view, 0.0)
    with pytest.raises(RuntimeError):
        second.set_identity_merging(g, 2)
    reader = H.DeviceMultiTracker("face", "facemesh", 1, 2)   # min_observations = 0 is no writer: it may step
    reader.set_recognition(model, g)
    reader.set_identity_merging(g, 0)
    reader.step(view, 0.0)
    dev.synchronize()
    second.step(view, 0.0)
    second.synchronize()
    reader.synchronize()
