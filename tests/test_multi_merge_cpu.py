"""Merging duplicate gallery rows, the parts that need no GPU:

  * zr_gallery_link's layout and the argument refusals of zr_identity_link_async (nothing is launched: the
    pointers are made up);
  * the sequential rule of tests/multi_merge_ref.py on a hand-written timeline.
"""
import ctypes as C
import math

import numpy as np

from zaru_amd import _lib

import multi_merge_ref as MG

f32 = np.float32


def _icfg(**kw):
    v = dict(slots=4, num_landmarks=468, aspect_w=1, aspect_h=1, crop_grow=0.4, threshold=math.inf, interval_ms=1000.0)
    v.update(kw)
    return _lib.IdentityCfg(**v)


def test_link_record_layout():
    L = _lib.GalleryLink
    assert C.sizeof(L) == 16
    assert (L.alias.offset, L.partner.offset, L.seen.offset, L.reserved.offset) == (0, 4, 8, 12)
    assert all(getattr(L, f).size == 4 for f in ("alias", "partner", "seen", "reserved"))


def test_entry_point_refuses_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    p, q = 4096, 8192  # stand for device pointers: none of these calls gets as far as using them

    def link(c=_icfg(), n=8, cap=16, min_obs=3, thr=0.5, **kw):
        a = dict(state=p, src=p, of=p, sin=p, sout=q, links=p, count=p, counts=p)
        a.update(kw)
        return lib.zr_identity_link_async(None if c is None else C.byref(c), a["state"], n, a["src"], a["of"], a["sin"],
                                          a["sout"], a["links"], a["count"], cap, min_obs, thr, a["counts"], None)

    assert link(c=None) == -1
    for name in ("state", "src", "of", "sin", "sout", "links", "count"):
        assert link(**{name: None}) == -1, name
    assert link(n=0) == -1 and link(n=(1 << 24) + 4) == -1
    for n, slots in ((8, 0), (8, 65), (9, 4), (8, -1)):
        assert link(c=_icfg(slots=slots), n=n) == -1, (n, slots)
    assert link(cap=0) == -1 and link(cap=2 ** 31) == -1
    assert link(sin=q, sout=q) == -1
    # min_observations (0, 0xffffffff), the threshold (NaN, +inf) and a NULL d_counts are settings, not errors:
    # checked on the GPU, where they run


# ---- the rule on a timeline ---------------------------------------------------------------------
SLOTS = 4


class Timeline:
    """Two streams of four slots over a gallery of 8 rows in use (capacity 10).  Every slot holds one
    object that stays where it is (src = own slot); a step names, per row, the nearest row of a due
    object's new look, at distance 0.25."""

    def __init__(self, min_observations, threshold=0.5, count=8, capacity=10):
        self.n = 2 * SLOTS
        self.links = MG.default_links(capacity)
        self.count, self.min_observations, self.threshold = count, min_observations, threshold
        self.state = [{"row": -1, "distance": f32(math.inf)} for _ in range(self.n)]
        self.tracked = [1] * self.n
        self.counts = {"merged": 0, "vetoed": 0, "observed": 0}

    def step(self, looks, src=None, tracked=None, distance=0.25):
        """looks: {row index: nearest gallery row}; rows not named are not due."""
        st_in = [dict(s) for s in self.state]
        st_out = [dict(s) for s in self.state]
        due_of = [-1] * self.n
        for k, (i, row) in enumerate(sorted(looks.items())):
            st_out[i] = {"row": row, "distance": f32(distance)}
            due_of[i] = k
        src = src or [i % SLOTS for i in range(self.n)]
        ev = MG.link_step(tracked or self.tracked, src, due_of, st_in, st_out, self.links, self.count, SLOTS,
                          self.min_observations, self.threshold, self.counts)
        self.state = st_out
        assert MG.is_flat(self.links, self.count), self.links
        assert all(l["alias"] <= r for r, l in enumerate(self.links))
        assert self.links[self.count:] == MG.default_links(len(self.links))[self.count:]   # the invariant
        return ev

    def rows(self):
        return [s["row"] for s in self.state]

    def link(self, r):
        return (self.links[r]["alias"], self.links[r]["partner"], self.links[r]["seen"])


def test_rule_on_a_timeline():
    t = Timeline(min_observations=2)
    # step 1: first looks; nobody has a history, so nothing is evidence
    assert t.step({0: 0, 1: 4, 4: 2, 5: 6}) == []
    # step 2: object 0 flips 0 -> 1 (one observation: pending), object 4 flips 2 -> 3 (pending)
    assert t.step({0: 1, 4: 3}) == [("observe", 0, 0, 1, 1), ("observe", 4, 2, 3, 1)]
    assert t.link(1) == (1, 0, 1) and t.link(3) == (3, 2, 1) and t.rows()[0] == 1
    # step 3: object 0 flips back 1 -> 0: the second observation of (0, 1), across two steps: merge; object 0
    # then reports row 0 (it does already).  Object 4 stays on 3: the same person twice is no evidence.
    assert t.step({0: 0, 4: 3}) == [("observe", 0, 0, 1, 2), ("merge", 0, 0, 1)]
    assert t.link(1) == (0, -1, 0) and t.counts == {"merged": 1, "vetoed": 0, "observed": 3}
    # step 4: object 0's nearest row is 1 again: the same person now (no evidence), reported as row 0 by
    # pass 2; object 5 (stream 1) holds 6
    assert t.step({0: 1}) == [("canonicalise", 0, 1, 0)] and t.rows()[0] == 0
    # step 5: a veto that resets a pending count of 1.  Object 4 flips 3 -> 2 (second sighting of (2, 3)), but
    # object 6 of its stream holds row 2 from this step on: both are in the frame (the veto reads the states
    # of this step, so a row that comes later in the walk counts)
    ev = t.step({4: 2, 6: 2})
    assert ev == [("veto", 4, 2, 3, 6)] and t.link(3) == (3, -1, 0) and t.counts["vetoed"] == 1


def test_a_pending_record_is_replaced_by_a_different_partner():
    t = Timeline(min_observations=2)
    t.step({1: 4, 2: 5})                   # two objects of stream 0 on rows 4 and 5: two people
    assert t.step({1: 6}) == [("observe", 1, 4, 6, 1)] and t.link(6) == (6, 4, 1)
    gone = [1] * t.n
    gone[1] = 0                            # object 1 leaves; object 2 flips 5 -> 6
    assert t.step({2: 6}, tracked=gone) == [("observe", 2, 5, 6, 1)] and t.link(6) == (6, 5, 1)
    # with object 1 still in the frame on row 6 it would have been a veto
    t = Timeline(min_observations=2)
    t.step({1: 4, 2: 5})
    t.step({1: 6})
    assert t.step({2: 6}) == [("veto", 2, 5, 6, 1)] and t.link(6) == (6, -1, 0)


def test_two_streams_complete_a_merge_in_one_step_and_a_chain():
    t = Timeline(min_observations=2)
    t.step({0: 0, 4: 0, 1: 2})
    # two observations within one step, from two streams
    ev = t.step({0: 1, 4: 1})
    assert ev == [("observe", 0, 0, 1, 1), ("observe", 4, 0, 1, 2), ("merge", 4, 0, 1), ("canonicalise", 0, 1, 0),
                  ("canonicalise", 4, 1, 0)]
    assert t.counts == {"merged": 1, "vetoed": 0, "observed": 2}
    # a chain within one call, min_observations 1: (0, 1) merges at row 0, then p = 2, b = 1 is the pair (0, 2)
    t = Timeline(min_observations=1)
    t.step({0: 0, 5: 2})
    ev = t.step({0: 1, 5: 1})
    assert ev == [("observe", 0, 0, 1, 1), ("merge", 0, 0, 1), ("observe", 5, 0, 2, 1), ("merge", 5, 0, 2),
                  ("canonicalise", 0, 1, 0), ("canonicalise", 5, 1, 0)]
    assert [l["alias"] for l in t.links[:4]] == [0, 0, 0, 3]
    # a person of three rows relabelled as one: rows 3 and 4 merge, then (0, 3) takes both along
    t.step({2: 3})
    t.step({2: 4})
    assert [l["alias"] for l in t.links[:5]] == [0, 0, 0, 3, 3]
    assert ("merge", 5, 0, 3) in t.step({5: 4}) and [l["alias"] for l in t.links[:5]] == [0] * 5


def test_new_and_untracked_rows_are_ignored():
    t = Timeline(min_observations=1)
    t.step({0: 0, 1: 2, 2: 4})
    src = [i % SLOTS for i in range(t.n)]
    src[0], src[1] = -1, SLOTS             # new objects: no history
    tracked = [1] * t.n
    tracked[2] = 0
    assert t.step({0: 1, 1: 3, 2: 5}, src=src, tracked=tracked) == [] and t.counts["observed"] == 0
    # an object that moved between slots takes its history along: row 3 now holds what slot 1 held (row 3)
    src = [i % SLOTS for i in range(t.n)]
    src[3] = 1
    tracked = [1] * t.n
    tracked[1] = 0                         # (the slot it left is empty)
    assert t.step({3: 2}, src=src, tracked=tracked)[:2] == [("observe", 3, 2, 3, 1), ("merge", 3, 2, 3)]
    # an untracked row of the stream does not veto either
    t = Timeline(min_observations=1)
    t.step({0: 0, 1: 1})
    tracked = [1] * t.n
    tracked[1] = 0
    assert t.step({0: 1}, tracked=tracked)[0] == ("observe", 0, 0, 1, 1)
    # rows at or past the count are no evidence, and are not canonicalised
    t = Timeline(min_observations=1, count=4)
    t.step({0: 0, 1: 5})
    assert t.step({0: 4, 1: 3}) == [] and t.rows()[:2] == [4, 3]


def test_thresholds_and_read_only_mode():
    for thr, want in ((math.nan, 0), (math.inf, 1), (0.25, 1), (0.2499, 0), (0.0, 0)):
        t = Timeline(min_observations=3, threshold=thr)
        t.step({0: 0})
        assert len(t.step({0: 1})) == want, thr
    t = Timeline(min_observations=3, threshold=math.inf)
    t.step({0: 0}, distance=math.inf)
    assert t.step({0: 1}, distance=1e30) == [("observe", 0, 0, 1, 1)]      # +inf: every known pair
    # min_observations = 0: pass 1 is skipped, pass 2 runs
    t = Timeline(min_observations=0)
    t.links[1]["alias"] = 0
    t.step({0: 0})
    assert t.step({0: 1, 1: 3, 2: 2}) == [("canonicalise", 0, 1, 0)] and t.rows()[:3] == [0, 3, 2]
    assert t.counts == {"merged": 0, "vetoed": 0, "observed": 0} and t.link(3) == (3, -1, 0)
    # an alias outside [0, r] reads as r
    for bad in (-1, 3, 2 ** 31 - 1):
        links = MG.default_links(4)
        links[2]["alias"] = bad
        assert MG.alias(links, 2) == 2
