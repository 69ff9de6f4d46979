"""The oracle of merging duplicate gallery rows (DeviceMultiTracker.set_identity_merging,
zr_identity_link_async): the sequential rule of include/zaru_hip.h as plain Python over lists of dicts;
it needs no GPU.

``link_step`` is the rule alone: pass 1 over the rows in row order, then pass 2.  ``MultiMergeRef`` is
the loop: tests/multi_template_ref.py's, with the rule after the enrolment and before the bookkeeping.
"""
import math

import numpy as np

import multi_identity_ref as IR
import multi_template_ref as TR

f32 = np.float32
NO_MATCH = IR.NO_MATCH
U32 = 0xFFFFFFFF


def default_links(capacity):
    return [{"alias": r, "partner": -1, "seen": 0, "reserved": 0} for r in range(capacity)]


def alias(links, r):
    """The canonical row of r; a stored alias outside [0, r] reads as r."""
    a = links[r]["alias"]
    return a if 0 <= a <= r else r


def is_flat(links, count):
    return all(alias(links, alias(links, r)) == alias(links, r) for r in range(count))


def link_step(tracked, src, due_of, st_in, st_out, links, count, slots, min_observations, threshold, counts=None):
    """tracked, src, due_of: one entry per row; st_in, st_out: the rows' identity states before and after
    the step, dicts with "row" and "distance" (st_out is changed in place: pass 2); links: the table,
    dicts as default_links makes them, changed in place; count: the device's row count (clamped here);
    counts: None or a dict whose "merged", "vetoed" and "observed" are added to.
    Returns the events: ("observe", i, lo, hi, seen), ("veto", i, lo, hi, j), ("merge", i, lo, hi),
    ("canonicalise", i, from, to)."""
    n = len(st_out)
    assert n % slots == 0 and len(st_in) == n
    G = min(max(int(count), 0), len(links))
    thr = f32(threshold)
    events = []
    tally = {"merged": 0, "vetoed": 0, "observed": 0}
    for i in range(n if min_observations else 0):
        if not (0 <= due_of[i] < n and tracked[i] and 0 <= src[i] < slots):
            continue
        base = i // slots * slots
        carried = st_in[base + src[i]]
        p, b = int(carried["row"]), int(st_out[i]["row"])
        if not (0 <= p < G and 0 <= b < G):
            continue
        if not (f32(carried["distance"]) <= thr and f32(st_out[i]["distance"]) <= thr):   # False for a NaN
            continue
        ap, ab = alias(links, p), alias(links, b)
        if ap == ab:
            continue
        lo, hi = min(ap, ab), max(ap, ab)
        veto = None
        for j in range(base, base + slots):
            r = int(st_out[j]["row"])
            if j != i and tracked[j] and 0 <= r < G and alias(links, r) in (lo, hi):
                veto = j
                break
        if veto is not None:
            links[hi].update(alias=hi, partner=-1, seen=0, reserved=0)
            tally["vetoed"] += 1
            events.append(("veto", i, lo, hi, veto))
            continue
        tally["observed"] += 1
        seen = (links[hi]["seen"] + 1) & U32 if links[hi]["partner"] == lo else 1
        events.append(("observe", i, lo, hi, seen))
        if seen >= min_observations:
            for r in range(G):
                if alias(links, r) == hi:
                    links[r]["alias"] = lo
            links[hi].update(partner=-1, seen=0)
            tally["merged"] += 1
            events.append(("merge", i, lo, hi))
        else:
            links[hi].update(partner=lo, seen=seen)
    for i in range(n):
        r = int(st_out[i]["row"])
        if 0 <= r < G and alias(links, r) != r:
            st_out[i]["row"] = alias(links, r)
            events.append(("canonicalise", i, r, st_out[i]["row"]))
    if counts is not None:
        for k, v in tally.items():
            counts[k] += v
    return events


class MultiMergeRef(TR.MultiTemplateRef):
    """MultiTemplateRef with the rule after each step's enrolment.  The parent keeps a person id per
    object; the gallery's ids are distinct, so the row is their index.  An object that the parent's step
    gave a new identity record was due; its previous record is what the device's select carried."""

    def __init__(self, *a, slots, merge_capacity, min_observations=3, link_threshold=math.nan, links=None, **kw):
        super().__init__(*a, **kw)
        self.slots = slots
        self.links = links if links is not None else default_links(merge_capacity)
        self.min_observations = min_observations
        self.link_threshold = link_threshold
        self.counts = {"merged": 0, "vetoed": 0, "observed": 0}
        self.link_events = []   # (step, stream, object id, due, event)

    def _row(self, identity):
        if identity is None or identity["id"] == NO_MATCH:
            return -1
        return self.gallery.ids.index(identity["id"])

    def step(self, frames, now_ms, injected):
        k, slots = self.k, self.slots
        before = [[(o, getattr(o, "identity", None)) for o in t.objs if o.pending is not None] for t in self.trackers]
        # the parent's bookkeeping moves and drops objects, not their identities: the rule may follow it
        super().step(frames, now_ms, injected)
        # one row per tracked object in slot order, each stream padded to `slots` rows with untracked ones
        # (the rule reads a row's stream and its order in it, never the slot itself)
        tracked, src, due_of, st_in, st_out, owners = [], [], [], [], [], []
        default = {"row": -1, "distance": f32(math.inf)}
        for s, objs in enumerate(before):
            assert len(objs) <= slots
            for j in range(slots):
                if j >= len(objs):
                    tracked.append(0), src.append(-1), due_of.append(-1), owners.append(None)
                    st_in.append(dict(default)), st_out.append(dict(default))
                    continue
                o, was = objs[j]
                now = getattr(o, "identity", None)
                due = now is not was
                tracked.append(1), src.append(j), due_of.append(len(due_of) if due else -1), owners.append((s, o, due))
                st_in.append({"row": self._row(was), "distance": was["distance"] if was else f32(math.inf)})
                st_out.append({"row": self._row(now), "distance": now["distance"] if now else f32(math.inf)})
        thr = self.threshold if math.isnan(self.link_threshold) else self.link_threshold
        for ev in link_step(tracked, src, due_of, st_in, st_out, self.links, len(self.gallery.rows), slots,
                            self.min_observations, thr, self.counts):
            s, o, due = owners[ev[1]]
            self.link_events.append((k, s, o.id, due, ev))
            if ev[0] == "canonicalise":
                o.identity["id"] = self.gallery.ids[ev[3]]
