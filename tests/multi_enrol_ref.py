"""The oracle of automatic enrolment (DeviceMultiTracker.set_enrolment, zr_identity_enrol_async).

``enrol_step`` is the sequential rule alone, over plain records in row order, in numpy f32 with one
rounding per operation in match.hip's order; it needs no GPU.  ``MultiEnrolRef`` is the loop: one
tests/multi_tracker_ref.py tracker per stream, every due object embedded and matched as
tests/multi_identity_ref.py does it, then the rule over all streams' objects (stream-major, slot
order), then the bookkeeping.  ``embed`` and ``match`` are the caller's, as there.
"""
import math

import numpy as np

import multi_identity_ref as IR

f32 = np.float32
EVER_KNOWN, ENROLLED = 1, 2
NO_MATCH = IR.NO_MATCH


def distances(a, rows):
    """Embedding::difference of `a` against every row of `rows` ([m][D]): d = a[k] - b[k]; s = s + d * d
    for k in order, each operation rounded to f32 on its own, then a correctly rounded sqrt."""
    a = np.asarray(a, f32)
    rows = np.asarray(rows, f32).reshape(-1, a.shape[0])
    s = np.zeros(len(rows), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(a.shape[0]):
            d = a[k] - rows[:, k]
            s = s + d * d
        return np.sqrt(s)


def nearest(dist, first=0):
    """(row, distance) of the smallest distance, the lowest row among equals, a NaN never; None if
    there is none."""
    best = None
    for j, d in enumerate(dist):
        if d == d and (best is None or d < best[1]):
            best = (first + j, d)
    return best


class GalleryRef:
    def __init__(self, capacity, rows=(), ids=(), next_id=0):
        self.capacity = capacity
        self.rows = [np.asarray(r, f32).copy() for r in rows]
        self.ids = list(ids)
        self.next_id = next_id
        self.enrolled_total = 0
        self.dropped = 0


def enrol_step(items, gallery, threshold, min_embeddings=1):
    """items: the rows in row order, dicts with "due" (bool), "row", "distance", "embeddings", "flags"
    and "embedding" as the commit left them; changed in place.  Returns the events, (index, kind, row)
    with kind in "known" (a due row that had a row), "match" (a row appended earlier in this call),
    "enrol", "dropped"."""
    first = len(gallery.rows)
    thr = f32(threshold)
    events = []
    for i, it in enumerate(items):
        if not it["due"]:
            continue
        if it["row"] >= 0:
            it["flags"] |= EVER_KNOWN
            events.append((i, "known", it["row"]))
            continue
        e = np.asarray(it["embedding"], f32)
        if it["row"] != -1 or it["flags"] & EVER_KNOWN or it["embeddings"] < min_embeddings \
                or not np.isfinite(e).all():
            continue
        best = nearest(distances(e, gallery.rows[first:]), first) if len(gallery.rows) > first else None
        if best is not None and best[1] <= thr:   # False for a NaN threshold
            it["row"], it["distance"] = best[0], f32(best[1])
            it["flags"] |= EVER_KNOWN
            events.append((i, "match", best[0]))
        elif len(gallery.rows) < gallery.capacity:
            row = len(gallery.rows)
            gallery.rows.append(e.copy())
            gallery.ids.append(gallery.next_id)
            gallery.next_id += 1
            gallery.enrolled_total += 1
            it["row"], it["distance"] = row, f32(0.0)
            it["flags"] |= EVER_KNOWN | ENROLLED
            events.append((i, "enrol", row))
        else:
            gallery.dropped += 1
            events.append((i, "dropped", -1))
    return events


class MultiEnrolRef:
    def __init__(self, H, trackers, embed, match, gallery, on_append=None, interval=1000.0, threshold=math.inf,
                 min_embeddings=1, enrol=True):
        """trackers: one MultiTrackerRef per stream.  embed(frame, H.Rect) -> 128 floats;
        match(embedding) -> (id or NO_MATCH, distance) against the rows the gallery had before this
        step; gallery: a GalleryRef with those rows; on_append(rows, ids) makes `match` see a step's
        new rows from the next step on."""
        self.H, self.trackers, self.embed, self.match = H, trackers, embed, match
        self.gallery, self.on_append = gallery, on_append
        self.interval, self.threshold, self.min_embeddings, self.enrol = interval, threshold, min_embeddings, enrol
        self.images = 0
        self.events = []   # (step, stream, object id, kind, row)
        self.k = 0

    def step(self, frames, now_ms, injected):
        items, owners = [], []
        for s, t in enumerate(self.trackers):
            for o in t.objs:   # slot order
                if o.pending is None:
                    continue
                identity = getattr(o, "identity", None)
                if not IR.is_due(identity, now_ms):
                    continue
                xy = [(float(p[0]), float(p[1])) for p in o.pending["landmarks"]]
                if not all(math.isfinite(v) for p in xy for v in p):
                    continue
                e = np.asarray(self.embed(frames[s], self.H.Rect.bounding(xy)), f32)
                best, dist = self.match(e)
                pid = IR.known(best, dist, self.threshold)
                o.identity = {"id": pid, "distance": f32(dist), "embedding": e, "next_ms": now_ms + self.interval,
                              "embeddings": (identity["embeddings"] if identity else 0) + 1,
                              "flags": identity["flags"] if identity else 0}
                self.images += 1
                # the rule sees a row index: any row >= 0 for a known object, -1 for an unknown one
                items.append({"due": True, "row": 0 if pid != NO_MATCH else -1, "distance": f32(dist),
                              "embeddings": o.identity["embeddings"], "flags": o.identity["flags"], "embedding": e})
                owners.append((s, o))
        if self.enrol:
            before = len(self.gallery.rows)
            for i, kind, row in enrol_step(items, self.gallery, self.threshold, self.min_embeddings):
                s, o = owners[i]
                self.events.append((self.k, s, o.id, kind, row))
                o.identity["flags"] = items[i]["flags"]
                if kind in ("match", "enrol"):
                    o.identity["id"], o.identity["distance"] = self.gallery.ids[row], items[i]["distance"]
            if self.on_append and len(self.gallery.rows) > before:
                self.on_append(np.stack(self.gallery.rows[before:]), self.gallery.ids[before:])
        for s, t in enumerate(self.trackers):
            t.step(frames[s], now_ms, injected[s])
        self.k += 1

    def objects(self, s):
        """(object, identity or None) for stream s's objects that have a result, in order."""
        return [(o, getattr(o, "identity", None)) for o in self.trackers[s].objects()]
