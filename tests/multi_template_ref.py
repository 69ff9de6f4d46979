"""The oracle of identities that learn (DeviceMultiTracker.set_identity_smoothing /
set_gallery_refinement, zr_identity_blend_async / zr_identity_refine_async), in numpy f32 with one
rounding per operation; it needs no GPU.

One update of a vector m by a sample e with the divisor w is, per float, ``m + (e - m) / f32(w)``.

``blend`` is the object's template, ``refine`` the gallery rows' running means over plain records in
row order, and ``MultiTemplateRef`` the loop: tests/multi_enrol_ref.py's, with the blend before the
match, the refinement between the commit and the enrolment, and the gallery the matches see rebuilt
from the reference's rows after every step that changed them.
"""
import math

import numpy as np

import multi_enrol_ref as ER
import multi_identity_ref as IR

f32 = np.float32
U32_MAX = 0xFFFFFFFF
NO_MATCH = IR.NO_MATCH


def update(m, e, w):
    """m + (e - m) / f32(w): the subtraction, the division and the addition each rounded to f32."""
    m, e = np.asarray(m, f32), np.asarray(e, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (m + (e - m) / f32(w)).astype(f32)


def blend(t, e, c, template_cap):
    """The query of a due object: t its stored embedding, e this step's network output, c its
    embeddings before this step.  e itself (the same bits) when c == 0 or t or e is not finite."""
    t, e = np.asarray(t, f32), np.asarray(e, f32)
    if c == 0 or not (np.isfinite(t).all() and np.isfinite(e).all()):
        return e.copy()
    return update(t, e, min(c + 1, template_cap))


def refine(items, rows, updates, count, max_samples, threshold):
    """items: the rows in row order, dicts with "due" (bool), "row", "distance" as the commit left them
    and "sample" (the raw network output); rows: the gallery's allocation, a list of f32 vectors or an
    [capacity][128] array; updates: its counts; count: the device's row count.  rows and updates are
    changed in place.  Returns the contributions, (index, row, w)."""
    limit = min(max(int(count), 0), len(rows))
    thr = f32(threshold)
    done = []
    for i, it in enumerate(items):
        r = int(it["row"])
        if not it["due"] or not 0 <= r < limit:
            continue
        if not f32(it["distance"]) <= thr:   # False for a NaN on either side
            continue
        e = np.asarray(it["sample"], f32)
        if not np.isfinite(e).all():
            continue
        w = min(int(updates[r]) + 2, max_samples)
        rows[r] = update(rows[r], e, w)
        updates[r] = min(int(updates[r]) + 1, U32_MAX)
        done.append((i, r, w))
    return done


class MultiTemplateRef:
    def __init__(self, H, trackers, embed, make_match, gallery, interval=1000.0, threshold=math.inf,
                 template_cap=1, refine=False, max_samples=64, update_threshold=math.nan, enrol=False,
                 min_embeddings=1):
        """trackers: one MultiTrackerRef per stream.  embed(frame, H.Rect) -> 128 floats;
        make_match(rows, ids) -> match(embedding) -> (id or NO_MATCH, distance) against those rows;
        gallery: an ER.GalleryRef (its ids are distinct).  update_threshold NaN: the identity threshold."""
        self.H, self.trackers, self.embed, self.make_match = H, trackers, embed, make_match
        self.gallery = gallery
        self.updates = [0] * len(gallery.rows)
        self.interval, self.threshold = interval, threshold
        self.template_cap, self.refining, self.max_samples = template_cap, refine, max_samples
        self.update_threshold = threshold if math.isnan(update_threshold) else update_threshold
        self.enrol, self.min_embeddings = enrol, min_embeddings
        self.match = make_match(list(gallery.rows), list(gallery.ids))
        self.images = 0
        self.refined_total = 0
        self.events = []    # (step, stream, object id, kind, row): the enrolment's
        self.refined = []   # (step, stream, object id, row, w, the object's distance)
        self.gated = []     # (step, stream, object id, row): known, but past the update threshold
        self.blended = []   # (step, stream, object id, embeddings before, w)
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
                raw = np.asarray(self.embed(frames[s], self.H.Rect.bounding(xy)), f32)
                c = identity["embeddings"] if identity else 0
                q = raw
                if self.template_cap > 1:
                    q = blend(identity["embedding"] if identity else np.zeros(128, f32), raw, c, self.template_cap)
                    if q.tobytes() != raw.tobytes():
                        self.blended.append((self.k, s, o.id, c, min(c + 1, self.template_cap)))
                best, dist = self.match(q)
                pid = IR.known(best, dist, self.threshold)
                o.identity = {"id": pid, "distance": f32(dist), "embedding": q, "next_ms": now_ms + self.interval,
                              "embeddings": c + 1, "flags": identity["flags"] if identity else 0}
                self.images += 1
                items.append({"due": True, "row": self.gallery.ids.index(pid) if pid != NO_MATCH else -1,
                              "distance": f32(dist), "embeddings": c + 1, "flags": o.identity["flags"],
                              "embedding": q, "sample": raw})
                owners.append((s, o))
        changed = False
        if self.refining:
            done = refine(items, self.gallery.rows, self.updates, len(self.gallery.rows), self.max_samples,
                          self.update_threshold)
            for i, r, w in done:
                self.refined.append((self.k, owners[i][0], owners[i][1].id, r, w, float(items[i]["distance"])))
            taken = {i for i, _, _ in done}
            self.gated += [(self.k, owners[i][0], owners[i][1].id, it["row"]) for i, it in enumerate(items)
                           if it["row"] >= 0 and i not in taken]
            self.refined_total += len(done)
            changed = bool(done)
        if self.enrol:
            before = len(self.gallery.rows)
            for i, kind, row in ER.enrol_step(items, self.gallery, self.threshold, self.min_embeddings):
                s, o = owners[i]
                self.events.append((self.k, s, o.id, kind, row))
                o.identity["flags"] = items[i]["flags"]
                if kind in ("match", "enrol"):
                    o.identity["id"], o.identity["distance"] = self.gallery.ids[row], items[i]["distance"]
            self.updates += [0] * (len(self.gallery.rows) - before)
            changed = changed or len(self.gallery.rows) > before
        if changed:   # the next step's matches see the refined and the appended rows
            self.match = self.make_match(list(self.gallery.rows), list(self.gallery.ids))
        for s, t in enumerate(self.trackers):
            t.step(frames[s], now_ms, injected[s])
        self.k += 1

    def objects(self, s):
        """(object, identity or None) for stream s's objects that have a result, in order."""
        return [(o, getattr(o, "identity", None)) for o in self.trackers[s].objects()]
