"""The oracle of DeviceMultiTracker's recognition: tests/multi_tracker_ref.py's MultiTrackerRef with
an identity per object, made with the existing host API only -- ``FaceEmbedder.embed`` on the
bounding rect of the object's landmarks (it applies the grow of 0.4 and the aspect fit itself) and
``Gallery.match``.

Schedule, as the device runs it: after a step's tracker updates (the estimates made on the previous
frame, ``_Object.pending``) and before its bookkeeping, every tracked object that was never
embedded, or whose ``next_ms`` the step's clock reached, is embedded from *this* step's frame at the
place those landmarks give, and matched against the gallery as it is now.  The identity lives on
the object, so it follows it wherever the bookkeeping moves it.

``embed`` and ``match`` are replaceable, so the schedule can be pinned without a GPU
(tests/test_multi_identity_cpu.py)."""
import math

NO_MATCH = 2**64 - 1


def is_due(identity, now_ms):
    """identity: None (never embedded) or a dict with "next_ms"."""
    return identity is None or now_ms >= identity["next_ms"]


def known(best_id, distance, threshold):
    """The id a match counts as: the nearest row's when distance <= threshold (NaN on either side:
    unknown)."""
    return best_id if (best_id != NO_MATCH and distance <= threshold) else NO_MATCH


class MultiIdentityRef:
    def __init__(self, H, tracker, embed, match, interval=1000.0, threshold=math.inf):
        """tracker: a MultiTrackerRef.  embed(frame, H.Rect) -> 128 floats; match(embedding) ->
        (id or NO_MATCH, distance)."""
        self.H = H
        self.tracker = tracker
        self.embed = embed
        self.match = match
        self.interval = interval
        self.threshold = threshold
        self.images = 0          # embeddings made, summed: identity_images()
        self.last_due = []       # ids embedded by the last step
        self.last_tracked = []   # ids that had landmarks at the last step

    def step(self, frame, now_ms, injected=()):
        self.last_due, self.last_tracked = [], []
        for o in self.tracker.objs:
            if o.pending is None:  # new at the last step's bookkeeping, or lost: no landmarks
                continue
            self.last_tracked.append(o.id)
            identity = getattr(o, "identity", None)
            if not is_due(identity, now_ms):
                continue
            xy = [(float(p[0]), float(p[1])) for p in o.pending["landmarks"]]
            if not all(math.isfinite(v) for p in xy for v in p):
                continue
            e = self.embed(frame, self.H.Rect.bounding(xy))
            best, dist = self.match(e)
            o.identity = {"id": known(best, dist, self.threshold), "distance": dist,
                          "embeddings": (identity["embeddings"] if identity else 0) + 1,
                          "embedding": e, "next_ms": now_ms + self.interval}
            self.images += 1
            self.last_due.append(o.id)
        self.tracker.step(frame, now_ms, injected)

    def objects(self):
        """(object, identity or None) for the objects that have a result, in order."""
        return [(o, getattr(o, "identity", None)) for o in self.tracker.objects()]


def host_embed(embedder):
    import numpy as np
    return lambda frame, rect: np.asarray(embedder.embed(frame, [rect]), np.float32)[0].copy()


def host_match(gallery):
    """Against the gallery as it is at the call (rows may have been added since)."""
    import numpy as np

    def match(e):
        ids, dist = gallery.match(np.ascontiguousarray(e, np.float32)[None])
        return int(ids[0]), np.float32(dist[0])
    return match
