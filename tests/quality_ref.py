"""The oracle of the face quality gate (zr_identity_quality_async, zr_face_quality_host,
DeviceMultiTracker.set_identity_quality), in numpy with int64 sums throughout; it needs no GPU.

``luma_grid`` samples a view's ow x oh grid through the repository's CPU oracle (``oracle.view_get``,
the reference's own ViewData::get), ``measure`` is the measurement, ``judge`` the tiers, ``record`` both.
Test frames carry alpha 255 everywhere, so an outside pixel (Color::NONE, 0) is unambiguous.

A tier is a tuple (min_size, min_inside, min_sharpness, min_frontal); ``SKIP`` is all -inf.

``MultiQualityRef`` is the loop: tests/multi_template_ref.py's (which is multi_enrol_ref's and
multi_identity_ref's), with the gate before the embedding and the learn mask before the refinement and
the enrolment.
"""
import math

import numpy as np

import multi_enrol_ref as ER
import multi_identity_ref as IR
import multi_template_ref as TR

f32 = np.float32
MEASURED, EMBED, LEARN = 1, 2, 4
FAIL_SIZE, FAIL_INSIDE, FAIL_SHARPNESS, FAIL_FRONTAL = 16, 32, 64, 128
U32_MAX = 0xFFFFFFFF
SKIP = (-math.inf,) * 4
KEYS = ("size", "inside", "sharpness", "frontal", "flags", "rejected", "samples")


def _round_away(v):
    """roundf of a non-negative f32: half away from zero, exact (no v + 0.5 rounding)."""
    t = np.trunc(v)
    return f32(t + f32(1.0)) if f32(v - t) >= f32(0.5) else f32(t)


def _sat_u32(v):
    if not v > 0:
        return 0
    return U32_MAX if v >= f32(4294967296.0) else int(v)


def luma_grid(img, view, ow, oh):
    """(oh, ow) int64: Y = (77 R + 150 G + 29 B + 128) >> 8 of the pixel each grid pixel samples, -1
    outside.  view: an oracle.RRect; the grid pixel's view coordinate is the stem's (nn/mod.rs:54-58)."""
    import oracle as O
    img = np.ascontiguousarray(img, np.uint8)
    assert (img[..., 3] == 255).all(), "test frames carry alpha 255"
    vw, vh = f32(view.rect.w), f32(view.rect.h)
    g = np.empty((oh, ow), np.int64)
    sxs = [_sat_u32(_round_away(f32(f32(f32(x) / f32(ow)) * vw))) for x in range(ow)]
    for y in range(oh):
        sy = _sat_u32(_round_away(f32(f32(f32(y) / f32(oh)) * vh)))
        for x in range(ow):
            px = O.view_get(img, view, sxs[x], sy) & 0xFFFFFFFF
            if px == 0:
                g[y, x] = -1
            else:
                r, gg, b = px & 255, (px >> 8) & 255, (px >> 16) & 255
                g[y, x] = (77 * r + 150 * gg + 29 * b + 128) >> 8
    return g


def sums(grid):
    """(n_in, n, s1, s2) as Python ints from a luma grid."""
    g = np.asarray(grid, np.int64)
    n_in = int((g >= 0).sum())
    if g.shape[0] < 3 or g.shape[1] < 3:
        return n_in, 0, 0, 0
    c, l, r, u, d = g[1:-1, 1:-1], g[1:-1, :-2], g[1:-1, 2:], g[:-2, 1:-1], g[2:, 1:-1]
    ok = (c >= 0) & (l >= 0) & (r >= 0) & (u >= 0) & (d >= 0)
    lap = (4 * c - l - r - u - d)[ok]
    return n_in, int(ok.sum()), int(lap.sum()), int((lap * lap).sum())


def variance(n, s1, s2):
    if n == 0:
        return f32(0.0)
    num, den = n * s2 - s1 * s1, n * n
    assert 0 <= num < 2 ** 53 and den < 2 ** 53
    return f32(np.float64(num) / np.float64(den))


def measure(img, view, ow, oh, pose=None):
    """view: an oracle.RRect.  pose: None or the 21 f32 of a zr_pose (valid: word 7, rot[8]: word 20)."""
    n_in, n, s1, s2 = sums(luma_grid(img, view, ow, oh))
    frontal = f32(math.nan)
    if pose is not None:
        p = np.asarray(pose, f32)
        if p.view(np.uint32)[7] != 0:
            frontal = p[20]
    return {"size": np.fmin(f32(view.rect.w), f32(view.rect.h)), "inside": f32(f32(n_in) / f32(ow * oh)),
            "sharpness": variance(n, s1, s2), "frontal": frontal, "samples": n}


def _passes(value, minimum):
    return minimum == -math.inf or bool(f32(value) >= f32(minimum))   # a NaN value fails


def failures(tier, m):
    return sum(bit for bit, key, mn in zip((FAIL_SIZE, FAIL_INSIDE, FAIL_SHARPNESS, FAIL_FRONTAL),
                                           ("size", "inside", "sharpness", "frontal"), tier)
               if not _passes(m[key], mn))


def judge(m, embed=SKIP, learn=None, rejected_before=0):
    """The measurement `m` as a record: flags and rejected added."""
    learn = embed if learn is None else learn
    fail = failures(embed, m)
    r = dict(m)
    if fail:
        r["flags"], r["rejected"] = MEASURED | fail, min(rejected_before + 1, U32_MAX)
    else:
        r["flags"], r["rejected"] = MEASURED | EMBED | (0 if failures(learn, m) else LEARN), 0
    return r


def record(img, view, ow, oh, pose=None, embed=SKIP, learn=None, rejected_before=0):
    return judge(measure(img, view, ow, oh, pose), embed, learn, rejected_before)


def bits(r):
    """A record (a dict, or a row of the packed structured array) as comparable bytes."""
    return (np.array([r["size"], r["inside"], r["sharpness"], r["frontal"]], f32).tobytes(),
            int(r["flags"]), int(r["rejected"]), int(r["samples"]))


def oracle_view(H, view):
    """A host ViewData as the oracle's RRect."""
    import oracle as O
    cx, cy, w, h, rad = view.zr_view()
    return O.RRect(O.Rect(cx, cy, w, h), rad)


DEFAULT = {"size": f32(0), "inside": f32(0), "sharpness": f32(0), "frontal": f32(0), "flags": 0, "rejected": 0,
           "samples": 0}


class MultiQualityRef(TR.MultiTemplateRef):
    """MultiTemplateRef with the gate.  measure(frame, view, pose) -> a measurement (as ``measure``
    above; view a host ViewData); pose_of(landmarks) -> the 21 f32 of the object's pose or None;
    crop(landmarks, frame) -> the host ViewData of the embedding crop.  A due object that misses the
    embed tier is not embedded and stays due; one that misses the learn tier is embedded, matched and
    committed, and is no item of the refinement or the enrolment."""

    def __init__(self, H, trackers, embed, make_match, gallery, embed_tier=SKIP, learn_tier=None, measure=None,
                 pose_of=None, crop=None, **kw):
        super().__init__(H, trackers, embed, make_match, gallery, **kw)
        self.embed_tier, self.learn_tier = embed_tier, embed_tier if learn_tier is None else learn_tier
        self.measure, self.pose_of, self.crop = measure, pose_of or (lambda lm: None), crop
        self.measured = self.rejected = self.held_back = 0
        self.cases = []   # (step, stream, object id, "reject" | "held" | "learn")

    def step(self, frames, now_ms, injected):
        items, owners = [], []
        for s, t in enumerate(self.trackers):
            for o in t.objs:   # slot order
                if o.pending is None:
                    continue
                identity = getattr(o, "identity", None)
                if not IR.is_due(identity, now_ms):
                    continue
                lm = o.pending["landmarks"]
                xy = [(float(p[0]), float(p[1])) for p in lm]
                if not all(math.isfinite(v) for p in xy for v in p):
                    continue
                before = getattr(o, "quality", DEFAULT)["rejected"]
                q = judge(self.measure(frames[s], self.crop(lm, frames[s]), self.pose_of(lm)), self.embed_tier,
                          self.learn_tier, before)
                o.quality = q
                self.measured += 1
                if not q["flags"] & EMBED:
                    self.rejected += 1
                    self.cases.append((self.k, s, o.id, "reject"))
                    continue   # not embedded: it stays due
                learn = bool(q["flags"] & LEARN)
                self.held_back += 0 if learn else 1
                self.cases.append((self.k, s, o.id, "learn" if learn else "held"))
                raw = np.asarray(self.embed(frames[s], self.H.Rect.bounding(xy)), f32)
                c = identity["embeddings"] if identity else 0
                qv = raw
                if self.template_cap > 1:
                    qv = TR.blend(identity["embedding"] if identity else np.zeros(128, f32), raw, c, self.template_cap)
                best, dist = self.match(qv)
                pid = IR.known(best, dist, self.threshold)
                o.identity = {"id": pid, "distance": f32(dist), "embedding": qv, "next_ms": now_ms + self.interval,
                              "embeddings": c + 1, "flags": identity["flags"] if identity else 0}
                self.images += 1
                items.append({"due": learn, "row": self.gallery.ids.index(pid) if pid != IR.NO_MATCH else -1,
                              "distance": f32(dist), "embeddings": c + 1, "flags": o.identity["flags"],
                              "embedding": qv, "sample": raw})
                owners.append((s, o))
        changed = False
        if self.refining:
            done = TR.refine(items, self.gallery.rows, self.updates, len(self.gallery.rows), self.max_samples,
                             self.update_threshold)
            for i, r, w in done:
                self.refined.append((self.k, owners[i][0], owners[i][1].id, r, w, float(items[i]["distance"])))
            self.refined_total += len(done)
            changed = bool(done)
        if self.enrol:
            first = len(self.gallery.rows)
            for i, kind, row in ER.enrol_step(items, self.gallery, self.threshold, self.min_embeddings):
                s, o = owners[i]
                self.events.append((self.k, s, o.id, kind, row))
                o.identity["flags"] = items[i]["flags"]
                if kind in ("match", "enrol"):
                    o.identity["id"], o.identity["distance"] = self.gallery.ids[row], items[i]["distance"]
            self.updates += [0] * (len(self.gallery.rows) - first)
            changed = changed or len(self.gallery.rows) > first
        if changed:   # the next step's matches see the refined and the appended rows
            self.match = self.make_match(list(self.gallery.rows), list(self.gallery.ids))
        for s, t in enumerate(self.trackers):
            t.step(frames[s], now_ms, injected[s])
        self.k += 1

    def objects(self, s):
        """(object, identity or None, quality or None) for stream s's objects that have a result."""
        return [(o, getattr(o, "identity", None), getattr(o, "quality", None)) for o in self.trackers[s].objects()]
