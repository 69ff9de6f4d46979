"""The model of landmark filters in a loop whose objects move between slots (DeviceMultiTracker,
zr_lm_filter_indexed_async): a filter's state belongs to an object, so it follows the object.

``SlotFilters`` keeps one filter per slot in a list and permutes that list by ``src`` (the slot,
within its stream, that each row's object held one step earlier; outside [0, slots): a new object,
which gets a fresh filter) before it filters.  A row with nothing to filter -- not active, or
active with no estimate -- ends with no filter: the default state.

The scripts say which object id sits in which slot at every step; ``tables`` derives the src /
active / index tables of a step from them, and ``per_object`` is the yardstick the model is pinned
against without a GPU (tests/test_multi_filter_cpu.py): one filter per object id, no slots at all."""
import numpy as np

F = np.float32
ELAPSED = (0.033, 0.05, 0.016, 0.033, 0.1, 0.02)  # tests/test_gpu_lm_filter.py's sequence


class SlotFilters:
    def __init__(self, streams, slots, make):
        """make() -> a fresh filter with .filter((L, 3) float32, elapsed) -> (L, 3) float32."""
        self.K, self.n, self.make = slots, streams * slots, make
        self.f = [None] * self.n
        self.primed = [False] * self.n  # after a step: rows whose value went through a primed filter

    def step(self, src, live, raw, elapsed):
        """src: n ints; live: n bools (active and with an estimate); raw: n x (L, 3) extracts (rows
        that are not live are not read).  Returns n x L x 3 float32, NaN rows where nothing was
        filtered."""
        K = self.K
        new, primed = [None] * self.n, [False] * self.n
        for i in range(self.n):
            if not live[i]:
                continue
            s = int(src[i])
            f = self.f[(i // K) * K + s] if 0 <= s < K else None
            primed[i] = f is not None
            new[i] = f if f is not None else self.make()
        moved = [id(f) for f in new if f is not None]
        assert len(moved) == len(set(moved)), "two rows took one state"
        self.f, self.primed = new, primed
        L = next((np.asarray(raw[i]).shape[0] for i in range(self.n) if live[i]), 1)
        out = np.full((self.n, L, 3), np.nan, F)
        for i in range(self.n):
            if live[i]:
                out[i] = new[i].filter(np.asarray(raw[i], F), elapsed)
        return out


class _Pass:
    """Filter kind none: the extract as it is."""

    def filter(self, value, elapsed):
        return np.asarray(value, F)


def numpy_filter(spec):
    """A filter_ref filter over a whole (L, 3) array: its values are primed together, so the
    per-value classes of filter_ref.py work elementwise."""
    import filter_ref as R
    return _Pass() if spec is None else R.make(spec)


# ---- scripts: per step, per stream, the object id in every slot (None: idle) --------------------
# 2 streams x 3 slots x 6 steps: a compaction (step 2: 0 leaves, 1 and 2 move down), a new object
# in a just-vacated slot (step 3: 3 in slot 2; step 5: 13 in the slot 11 left), a swap into the
# middle (step 4: the sweep removes 2, the last object 3 takes slot 1), a swap into the first slot
# (stream 1, step 3), idle slots throughout stream 1
CPU_SCRIPT = [
    [(0, 1, 2), (10, None, None)],
    [(0, 1, 2), (10, 11, None)],
    [(1, 2, None), (10, 11, 12)],
    [(1, 2, 3), (12, 11, None)],
    [(1, 3, None), (12, 11, None)],
    [(1, 3, 4), (11, 13, None)],
]
# the same moves at 3 streams x 4 slots: a fourth slot, and a third stream that fills up, loses
# its first two objects at once and is empty at the end
GPU_SCRIPT = [
    [(0, 1, 2, None), (10, None, None, None), (20, 21, 22, 23)],
    [(0, 1, 2, 5), (10, 11, None, None), (20, 21, 22, 23)],
    [(1, 2, 5, None), (10, 11, 12, None), (22, 23, None, None)],
    [(1, 2, 5, 3), (12, 11, None, None), (22, 23, 24, None)],
    [(1, 3, 5, None), (12, 11, 14, 15), (23, 24, None, None)],
    [(1, 3, 5, 4), (11, 14, 15, 13), (None, None, None, None)],
]
# (step, row): an active row whose index holds no image (no estimate: its state goes back to the
# default, so the id counts as a new object in the next step), and the value its index holds
GPU_NO_ESTIMATE = {(1, 3): -1, (3, 10): 12}      # object 5's first estimate is missing; object 24's
# (step, row): a new object whose src is outside [0, slots) on the far side
GPU_BAD_SRC = {(3, 3): 4, (4, 6): 64, (4, 7): -7}
# steps whose estimates are stored shuffled (dense order != slot order); the others pass index NULL
GPU_SHUFFLED = (1, 3, 4)


def tables(script, t, slots, no_estimate=None, bad_src=None):
    """Step t's (ids, src, active, live) by row.  src[i] is the slot the row's object held at step
    t - 1 (-1: new, or what bad_src says); an object that had no estimate at step t - 1 counts as
    new, as its state went back to the default."""
    no_estimate, bad_src = no_estimate or {}, bad_src or {}
    ids = [o for stream in script[t] for o in stream]
    n = len(ids)
    prev = [o for stream in script[t - 1] for o in stream] if t else [None] * n
    src, active, live = [-1] * n, [o is not None for o in ids], [False] * n
    for i, o in enumerate(ids):
        if o is None:
            continue
        base = (i // slots) * slots
        for k in range(slots):
            if prev[base + k] == o and (t - 1, base + k) not in no_estimate:
                src[i] = k
        if (t, i) in bad_src:
            assert src[i] == -1, "bad_src is for new objects"
            src[i] = bad_src[(t, i)]
        live[i] = (t, i) not in no_estimate
    return ids, src, active, live


def object_tracks(script, L, seed, side=192.0):
    """Seeded extracts of landmark-like magnitude, (L, 3) float32 per (step, object id): an object
    starts anywhere and moves a little every step."""
    rng = np.random.default_rng(seed)
    cur, out = {}, {}
    for t, streams in enumerate(script):
        for o in (o for stream in streams for o in stream if o is not None):
            if o not in cur:
                cur[o] = rng.normal(side / 2, side / 5, (L, 3))
            else:
                cur[o] = cur[o] + rng.normal(0.0, 2.0, (L, 3))
            out[(t, o)] = cur[o].astype(F)
    return out


def per_object(script, tracks, spec, elapsed=ELAPSED, no_estimate=None, slots=None):
    """One filter_ref filter per object id, fed that object's extracts in step order: what every
    (step, id) must give, {(t, id): (L, 3)}, and whether it went through a primed filter.  An object
    without an estimate at a step starts over (it is lost there)."""
    no_estimate = no_estimate or {}
    filters, out, primed = {}, {}, {}
    for t, streams in enumerate(script):
        row = 0
        for stream in streams:
            for o in stream:
                if o is not None:
                    if (t, row) in no_estimate:
                        filters.pop(o, None)
                    else:
                        primed[(t, o)] = o in filters
                        f = filters.setdefault(o, numpy_filter(spec))
                        out[(t, o)] = f.filter(tracks[(t, o)], elapsed[t])
                row += 1
        for o in [o for o in filters if all(o not in stream for stream in streams)]:
            del filters[o]  # it left: the id is never reused by the scripts
    return out, primed
