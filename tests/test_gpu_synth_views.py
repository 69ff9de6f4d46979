"""The two entries the device loops run their networks through, zr_cnn_estimate_device_views_async
and zr_cnn_estimate_device_views_count_async, on synthetic graphs fed through device view tables
(tests/synth_views.py): every kernel that tests the device count, the frame-sampling (PRE) stems
among them, and some that ignore it.

Full run: every output stays within test_gpu_synth's bound against the float64 reference of the
oracle-preprocessed views (err <= 8 max(e32, floor), from the reference alone; the largest ratio
err / max(e32, floor) measured on an MI355X is 1.70 there and 1.30 here, over every case and
output: profiles/synth_views_pytest_gpu.log), equals NeuralNetwork.estimate of the preprocessed
tensor bit for bit, and the profile shows the kernel the case is there for -- the `true`
instantiation where the stem samples the frames, with no preproc_kernel beside it.

Count runs, for c in 0, 1, an interior value that cuts a column tile, n - 1 and n: the full entry
first runs on other frames, so the arena holds wrong values and a wrongly skipped image cannot
inherit right ones; the outputs and their guards are refilled with a NaN pattern; then the count
entry runs on the real frames.  Rows [0, c) of every output equal the full run's bit for bit, the
guards are intact and the kernels are those of the full run.  Rows [c, n) are undefined and
asserted on nowhere.

Edges: c = -1 behaves as 0 and c = n + 3 as n; a null count, no frames and no views are refused
with nothing launched."""
import re

import numpy as np
import pytest

import synth_views as V

pytestmark = pytest.mark.gpu

WORST = {}  # case -> its largest ratio, for the log


@pytest.fixture(scope="module")
def runners():
    cache = {}
    yield cache
    for r, _ in cache.values():
        r.close()


def loaded(name, runners):
    """(runner, result of the full run on the real frames) of a case: one session serves all tests."""
    if name not in runners:
        r = V.Runner(name)
        runners[name] = (r, r.full())
    return runners[name]


def rows_differ(a, b, rows):
    return not np.array_equal(a[:rows].view(np.uint32), b[:rows].view(np.uint32))


@pytest.mark.parametrize("name", V.SELECTED)
def test_full_views_run_matches_f64_reference_and_the_tensor_entry(name, runners):
    r, full = loaded(name, runners)
    assert full.rc == 0 and full.guards_intact()
    bad, WORST[name] = V.check_outputs(name, full.outs)
    for o, (got, est) in enumerate(zip(full.outs, r.estimate())):
        if rows_differ(got, est, r.n):
            bad.append(f"{name} output {o}: the views entry differs from estimate(x) by {float(np.abs(got - est).max()):.3e}")
    if not any(re.match(V.want_of(name), k) for k in full.kernels):
        bad.append(f"{name}: no kernel matches {V.want_of(name)!r}: {full.kernels}")
    if r.case.forbid and any(re.match(r.case.forbid, k) for k in full.kernels):
        bad.append(f"{name}: a kernel matches {r.case.forbid!r}: {full.kernels}")
    if ("preproc_kernel" in full.kernels) == V.fused_input(name):
        bad.append(f"{name}: preproc_kernel {'ran beside a frame-sampling stem' if V.fused_input(name) else 'did not run'}: {full.kernels}")
    if V.fused_input(name) and any(k.endswith("false>") and k.startswith("stem") for k in full.kernels):
        bad.append(f"{name}: a tensor-reading stem ran: {full.kernels}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", V.SELECTED)
def test_count_runs_equal_the_full_run_below_the_count(name, runners):
    r, full = loaded(name, runners)
    bad = []
    for c in V.counts_of(name):
        res = r.counted(c)
        assert res.rc == 0, (name, c, res.rc)
        for o, (got, ref) in enumerate(zip(res.outs, full.outs)):
            if rows_differ(got, ref, c):
                rows = [i for i in range(c) if rows_differ(got[i:i + 1], ref[i:i + 1], 1)]
                bad.append(f"{name} count {c} output {o}: rows {rows[:8]} of {len(rows)} differ from the full run")
        if not res.guards_intact():
            bad.append(f"{name} count {c}: a guard was written")
        if res.kernels != full.kernels:
            bad.append(f"{name} count {c}: kernels {res.kernels} instead of {full.kernels}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", V.EDGE_CASES)
def test_count_outside_the_range_is_clamped_and_bad_arguments_are_refused(name, runners):
    r, full = loaded(name, runners)
    under = r.counted(-1)
    assert under.rc == 0 and under.guards_intact() and under.kernels == full.kernels
    over = r.counted(r.n + 3)
    assert over.rc == 0 and over.guards_intact() and over.kernels == full.kernels
    for o, (got, ref) in enumerate(zip(over.outs, full.outs)):
        assert not rows_differ(got, ref, r.n), (name, o)
    for kw in (dict(d_count=False), dict(n_frames=0), dict(n_views=0)):
        res = r.counted(r.n, **kw)
        assert res.rc == V.ZR_ERR_INVALID_ARGUMENT, (name, kw, res.rc)
        assert res.kernels == [] and res.untouched() and res.guards_intact(), (name, kw, res.kernels)


def test_the_selection_reaches_every_required_kernel(runners):
    seen = sorted({k for name in V.SELECTED for k in loaded(name, runners)[1].kernels})
    missing = [what for what, pat in V.REQUIRED.items() if not any(re.search(pat, k) for k in seen)]
    assert not missing, (missing, seen)
    for inst in {V.want_of(n) for n in V.STEMS}:  # each frame-sampling instantiation by its full name
        assert any(re.match(inst, k) for k in seen), (inst, seen)
    if WORST:
        name = max(WORST, key=WORST.get)
        print(f"synthviews largest ratio {WORST[name]:.3f} ({name}) over {len(WORST)} cases")
