"""Every kernel form against a float64 reference at the shapes on both sides of its guards
(tests/synth_models.py).  The bound comes from the reference alone: with e32 the error of the
oracle's f32 interpreter (plain f32 accumulation in index order) against the torch f64 reference
and floor = 2^-23 max|reference|, a kernel must stay within 8 max(e32, floor) -- room for another
summation order over at most 256 * 25 terms, while a wrong tap, weight, channel or stride is off
by 1e-2 .. 1 (the largest ratio err / max(e32, floor) measured on an MI355X is 1.70, over every
case, batch and both form settings).  The session profile shows that the form a case is meant for
ran (or did not)."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle as O
import synth_models as S
from test_gpu_forms import SWITCHES

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in S.CASES]
FACTOR = 8.0


@functools.lru_cache(maxsize=None)
def reference(name, batch):
    """(f64 reference outputs, per-output e32, per-output floor) of a case at a batch; computed once."""
    case = S.BY_NAME[name]
    x = case.input(batch)
    want = case.ref(x)
    with tempfile.NamedTemporaryFile(suffix=".onnx") as f:
        f.write(case.onnx)
        f.flush()
        net = O.Net(f.name, f64=False)
        per_image = [net.run(x[i:i + 1]) for i in range(batch)]
    f32 = [np.concatenate([im[o] for im in per_image]) for o in range(len(want))]
    e32 = [float(np.abs(a.astype(np.float64) - w).max()) for a, w in zip(f32, want)]
    floor = [2.0 ** -23 * float(np.abs(w).max()) for w in want]
    return want, e32, floor


def check_outputs(case, run, label=""):
    """Failures (strings) of one case's outputs against the f64 bound; prints every figure."""
    bad = []
    for b in case.batches:
        want, e32, floor = reference(case.name, b)
        outs = run[b][0]
        assert len(outs) == len(want)
        for o, (got, w) in enumerate(zip(outs, want)):
            assert got.shape == w.shape, (got.shape, w.shape)
            err = float(np.abs(got.astype(np.float64) - w).max())
            unit = max(e32[o], floor[o])
            print(f"synth{label} {case.name} batch={b} out={o} err={err:.3e} e32={e32[o]:.3e} ratio={err / unit:.3f}")
            if not err <= FACTOR * unit:
                bad.append(f"{case.name} batch {b} output {o}: err {err:.3e} > 8 * max(e32 {e32[o]:.3e}, floor {floor[o]:.3e})")
    return bad


def check_case(case, run):
    if run is None:  # refused at compile time with the case's error: never a wrong tensor
        return []
    bad = check_outputs(case, run)
    for b in case.batches:
        msg = S.kernels_ok(case, run[b][1])
        if msg:
            bad.append(f"{case.name} batch {b}: {msg}")
    if "alone" in run:
        for o, (a, g) in enumerate(zip(run["alone"][0], run[3][0])):
            if not np.array_equal(a[0], g[1]):
                bad.append(f"{case.name} output {o}: image 1 of the batch of 3 differs from the same image alone "
                           f"by {float(np.abs(a[0] - g[1]).max()):.3e} ({run['alone'][1]} vs {run[3][1]})")
    return bad


@pytest.fixture(scope="module")
def runs():
    return {}


def default_run(case, runs):
    if case.name not in runs:
        runs[case.name] = S.run_case(case)
    return runs[case.name]


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_case_matches_f64_reference(case, runs):
    bad = check_case(case, default_run(case, runs))
    assert not bad, "\n".join(bad)


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import synth_models as S
out = {}
for ci, c in enumerate(S.CASES):
    run = S.run_case(c)
    for b, (outs, _) in (run or {}).items():
        for o, a in enumerate(outs):
            out[f"{ci}_{b}_{o}"] = a
np.savez(sys.argv[2], **out)
"""


def test_every_form_off_is_bitwise_equal_and_within_the_bound(runs, tmp_path):
    """The whole table in one child process with every optional form switched off (the forms are
    process-wide): the generic kernels meet the same f64 bound, and the default forms' outputs
    equal theirs bit for bit."""
    path = str(tmp_path / "all_off.npz")
    env = dict(os.environ, ZARU_HIP_FORMS=SWITCHES["all_off"] + ",-bneck")
    subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, check=True, timeout=300)
    bad = []
    with np.load(path) as z:
        off = {k: z[k] for k in z.files}
    for ci, case in enumerate(S.CASES):
        run = default_run(case, runs)
        if run is None:
            assert not [k for k in off if k.startswith(f"{ci}_")], case.name
            continue
        off_run = {b: ([off[f"{ci}_{b}_{o}"] for o in range(len(outs))], None) for b, (outs, _) in run.items()}
        bad += check_outputs(case, off_run, label="/all_off")
        for b, (outs, kernels) in run.items():
            for o, a in enumerate(outs):
                if not np.array_equal(a, off_run[b][0][o]):
                    bad.append(f"{case.name} batch {b} output {o}: default forms {kernels} differ from all-off by "
                               f"{float(np.abs(a - off_run[b][0][o]).max()):.3e}")
    assert not bad, "\n".join(bad)
