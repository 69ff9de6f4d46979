"""The fused stem + first BlazeBlock launch (form "stemblock", kernels/stemblock.hip) on synthetic
pairs on both sides of its guards (tests/stemblock_models.py) and on the two face networks through
the view-sampling entry.

Every GPU run happens in a child process under a timeout (the forms are process-wide): one child
runs the whole table with the default forms, one with -stemblock.  The fused cases must show the
fused symbol, stay within test_gpu_synth's bound against the float64 reference (FACTOR x max(e32,
floor), from the reference alone) and equal the unfused run bit for bit; the guard cases must run
as the two launches and meet the same bound.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import stemblock_models as M
import synth_models as S
from test_gpu_synth import check_outputs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import synth_models as S
import stemblock_models as M
out = {}
for ci, c in enumerate(M.ALL):
    for b, (outs, kernels) in S.run_case(c).items():
        out[f"k_{ci}_{b}"] = np.array(kernels)
        for o, a in enumerate(outs):
            out[f"o_{ci}_{b}_{o}"] = a
np.savez(sys.argv[2], **out)
"""


def _load(path, ci, case):
    """The child's results of one case in run_case's shape: {batch: (outputs, kernel names)}."""
    with np.load(path) as z:
        run = {}
        for b in case.batches + ("alone",):
            n = len([k for k in z.files if k.startswith(f"o_{ci}_{b}_")])
            run[b] = ([z[f"o_{ci}_{b}_{o}"] for o in range(n)], [str(k) for k in z[f"k_{ci}_{b}"]])
    return run


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("stemblock")
    paths = {}
    for name, forms in (("on", ""), ("off", "-stemblock")):
        paths[name] = str(d / f"{name}.npz")
        subprocess.run([sys.executable, "-c", CHILD, REPO, paths[name]], env=dict(os.environ, ZARU_HIP_FORMS=forms),
                       check=True, timeout=240)
    return paths


def _check(case, run):
    bad = check_outputs(case, run, label="/stemblock")
    for b in case.batches + ("alone",):
        msg = S.kernels_ok(case, run[b][1])
        if msg:
            bad.append(f"{case.name} batch {b}: {msg}")
    for o, (a, g) in enumerate(zip(run["alone"][0], run[3][0])):
        if not np.array_equal(a[0], g[1]):
            bad.append(f"{case.name} output {o}: image 1 of the batch of 3 differs from the same image alone by "
                       f"{float(np.abs(a[0] - g[1]).max()):.3e}")
    return bad


@pytest.mark.parametrize("ci", range(len(M.FUSED)), ids=[c.name for c in M.FUSED])
def test_fused_pair_runs_fused_within_the_bound_and_equals_unfused(tables, ci):
    case = M.ALL[ci]
    on, off = _load(tables["on"], ci, case), _load(tables["off"], ci, case)
    bad = _check(case, on)
    for b in on:
        if any(k.startswith("stem_dwpw_kernel") for k in off[b][1]):
            bad.append(f"{case.name} batch {b}: -stemblock still ran {off[b][1]}")
        for o, (a, g) in enumerate(zip(on[b][0], off[b][0])):
            if not np.array_equal(a, g):
                bad.append(f"{case.name} batch {b} output {o}: fused {on[b][1]} differs from unfused {off[b][1]} by "
                           f"{float(np.abs(a - g).max()):.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("ci", range(len(M.FUSED), len(M.ALL)), ids=[c.name for c in M.GUARDS])
def test_guarded_pair_runs_unfused_within_the_bound(tables, ci):
    case = M.ALL[ci]
    bad = _check(case, _load(tables["on"], ci, case))
    assert not bad, "\n".join(bad)


# The two face networks through the estimate-views entry (the stem samples the RGBA frame itself:
# the PRE instances) on five views of a small seeded frame: plain, scaled, partly outside the
# frame, rotated, and rotated across a corner.
VIEWS_CHILD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, sys.argv[1])
from zaru_amd.nn import Cnn, ColorMapper, NeuralNetwork, model_bytes
from zaru_amd._lib import lib, check
img = np.random.default_rng(11).integers(0, 256, size=(150, 200, 4), dtype=np.uint8)
views = [(100.0, 75.0, 120.0, 120.0, 0.0), (60.5, 50.25, 64.0, 48.0, 0.0), (10.0, 140.0, 90.0, 90.0, 0.0),
         (120.0, 70.0, 100.0, 80.0, 0.6), (190.0, 5.0, 70.0, 70.0, -1.1)]
out = {}
for model in ("face_detection_short_range", "face_landmark"):
    net = NeuralNetwork.from_onnx(model_bytes(model)).load()
    check(lib().zr_profile_enable(net._h, 1))
    for i, o in enumerate(Cnn(net, ColorMapper.linear(-1.0, 1.0)).estimate_views(img, views)):
        out[f"{model}/{i}"] = o
    need = C.c_size_t()
    buf = C.create_string_buffer(1 << 20)
    check(lib().zr_profile_read(net._h, buf, len(buf), C.byref(need)))
    out[f"{model}/kernels"] = np.array([l.split()[0] for l in buf.value.decode().splitlines() if l.strip()])
np.savez(sys.argv[2], **out)
"""


def test_views_path_fused_equals_unfused(tmp_path):
    res = {}
    for name, forms in (("on", ""), ("off", "-stemblock")):
        path = str(tmp_path / f"{name}.npz")
        subprocess.run([sys.executable, "-c", VIEWS_CHILD, REPO, path], env=dict(os.environ, ZARU_HIP_FORMS=forms),
                       check=True, timeout=110)
        with np.load(path) as z:
            res[name] = {k: z[k] for k in z.files}
    for model, symbol in (("face_detection_short_range", "stem_dwpw_kernel<5,2,24,32,true>"),
                          ("face_landmark", "stem_dwpw_kernel<3,2,16,16,true>")):
        on, off = list(res["on"][f"{model}/kernels"]), list(res["off"][f"{model}/kernels"])
        assert symbol in on, on
        assert not [k for k in on if k.startswith("stem_kernel")], on
        assert not [k for k in off if k.startswith("stem_dwpw_kernel")], off
        assert [k for k in off if k.startswith("stem_kernel<") and k.endswith(",true>")], off
    assert res["on"].keys() == res["off"].keys()
    for k in res["on"]:
        if not k.endswith("/kernels"):
            assert np.isfinite(res["on"][k]).all(), k
            assert np.array_equal(res["on"][k], res["off"][k]), (k, float(np.abs(res["on"][k] - res["off"][k]).max()))
