"""The synthetic case table (tests/synth_models.py) without a GPU: the oracle's f64 interpreter
must agree with each case's torch f64 restatement (two independent statements of the operation,
so the oracle is pinned at shapes no golden covers and the reference is checked before anything
runs on a GPU), and the plan compiler must lower each graph to the steps its case names -- or
refuse it where the table says so."""
import pytest

import numpy as np

import oracle as O
import synth_models as S
from zaru_amd import _lib

IDS = [c.name for c in S.CASES]


def oracle_net(case, tmp_path_factory, f64):
    path = tmp_path_factory.mktemp("synth") / "m.onnx"
    path.write_bytes(case.onnx)
    return O.Net(str(path), f64=f64)


def test_table_covers_every_family():
    fams = {c.name.split("/")[0] for c in S.CASES}
    assert fams == set("ABCDEFG") and len(set(IDS)) == len(IDS) and 120 <= len(IDS)


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_oracle_f64_agrees_with_torch_f64(case, tmp_path_factory):
    x = case.input(1)
    want = case.ref(x)
    got = oracle_net(case, tmp_path_factory, True).run(x, as_f64=True)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape, (g.shape, w.shape)
        assert np.isfinite(w).all() and float(np.abs(w).max()) > 1e-3  # (a dead output checks nothing)
        assert float(np.abs(g - w).max()) <= 1e-12, float(np.abs(g - w).max())


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_plan_steps(case):
    if case.error:
        with pytest.raises(_lib.ZaruError, match="model error.*" + case.error):
            _lib.plan_describe(case.onnx)
        return
    assert S.plan_tokens(_lib.plan_describe(case.onnx)) == list(case.kinds)


def test_nhwc_on_gemm_steps_carries_the_position_stride():
    """The Transpose folds into the store addressing of the GEMM epilogues: channel stride 1,
    position stride C."""
    txt = _lib.plan_describe(S.BY_NAME["G/dwpw_mfma_nhwc"].onnx)
    last = [l for l in txt.splitlines() if l.startswith("dwpw ")][-1]
    assert " oC=1 " in last and " oP=24 " in last, last
