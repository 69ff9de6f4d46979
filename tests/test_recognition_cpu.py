"""Face recognition without a GPU: MobileFaceNet compiles to a plan (Constant nodes, the 64-channel
stem, the full-plane depthwise), small synthetic graphs pin the compiler's new cases, the golden
regenerates, and Embedding.difference is the reference's arithmetic bit for bit."""
import re

import numpy as np
import pytest

import onnx_build as ob
from recognition_util import difference_matrix, golden, graph, model_bytes, tool
from zaru_amd import _lib

KINDS = ("gemm", "dw", "direct", "elt", "resize", "gap", "dwpw", "dwgap", "gdc")


def _steps(txt):
    return [l for l in txt.splitlines() if l.split(" ")[0] in KINDS]


def test_mobilefacenet_compiles(golden_dir):
    txt = _lib.plan_describe(model_bytes(golden_dir))
    outs = [l for l in txt.splitlines() if l.startswith("output ")]
    assert len(outs) == 1 and outs[0].endswith("per_image=128"), outs
    assert " fusable=1" in txt.splitlines()[0], "the stem must be able to sample the RGBA frame itself"
    steps = _steps(txt)
    assert steps[0].startswith("direct stem ") and " M=64 " in steps[0], steps[0]
    assert not [l for l in steps if l.startswith("direct ") and not l.startswith("direct stem ")], txt
    gdc = [l for l in steps if l.startswith("gdc ")]
    assert len(gdc) == 1 and "in=t" in gdc[0] and "[512x7x7]" in gdc[0] and "[512x1x1]" in gdc[0], gdc
    # the last step writes the graph output, 128 floats per image with image stride 128
    assert " out=out0[128x1x1]" in steps[-1] and " oN=128 " in steps[-1], steps[-1]
    # every tensor is read only after it was produced
    produced = set()
    for line in steps:
        reads = [re.search(r" in=(\S+)", line).group(1)]
        m = re.search(r" in2=(\S+)", line)
        if m and m.group(1) != "-":
            reads.append(m.group(1))
        for r in reads:
            t = r.split("[")[0]
            assert t == "in0" or t in produced, line
        produced.add(re.search(r" out=(\S+)", line).group(1).split("[")[0])


def _conv_w(rng, co, ci, k):
    return rng.normal(0, 0.1, size=(co, ci, k, k)).astype(np.float32)


def test_clip_bounds_from_constant_nodes():
    rng = np.random.default_rng(1)
    nodes = [
        ob.node("Constant", [], ["lo"], value=np.array(0.0, np.float32)),
        ob.node("Constant", [], ["hi"], value=np.array(6.0, np.float32)),
        ob.node("Conv", ["x", "w", "b"], ["c"], kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]),
        ob.node("Clip", ["c", "lo", "hi"], ["y"]),
    ]
    m = ob.model(nodes, {"x": [1, 3, 16, 16]}, {"y": [1, 8, 8, 8]},
                 {"w": _conv_w(rng, 8, 3, 3), "b": np.zeros(8, np.float32)})
    steps = _steps(_lib.plan_describe(m))
    assert len(steps) == 1 and steps[0].startswith("direct stem ") and " pre=clip " in steps[0], steps


def test_reshape_target_from_int64_constant():
    rng = np.random.default_rng(2)
    nodes = [
        ob.node("Conv", ["x", "w"], ["c"], kernel_shape=[4, 4], group=3),
        ob.node("Constant", [], ["shape"], value=np.array([1, -1], np.int64)),
        ob.node("Reshape", ["c", "shape"], ["y"]),
    ]
    m = ob.model(nodes, {"x": [1, 3, 4, 4]}, {"y": [1, 3]}, {"w": _conv_w(rng, 3, 1, 4)})
    txt = _lib.plan_describe(m)
    assert "output y per_image=3" in txt and _steps(txt)[0].startswith("gdc "), txt


def test_clip_min_from_graph_input_is_a_model_error():
    rng = np.random.default_rng(3)
    nodes = [
        ob.node("Conv", ["x", "w"], ["c"], kernel_shape=[1, 1]),
        ob.node("Clip", ["c", "lo"], ["y"]),
    ]
    m = ob.model(nodes, {"x": [1, 3, 8, 8], "lo": [1]}, {"y": [1, 4, 8, 8]}, {"w": _conv_w(rng, 4, 3, 1)})
    with pytest.raises(_lib.ZaruError, match="model error"):
        _lib.plan_describe(m)


@pytest.mark.parametrize("attrs", [
    {"value_string": "six"},
    {"value_float": 6.0},
    {"value": np.array(6.0, np.float64)},
    {},
])
def test_constant_in_another_form_is_a_model_error(attrs):
    rng = np.random.default_rng(4)
    nodes = [
        ob.node("Constant", [], ["hi"], name="the_const", **attrs),
        ob.node("Conv", ["x", "w"], ["c"], kernel_shape=[1, 1]),
        ob.node("Clip", ["c", "", "hi"], ["y"]),
    ]
    m = ob.model(nodes, {"x": [1, 3, 8, 8]}, {"y": [1, 4, 8, 8]}, {"w": _conv_w(rng, 4, 3, 1)})
    with pytest.raises(_lib.ZaruError, match="model error.*Constant the_const"):
        _lib.plan_describe(m)


def _plane_dw(hw, k, pad):
    rng = np.random.default_rng(5)
    o = hw + 2 * pad - k + 1
    nodes = [
        ob.node("Conv", ["x", "w0"], ["a"], kernel_shape=[1, 1]),
        ob.node("Conv", ["a", "w1", "b1"], ["y"], kernel_shape=[k, k], pads=[pad] * 4, group=16),
    ]
    return ob.model(nodes, {"x": [1, 3, hw, hw]}, {"y": [1, 16, o, o]},
                    {"w0": _conv_w(rng, 16, 3, 1), "w1": _conv_w(rng, 16, 1, k), "b1": np.zeros(16, np.float32)})


def test_full_plane_depthwise_compiles_to_its_own_step():
    steps = _steps(_lib.plan_describe(_plane_dw(7, 7, 0)))
    assert [s.split(" ")[0] for s in steps] == ["gemm", "gdc"], steps
    assert "in=t0[16x7x7]" in steps[1] and "out=out0[16x1x1]" in steps[1] and "k=7x7" in steps[1], steps[1]


@pytest.mark.parametrize("hw,k,pad", [(7, 7, 1), (9, 7, 0), (5, 7, 1)])
def test_other_large_depthwise_is_not_taken_by_the_new_step(hw, k, pad):
    """A padded 7x7 depthwise, or one on a plane larger than its kernel, is refused (or lowered some
    other way) -- never run as the full-plane step, which reads exactly kernel = plane, pad 0."""
    try:
        txt = _lib.plan_describe(_plane_dw(hw, k, pad))
    except _lib.ZaruError as e:
        assert "model error" in str(e) and "unsupported configuration" in str(e), e
        return
    assert not [s for s in _steps(txt) if s.startswith("gdc ")], txt


def test_golden_regenerates(golden_dir):
    g = golden(golden_dir)
    t = tool()
    assert np.array_equal(g["0/codes"], t.random_codes(0)) and np.array_equal(g["1/codes"], t.random_codes(1))
    out = t.run_model(graph(golden_dir), t.codes_to_input(g["0/codes"])[None], np.float64)[0]
    assert out.shape == (128,)
    assert float(np.abs(out - g["0/out"]).max()) <= 1e-6


def test_embedding_difference_is_the_reference_arithmetic():
    from zaru_amd import host
    rng = np.random.default_rng(6)
    a = rng.normal(0, 14 / np.sqrt(128), size=(202, 128)).astype(np.float32)
    b = rng.normal(0, 14 / np.sqrt(128), size=(202, 128)).astype(np.float32)
    b[200] = a[200]          # equal vectors: exactly 0
    a[201, 5] = 1e19         # (1e19)^2 overflows f32: +inf
    b[201, 5] = -1e19
    for i in range(202):
        got = np.float32(host.Embedding(a[i]).difference(host.Embedding(b[i])))
        ref = difference_matrix(a[i:i + 1], b[i:i + 1])[0, 0]
        assert got.tobytes() == ref.tobytes(), (i, got, ref)
    assert host.Embedding(a[200]).difference(host.Embedding(b[200])) == 0.0
    assert np.isposinf(host.Embedding(a[201]).difference(host.Embedding(b[201])))
