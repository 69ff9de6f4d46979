"""mark_stem_blocks (plan.cpp, form "stemblock") as zr_plan_describe shows it, without a GPU: a
stem is marked (a trailing sb=1 field) exactly when the next step is the depthwise -> 1x1 that
alone reads its output, as input and as residual; the mark changes no other field of any plan."""
import glob
import os
import subprocess
import sys

import pytest

from zaru_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("gemm", "dw", "direct", "elt", "resize", "gap", "dwpw", "dwgap", "gdc")

CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); from zaru_amd import _lib\n"
         "for p in sys.argv[2:]:\n"
         "    print('#model ' + p); print(_lib.plan_describe(open(p, 'rb').read()))")


def _steps(txt):
    return [l for l in txt.splitlines() if l.split(" ")[0] in KINDS]


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split() if "=" in kv) | {"kind": line.split(" in=")[0]}


def _describe(models_dir, model):
    return _lib.plan_describe(open(os.path.join(models_dir, model + ".onnx"), "rb").read())


@pytest.mark.parametrize("model,pairs", [("face_detection_short_range", 1), ("face_landmark", 1), ("slim_160_latest", 0)])
def test_stem_block_pairs(models_dir, model, pairs):
    steps = [_fields(l) for l in _steps(_describe(models_dir, model))]
    marked = [i for i, s in enumerate(steps) if s.get("sb") == "1"]
    assert len(marked) == pairs, marked
    for i in marked:
        e, d = steps[i], steps[i + 1]
        assert e["kind"] == "direct stem" and d["kind"] == "dwpw" and int(e["M"]) <= 32
        assert d["in"] == e["out"] and d["in2"] == e["out"] and d["res"] != "0"
        assert [s for s in steps if s["in"] == e["out"] or s.get("in2") == e["out"]] == [d]


def test_mark_changes_no_other_field_and_the_switch_removes_it(models_dir):
    """Every model's description with the form off (a child process: the switch is process-wide)
    has no mark, and equals the default description with the new field stripped, line for line."""
    paths = sorted(glob.glob(os.path.join(models_dir, "*.onnx")))
    assert len(paths) >= 9
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, *paths], env=dict(os.environ, ZARU_HIP_FORMS="-stemblock"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert " sb=" not in r.stdout
    off = {}
    for block in r.stdout.split("#model ")[1:]:
        path, txt = block.split("\n", 1)
        off[path] = txt.strip().splitlines()
    for p in paths:
        on = _lib.plan_describe(open(p, "rb").read()).strip().splitlines()
        for line in on:  # the new field comes last, on marked step lines only
            assert " sb=" not in line or (line.endswith(" sb=1") and line.startswith("direct stem ")), line
        assert [l[:-len(" sb=1")] if l.endswith(" sb=1") else l for l in on] == off[p], p


def test_synthetic_pairs_compile_to_the_expected_steps():
    """tests/stemblock_models.py: every pair is a stem step and a dwpw step; the fused cases are
    marked, and so is no pair whose stem output has a second reader, has more than 32 channels or
    is not the block's residual."""
    import stemblock_models as M
    import synth_models as S
    unmarked = {"SB/guard/stem_read_twice", "SB/guard/stem_Cout40", "SB/guard/no_shortcut"}
    for c in M.ALL:
        txt = _lib.plan_describe(c.onnx)
        assert S.plan_tokens(txt) == list(c.kinds), (c.name, S.plan_tokens(txt))
        marks = [_fields(l).get("sb") for l in _steps(txt)]
        assert marks == ([None if c.name in unmarked else "1"] + [None] * (len(marks) - 1)), (c.name, marks)
