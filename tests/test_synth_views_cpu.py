"""What keeps tests/test_gpu_synth_views.py from passing emptily, checked with the oracle alone: the
selection exists and names every kernel it is there for, every view kind samples what it is meant
to, a padded stem sees zero padding beside NONE samples, and the interior device count cuts through
a column tile."""
import re

import numpy as np
import pytest

import oracle as O
import synth_models as S
import synth_views as V
from zaru_amd import _lib

# inputs too small for a view that is partly outside the frame: one sample is inside or not
LEFT_OUT = {"E/1x1_K3_M1_P1_plain": ("c", "d")}
# stems whose padding no window reads: 3x3 stride 2 with TF pads (bottom / right only) on odd sides
PADS_UNREAD = {"F/stem/k3s2tf_17x19_3to7", "F/stem/k3s2tf_17x19_3to64"}
# every plane of these is a whole number of 128-column tiles: no tile straddles any count
WHOLE_TILES = {"F/stem/k3s2sym_16x64_3to16", "A/valu,P=256,vres/k3s1tf_16x16_8to8_id", "A/valu,s2,pool_vres/k3s2tf_32x32_8to16_poolpad",
               "A/valu,M=40:CO48,s1_single_buffer/k5s1tf_16x16_24to40_plain_dwclip", "D/C32_64x64/k3s1tf_64x64_32-16-32_id"}


def test_every_selected_name_exists():
    assert len(set(V.SELECTED)) == len(V.SELECTED)
    for name in V.SELECTED + list(V.EDGE_CASES):
        assert name in S.BY_NAME, name
    assert set(V.EDGE_CASES) <= set(V.SELECTED)
    assert sum(n.startswith("F/stem/") for n in V.SELECTED) == 9
    for name in V.SELECTED:
        assert V.case_of(name).error is None and V.case_of(name).want, name


def test_selected_cases_name_every_required_kernel():
    wants = {name: V.want_of(name) for name in V.SELECTED}
    missing = [k for k, pat in V.REQUIRED.items() if not any(re.search(pat, w) for w in wants.values())]
    assert not missing, missing
    # the frame-sampling instances: every stem and stem-block case names a `true>` instantiation
    for name in V.STEMS:
        assert re.search(r"stem(_dwpw)?_kernel<.*true>$", wants[name]), (name, wants[name])
    fused = {V.want_of(n) for n in V.STEMS if n.startswith("SB/")}
    assert fused == {c.want[:-len("false>")] + "true>" for c in V.M.FUSED}  # one per instantiation FUSED reaches


@pytest.mark.parametrize("name", V.SELECTED)
def test_plan_lowers_as_the_case_says_and_samples_where_expected(name):
    case = V.case_of(name)
    txt = _lib.plan_describe(case.onnx)
    assert S.plan_tokens(txt) == list(case.kinds)
    assert (" fusable=1" in txt.splitlines()[0]) == V.fused_input(name), txt.splitlines()[0]


@pytest.mark.parametrize("name", V.SELECTED)
def test_view_kinds_sample_what_they_are_meant_to(name):
    sc, case = V.scene(name), V.case_of(name)
    _, H, W = case.in_shape
    assert sc.n == V.views_of(name) and sc.x.shape == (sc.n, 3, H, W) and sc.desc.shape == (sc.n, 10)
    assert sc.left_out == LEFT_OUT.get(name, ())
    assert set(sc.kinds) == set("abcde") - set(sc.left_out)
    for f, o in zip(sc.frames, sc.other):
        assert f.shape == o.shape == (H + 7, W + 5, 4) and f.min() >= 1 and not np.array_equal(f, o)
    for i, (kind, v, f) in enumerate(zip(sc.kinds, sc.views, sc.frame_of)):
        share = float((sc.x[i] == np.float32(V.LO)).all(0).mean())
        if kind in "ab":
            assert share == 0.0 and f < V.N_FRAMES, (i, kind, share)
        elif kind in "cd":
            assert V.BAND[0] <= share <= V.BAND[1] and f < V.N_FRAMES, (i, kind, share)
        else:
            assert share == 1.0 and f == V.N_FRAMES, (i, kind, share)
        if kind != "e":  # the reference input is the oracle's preprocessing of that view
            assert np.array_equal(sc.x[i], O.preproc(sc.frames[f], v, W, H, V.LO, V.HI))
        if kind in "ace":
            assert v.rad == 0.0 and (v.rect.w, v.rect.h) == (W, H)
        elif kind == "b":
            assert v.rad == 0.0 and v.rect.w != v.rect.h
            assert all(r != round(r) for r in (v.rect.w / W, v.rect.h / H, W / v.rect.w, H / v.rect.h))
        else:
            assert 0.02 < v.rad % (np.pi / 2) < np.pi / 2 - 0.02  # (no multiple of a quarter turn)
        assert sc.desc[i, 8] == f  # the descriptor carries the frame index
    # the views of a case give different inputs, apart from the NONE tensors of kind e: all of them
    # at the default count, and but for a few whose samples round to the same pixels among hundreds
    # (an input of 2 x 2 has too few rotated views that differ: most of them do)
    live = [sc.x[i].tobytes() for i, k in enumerate(sc.kinds) if k != "e"]
    assert len(set(live)) >= (len(live) if sc.n == 5 else 0.98 * len(live) if H * W >= 9 else 0.8 * len(live))


@pytest.mark.parametrize("name", list(V.STEMS))
def test_padded_stems_see_padding_beside_none_samples(name):
    k, s, pad = V.STEMS[name]
    case = V.case_of(name)
    _, H, W = case.in_shape
    pt, pl, pb, pr = S.PADS[pad](k, s)
    # the pads the helper states are the case's: the first operator's output plane follows from them
    g, _ = case._built
    assert g.shape[g.ops[0][0]][2:] == ((H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1)
    hits, reads_padding = V.pad_meets_none(name)
    assert reads_padding == (any((pt, pl, pb, pr)) and name not in PADS_UNREAD)
    if reads_padding:
        assert hits, name
        assert {V.scene(name).kinds[i] for i, _, _ in hits} <= set("cd")


@pytest.mark.parametrize("name", V.SELECTED)
def test_interior_count_cuts_a_column_tile(name):
    n, c = V.views_of(name), V.interior_count(name)
    assert V.counts_of(name) == (0, 1, c, n - 1, n) and 1 < c < n - 1
    assert n % 4 != 0 or name == V.WS_CASE.name  # (Ns rounds up; the 480 are what dwpw_ws_kernel needs)
    ps = V.planes(V.case_of(name))
    assert V.case_of(name).in_shape[1] * V.case_of(name).in_shape[2] in ps
    assert all(c * p % 128 != 0 for p in ps if p % 128), (c, ps)
    assert all(p % 128 == 0 for p in ps) == (name in WHOLE_TILES), ps
    if n >= 257:
        assert c % 2 == 1


def test_view_counts():
    for name in V.SELECTED:
        P = V.case_of(name).in_shape[1] * V.case_of(name).in_shape[2]
        want = 257 if "257_images" in name else 480 if name == V.WS_CASE.name else 37 if P <= 9 else 5
        assert V.views_of(name) == want, name
