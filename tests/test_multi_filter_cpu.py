"""CPU-side checks of the landmark filters of the multi-object loop: what the two new C entry points
(zr_lm_filter_indexed_async, zr_track_update_positions_indexed_async) refuse before they touch a
device, and the model tests/test_gpu_multi_filter.py holds the kernel to (tests/multi_filter_ref.py:
a per-slot list of filters permuted by src) pinned against one filter per object id."""
import ctypes as C

import numpy as np
import pytest

import zaru_amd.host as H
from zaru_amd import _lib

import filter_ref as R
import multi_filter_ref as M

FILTERS = {1: ("ema", 0.6), 2: ("alpha_beta", 0.5, 0.1), 3: ("one_euro", 1.0, 0.05)}


def _cfg(**kw):
    c = dict(kind=0, num_landmarks=468, in_w=192, in_h=192, aspect_w=1, aspect_h=1, loss_thresh=0.5, padding=0.3,
             rois_per_frame=4)
    c.update(kw)
    return _lib.TrackCfg(**c)


def test_indexed_entry_points_refuse_bad_arguments():
    """ZR_ERR_INVALID_ARGUMENT (-1) before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    p, q = 4096, 8192  # stand for device pointers: none of these calls gets as far as using them
    mk = _lib.LmFilter.make
    cfg = _cfg()

    def filt(f, c=cfg, state=p, n=8, slots=4, lm=p, lm_stride=1404, flag=p, flag_stride=1, index=p, src=p,
             elapsed=0.033, fin=p, fout=q, pos=p):
        return lib.zr_lm_filter_indexed_async(None if f is None else C.byref(f), C.byref(c), state, n, slots, lm,
                                              lm_stride, flag, flag_stride, index, src, elapsed, fin, fout, pos, None)

    ema, ab, euro = mk(1, 0.6), mk(2, 0.5, 0.1), mk(3, 1.0, 0.05, 1.0)
    # zr_lm_filter_async's checks
    assert filt(None) == -1
    assert filt(mk(4)) == -1 and filt(mk(1, 1.5)) == -1 and filt(mk(3, 0.0, 0.05, 1.0)) == -1
    assert filt(ema, n=0) == -1 and filt(ema, lm=None) == -1 and filt(ema, flag=None) == -1
    assert filt(ema, pos=None) == -1 and filt(ema, fout=None) == -1
    assert filt(ema, lm_stride=1403) == -4  # ZR_ERR_SHAPE
    assert filt(ema, c=_cfg(kind=4)) == -1
    for f in (ab, euro):  # a bad elapsed for the time-based kinds, whatever else is right
        for bad in (0.0, -0.033, float("nan"), float("inf")):
            assert filt(f, elapsed=bad) == -1, (f.kind, bad)
            assert b"elapsed" in lib.zr_last_error()
    # its own
    assert filt(ema, state=None) == -1
    assert filt(ema, src=None) == -1
    for n, slots in ((8, 0), (8, 65), (8, 3), (9, 4), (130, 64)):  # slots outside 1..64, n % slots != 0
        assert filt(ema, n=n, slots=slots) == -1, (n, slots)
    for f in (ema, ab, euro):
        assert filt(f, fin=p, fout=p) == -1, f.kind   # in == out
        assert filt(f, fin=None) == -1, f.kind
    none = mk(0)
    assert filt(none, src=None) == -1 and filt(none, state=None) == -1 and filt(none, n=9) == -1

    # zr_track_update_positions_indexed_async validates like the update it mirrors
    def upd(c=cfg, state=p, n=8, pos=p, flag=p, flag_stride=1, index=p, views=p):
        return lib.zr_track_update_positions_indexed_async(state, n, C.byref(c), pos, flag, flag_stride, index, p,
                                                           views, None)

    assert upd(state=None) == -1 and upd(n=0) == -1 and upd(views=None) == -1 and upd(pos=None) == -1
    assert upd(flag=None) == -1 and upd(flag_stride=0) == -1
    for field, value in (("kind", 4), ("num_landmarks", 263), ("padding", -0.1), ("rois_per_frame", -1)):
        assert upd(c=_cfg(**{field: value})) == -1, (field, value)


@pytest.mark.parametrize("fkind", [1, 2, 3])
def test_scripted_moves_follow_the_object(fkind):
    """Host LandmarkFilters kept per slot and permuted by src, over the 2 x 3 x 6 script, against one
    numpy filter per object id: bit for bit at every live slot-step."""
    spec, S, K, L = FILTERS[fkind], 2, 3, 7
    tracks = M.object_tracks(M.CPU_SCRIPT, L, seed=fkind)
    want, primed = M.per_object(M.CPU_SCRIPT, tracks, spec)
    model = M.SlotFilters(S, K, lambda: H.LandmarkFilter(R.host_filter(H, spec), L))
    compared = moved = 0
    seen_src = set()
    for t in range(len(M.CPU_SCRIPT)):
        ids, src, active, live = M.tables(M.CPU_SCRIPT, t, K)
        raw = [tracks[(t, o)] if o is not None else None for o in ids]
        got = model.step(src, live, raw, M.ELAPSED[t])
        for i, o in enumerate(ids):
            if o is None:
                assert np.isnan(got[i]).all(), (t, i)
                continue
            assert model.primed[i] == primed[(t, o)], (t, i, o)
            assert np.array_equal(got[i].view(np.uint32), want[(t, o)].view(np.uint32)), (fkind, t, i, o)
            if primed[(t, o)]:
                moved += int(not np.array_equal(got[i], raw[i]))
                seen_src.add((i % K, src[i]))
            else:
                assert np.array_equal(got[i], raw[i]), (t, i, o)  # the first estimate passes through
            compared += 1
    assert compared == sum(o is not None for step in M.CPU_SCRIPT for stream in step for o in stream)
    assert moved == sum(primed.values())  # every primed slot-step was filtered, none passed through
    # the script's moves: compaction (1 -> 0, 2 -> 1), the swap into the middle (2 -> 1 with slot 0
    # in place) and into the first slot (2 -> 0)
    assert {(0, 1), (1, 2), (0, 2), (0, 0), (1, 1)} <= seen_src, seen_src


@pytest.mark.parametrize("fkind", [0, 1, 2, 3])
@pytest.mark.parametrize("L", [468, 21])
def test_gpu_script_model_is_consistent_and_never_passes_through(L, fkind):
    """The 3 x 4 x 6 script tests/test_gpu_multi_filter.py runs on the device, on the CPU: the slot
    model equals the per-object filters, and every primed live slot-step has a value that differs
    from its raw extract, so the device comparison is not of pass-through values."""
    spec = FILTERS.get(fkind)
    tracks = M.object_tracks(M.GPU_SCRIPT, L, seed=100 + fkind + L)
    want, primed = M.per_object(M.GPU_SCRIPT, tracks, spec, no_estimate=M.GPU_NO_ESTIMATE)
    model = M.SlotFilters(3, 4, lambda: M.numpy_filter(spec))
    live_steps = 0
    for t in range(len(M.GPU_SCRIPT)):
        ids, src, active, live = M.tables(M.GPU_SCRIPT, t, 4, M.GPU_NO_ESTIMATE, M.GPU_BAD_SRC)
        raw = [tracks[(t, o)] if o is not None else None for o in ids]
        got = model.step(src, live, raw, M.ELAPSED[t])
        for i, o in enumerate(ids):
            if not live[i]:
                assert np.isnan(got[i]).all(), (t, i)
                continue
            live_steps += 1
            assert np.array_equal(got[i].view(np.uint32), want[(t, o)].view(np.uint32)), (t, i, o)
            assert model.primed[i] == primed[(t, o)], (t, i, o)
            if fkind and primed[(t, o)]:
                assert not np.array_equal(got[i], raw[i]), (t, i, o)
    # counted from the script by hand: 8 + 10 + 8 + 9 + 9 + 8 occupied slot-steps less the two
    # without an estimate; 8 + 1 + 2 + 1 + 3 + 2 of them are an object's first
    assert live_steps == 50 and sum(primed.values()) == 33, (live_steps, sum(primed.values()))
