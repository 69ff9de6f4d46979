"""The landmark temporal filters of zaru_amd.host (csrc/host/filter.cpp: Ema, AlphaBeta, OneEuro,
LandmarkFilter; crates/zaru/src/filter, landmark.rs:142-202) without a GPU: the reference's own
unit vectors, a bitwise comparison with the numpy restatement (filter_ref.py), the per-landmark
and per-coordinate independence of LandmarkFilter, and the argument errors of the host API and
of the C ABI (which return before touching a device)."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as R
from zaru_amd import _lib

F = np.float32
SPECS = [("ema", 0.6), ("alpha_beta", 0.5, 0.1), ("one_euro", 1.0, 0.05), ("one_euro", 0.3, 0.7, 2.5)]


def _host():
    import zaru_amd.host as Hm
    return Hm


def _scalar(Hm, spec):
    """A host filter over one landmark; its x coordinate is the scalar filter."""
    f = Hm.LandmarkFilter(R.host_filter(Hm, spec), 1)
    return lambda v, dt: f.filter(np.array([[v, 0.0, 0.0]], F), dt)[0, 0]


def test_reference_unit_vectors():
    Hm = _host()
    ema = _scalar(Hm, ("ema", 0.5))  # ema.rs test_ema
    got = [ema(v, 1.0 / 30.0) for v in (1.0, 2.0, 2.0)]
    assert got == [F(1.0), F(1.5), F(1.75)], got
    ab = _scalar(Hm, ("alpha_beta", 0.5, 0.1))  # alpha_beta.rs test_alpha_beta_filter
    got = [ab(v, 0.2) for v in (10.0, 10.0, 10.0, 10.0, -10.0, -10.0, -10.0)]
    want = [F(v) for v in (10.0, 10.0, 10.0, 10.0, 0.0, -6.0, -9.4)]
    assert all(type(g) is F or g.dtype == F for g in got)
    assert got == want, got
    # and the yardstick itself reproduces them
    ref = R.make(("alpha_beta", 0.5, 0.1))
    assert [ref.filter(v, 0.2) for v in (10.0, 10.0, 10.0, 10.0, -10.0, -10.0, -10.0)] == want


def _walk(seed, steps=200):
    """A seeded random walk with jumps, and an elapsed time per step in [0.005, 0.1]."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0.0, 1.5, steps)) + 96.0
    jumps = rng.random(steps) < 0.05
    x = x + np.cumsum(np.where(jumps, rng.normal(0.0, 40.0, steps), 0.0))
    return x.astype(F), rng.uniform(0.005, 0.1, steps).astype(F)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "-".join(map(str, s)))
def test_filters_match_numpy_restatement_bitwise(spec):
    Hm = _host()
    xs, dts = _walk(11)
    host, ref = _scalar(Hm, spec), R.make(spec)
    moved = 0
    for t, (x, dt) in enumerate(zip(xs, dts)):  # t = 0 is the priming call
        got, want = F(host(x, dt)), F(ref.filter(x, dt))
        assert got.view(np.uint32) == want.view(np.uint32), (spec, t, got, want)
        if t == 0:
            assert got == x
        moved += int(got != x)
    assert moved > 150  # the filter really filtered


def test_landmark_filter_states_are_independent():
    Hm = _host()
    L, T = 7, 12
    rng = np.random.default_rng(3)
    seq = rng.normal(100.0, 30.0, (T, L, 3)).astype(F)
    dts = rng.uniform(0.01, 0.05, T).astype(F)
    spec = ("one_euro", 1.0, 0.05)
    f = Hm.LandmarkFilter(R.host_filter(Hm, spec), L)
    assert f.num_landmarks() == L
    refs = [[R.make(spec) for _ in range(3)] for _ in range(L)]
    perm = [2, 0, 1]
    fp = Hm.LandmarkFilter(R.host_filter(Hm, spec), L)
    for t in range(T):
        got = f.filter(seq[t], dts[t])
        assert got.shape == (L, 3) and got.dtype == F
        want = np.array([[refs[j][c].filter(seq[t, j, c], dts[t]) for c in range(3)] for j in range(L)], F)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
        # permuting the input columns permutes the output
        gp = fp.filter(np.ascontiguousarray(seq[t][:, perm]), dts[t])
        assert np.array_equal(gp.view(np.uint32), got[:, perm].view(np.uint32)), t
    with pytest.raises(Exception):
        f.filter(np.zeros((L + 1, 3), F), 0.03)
    with pytest.raises(Exception):
        f.filter(np.zeros((L - 1, 3), F), 0.03)
    # a rejected call changed nothing; reset() starts over with a pass-through
    again = f.filter(seq[0], 0.03)
    assert not np.array_equal(again, seq[0])
    f.reset()
    assert np.array_equal(f.filter(seq[0], 0.03), seq[0])


def test_host_argument_errors():
    Hm = _host()
    nan = float("nan")
    for bad in (-0.1, 1.1, nan):
        with pytest.raises(RuntimeError):
            Hm.Ema(bad)
        with pytest.raises(RuntimeError):
            Hm.AlphaBeta(bad, 0.1)
        with pytest.raises(RuntimeError):
            Hm.AlphaBeta(0.5, bad)
    for bad in (0.0, -1.0, nan):
        with pytest.raises(RuntimeError):
            Hm.OneEuro(bad, 0.0)
    for bad in (-0.1, nan):
        with pytest.raises(RuntimeError):
            Hm.OneEuro(1.0, bad)
    Hm.Ema(0.0), Hm.Ema(1.0), Hm.AlphaBeta(0.0, 1.0), Hm.OneEuro(1e-3, 0.0, 2.0)  # the bounds are inclusive
    with pytest.raises(RuntimeError):
        Hm.LandmarkFilter(None, 4)
    with pytest.raises(RuntimeError):
        Hm.LandmarkFilter(Hm.Ema(0.5), 0)
    x = np.ones((2, 3), F)
    for mk in (lambda: Hm.AlphaBeta(0.5, 0.1), lambda: Hm.OneEuro(1.0, 0.05)):
        f = Hm.LandmarkFilter(mk(), 2)
        f.filter(x, 0.03)
        for bad in (0.0, -0.01, nan, float("inf")):
            with pytest.raises(RuntimeError):
                f.filter(x, bad)
        # the rejected calls left the state as it was: same result as a filter that never saw them
        g = Hm.LandmarkFilter(mk(), 2)
        g.filter(x, 0.03)
        y = (2 * x).astype(F)
        assert np.array_equal(f.filter(y, 0.03).view(np.uint32), g.filter(y, 0.03).view(np.uint32))
    # EMA takes no time: any elapsed passes
    Hm.LandmarkFilter(Hm.Ema(0.5), 2).filter(x, 0.0)


def _cfg(kind=0, L=468):
    return _lib.TrackCfg(kind, L, 192, 192, 1, 1, 0.5, 0.3, 0)


def _filter_async(f, cfg=None, n=1, lm=0x1000, lm_stride=None, flag=0x1000, flag_stride=1, elapsed=0.03,
                  fstate=0x1000, pos=0x1000):
    """zr_lm_filter_async with placeholder device pointers: only calls that fail validation (they
    return before any device work) may be made with them."""
    cfg = cfg or _cfg()
    if lm_stride is None:
        lm_stride = 3 * cfg.num_landmarks
    return _lib.lib().zr_lm_filter_async(C.byref(f), C.byref(cfg), None, n, lm, lm_stride, flag, flag_stride,
                                         elapsed, fstate, pos, None)


def test_c_abi_argument_errors():
    mk = _lib.LmFilter.make
    nan = float("nan")
    bad_filters = [mk(1, -0.1), mk(1, 1.5), mk(1, nan), mk(2, 0.5, 1.5), mk(2, -1.0, 0.1), mk(2, 0.5, nan),
                   mk(3, 0.0, 0.1, 1.0), mk(3, -1.0, 0.1, 1.0), mk(3, 1.0, -0.1, 1.0), mk(3, nan, 0.0, 1.0),
                   mk(4, 0.5), mk(-1, 0.5)]
    for f in bad_filters:
        with pytest.raises(_lib.ZaruError) as e:
            _lib.lm_filter_state_size(f, 468)
        assert e.value.code == -1, (f.kind, list(f.p))
        assert _filter_async(f) == -1, (f.kind, list(f.p))
    with pytest.raises(_lib.ZaruError):
        _lib.lm_filter_state_size(mk(1, 0.5), 0)
    # sizes: none 0; the layout is opaque but holds at least the reference's state per value
    assert _lib.lm_filter_state_size(mk(0), 468) == 0
    assert _lib.lm_filter_state_size(mk(1, 0.5), 468) >= 468 * 3 * 4
    for f in (mk(2, 0.5, 0.1), mk(3, 1.0, 0.05, 1.0)):
        assert _lib.lm_filter_state_size(f, 468) >= 468 * 3 * 8
        for bad in (0.0, -0.03, nan, float("inf")):
            assert _filter_async(f, elapsed=bad) == -1, (f.kind, bad)
    ok = mk(1, 0.5)
    # the checks of zr_track_update_async: kinds, strides, missing outputs
    assert _filter_async(ok, n=0) == -1
    assert _filter_async(ok, cfg=_cfg(kind=4)) == -1
    assert _filter_async(ok, cfg=_cfg(kind=0, L=200)) == -1      # angle landmark 263 out of range
    assert _filter_async(ok, lm=None) == -1
    assert _filter_async(ok, flag=None) == -1                    # kind 0 reads a flag output
    assert _filter_async(ok, lm_stride=3 * 468 - 1) == -4        # ZR_ERR_SHAPE
    assert _filter_async(ok, cfg=_cfg(kind=2, L=76), lm_stride=213, flag_stride=14) == -1
    assert _filter_async(ok, cfg=_cfg(kind=3, L=68), lm_stride=135, flag=None, flag_stride=0) == -4
    assert _filter_async(ok, pos=None) == -1
    assert _filter_async(ok, fstate=None) == -1
    msg = _lib.lib().zr_last_error().decode()
    assert "filter state" in msg, msg
    # zr_track_update_positions_async validates like the update it mirrors
    cfg = _cfg()
    upd = _lib.lib().zr_track_update_positions_async
    assert upd(0x1000, 1, C.byref(cfg), None, 0x1000, 1, None, 0x1000, None) == -1    # no positions
    assert upd(0x1000, 1, C.byref(cfg), 0x1000, None, 0, None, 0x1000, None) == -1    # kind 0 needs the flag
    assert upd(None, 1, C.byref(cfg), 0x1000, 0x1000, 1, None, 0x1000, None) == -1
    assert upd(0x1000, 0, C.byref(cfg), 0x1000, 0x1000, 1, None, 0x1000, None) == -1
