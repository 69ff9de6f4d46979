"""The packed export without a device: tests/export_ref.py against hand-written cases, and every
refusal of zr_multi_export_async (ZR_ERR_INVALID_ARGUMENT before anything is launched)."""
import ctypes as C

import numpy as np

import export_ref as XR
from zaru_amd import _lib

K, L = 3, 2


def _inputs(S, seed=5):
    """Distinct words everywhere, so a record says where each of its parts came from."""
    rng = np.random.default_rng(seed)
    rows = S * K
    u = lambda *shape: rng.integers(1, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    ist = np.zeros(rows, XR.IDENT)
    ist["row"] = rng.integers(-1, 50, rows)
    ist["distance"], ist["embeddings"], ist["flags"] = u(rows), rng.integers(1, 9, rows), rng.integers(0, 4, rows)
    return dict(ids=np.arange(100, 100 + rows, dtype=np.uint64), roi=u(rows, 5), confidence=u(rows), lm=u(rows, 3 * L),
                pose=u(rows, 21), ist=ist, emb=u(rows, 128), eye_valid=np.ones(2 * rows, np.int32), eye_diam=u(2 * rows),
                eye_crop=u(2 * rows, 5), eye_lm=u(2 * rows, 228))


def test_selection_order_and_sources():
    # stream 0: count -3 (nothing); 1: count K + 2 (clamped to K) with src -1 and K among its slots;
    # 2: two objects that swapped down a slot; 3: none, between two that have some; 4: one object
    nobjects = np.array([-3, K + 2, 2, 0, 1], np.int32)
    src = np.array([0, 1, 2,
                    -1, 2, K,
                    1, 2, 0,
                    0, 1, 2,
                    0, 0, 0], np.int32)
    assert XR.exported(nobjects, src, K) == [(1, 1, 2), (2, 0, 1), (2, 1, 2), (4, 0, 0)]
    a = _inputs(5)
    a["ist"]["embeddings"][2 * K + 1] = 0     # stream 2, source slot 1: not embedded yet
    a["eye_valid"][2 * (2 * K + 2) + 1] = 0   # stream 2, source slot 2: the right eye invalid
    a["eye_valid"][2 * (4 * K + 0)] = 7       # any non-zero flag is valid, and is reported as 1
    out = XR.export(K, nobjects, src, **a)
    assert out["count"] == 4 and list(out["offsets"]) == [0, 0, 1, 3, 3, 4]
    h = out["header"]
    assert list(h["stream"]) == [1, 2, 2, 4] and list(h["slot"]) == [1, 0, 1, 0]
    # id, roi and confidence from the slot the object holds now ...
    here = [1 * K + 1, 2 * K + 0, 2 * K + 1, 4 * K + 0]
    assert list(h["id"]) == [100 + i for i in here]
    assert np.array_equal(h["roi"], a["roi"][here]) and np.array_equal(h["confidence"], a["confidence"][here])
    # ... everything else from the slot it held before the bookkeeping
    frm = [1 * K + 2, 2 * K + 1, 2 * K + 2, 4 * K + 0]
    assert np.array_equal(out["lm"], a["lm"][frm]) and np.array_equal(out["pose"], a["pose"][frm])
    every = XR.POSE | XR.IDENTITY | XR.EYE_LEFT | XR.EYE_RIGHT
    assert list(h["flags"]) == [every, every & ~XR.IDENTITY, every & ~XR.EYE_RIGHT, every]
    assert not h["reserved"].any()
    # identity with embeddings == 0: absent, written as zeros
    assert out["ident"][1] == np.zeros(1, XR.IDENT)[0] and not out["emb"][1].any()
    for k in (0, 2, 3):
        assert out["ident"][k] == a["ist"][frm[k]] and np.array_equal(out["emb"][k], a["emb"][frm[k]])
    # one eye invalid: zeros for it, the other eye its own
    assert list(out["eye_valid"]) == [1, 1, 1, 1, 1, 0, 1, 1]
    assert out["eye_diam"][5] == 0 and not out["eye_crop"][5].any() and not out["eye_lm"][5].any()
    e = 2 * frm[2]
    assert out["eye_diam"][4] == a["eye_diam"][e] and np.array_equal(out["eye_lm"][4], a["eye_lm"][e])
    assert np.array_equal(out["eye_crop"][6], a["eye_crop"][2 * frm[3]])


def test_optional_groups_off_and_nothing_exported():
    a = _inputs(2)
    plain = {k: a[k] for k in ("ids", "roi", "confidence", "lm")}
    out = XR.export(K, np.array([1, 2], np.int32), np.array([0, 0, 0, 1, 0, 0], np.int32), **plain)
    assert sorted(out) == ["count", "header", "lm", "offsets"] and out["count"] == 3
    assert list(out["header"]["flags"]) == [0, 0, 0]
    # the first step: objects everywhere, none with a result
    out = XR.export(K, np.array([2, 1], np.int32), np.full(6, -1, np.int32), **a)
    assert out["count"] == 0 and list(out["offsets"]) == [0, 0, 0] and len(out["header"]) == 0


def test_structures_match_the_header():
    assert C.sizeof(_lib.ExportHeader) == XR.HEADER.itemsize == 48
    assert C.sizeof(_lib.ExportIdentity) == XR.IDENT.itemsize == 16
    assert [f for f, _ in _lib.ExportHeader._fields_] == list(XR.HEADER.names)
    assert _lib.ExportHeader.flags.offset == XR.HEADER.fields["flags"][1] == 40
    assert C.sizeof(_lib.MultiExportArgs) == 24 * C.sizeof(C.c_void_p)
    assert (_lib.EXPORT_POSE, _lib.EXPORT_IDENTITY, _lib.EXPORT_EYE_LEFT, _lib.EXPORT_EYE_RIGHT) == (
        XR.POSE, XR.IDENTITY, XR.EYE_LEFT, XR.EYE_RIGHT)


def test_export_refuses_bad_arguments():
    """-1 before anything is launched: no device is needed (or touched)."""
    lib = _lib.lib()
    p = 4096  # stands for a device pointer: none of these calls gets as far as using it
    A = _lib.MultiExportArgs
    required = A.INPUTS + ("d_count", "d_stream_offsets", "d_header", "d_out_landmarks")

    def call(args, n=8, k=4, l=21):
        return lib.zr_multi_export_async(None if args is None else C.byref(args), n, k, l, None)

    def make(*groups):
        a = A()
        for name in required + tuple(f for g in groups for f in g):
            setattr(a, name, p)
        return a

    assert call(None) == -1 and b"null" in lib.zr_last_error()
    for name in required:                       # a NULL required pointer
        a = make(A.POSE, A.IDENTITY, A.EYES)
        setattr(a, name, None)
        assert call(a) == -1, name
        assert b"null" in lib.zr_last_error()
    for group in (A.POSE, A.IDENTITY, A.EYES):  # an optional group given only in part
        for name in group:
            a = make(group)
            setattr(a, name, None)
            assert call(a) == -1, name
            assert b"optional group" in lib.zr_last_error()
            a = make()
            setattr(a, name, p)
            assert call(a) == -1, name
    for groups in ((), (A.POSE,), (A.IDENTITY, A.EYES), (A.POSE, A.IDENTITY, A.EYES)):
        a = make(*groups)
        for n, k, l in ((0, 4, 21), (8, 0, 21), (8, 65, 21), (8, 4, 0), (2 ** 30, 2, 21), (2 ** 31 - 1, 2, 21),
                        (2 ** 40, 1, 21), (8, 4, 2 ** 20 + 1)):
            assert call(a, n, k, l) == -1, (n, k, l)
