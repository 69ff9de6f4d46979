"""det_post_kernel (kernels/detpost.hip) and cand_kernel (kernels/misc.hip) alone on crowded frames:
the frames of tests/detpost_scenes.py, which tests/test_detpost_crowded_cpu.py shows to be tie-free
(an order the reference pins) and on which the host restatement and the oracle agree bit for bit.
They take what no other kernel-alone test takes: the rank sort with more than 64 distinct keys, the
in-place retain of `ord[]` across 64-candidate chunks with candidates already retained, groups
assembled from several chunks, detection counts above dcap and rmax, and the face-full shape's
73,728 B of LDS with up to 2304 candidates; and the candidate compaction's count > cap branch."""
import ctypes as C

import numpy as np
import pytest

import detpost_scenes as S
import track_kernels_ref as R
from zaru_amd._lib import DeviceBuffer, check, lib

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
SHAPES = list(S.SHAPES)


class Cfg(C.Structure):
    _fields_ = [("face", C.c_int), ("anchors", C.c_int), ("params", C.c_int), ("keypoints", C.c_int),
                ("in_w", C.c_int), ("in_h", C.c_int), ("thresh", C.c_float), ("iou", C.c_float),
                ("mode", C.c_int)]


def sentinel(*shape):
    return DeviceBuffer.from_array(np.full(shape, SENT, np.uint32))


def detect_post(fr, sel, remove, dcap, rmax=0, first_id=0, id_stride=1, fmap=None, nframes=None):
    """One launch over the frames `sel` of a shape, every output sentinel-filled before it.  With `fmap`,
    the mapped form over the first `nframes` rows, the letterbox taken per slot.  Returns count [n],
    dets [n][dcap][20], ties [n][2] and the records [n][2 + 20 rmax] (None without rmax), as uint32,
    after checking that the spare slot behind each of them kept the sentinel."""
    n = len(sel)
    lbox = fr.letterbox[sel]
    if fmap is not None:
        lbox = np.empty_like(lbox)
        lbox[fmap] = fr.letterbox[sel]
    bufs = [DeviceBuffer.from_array(a) for a in (fr.logits[sel], fr.boxes[sel], fr.anchors, lbox)]
    d_count, d_dets, d_ties = sentinel(n + 1), sentinel(n + 1, dcap, 20), sentinel(n + 1, 2)  # (a spare slot behind)
    d_rec = sentinel(n + 1, 2 + 20 * rmax) if rmax else None
    cfg = Cfg(fr.face, fr.A, fr.D, fr.nkp, fr.side, fr.side, 0.5, 0.3, 1 if remove else 0)
    if fmap is None:
        check(lib().zr_detect_post_async(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, C.byref(cfg),
                                         d_count.ptr, d_dets.ptr, dcap, d_rec.ptr if rmax else None, rmax,
                                         first_id, id_stride, d_ties.ptr, None))
    else:
        d_map = DeviceBuffer.from_array(np.asarray(fmap, np.int32))
        d_n = DeviceBuffer.from_array(np.array([nframes], np.int32))
        check(lib().zr_detect_post_mapped_async(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, d_map.ptr,
                                                d_n.ptr, C.byref(cfg), d_count.ptr, d_dets.ptr, dcap, d_ties.ptr,
                                                None))
    out = [d_count.download((n + 1,), np.uint32), d_dets.download((n + 1, dcap, 20), np.uint32),
           d_ties.download((n + 1, 2), np.uint32), d_rec.download((n + 1, 2 + 20 * rmax), np.uint32) if rmax else None]
    assert all((a[n] == SENT).all() for a in out if a is not None), "a write behind the last frame's slot"
    return [a[:n] if a is not None else None for a in out]


def same(name, got_u32, want_f32):
    """Bit equality; in the `nonfinite` frame a NaN equals a NaN at the same position."""
    if name == "nonfinite":
        return S.same_words(got_u32.view(np.float32), want_f32)
    return np.array_equal(got_u32, np.ascontiguousarray(want_f32, np.float32).view(np.uint32))


@pytest.mark.parametrize("mode", ["average", "remove"])
@pytest.mark.parametrize("shape", SHAPES)
def test_crowded_scenes_bit_for_bit(shape, mode):
    """Every crowded scene and edge frame of a shape in one launch (0 to A candidates side by side),
    dcap = A: the count, the rows up to it and the tie counts (candidates, 0) equal the host's and
    the oracle's; every word past the count keeps the sentinel."""
    fr, remove = S.frames(shape), mode == "remove"
    count, dets, ties, _ = detect_post(fr, np.arange(fr.n), remove, fr.A)
    for i, name in enumerate(fr.names):
        host, orc = R.det_rows(fr.host(i, remove), True), R.det_rows(fr.oracle(i, remove), False)
        print(f"{shape} {mode} {name}: device {count[i]} host {len(host)} oracle {len(orc)} ties {ties[i].tolist()}")
        assert count[i] == len(host) == len(orc), (shape, mode, name)
        assert same(name, dets[i, :count[i]], host), (shape, mode, name, "host")
        assert same(name, dets[i, :count[i]], orc), (shape, mode, name, "oracle")
        assert ties[i].tolist() == [fr.candidates[i], 0], (shape, mode, name)
        assert (dets[i, count[i]:] == SENT).all(), (shape, mode, name)


@pytest.mark.parametrize("shape", SHAPES)
def test_truncation(shape):
    """dcap = 8 and rmax = 4 on the scenes with more than 64 detections, both modes: d_count stays
    exact, the 8 rows are the full run's first 8 and nothing is written past them, and the record is
    H.pack_detection_records of the host's detections (ids 100 + 3 f, zeros past min(count, rmax))."""
    import zaru_amd.host as H
    fr = S.frames(shape)
    for remove in (False, True):
        sel = np.array([i for i in range(fr.n) if len(fr.host(i, remove)) > 64])
        assert len(sel) >= 1
        full_count, full, full_ties, _ = detect_post(fr, sel, remove, fr.A)
        count, dets, ties, rec = detect_post(fr, sel, remove, 8, rmax=4, first_id=100, id_stride=3)
        want = [fr.host(i, remove) for i in sel]
        assert count.tolist() == full_count.tolist() == [len(w) for w in want]
        assert np.array_equal(dets, full[:, :8]) and np.array_equal(ties, full_ties)
        packed = H.pack_detection_records(want, [100 + 3 * f for f in range(len(sel))], 4)
        assert np.array_equal(rec, np.ascontiguousarray(packed, np.float32).view(np.uint32))
        assert rec[:, 0].tolist() == [100 + 3 * f for f in range(len(sel))] and rec[:, 1].tolist() == count.tolist()
        assert np.array_equal(rec[:, 2:].reshape(len(sel), 4, 20), full[:, :4])
        # one frame with fewer detections than rmax: zero padding after its rows
        two = np.array([fr.names.index("edge129")])
        c2, d2, _, r2 = detect_post(fr, two, remove, 8, rmax=4, first_id=100, id_stride=3)
        assert c2[0] == 2 and (d2[0, 2:] == SENT).all()
        assert np.array_equal(r2[0, 2:42].reshape(2, 20), d2[0, :2]) and not r2[0, 42:].any()
        assert np.array_equal(r2, H.pack_detection_records([fr.host(int(two[0]), remove)], [100], 4).view(np.uint32))


def test_mapped_form_face_full():
    """The crowded face-full scenes through zr_detect_post_mapped_async with a permutation map and
    *d_nframes two below n: slot map[f] is row f of the plain call (letterbox per slot), the two
    skipped slots keep the sentinel."""
    fr = S.frames("face_full")
    sel = np.flatnonzero(fr.crowded)[::-1].copy()  # the most crowded first: the skipped rows are the lightest
    n = len(sel)
    fmap = np.array([3, 0, 4, 1, 2])
    assert n == len(fmap)
    for remove in (False, True):
        count, dets, ties, _ = detect_post(fr, sel, remove, fr.A)
        mcount, mdets, mties, _ = detect_post(fr, sel, remove, fr.A, fmap=fmap, nframes=n - 2)
        for f in range(n - 2):
            assert mcount[fmap[f]] == count[f] == len(fr.host(int(sel[f]), remove))
            assert np.array_equal(mdets[fmap[f]], dets[f]) and np.array_equal(mties[fmap[f]], ties[f])
        for f in range(n - 2, n):
            assert mcount[fmap[f]] == SENT and (mdets[fmap[f]] == SENT).all() and (mties[fmap[f]] == SENT).all()


def candidates(logits, boxes, floor, cap):
    """zr_detection_candidates_async over frames [n][A] / [n][A][D] into sentinel-filled buffers with
    one spare record behind the last block.  Returns count [n] and the words [n * cap + 1][2 + D]."""
    n, A, D = boxes.shape
    bufs = [DeviceBuffer.from_array(np.ascontiguousarray(a, np.float32)) for a in (logits, boxes)]
    d_count, d_rec = sentinel(n), sentinel(n * cap + 1, 2 + D)
    check(lib().zr_detection_candidates_async(bufs[0].ptr, bufs[1].ptr, n, A, D, floor, cap, d_count.ptr, d_rec.ptr,
                                              None))
    return d_count.download((n,), np.uint32), d_rec.download((n * cap + 1, 2 + D), np.uint32)


def check_candidates(logits, boxes, floor, cap, tag):
    """The contract of cand_kernel: d_count is the number of anchors with logit >= floor (a NaN never
    qualifies), the first min(count, cap) records of a frame's block are distinct qualifying anchors,
    each with its own logit and box row -- all of them when cap >= count -- and no other word of the
    block, of another frame's block or behind the last block changes."""
    n, A, D = boxes.shape
    count, words = candidates(logits, boxes, floor, cap)
    assert (words[n * cap] == SENT).all(), tag
    lb, bb = np.ascontiguousarray(logits, np.float32).view(np.uint32), np.ascontiguousarray(boxes, np.float32).view(np.uint32)
    for f in range(n):
        with np.errstate(invalid="ignore"):
            q = np.flatnonzero(logits[f] >= np.float32(floor))
        assert count[f] == len(q), (tag, f)
        m = min(len(q), cap)
        block = words[f * cap:(f + 1) * cap]
        rec = block[:m][np.argsort(block[:m, 0], kind="stable")]
        a = rec[:, 0].astype(np.int64)
        assert len(np.unique(a)) == m and np.isin(a, q).all(), (tag, f)
        if cap >= len(q):
            assert np.array_equal(a, q), (tag, f)
        assert np.array_equal(rec[:, 1], lb[f, a]) and np.array_equal(rec[:, 2:], bb[f, a]), (tag, f)
        assert (block[m:] == SENT).all(), (tag, f)
    return count


@pytest.mark.parametrize("shape", SHAPES)
def test_detection_candidates(shape):
    """cand_kernel on the crowded scenes and the `nonfinite` frame, with the host path's floor
    (H.candidate_logit_floor(0.5)) and with -inf, which admits every anchor but a NaN's: cap = A
    (every record), cap = 16 and 1 (count > cap: the true count, exactly cap records)."""
    import zaru_amd.host as H
    fr = S.frames(shape)
    sel = np.append(np.flatnonzero(fr.crowded), fr.names.index("nonfinite"))
    logits, boxes = fr.logits[sel], fr.boxes[sel]
    for floor in (H.candidate_logit_floor(0.5), -np.inf):
        for cap in (fr.A, 16, 1):
            count = check_candidates(logits, boxes, floor, cap, (shape, floor, cap))
            print(f"{shape} floor {floor} cap {cap}: counts {count.tolist()}")
            # the scenes' candidates (+inf among them in `nonfinite`; its NaNs and -inf do not qualify) / every anchor
            want = [c for c in np.array(fr.candidates)[sel]] if np.isfinite(floor) else [fr.A] * len(sel)
            want[-1] = 41 if np.isfinite(floor) else fr.A - 2
            assert count.tolist() == want


@pytest.mark.parametrize("shape", SHAPES)
def test_detection_candidates_batch_blocks(shape):
    """Three frames with 0, 5 and A qualifying anchors in one launch keep their blocks apart."""
    import zaru_amd.host as H
    fr = S.frames(shape)
    rng = np.random.default_rng(5)
    logits = np.full((3, fr.A), -9.0, np.float32)
    logits[1, rng.choice(fr.A, 5, replace=False)] = rng.uniform(0.0, 4.0, 5)
    logits[2] = rng.uniform(0.0, 4.0, fr.A)
    boxes = rng.uniform(-3.0, 3.0, (3, fr.A, fr.D)).astype(np.float32)
    for cap in (fr.A, 16):
        count = check_candidates(logits, boxes, H.candidate_logit_floor(0.5), cap, (shape, cap))
        assert count.tolist() == [0, 5, fr.A]
