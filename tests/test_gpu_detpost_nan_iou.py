"""A NaN IoU in the device NMS (zr_detect_post_async, kernels/detpost.hip), beside
tests/test_gpu_detpost.py: two zero-area boxes have IoU 0 / 0, and the reference's comparisons decide
what happens to them.  SuppressionMode::Remove retains a candidate only while iou < thresh
(detection/nms.rs:70-76), so a NaN removes it; Average groups on iou >= thresh (nms.rs:77-90), so a
NaN leaves it alone.  The host (host/detection.cpp) and the oracle (oracle/geom.c zo_nms) do the same,
which tests/test_track_kernels_cpu.py shows on this very frame without a GPU."""
import ctypes as C

import numpy as np
import pytest

import track_kernels_ref as R
from zaru_amd._lib import DeviceBuffer, check, lib

pytestmark = pytest.mark.gpu


class Cfg(C.Structure):
    _fields_ = [("face", C.c_int), ("anchors", C.c_int), ("params", C.c_int), ("keypoints", C.c_int),
                ("in_w", C.c_int), ("in_h", C.c_int), ("thresh", C.c_float), ("iou", C.c_float),
                ("mode", C.c_int)]


@pytest.mark.parametrize("mode", ["average", "remove"])
def test_detect_post_nan_iou(mode):
    """One BlazeFace-shaped frame (track_kernels_ref.nms_nan_frame: 896 anchors, D = 16, three
    zero-size boxes, an overlapping pair, two disjoint boxes, distinct confidences) against the host
    and the oracle, count and detections bit for bit: in Remove mode the first zero-size box removes
    the other two (4 detections), in Average mode each stays alone (6)."""
    import oracle as O
    import zaru_amd.host as H
    A, D, dcap = 896, 16, 16
    boxes, logits, (w, h) = R.nms_nan_frame(H.anchors("face"))
    remove = mode == "remove"
    host = R.det_rows(H.detect_post("face", boxes, logits, w, h, remove=remove), True)
    orc = R.det_rows(O.detect_post(O.FACE, boxes, logits, w, h, 128, 128, remove=remove), False)
    lbox = np.array([H.letterbox_view(w, h, 128, 128)[1].tuple()], np.float32)
    bufs = [DeviceBuffer.from_array(a) for a in (logits, boxes, H.anchors("face").astype(np.float32), lbox)]
    d_count = DeviceBuffer.from_array(np.full(1, 0xA5A5A5A5, np.uint32))
    d_dets = DeviceBuffer.from_array(np.full((dcap, 20), 0xA5A5A5A5, np.uint32))
    cfg = Cfg(1, A, D, 6, 128, 128, 0.5, 0.3, 1 if remove else 0)
    check(lib().zr_detect_post_async(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 1, C.byref(cfg),
                                     d_count.ptr, d_dets.ptr, dcap, None, 0, 0, 1, None, None))
    count = int(d_count.download((1,), np.int32)[0])
    dets = d_dets.download((dcap, 20), np.uint32)
    print(mode, "device", count, "host", len(host), "oracle", len(orc))
    for name, want in (("host", host), ("oracle", orc)):
        assert count == len(want), (mode, name, count, len(want))
        assert np.array_equal(dets[:count], want.view(np.uint32)), (mode, name)
    assert count == (4 if remove else 6) and (dets[count:] == 0xA5A5A5A5).all()
