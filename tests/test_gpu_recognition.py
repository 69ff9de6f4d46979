"""Face recognition on the GPU: MobileFaceNet against its f64 golden, batch independence, the
fused stem against preprocess + run, embedding matching bit for bit against the reference's
arithmetic, and FaceEmbedder / Gallery / FaceRecognizer against their per-frame CPU chains."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
from recognition_util import difference_matrix, golden, graph, model_bytes, tool
from zaru_amd import _lib
from zaru_amd._lib import DeviceBuffer, Frame, View, check, lib

pytestmark = pytest.mark.gpu

ABS_TOL = 2e-3  # max abs error against the f64 reference
D = 128


@pytest.fixture(scope="module")
def net(golden_dir):
    from zaru_amd.nn import NeuralNetwork
    return NeuralNetwork.from_onnx(model_bytes(golden_dir)).load()


def _kernels(net):
    need = C.c_size_t()
    buf = C.create_string_buffer(1 << 20)
    check(lib().zr_profile_read(net._h, buf, len(buf), C.byref(need)))
    return [l.split()[0] for l in buf.value.decode().splitlines() if l.strip()]


def test_model_vs_f64_golden(net, golden_dir):
    g = golden(golden_dir)
    x = tool().codes_to_input(np.stack([g["0/codes"], g["1/codes"]]))
    check(lib().zr_profile_enable(net._h, 1))
    (out,) = net.estimate(x)
    kernels = _kernels(net)
    check(lib().zr_profile_enable(net._h, 0))
    assert out.shape == (2, D)
    err = float(np.abs(out - np.stack([g["0/out"], g["1/out"]])).max())
    print(f"mobilefacenet max|gpu - f64| = {err:.3e}")
    assert err <= ABS_TOL
    assert any(k.startswith("stem_kernel<3,2,64,") for k in kernels), kernels
    assert "gdc_kernel<49>" in kernels, kernels
    assert not any(k.startswith(("direct_kernel", "preproc_kernel")) for k in kernels), kernels


@pytest.fixture(scope="module")
def pool(net, golden_dir):
    """Six distinct inputs (the two golden ones and four of seeded random codes) and each one's
    batch-1 output."""
    g = golden(golden_dir)
    rng = np.random.default_rng(21)
    codes = np.concatenate([np.stack([g["0/codes"], g["1/codes"]]),
                            rng.integers(0, 256, size=(4, 3, 112, 112), dtype=np.uint8)])
    x = tool().codes_to_input(codes)
    return x, np.stack([net.estimate(x[i:i + 1])[0][0] for i in range(len(x))])


# gdc_kernel takes 256 images per workgroup: 257 is one tile + 1, 515 is more than two tiles; 33
# straddles the 32-column MFMA tiles of the 1x1 heads, 2 is below every tile
@pytest.mark.parametrize("n", [2, 33, 257, 515])
def test_batch_independence(net, pool, n):
    x, single = pool
    idx = np.random.default_rng(n).integers(0, len(x), size=n)
    idx[:2] = (1, 0)
    (out,) = net.estimate(x[idx])
    for i in range(n):
        assert np.array_equal(out[i], single[idx[i]]), (n, i, int(idx[i]))


def test_estimate_views_matches_session(net):
    from zaru_amd.nn import Cnn, ColorMapper, preprocess_views_device
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, size=(96, 160, 4), dtype=np.uint8)
    views = [O.RRect(O.Rect(80.0, 48.0, 60.0, 60.0), 0.0),     # inside the frame
             O.RRect(O.Rect(80.0, 48.0, 70.0, 70.0), 0.3),     # rotated
             O.RRect(O.Rect(150.0, 90.0, 80.0, 80.0), 0.0)]    # partly outside
    vt = [(v.rect.cx, v.rect.cy, v.rect.w, v.rect.h, v.rad) for v in views]
    cnn = Cnn(net, ColorMapper.linear(-1.0, 1.0))
    check(lib().zr_profile_enable(net._h, 1))
    (got,) = cnn.estimate_views(img, vt)
    kernels = _kernels(net)
    check(lib().zr_profile_enable(net._h, 0))
    # the RGBA frame is sampled inside the stem: no preprocessing launch, no f32 input tensor
    assert "stem_kernel<3,2,64,true>" in kernels and not any(k.startswith("preproc") for k in kernels), kernels
    d_img = DeviceBuffer.from_array(img)
    d_x = DeviceBuffer(3 * 3 * 112 * 112 * 4)
    d_out = DeviceBuffer(3 * D * 4)
    preprocess_views_device([Frame(d_img.ptr, 160, 96, 640)], vt, [0, 0, 0], 112, 112, -1.0, 1.0, d_x.ptr)
    net.estimate_device(3, d_x.ptr, [d_out.ptr])
    _lib.synchronize()
    x = d_x.download((3, 3, 112, 112), np.float32)
    want = d_out.download((3, D), np.float32)
    ref = np.stack([O.preproc(img, v, 112, 112, -1.0, 1.0) for v in views])
    assert x.tobytes() == ref.tobytes()
    assert got.tobytes() == want.tobytes()
    # and the device-resident entry point runs the same fused stem
    d_got = DeviceBuffer(3 * D * 4)
    cnn.estimate_views_device([Frame(d_img.ptr, 160, 96, 640)], vt, [0, 0, 0], [d_got.ptr])
    _lib.synchronize()
    assert d_got.download((3, D), np.float32).tobytes() == want.tobytes()


# ------------------------------------------------------------------ matching
def _match(q, g, valid=None, want_dist=True):
    q = np.ascontiguousarray(q, np.float32)
    g = np.ascontiguousarray(g, np.float32).reshape(-1, q.shape[1])
    nq, ng = len(q), len(g)
    d_q, d_g = DeviceBuffer.from_array(q), DeviceBuffer.from_array(g) if ng else None
    d_idx, d_best = DeviceBuffer(nq * 4), DeviceBuffer(nq * 4)
    d_dist = DeviceBuffer(nq * max(ng, 1) * 4) if want_dist else None
    d_valid = DeviceBuffer.from_array(np.asarray(valid, np.int32)) if valid is not None else None
    check(lib().zr_embed_match_async(d_q.ptr, nq, d_g.ptr if ng else None, ng, q.shape[1],
                                     d_valid.ptr if d_valid else None, d_idx.ptr, d_best.ptr,
                                     d_dist.ptr if d_dist else None, None))
    _lib.synchronize()
    dist = d_dist.download((nq, ng), np.float32) if want_dist and ng else None
    return d_idx.download((nq,), np.int32), d_best.download((nq,), np.float32), dist


def _normal(rng, n):
    return rng.normal(0, 14 / np.sqrt(D), size=(n, D)).astype(np.float32)


def _same_bits(a, b):
    """Bit equality, except that a NaN equals a NaN: IEEE 754 leaves the sign and payload of a
    NaN result open, and x86 (numpy, the reference) and the GPU choose differently."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _reference(q, g, valid=None):
    """(best index, best distance, matrix) by numpy: first minimum, NaN never wins, masked or
    unmatched queries -1 / +inf."""
    m = difference_matrix(q, g)
    idx = np.full(len(q), -1, np.int32)
    best = np.full(len(q), np.inf, np.float32)
    for i in range(len(q)):
        if valid is not None and not valid[i]:
            m[i] = np.inf
            continue
        ok = ~np.isnan(m[i])
        if ok.any():
            j = int(np.argmin(np.where(ok, m[i], np.inf)))
            idx[i], best[i] = j, m[i, j]
    return idx, best, m


@pytest.mark.parametrize("nq,ng", [(1, 1), (5, 3), (70, 257), (3, 1000)])
def test_match_bit_exact(nq, ng):
    rng = np.random.default_rng(100 * nq + ng)
    q, g = _normal(rng, nq), _normal(rng, ng)
    idx, best, dist = _match(q, g)
    ridx, rbest, rdist = _reference(q, g)
    assert dist.tobytes() == rdist.tobytes()
    assert np.array_equal(idx, ridx) and best.tobytes() == rbest.tobytes()
    idx2, best2, _ = _match(q, g, want_dist=False)  # d_dist = NULL
    assert np.array_equal(idx2, ridx) and best2.tobytes() == rbest.tobytes()


def test_match_special_cases():
    rng = np.random.default_rng(7)
    q, g = _normal(rng, 70), _normal(rng, 257)
    g[200] = g[13]           # two identical rows: the lower index wins
    q[0] = g[13] + np.float32(1e-3)
    q[1] = g[77]             # a query equal to a row: distance exactly 0
    g[5, 9] = np.nan         # a row with a NaN never wins
    q[2] = g[5]
    q[2, 9] = 0.0
    valid = np.ones(70, np.int32)
    valid[[3, 64, 69]] = 0
    valid[4] = 5             # detection counts: any non-zero value keeps the query
    idx, best, dist = _match(q, g, valid)
    ridx, rbest, rdist = _reference(q, g, valid)
    assert _same_bits(dist, rdist)
    assert np.array_equal(idx, ridx) and best.tobytes() == rbest.tobytes()
    assert idx[0] == 13 and dist[0, 13].tobytes() == dist[0, 200].tobytes()
    assert idx[1] == 77 and best[1] == 0.0
    assert np.isnan(dist[valid != 0, 5]).all() and not (idx == 5).any()
    assert (idx[[3, 64, 69]] == -1).all() and np.isposinf(best[[3, 64, 69]]).all()
    # every distance NaN: no match
    idx, best, _ = _match(q[:3], np.full((2, D), np.nan, np.float32))
    assert (idx == -1).all() and np.isposinf(best).all()
    # an overflowing sum is +inf and still a match (numpy's argmin of [inf] is 0)
    big = np.zeros((1, D), np.float32)
    big[0, 0] = 1e19
    idx, best, _ = _match(-big, big)
    assert idx[0] == 0 and np.isposinf(best[0])
    # empty gallery
    idx, best, _ = _match(q, np.zeros((0, D), np.float32))
    assert (idx == -1).all() and np.isposinf(best).all()


def test_match_argument_errors():
    L = lib()
    buf = DeviceBuffer(4096)
    p = buf.ptr
    bad = [
        (None, 1, p, 1, D, None, p, p, None),      # NULL query
        (p, 1, None, 1, D, None, p, p, None),      # NULL gallery with g > 0
        (p, 1, p, 1, D, None, None, p, None),      # NULL best index
        (p, 1, p, 1, D, None, p, None, None),      # NULL best distance
        (p, 1, p, 1, 0, None, p, p, None),         # dim == 0
        (p, 0, p, 1, D, None, p, p, None),         # no queries
        (p, 1 << 31, p, 1, D, None, p, p, None),   # beyond 32-bit row indices
        (p, 1, p, 1 << 31, D, None, p, p, None),
        (p, 1 << 24, p, 1 << 24, D, None, p, p, None),  # tile count beyond 31 bits
    ]
    for args in bad:
        assert L.zr_embed_match_async(*args, None) == -1, args
        assert L.zr_last_error()


# ------------------------------------------------------------------ host classes
def _face_frame(golden_dir):
    g = np.load(os.path.join(golden_dir, "sad_linus_face.npz"))
    f = np.full((128, 128, 4), 255, np.uint8)
    f[..., :3] = g["codes"].transpose(1, 2, 0)
    return f


def _view_desc(view):
    out = np.zeros(10, np.float32)
    v = View(view.rect.cx, view.rect.cy, view.rect.w, view.rect.h, view.rad)
    check(lib().zr_view_describe(C.byref(v), 1, 0, out.ctypes.data))
    return out[:8]


@pytest.fixture(scope="module")
def recognizer(golden_dir):
    from zaru_amd import host
    return host.FaceRecognizer(model_bytes(golden_dir), "face")


def test_embedder_matches_cpu_chain(golden_dir, recognizer):
    from zaru_amd import host
    frame = _face_frame(golden_dir)
    det = host.Detector("face")
    emb = host.FaceEmbedder(model_bytes(golden_dir))
    dets = det.detect(frame)
    assert dets, "the reference face must be detected"
    got = emb.embed_first_face(det, frame)
    assert got is not None and got.shape == (D,)
    # The fixture's own detection (its raw outputs decoded for this 128x128 frame) is the one the
    # detector reports, up to the network's error; the CPU chain starts from the reported rect,
    # so that the view comparison below can be bit for bit.
    fx = np.load(os.path.join(golden_dir, "sad_linus_face.npz"))
    fdet = O.detect_post(O.FACE, fx["regressors"][0], fx["classificators"][0], 128, 128, 128, 128)[0]
    rect = O.Rect.from_center(*dets[0].bounding_rect().tuple())
    assert np.abs(np.array(rect.tuple()) - np.array(fdet.rect.tuple())).max() <= 0.05, (rect.tuple(), fdet.rect.tuple())
    crop = O.grow_to_fit_aspect(O.grow_rel(rect, 0.4), 1, 1)
    view = O.view_compose(O.view_full(128, 128), crop)
    x = O.preproc(frame, view, 112, 112, -1.0, 1.0)
    want = tool().run_model(graph(golden_dir), x[None], np.float32)[0]
    err = float(np.abs(got - want).max())
    print(f"embed_first_face max|gpu - cpu f32| = {err:.3e}")
    assert err <= ABS_TOL
    # the crop view the device builds for this frame is the CPU view's descriptor
    d_frame = DeviceBuffer.from_array(frame)
    found, demb, _, _ = recognizer.recognize([(d_frame.ptr, 128, 128, 512)], host.Gallery())
    assert found[0]
    desc, vframe = recognizer.views()
    assert vframe[0] == 0 and desc[0].tobytes() == _view_desc(view).tobytes()
    assert demb[0].tobytes() == got.tobytes()


def test_recognizer_equals_per_frame_api(golden_dir, recognizer):
    from zaru_amd import host
    face = _face_frame(golden_dir)
    shifted = np.roll(face, 7, axis=1)
    noise = np.random.default_rng(41).integers(0, 256, size=(128, 128, 4), dtype=np.uint8)
    noise[..., 3] = 255
    frames = [face, shifted, np.zeros((128, 128, 4), np.uint8), face.copy(), noise]
    det = host.Detector("face")
    emb = host.FaceEmbedder(model_bytes(golden_dir))
    per_frame = [emb.embed_first_face(det, f) for f in frames]
    assert per_frame[0] is not None and per_frame[2] is None
    gal = host.Gallery()
    rows = np.concatenate([per_frame[0][None], _normal(np.random.default_rng(42), 2)])
    gal.add(rows, [7, 1000, 2 ** 40 + 3])
    assert len(gal) == 3
    bufs = [DeviceBuffer.from_array(f) for f in frames]
    found, embs, ids, dist = recognizer.recognize([(b.ptr, 128, 128, 512) for b in bufs], gal)
    for i, e in enumerate(per_frame):
        assert bool(found[i]) == (e is not None), i
        if e is None:
            assert ids[i] == host.NO_MATCH and np.isposinf(dist[i]) and not embs[i].any(), i
            continue
        assert embs[i].tobytes() == e.tobytes(), i
        mid, mdist = gal.match(e[None])
        assert ids[i] == mid[0] and dist[i].tobytes() == mdist[0].tobytes(), i
        ref = difference_matrix(e[None], rows)[0]
        assert dist[i].tobytes() == ref.min().tobytes() and ids[i] == [7, 1000, 2 ** 40 + 3][int(np.argmin(ref))], i
    assert not found[2]
    assert found[3] and ids[3] == 7 and dist[3] == 0.0
    # a gallery grown past its first allocation keeps its rows
    more = _normal(np.random.default_rng(43), 100)
    gal.add(more, list(range(2000, 2100)))
    mid, mdist = gal.match(np.concatenate([per_frame[0][None], more[99:100]]))
    assert list(mid) == [7, 2099] and (mdist == 0.0).all()
    gal.clear()
    mid, mdist = gal.match(per_frame[0][None])
    assert mid[0] == host.NO_MATCH and np.isposinf(mdist[0])


def test_same_face_is_nearest(net, golden_dir):
    from zaru_amd.nn import Cnn, ColorMapper
    from zaru_amd import host
    g = golden(golden_dir)
    cnn = Cnn(net, ColorMapper.linear(-1.0, 1.0))
    full = O.view_full(192, 192)
    vt = [(full.rect.cx, full.rect.cy, full.rect.w, full.rect.h, full.rad)]
    embs = np.stack([cnn.estimate_views(f, vt)[0][0] for f in tool().views_frames(golden_dir)])
    err = float(np.abs(embs - g["views/out"]).max())
    print(f"views max|gpu - f64| = {err:.3e}")
    assert err <= ABS_TOL
    # gallery {0 degrees, noise, grey}; the +10 and -10 degree views must both land on the face
    gal = host.Gallery()
    gal.add(embs[[0, 3, 4]], [10, 11, 12])
    ids, dist = gal.match(embs[[1, 2]])
    print("same-face distances", dist, "all", difference_matrix(embs[[1, 2]], embs[[0, 3, 4]]))
    assert list(ids) == [10, 10]
