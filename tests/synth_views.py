"""Synthetic graphs (tests/synth_models.py, tests/stemblock_models.py) fed through device view
tables: the two entries the device loops use, zr_cnn_estimate_device_views_async and
zr_cnn_estimate_device_views_count_async, on cases chosen to reach every kernel that tests the
device count (REQUIRED, first part) and some that ignore it (second part).

A case's input is not a tensor but n views of two small RGBA frames.  The frame is a little larger
than the network input, (H + 7) x (W + 5), its bytes are drawn from 1..255, and the ColorMapper is
lo = -1, hi = 1: a sample that maps to lo can only be Color::NONE (a sample outside the frame, or of
a frame past the frame table), and differs from ONNX zero padding (0).  The views cycle through
    a  axis-aligned, the size of the network input, inside the frame
    b  scaled (neither square nor at an integer ratio), inside the frame
    c  axis-aligned, hanging over the frame's bottom-right corner
    d  rotated by an arbitrary angle across the frame's top-left corner
    e  as a, but of frame index N_FRAMES, one past the table: NONE everywhere
with parameters that change from one cycle to the next.  c and d are searched among a few fixed
candidates for one whose share of NONE samples lies in 10 % .. 90 %; an input too small for any of
them (1 x 1) leaves the kind out (Scene.left_out).  The reference input is the oracle's
preprocessing of each view (for e: a tensor of lo), the reference output case.ref of it in float64
and the bound test_gpu_synth's: err <= 8 max(e32, 2^-23 max|ref|), e32 the error of the oracle's f32
interpreter on the same input.

The device count c of a case runs over 0, 1, an interior value, n - 1 and n.  A column tile (128
columns of n * P) straddles the count when c * P is no multiple of 128; planes that are themselves
multiples of 128 positions never straddle, so the interior c is the odd value nearest n / 2 for
which c * P % 128 != 0 holds on every other plane of the graph (odd: a workgroup of irl_kernel holds
two images, one live and one dead).

dwpw_ws_kernel (no count test of its own: it must compute every image) takes a layer only with
about a tile per compute unit, 205 tiles of 448 columns on 256 units: 480 views of a 14 x 14 block
reach it (WS_CASE).

Nothing here needs a GPU to import; Runner does to construct.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import re
import tempfile
import zlib
from dataclasses import dataclass

import numpy as np

import oracle as O
import synth_models as S
import stemblock_models as M
from zaru_amd import _lib

LO, HI = -1.0, 1.0
N_FRAMES = 2
GUARD = 256                      # floats behind every output
NAN_BITS = 0x7FC5A5A5            # a quiet NaN no kernel produces
FACTOR = 8.0                     # test_gpu_synth.FACTOR
BAND = (0.10, 0.90)              # share of NONE samples of a view of kind c or d
ZR_ERR_INVALID_ARGUMENT = -1

# ---------------------------------------------------------------- the selection
_STEMS = ((3, 1, "tf", (9, 35), 1), (3, 2, "tf", (17, 19), 7), (3, 2, "sym", (16, 64), 16), (3, 1, "tf", (8, 33), 24),
          (3, 2, "tf", (17, 19), 64), (5, 1, "tf", (9, 35), 7), (5, 2, "tf", (17, 19), 24), (5, 2, "sym", (17, 19), 32),
          (5, 1, "none", (12, 37), 16))
# stem cases: name -> (k, stride, pad spelling) of the conv that samples the frames
STEMS = {f"F/stem/k{k}s{s}{pad}_{hw[0]}x{hw[1]}_3to{co}": (k, s, pad) for k, s, pad, hw, co in _STEMS}
STEMS.update({"SB/k3_16to16_prelu_40x72": (3, 2, "tf"), "SB/k5_24to28_relu_34x80": (5, 2, "tf"),
              "SB/k3_sym_pads_16to16_37x71": (3, 2, "sym")})

_build, _kinds = S.dwpw(3, 1, "tf", (14, 14), 16, 16, "id", "relu")
WS_CASE = S.Case("V/ws,480_images/k3s1tf_14x14_16to16_id", (3, 14, 14), _build, batches=(480,), kinds=_kinds,
                 want=r"dwpw_ws_kernel<3,1,14,")
S.BY_NAME.setdefault(WS_CASE.name, WS_CASE)

SELECTED = list(STEMS) + [
    "F/stem_Cout65:direct",
    "E/1x1_K130_M32_P49_plain", "E/1x1_K256_M100_P9_add", "E/1x1_K3_M1_P1_plain", "E/patch_2x2s2",
    "E/full_plane_9_chunks", "E/heads_grouped",
    "A/K%4!=0,v4/k3s1tf_8x8_17to32_padc", "A/mfma,2x2/k3s1tf_2x2_24to40_padc", "A/mfma,Mpad96/k5s1tf_6x6_96to96_id",
    "A/tf_pads:row_tasks/k3s2tf_12x12_24to48_poolpad", "A/valu,P=256,vres/k3s1tf_16x16_8to8_id",
    "A/valu,s2,pool_vres/k3s2tf_32x32_8to16_poolpad", "A/valu,M=40:CO48,s1_single_buffer/k5s1tf_16x16_24to40_plain_dwclip",
    "A/siblings_one_launch/k3s1tf_6x6_32to32+24",
    "B/partial_tiles/k3s1tf_20x40_16-64-24_plain", "B/s2_pooled_padded/k3s2tf_40x48_16-64-24_poolpad",
    "C/14_cx48_k3/k3s1tf_14x14_48-96-48_id", "C/7_cx112_k5,257_images/k5s1tf_7x7_112-64-112_id",
    "C/14to7_cx64_k5s2,257_images/k5s2tf_14x14_64-64-112_plain",
    "D/C32_64x64/k3s1tf_64x64_32-16-32_id",
    "F/resize_shortcut_after_its_conv", "F/dw_gap_16x32:fused", "F/whole_plane_depthwise_7x7", "F/gap_global",
    "F/dw_two_readers/k5s2tf_3x3", "F/maxpool_pad_materialised",  # (the suggested names reach neither dw nor elt)
    WS_CASE.name,
]
EDGE_CASES = ("F/stem/k5s2tf_17x19_3to24", "C/14to7_cx64_k5s2,257_images/k5s2tf_14x14_64-64-112_plain",
              "E/1x1_K130_M32_P49_plain")

# Kernels the selection must reach.  Each pattern is searched both in a case's `want` pattern (the
# CPU test: the kernel a case names) and in the profiled kernel names (the GPU test), so it is
# written to fit either spelling.
REQUIRED = {
    # these test the device count
    "gemm_body": r"gemm_kernel<", "gemm_tiled": r"gemm_tiled_kernel<",
    "gemm group launch": r"gemm_(\\w\*|\w*)group_kernel",
    "dwpw_mfma register-staged": r"(?<![a-z_])dwpw_kernel<", "dwpw_mfma LDS-DMA": r"dwpw_dma(?!_group)",
    "dwpw LDS-DMA group launch": r"dwpw_dma_group_kernel<",
    "dwpw_valu": r"dwpw_valu_kernel<", "dwpw_vres": r"dwpw_vres_kernel<",
    "stem": r"stem_kernel<", "stem_dwpw": r"stem_dwpw_kernel<",
    "ir": r"(?<![a-z_])ir_kernel<", "irl": r"irl_kernel<", "bneck": r"bneck_kernel<", "resize": r"resize_kernel",
    # these ignore it
    "gemm_smallk": r"gemm_smallk_kernel<", "gemm_rows": r"gemm_rows_kernel<", "dw": r"(?<![a-z_])dw_kernel",
    "direct": r"direct_kernel", "gap": r"(?<![a-z_])gap_kernel", "dwgap": r"dwgap_kernel", "gdc": r"gdc_kernel",
    "elt": r"elt_kernel", "dwpw_ws": r"dwpw_ws_kernel<",
}
assert all(c.name in STEMS for c in M.FUSED if c.name.startswith(("SB/k3_16to16_prelu", "SB/k5", "SB/k3_sym")))


def case_of(name) -> S.Case:
    assert name in S.BY_NAME, f"no synthetic case named {name!r}"
    return S.BY_NAME[name]


def views_of(name) -> int:
    """How many views a case runs on: 5 (no multiple of 4), 37 where a plane of at most 9 positions
    puts many images into one column tile, and the case's own count where its name gives one."""
    case = case_of(name)
    m = re.search(r",(\d+)_images", name)
    if m:
        return int(m.group(1))
    return 37 if case.in_shape[1] * case.in_shape[2] <= 9 else 5


def fused_input(name) -> bool:
    """The stem samples the frames itself (Plan::input_fusable): no preproc_kernel, the PRE instance."""
    return name in STEMS


def want_of(name):
    """The case's `want`, naming the frame-sampling instance where the stem samples the frames."""
    w = case_of(name).want
    if fused_input(name):
        assert w.endswith("false>"), w
        w = w[:-len("false>")] + "true>"
    return w


def planes(case):
    g, _ = case._built
    return sorted({s[2] * s[3] for s in g.shape.values() if len(s) == 4})


def interior_count(name) -> int:
    case, n = case_of(name), views_of(name)
    ps = [p for p in planes(case) if p % 128]
    for c in sorted(range(2, n - 1), key=lambda c: (c % 2 == 0, abs(2 * c - n))):
        if all(c * p % 128 for p in ps):
            assert 1 < c < n - 1 and c % 2 == 1, (name, c)
            return c
    raise AssertionError(f"{name}: no interior count")


def counts_of(name):
    n = views_of(name)
    return (0, 1, interior_count(name), n - 1, n)


# ---------------------------------------------------------------- frames and views
def frames_of(name, H, W, other=False):
    rng = np.random.default_rng(zlib.crc32(f"{name}/frames/{H}x{W}{'/other' if other else ''}".encode()))
    return [rng.integers(1, 256, size=(H + 7, W + 5, 4), dtype=np.uint8) for _ in range(N_FRAMES)]


def _none(x):
    return (x == np.float32(LO)).all(0)


def _view(frame, child, W, H):
    fh, fw = frame.shape[:2]
    v = O.view_compose(O.view_full(fw, fh), child)
    x = O.preproc(frame, v, W, H, LO, HI)
    return v, x


def _a(j, W, H):
    return O.RRect(O.Rect.from_top_left(float(j % 6), float(j // 6 % 8), float(W), float(H)), 0.0)


def _b(j, W, H):
    return O.RRect(O.Rect.from_top_left(0.4 + j % 3, 0.7 + j % 4, (0.8125 - 0.09 * (j // 12 % 8)) * W + 2.3,
                                        (0.640625 + 0.04 * (j // 12 % 8)) * H + 3.1), 0.0)


def _c_candidates(j, W, H):
    """Whole-pixel positions that hang over the frame's right or bottom edge, those over both (the
    corner) first and nearest to half outside first; cycle j starts at the j-th."""
    cands = []
    for ty in range(H + 7):
        for tx in range(W + 5):
            sx, sy = max(0, tx - 5), max(0, ty - 7)
            share = 1.0 - (1.0 - sx / W) * (1.0 - sy / H)
            if 0.2 <= share <= 0.8:
                cands.append((not (sx and sy), abs(share - 0.5), ty, tx))
    cands.sort()
    for _, _, ty, tx in cands[j % len(cands):] + cands[:j % len(cands)] if cands else ():
        yield O.RRect(O.Rect.from_top_left(tx + 0.25, ty + 0.25, float(W), float(H)), 0.0)


def _d_candidates(j, W, H):  # centred near the top-left corner, rotated
    rad = 0.6 + 0.2371 * j
    if not 0.05 < rad % (math.pi / 2) < math.pi / 2 - 0.05:  # (never near a quarter turn)
        rad += 0.11
    for fx, fy in ((0.3, 0.3), (0.2, 0.2), (0.4, 0.15), (0.0, 0.0), (0.5, 0.5)):
        yield O.RRect(O.Rect(fx * W + 0.31 * (j % 5), fy * H + 0.23 * (j % 3), float(W), float(H)), rad)
    if j:
        yield from _d_candidates(0, W, H)


def _banded(frame, candidates, W, H):
    for child in candidates:
        v, x = _view(frame, child, W, H)
        if BAND[0] <= float(_none(x).mean()) <= BAND[1]:
            return v, x
    return None


@dataclass
class Scene:
    n: int
    frames: list        # N_FRAMES RGBA arrays
    other: list         # frames of the same sizes and another seed
    kinds: list         # per view: "a" .. "e"
    left_out: tuple     # kinds the case's input is too small for
    views: list         # per view: oracle RRect
    frame_of: list      # per view: frame index (N_FRAMES for kind e)
    desc: np.ndarray    # [n][10] uint32: zr_view_describe of every view
    x: np.ndarray       # [n][3][H][W] f32: the reference input


@functools.lru_cache(maxsize=None)
def scene(name) -> Scene:
    case, n = case_of(name), views_of(name)
    _, H, W = case.in_shape
    frames = frames_of(name, H, W)
    left_out = tuple(k for k, cand in (("c", _c_candidates), ("d", _d_candidates))
                     if _banded(frames[0], cand(0, W, H), W, H) is None)
    cycle = [k for k in "abcde" if k not in left_out]
    kinds, views, frame_of, xs = [], [], [], []
    for i in range(n):
        kind, j = cycle[i % len(cycle)], i // len(cycle)
        f = (j // 48 + i % len(cycle)) % N_FRAMES  # (kind a has 48 positions: the other frame after them)
        if kind in "ae":
            v, x = _view(frames[f], _a(j, W, H), W, H)
        elif kind == "b":
            v, x = _view(frames[f], _b(j, W, H), W, H)
        else:
            found = _banded(frames[f], (_c_candidates if kind == "c" else _d_candidates)(j, W, H), W, H)
            assert found, (name, i, kind)
            v, x = found
        if kind == "e":
            f, x = N_FRAMES, np.full((3, H, W), LO, np.float32)
        kinds.append(kind), views.append(v), frame_of.append(f), xs.append(x)
    desc = np.zeros((n, 10), np.uint32)
    for i, (v, f) in enumerate(zip(views, frame_of)):
        one = np.array([[v.rect.cx, v.rect.cy, v.rect.w, v.rect.h, v.rad]], np.float32)
        _lib.check(_lib.lib().zr_view_describe(one.ctypes.data, 1, f, desc[i:i + 1].ctypes.data))
    return Scene(n, frames, frames_of(name, H, W, other=True), kinds, left_out, views, frame_of, desc, np.stack(xs))


def pad_meets_none(name):
    """Output positions of a stem case whose window holds both a zero-padding tap and a NONE sample
    of a view of kind c or d: [(view, oy, ox)]; and whether any window holds a padding tap at all (a
    stride-2 conv over an odd side never reads its one row of bottom / right padding)."""
    k, s, pad = STEMS[name]
    pt, pl, pb, pr = S.PADS[pad](k, s)
    sc = scene(name)
    _, H, W = case_of(name).in_shape
    is_pad = np.ones((H + pt + pb, W + pl + pr), bool)
    is_pad[pt:pt + H, pl:pl + W] = False
    hits, reads_padding = [], False
    for i, kind in enumerate(sc.kinds):
        if kind not in "cd":
            continue
        none = np.zeros_like(is_pad)
        none[pt:pt + H, pl:pl + W] = _none(sc.x[i])
        for oy in range((is_pad.shape[0] - k) // s + 1):
            for ox in range((is_pad.shape[1] - k) // s + 1):
                win = np.s_[oy * s:oy * s + k, ox * s:ox * s + k]
                reads_padding |= bool(is_pad[win].any())
                if is_pad[win].any() and none[win].any():
                    hits.append((i, oy, ox))
    return hits, reads_padding


# ---------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=None)
def reference(name):
    """(f64 reference outputs, per-output e32, per-output floor) of a case on its views' input;
    computed once, as test_gpu_synth.reference."""
    case, x = case_of(name), scene(name).x
    want = case.ref(x)
    with tempfile.NamedTemporaryFile(suffix=".onnx") as f:
        f.write(case.onnx)
        f.flush()
        net = O.Net(f.name, f64=False)
        per_image = [net.run(x[i:i + 1]) for i in range(len(x))]
    f32 = [np.concatenate([im[o] for im in per_image]) for o in range(len(want))]
    e32 = [float(np.abs(a.astype(np.float64) - w).max()) for a, w in zip(f32, want)]
    floor = [2.0 ** -23 * float(np.abs(w).max()) for w in want]
    return want, e32, floor


def check_outputs(name, outs):
    """Failures (strings) of a case's outputs against the f64 bound, and the largest ratio; prints
    every figure."""
    want, e32, floor = reference(name)
    bad, worst = [], 0.0
    assert len(outs) == len(want)
    for o, (got, w) in enumerate(zip(outs, want)):
        assert got.shape == w.shape, (got.shape, w.shape)
        err = float(np.abs(got.astype(np.float64) - w).max())
        unit = max(e32[o], floor[o])
        ratio = err / unit if unit else math.inf if err else 0.0
        worst = max(worst, ratio)
        print(f"synthviews {name} n={len(w)} out={o} err={err:.3e} e32={e32[o]:.3e} ratio={ratio:.3f}")
        if not err <= FACTOR * unit:
            bad.append(f"{name} output {o}: err {err:.3e} > 8 * max(e32 {e32[o]:.3e}, floor {floor[o]:.3e})")
    return bad, worst


# ---------------------------------------------------------------- the GPU runner
@dataclass
class Result:
    rc: int
    outs: list          # per output [n, ...] f32, as the entry left the buffers
    guards: list        # per output [GUARD] uint32
    kernels: list       # profiled kernel names

    def guards_intact(self):
        return all((g == NAN_BITS).all() for g in self.guards)

    def untouched(self):
        return all((o.view(np.uint32) == NAN_BITS).all() for o in self.outs)


class Runner:
    """One loaded session of a case with its frames, view table and output buffers on the device."""

    def __init__(self, name):
        from zaru_amd.nn import NeuralNetwork
        self.name, self.case, self.scene = name, case_of(name), scene(name)
        self.n = self.scene.n
        L = self.L = _lib.lib()
        self.net = NeuralNetwork.from_onnx(self.case.onnx).load()
        _lib.check(L.zr_profile_enable(self.net._h, 1))
        self.stream = C.c_void_p()
        _lib.check(L.zr_stream_create(C.byref(self.stream)))
        self._bufs, self.tables = [], {}
        for key, frames in (("real", self.scene.frames), ("other", self.scene.other)):
            bufs = [_lib.DeviceBuffer.from_array(f) for f in frames]
            self._bufs += bufs
            self.tables[key] = (_lib.Frame * N_FRAMES)(*[_lib.Frame(b.ptr, f.shape[1], f.shape[0], f.shape[1] * 4)
                                                         for b, f in zip(bufs, frames)])
        self.d_views = _lib.DeviceBuffer.from_array(self.scene.desc)
        self.d_count = _lib.DeviceBuffer(4)
        self.shapes = self.net.output_shapes(self.n)
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.outs = [_lib.DeviceBuffer((sz + GUARD) * 4) for sz in self.sizes]
        self.ptrs = (C.c_void_p * len(self.outs))(*[b.ptr for b in self.outs])
        self._buf = C.create_string_buffer(1 << 16)

    def close(self):
        if self.stream:
            self.L.zr_stream_synchronize(self.stream)
            self.L.zr_stream_destroy(self.stream)
            self.stream = None

    def _kernels(self):
        need = C.c_size_t()
        _lib.check(self.L.zr_profile_read(self.net._h, self._buf, len(self._buf), C.byref(need)))  # (returns and clears)
        return S.profile_kernels(self._buf.value.decode())

    def _refill(self):
        for b, sz in zip(self.outs, self.sizes):
            b.upload(np.full(sz + GUARD, NAN_BITS, np.uint32), self.stream)

    def _result(self, rc):
        _lib.check(self.L.zr_stream_synchronize(self.stream))
        outs, guards = [], []
        for b, sz, shape in zip(self.outs, self.sizes, self.shapes):
            a = b.download((sz + GUARD,), np.uint32, self.stream)
            outs.append(a[:sz].view(np.float32).reshape(shape))
            guards.append(a[sz:])
        return Result(rc, outs, guards, self._kernels())

    def full(self, frames="real") -> Result:
        """zr_cnn_estimate_device_views_async on NaN-filled buffers."""
        self._refill()
        self._kernels()
        rc = self.L.zr_cnn_estimate_device_views_async(self.net._h, self.tables[frames], N_FRAMES, self.d_views.ptr, self.n,
                                                       LO, HI, self.ptrs, self.stream)
        _lib.check(rc)
        return self._result(rc)

    def counted(self, c, *, d_count=True, n_frames=N_FRAMES, n_views=None) -> Result:
        """The full entry on the other frames (the arena and every intermediate then hold wrong
        values), NaN-filled buffers, then zr_cnn_estimate_device_views_count_async on the real
        frames with the count c written on the same stream.  A refusal is returned, not raised."""
        self.full("other")
        self._refill()
        host = np.array([c], np.int32)
        _lib.check(self.L.zr_memcpy_async(self.d_count.ptr, host.ctypes.data, 4, 0, self.stream))
        rc = self.L.zr_cnn_estimate_device_views_count_async(
            self.net._h, self.tables["real"], n_frames, self.d_views.ptr, self.n if n_views is None else n_views,
            self.d_count.ptr if d_count else None, LO, HI, self.ptrs, self.stream)
        return self._result(rc)

    def estimate(self):
        """NeuralNetwork.estimate on the preprocessed tensor: the host entry test_gpu_synth uses."""
        outs = self.net.estimate(self.scene.x)
        self._kernels()
        return outs
