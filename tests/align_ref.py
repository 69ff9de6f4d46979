"""The oracle of the aligned identity crop (zr_identity_align_async, zr_face_align_host,
zaru_amd.host.aligned_crop_view): a numpy f32 restatement of kernels/align_math.h, one rounding per
operation in the documented order, with the platform libm's atan2f / cosf / sinf (what the reference
calls; tests/test_glibc_math_cpu.py pins the project's restatement to it).  It needs no GPU.

``fit`` returns the record, the crop as (cx, cy, w, h, rad) and the intermediate quantities a test wants
to look at; ``view_desc`` is ViewData::full(w, h).view(crop) as the ten words of a zr_view_desc.
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

f32 = np.float32
ALIGNED, FALLBACK, FAIL_DEGENERATE, FAIL_RESIDUAL = 1, 2, 16, 32
VIEW_DESC = np.dtype([("f", f32, 8), ("frame", np.uint32), ("pad", np.uint32)])
RECORD = np.dtype([("scale", f32), ("rad", f32), ("residual", f32), ("flags", np.uint32)])

TEMPLATE = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]
GROUPS = [[33, 133], [362, 263], [1], [61], [291]]

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf"):
    getattr(_libm, _n).restype, getattr(_libm, _n).argtypes = C.c_float, [C.c_float]
_libm.atan2f.restype, _libm.atan2f.argtypes = C.c_float, [C.c_float, C.c_float]


def cosf(x):
    return f32(_libm.cosf(float(x)))


def sinf(x):
    return f32(_libm.sinf(float(x)))


def atan2f(y, x):
    return f32(_libm.atan2f(float(y), float(x)))


def canon(x):
    """Any NaN as the quiet NaN 0x7fc00000."""
    return np.array([0x7FC00000], np.uint32).view(f32)[0] if np.isnan(x) else f32(x)


def fit(template, groups, landmarks, ow=112, oh=112, max_residual=math.inf):
    """landmarks: [L][C >= 2].  Returns a dict: scale, rad, residual (canonical f32), flags, crop (None on a
    fallback), and a, b, mean_t, mean_q, q (the face points)."""
    lm = np.asarray(landmarks, f32)
    P = len(template)
    fP, zero, half = f32(P), f32(0), f32(0.5)
    with np.errstate(all="ignore"):
        t = [(f32(x), f32(y)) for x, y in template]
        sx = sy = zero
        for x, y in t:
            sx, sy = f32(sx + x), f32(sy + y)
        mtx, mty = f32(sx / fP), f32(sy / fP)
        tc = [(f32(x - mtx), f32(y - mty)) for x, y in t]
        den = zero
        for x, y in tc:
            den = f32(den + f32(x * x))
            den = f32(den + f32(y * y))
        q = []
        sqx = sqy = zero
        for g in groups:
            sx = sy = zero
            for idx in g:
                sx, sy = f32(sx + lm[idx, 0]), f32(sy + lm[idx, 1])
            m = f32(len(g))
            q.append((f32(sx / m), f32(sy / m)))
            sqx, sqy = f32(sqx + q[-1][0]), f32(sqy + q[-1][1])
        mqx, mqy = f32(sqx / fP), f32(sqy / fP)
        qc = [(f32(x - mqx), f32(y - mqy)) for x, y in q]
        sa = sb = zero
        for (tx, ty), (qx, qy) in zip(tc, qc):
            sa = f32(sa + f32(tx * qx))
            sa = f32(sa + f32(ty * qy))
            sb = f32(sb + f32(tx * qy))
            sb = f32(sb - f32(ty * qx))
        a, b = f32(sa / den), f32(sb / den)
        scale = f32(np.sqrt(f32(f32(a * a) + f32(b * b))))
        rad = atan2f(b, a)
        gx, gy = f32(f32(f32(ow) * half) - mtx), f32(f32(f32(oh) * half) - mty)
        cx = f32(mqx + f32(f32(a * gx) - f32(b * gy)))
        cy = f32(mqy + f32(f32(b * gx) + f32(a * gy)))
        w, h = f32(scale * f32(ow)), f32(scale * f32(oh))
        s = zero
        for (tx, ty), (qx, qy) in zip(tc, qc):
            ex = f32(qx - f32(f32(a * tx) - f32(b * ty)))
            ey = f32(qy - f32(f32(b * tx) + f32(a * ty)))
            s = f32(s + f32(ex * ex))
            s = f32(s + f32(ey * ey))
        residual = f32(f32(np.sqrt(f32(s / fP))) / scale)
    out = {"scale": canon(scale), "rad": canon(rad), "residual": canon(residual), "a": a, "b": b, "den": den,
           "mean_t": (mtx, mty), "mean_q": (mqx, mqy), "q": q, "crop": None}
    if not (np.isfinite(scale) and np.isfinite(cx) and np.isfinite(cy)) or not scale > 0:
        out["flags"] = FALLBACK | FAIL_DEGENERATE
    elif not residual <= f32(max_residual):
        out["flags"] = FALLBACK | FAIL_RESIDUAL
    else:
        out["flags"] = ALIGNED
        out["crop"] = (cx, cy, w, h, rad)
    return out


def view_desc(crop, frame_w, frame_h, frame=0):
    """ViewData::full(frame_w, frame_h).view(crop) as a zr_view_desc (one VIEW_DESC row)."""
    cx, cy, w, h, crad = crop
    zero, half = f32(0), f32(0.5)
    with np.errstate(all="ignore"):
        pw, ph = f32(frame_w), f32(frame_h)
        pcx, pcy = f32(zero + f32(pw * half)), f32(zero + f32(ph * half))
        rad = f32(zero + crad)
        hx, hy = f32(pw * half), f32(ph * half)
        vx, vy = f32(cx - hx), f32(cy - hy)
        c, s = cosf(zero), sinf(zero)
        ns = f32(-s)
        rx = f32(f32(zero + f32(c * vx)) + f32(ns * vy))
        ry = f32(f32(zero + f32(s * vx)) + f32(c * vy))
        tlx, tly = f32(pcx - f32(pw * half)), f32(pcy - f32(ph * half))
        ox, oy = f32(f32(rx + hx) + tlx), f32(f32(ry + hy) + tly)
        x0, y0 = f32(ox - f32(w * half)), f32(oy - f32(h * half))
        ncx, ncy = f32(x0 + f32(w * half)), f32(y0 + f32(h * half))
        d = np.zeros(1, VIEW_DESC)
        d["f"][0] = [f32(w * half), f32(h * half), f32(ncx - f32(w * half)), f32(ncy - f32(h * half)), w, h,
                     cosf(rad), sinf(rad)]
        d["frame"] = frame
    return d[0]


def record(r):
    """A fit as one RECORD row."""
    out = np.zeros(1, RECORD)
    out["scale"], out["rad"], out["residual"], out["flags"] = r["scale"], r["rad"], r["residual"], r["flags"]
    return out[0]


def sample_point(desc, gx, gy, ow, oh):
    """Where grid coordinate (gx, gy) of an ow x oh grid lands in the frame through a view's sampling map, in
    f64 and without the sampler's rounding to pixels: view px = grid * view_size / grid_size, rotated about
    the view's centre, moved to its top left."""
    hw, hh, tlx, tly, vw, vh, c, s = (float(v) for v in desc["f"])
    vx, vy = gx * vw / ow - hw, gy * vh / oh - hh
    return c * vx - s * vy + hw + tlx, s * vx + c * vy + hh + tly


def unsample_point(desc, px, py, ow, oh):
    """The inverse of sample_point: the grid coordinate whose sample is frame point (px, py)."""
    hw, hh, tlx, tly, vw, vh, c, s = (float(v) for v in desc["f"])
    rx, ry = px - tlx - hw, py - tly - hh
    vx, vy = c * rx + s * ry, -s * rx + c * ry
    return (vx + hw) * ow / vw, (vy + hh) * oh / vh
