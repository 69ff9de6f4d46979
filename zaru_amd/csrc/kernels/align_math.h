// align_math.h -- the arithmetic of the aligned identity crop: the least-squares similarity (no
// reflection) that maps a template of P points on the embedder's ow x oh input grid onto P points of a
// face, and the crop that similarity makes of the frame -- the rotated rect whose sampling grid puts
// the face's points where the template has them.
// One definition for both sides: the same source compiles for the host (g++: host/align.cpp,
// host/recognition.cpp) and for gfx950 (kernels/align.hip), and both produce the same bits for the
// crop and the whole record.
//
// f32 only; + - * / sqrt, comparisons, and glibc's atan2f / cosf / sinf as glibc_math.h restates them
// (on both sides).  The build forbids contraction (-ffp-contract=off) and rounds division and sqrt
// correctly, so every operation below is one IEEE rounding, in this order:
//   face points  template point p has a group of m = 1..4 landmark indices (-1 ends it):
//                sx = ((0.f + x[i0]) + x[i1]) ..., q_p = (sx / (float)m, sy / (float)m)
//   means        of t and of q: in-order sums from 0 over p, each / (float)P; t' = t - mean_t, q' = q - mean_q
//   den          s = 0; per p ascending: s = s + t'x * t'x; s = s + t'y * t'y
//   a            s = 0; per p: s = s + t'x * q'x; s = s + t'y * q'y;  a = s / den
//   b            s = 0; per p: s = s + t'x * q'y; s = s - t'y * q'x;  b = s / den
//                so that q ~ [[a, -b], [b, a]] t + T
//   scale, rad   sqrtf(a * a + b * b), atan2f(b, a)
//   crop         g = (ow * 0.5f - mean_t.x, oh * 0.5f - mean_t.y)
//                c = mean_q + (a * g.x - b * g.y, b * g.x + a * g.y)
//                RRect{c.x, c.y, scale * ow, scale * oh, rad}
//   residual     s = 0; per p: e = q' - (a * t'x - b * t'y, b * t'x + a * t'y); s = s + e.x * e.x;
//                s = s + e.y * e.y;  residual = sqrtf(s / (float)P) / scale   (grid pixels)
// The crop falls back (the caller keeps the bounding crop) when scale, c.x or c.y is not finite or
// !(scale > 0) (DEGENERATE), or !(residual <= max_residual) (RESIDUAL; a NaN residual falls back).
// The record's floats are canonicalised as procrustes_math.h does: any NaN becomes 0x7fc00000.
// crop_view is the crop as a view of the whole frame: geom_dev.h's view_of(full, crop) and view_desc
// (ViewData::full(w, h).view(crop), then make_view), operation for operation.
#pragma once
#include <stdint.h>

#include "glibc_math.h"

namespace zr {
namespace align {

enum { MAX_POINTS = 8, MAX_GROUP = 4 };

// Layouts mirrored by zr_align_cfg / zr_face_alignment in include/zaru_hip.h.
struct Cfg {
    int32_t num_points;  // P, 2..8
    int32_t ow, oh;      // the embedder's input grid
    float tmpl[MAX_POINTS][2];
    int32_t group[MAX_POINTS][MAX_GROUP];
    float max_residual;
};
struct Record {
    float scale, rad, residual;
    uint32_t flags;
};
enum : uint32_t { ALIGNED = 1, FALLBACK = 2, FAIL_DEGENERATE = 16, FAIL_RESIDUAL = 32 };

struct Crop {  // RRect: centre, size, rotation
    float cx, cy, w, h, rad;
};
struct View {  // the ten words of a ViewDesc / zr_view_desc
    float half_w, half_h, tl_x, tl_y, view_w, view_h, cos_r, sin_r;
    uint32_t frame, pad_;
};

ZR_HD float canon(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;
    return __builtin_bit_cast(float, u);
}
ZR_HD bool finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

// the centred template and its den; what a call refuses is den == 0 (or not finite)
ZR_HD float center_template(const Cfg &c, float *tx, float *ty, float &mtx, float &mty) {
    const int P = c.num_points;
    float sx = 0.f, sy = 0.f;
    for (int p = 0; p < P; ++p) {
        sx = sx + c.tmpl[p][0];
        sy = sy + c.tmpl[p][1];
    }
    mtx = sx / (float)P;
    mty = sy / (float)P;
    float den = 0.f;
    for (int p = 0; p < P; ++p) {
        tx[p] = c.tmpl[p][0] - mtx;
        ty[p] = c.tmpl[p][1] - mty;
        den = den + tx[p] * tx[p];
        den = den + ty[p] * ty[p];
    }
    return den;
}

// lm: the face's landmarks, `stride` floats per point (x, y first).  Returns true when the crop is
// aligned; false is the fallback, `crop` then holds what was computed and is not to be used.
ZR_HD bool fit(const Cfg &c, const float *lm, int stride, Crop &crop, Record &rec) {
    const int P = c.num_points;
    float tx[MAX_POINTS], ty[MAX_POINTS], qx[MAX_POINTS], qy[MAX_POINTS], mtx, mty;
    const float den = center_template(c, tx, ty, mtx, mty);
    float sqx = 0.f, sqy = 0.f;
    for (int p = 0; p < P; ++p) {
        float sx = 0.f, sy = 0.f;
        int m = 0;
        for (int j = 0; j < MAX_GROUP; ++j) {
            const int idx = c.group[p][j];
            if (idx < 0) break;
            sx = sx + lm[(int64_t)idx * stride];
            sy = sy + lm[(int64_t)idx * stride + 1];
            ++m;
        }
        qx[p] = sx / (float)m;
        qy[p] = sy / (float)m;
        sqx = sqx + qx[p];
        sqy = sqy + qy[p];
    }
    const float mqx = sqx / (float)P, mqy = sqy / (float)P;
    float sa = 0.f, sb = 0.f;
    for (int p = 0; p < P; ++p) {
        qx[p] = qx[p] - mqx;
        qy[p] = qy[p] - mqy;
        sa = sa + tx[p] * qx[p];
        sa = sa + ty[p] * qy[p];
        sb = sb + tx[p] * qy[p];
        sb = sb - ty[p] * qx[p];
    }
    const float a = sa / den, b = sb / den;
    const float scale = __builtin_sqrtf(a * a + b * b);
    const float rad = glibc::atan2f(b, a);
    const float gx = (float)c.ow * 0.5f - mtx, gy = (float)c.oh * 0.5f - mty;
    crop.cx = mqx + (a * gx - b * gy);
    crop.cy = mqy + (b * gx + a * gy);
    crop.w = scale * (float)c.ow;
    crop.h = scale * (float)c.oh;
    crop.rad = rad;
    float s = 0.f;
    for (int p = 0; p < P; ++p) {
        const float ex = qx[p] - (a * tx[p] - b * ty[p]);
        const float ey = qy[p] - (b * tx[p] + a * ty[p]);
        s = s + ex * ex;
        s = s + ey * ey;
    }
    const float residual = __builtin_sqrtf(s / (float)P) / scale;
    rec.scale = canon(scale);
    rec.rad = canon(rad);
    rec.residual = canon(residual);
    if (!finite(scale) || !finite(crop.cx) || !finite(crop.cy) || !(scale > 0.f)) {
        rec.flags = FALLBACK | FAIL_DEGENERATE;
        return false;
    }
    if (!(residual <= c.max_residual)) {
        rec.flags = FALLBACK | FAIL_RESIDUAL;
        return false;
    }
    rec.flags = ALIGNED;
    return true;
}

// ViewData::full(frame_w, frame_h).view(crop) as a view table entry (geom_dev.h: from_top_left,
// transform_out with the parent's rotation 0 evaluated like any other, view_of, view_desc)
ZR_HD void crop_view(View &vd, const Crop &k, uint32_t frame_w, uint32_t frame_h, uint32_t frame) {
    const float pw = (float)frame_w, ph = (float)frame_h;
    const float pcx = 0.f + pw * 0.5f, pcy = 0.f + ph * 0.5f, prad = 0.f;
    const float rad = prad + k.rad;
    const float hx = pw * 0.5f, hy = ph * 0.5f;
    const float vx = k.cx - hx, vy = k.cy - hy;
    const float c = glibc::cosf(prad), s = glibc::sinf(prad), ns = -s;
    const float rx = (0.f + c * vx) + ns * vy, ry = (0.f + s * vx) + c * vy;
    const float tlx = pcx - pw * 0.5f, tly = pcy - ph * 0.5f;
    const float ox = rx + hx + tlx, oy = ry + hy + tly;
    // from_top_left(o - size * 0.5, size)
    const float x0 = ox - k.w * 0.5f, y0 = oy - k.h * 0.5f;
    const float ncx = x0 + k.w * 0.5f, ncy = y0 + k.h * 0.5f;
    vd.half_w = k.w * 0.5f;
    vd.half_h = k.h * 0.5f;
    vd.tl_x = ncx - k.w * 0.5f;
    vd.tl_y = ncy - k.h * 0.5f;
    vd.view_w = k.w;
    vd.view_h = k.h;
    vd.cos_r = glibc::cosf(rad);
    vd.sin_r = glibc::sinf(rad);
    vd.frame = frame;
    vd.pad_ = 0;
}

}  // namespace align
}  // namespace zr
