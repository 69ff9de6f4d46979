// eye_math.h -- the arithmetic of the eye refinement that is not plain rect geometry: which mesh
// points bound an eye (face/landmark/mediapipe.rs:162-192; V2: 315-343, the same indices), the
// Estimator's map-out rect of a crop (landmark.rs:320-323), EyeLandmarks::flip_horizontal_in_place
// (face/eye.rs:121-125), the map-out of one point (landmark.rs:336-345) and
// EyeLandmarks::iris_diameter (eye.rs:105-114).  One definition for both sides: the same source
// compiles for the host (g++: host/eye.cpp) and for gfx950 (kernels/eye.hip).
//
// f32 only, nothing but + - * / sqrt and comparisons.  The build forbids contraction
// (-ffp-contract=off) and rounds division and sqrt correctly, so every operation is one IEEE
// rounding, in the reference's order.  The rect geometry itself (RotatedRect::bounding, grow_rel,
// grow_to_fit_aspect, ViewData::view, transform_out) stays where it is: host/geometry.cpp and
// kernels/geom_dev.h, which differ only in whose cosf / sinf they call.
#pragma once
#include <stdint.h>

#ifndef ZR_HD
#ifdef __HIPCC__
#define ZR_HD __host__ __device__ __forceinline__
#else
#define ZR_HD static inline
#endif
#endif

namespace zr {
namespace eye {

enum {
    POINTS = 76,       // EyeLandmarks::NUM_LANDMARKS: 5 iris points, then 71 contour points
    IRIS_POINTS = 5,
    CORNER_LEFT = 33,  // LandmarkIdx::LeftEyeOuterCorner / RightEyeOuterCorner: the face's rotation
    CORNER_RIGHT = 263,
    MIN_FACE_LANDMARKS = 387,  // the largest index used (RightEyeTop = 386) + 1
};

// the k-th point (k = 0..3) RotatedRect::bounding folds over, in the reference's order:
// left {Bottom 145, OuterCorner 33, InnerCorner 133, Top 159}, right {Bottom 374, InnerCorner 362,
// OuterCorner 263, Top 386}
ZR_HD int rect_point(int right, int k) {
    if (right) return k == 0 ? 374 : k == 1 ? 362 : k == 2 ? 263 : 386;
    return k == 0 ? 145 : k == 1 ? 33 : k == 2 ? 133 : 159;
}

ZR_HD bool finite(float v) { return v - v == 0.f; }  // false for +-inf and NaN

// x and y of the four rect points of eye `right` and of the two corners, in a mesh of `stride`
// floats per point
ZR_HD bool points_finite(const float *lm, int stride, int right) {
    bool ok = finite(lm[CORNER_LEFT * stride]) && finite(lm[CORNER_LEFT * stride + 1]) &&
              finite(lm[CORNER_RIGHT * stride]) && finite(lm[CORNER_RIGHT * stride + 1]);
    for (int k = 0; k < 4; k++) {
        const float *p = lm + rect_point(right, k) * stride;
        ok = ok && finite(p[0]) && finite(p[1]);
    }
    return ok;
}

// The rect the Estimator maps an estimate out with, for a view of size vw x vh (landmark.rs:320-323):
// Rect::from_top_left(0, 0, vw, vh).grow_to_fit_aspect(aw : ah) as {x(), y(), width()}
struct Local {
    float x, y, w;
};
ZR_HD Local local_rect(float vw, float vh, int aw, int ah) {
    const float cx = 0.f + vw * 0.5f, cy = 0.f + vh * 0.5f;
    float w = vw, h = vh;
    const float a = (float)aw / (float)ah;
    const float tw = h * a;  // rect.rs:104-117
    if (tw >= w) {
        w += tw - w;
    } else {
        const float th = w / a;
        h += th - h;
    }
    return {cx - w * 0.5f, cy - h * 0.5f, w};
}

// flip_horizontal_in_place on one x, `in_w` the width the estimate was made at
ZR_HD float flip_x(float x, int in_w) {
    const float half = (float)in_w / 2.0f;
    return -(x - half) + half;
}

// Estimator::estimate_impl's map-out of one point (p: x, y, z in network px)
ZR_HD void map_point(float *p, const Local &l, int in_w) {
    const float scale = l.w / (float)in_w;
    p[0] = p[0] * scale;
    p[1] = p[1] * scale;
    p[2] = p[2] * scale;
    p[0] += l.x;
    p[1] += l.y;
}

// iris_diameter of the first five points (p: 5 x 3): Vector::length is sqrt of the dot product's
// fold from 0 (vector.rs:285-306, 350-358)
ZR_HD float iris_diameter(const float *p) {
    float radius = 0.f;
    for (int k = 1; k <= 4; k++) {
        const float dx = p[0] - p[3 * k], dy = p[1] - p[3 * k + 1], dz = p[2] - p[3 * k + 2];
        const float d2 = ((0.f + dx * dx) + dy * dy) + dz * dz;
        radius += __builtin_sqrtf(d2);
    }
    return radius / 4.0f * 2.0f;
}

}  // namespace eye
}  // namespace zr
