// eye.cpp -- see eye.h.  Compiled with -ffp-contract=off; the arithmetic that is not rect
// geometry is kernels/eye_math.h, shared with kernels/eye.hip.
#include "eye.h"

#include <cmath>
#include <cstring>

#include "../kernels/eye_math.h"

namespace zh {

namespace ze = zr::eye;

EyeRects face_eye_rects(const float *landmarks, size_t L, size_t stride) {
    if (!landmarks || L < (size_t)ze::MIN_FACE_LANDMARKS || stride < 2 || stride > 64)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "face_eye_rects: a face mesh of >= 387 points with x and y first");
    EyeRects out;
    const float *a = landmarks + (size_t)ze::CORNER_RIGHT * stride, *b = landmarks + (size_t)ze::CORNER_LEFT * stride;
    for (int right = 0; right < 2; right++) {
        if (!ze::points_finite(landmarks, (int)stride, right)) continue;
        // rotation_radians (mediapipe.rs:146-160): estimate_angle's expression
        const float angle = signed_angle_to(Vec2{a[0], a[1]} - Vec2{b[0], b[1]}, Vec2{1.f, 0.f});
        Vec2 pts[4];
        for (int k = 0; k < 4; k++) {
            const float *p = landmarks + (size_t)ze::rect_point(right, k) * stride;
            pts[k] = {p[0], p[1]};
        }
        RotatedRect r;
        RotatedRect::bounding(angle, pts, 4, 2, r);
        if (!(r.rect().width() > 0.f && r.rect().height() > 0.f)) continue;
        (right ? out.right : out.left) = r;
    }
    return out;
}

RotatedRect eye_crop_rect(const RotatedRect &eye, float grow, AspectRatio aspect) {
    if (!(grow >= 0.f) || aspect.w == 0 || aspect.h == 0)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye crop: grow must be >= 0 and the aspect non-zero");
    return eye.grow_rel(grow).grow_to_fit_aspect(aspect);
}

ViewData eye_crop_view(const RotatedRect &eye, uint32_t image_w, uint32_t image_h, float grow, AspectRatio aspect) {
    const ViewData view = ViewData::full(image_w, image_h).view(eye_crop_rect(eye, grow, aspect));
    // Estimator::network_view (landmark.rs:320-323)
    return view.view(RotatedRect(view.local_rect().grow_to_fit_aspect(aspect), 0.f));
}

float EyeLandmarks::iris_diameter() const { return ze::iris_diameter(p_.data()); }

void EyeLandmarks::flip_horizontal_in_place(uint32_t full_width) {
    for (size_t j = 0; j < EYE_POINTS; j++) p_[3 * j] = ze::flip_x(p_[3 * j], (int)full_width);
}

EyeRefiner::EyeRefiner(int device) : est_(LandmarkNetwork::eye(), device) {}

namespace {
// sample.h's lookup on the host: the RGBA8 pixel of `img` that network-input pixel (x, y) of an
// ow x oh input samples through `d`, Color::NONE (0) outside -- the same operations in the same
// order, so the same pixel
uint32_t sat_u32(float f) {
    if (!(f > 0.f)) return 0u;
    if (f >= 4294967296.f) return 0xFFFFFFFFu;
    return (uint32_t)f;
}
uint32_t sample_pixel(const zr_view_desc &d, const Image &img, int x, int y, int ow, int oh) {
    const float u = (float)x / (float)ow;
    const float w = (float)y / (float)oh;
    const uint32_t sx = sat_u32(std::round(u * d.view_w));
    const uint32_t sy = sat_u32(std::round(w * d.view_h));
    const float px = (float)sx + 0.5f, py = (float)sy + 0.5f;
    const float vx = px - d.half_w, vy = py - d.half_h;
    const float ns = -d.sin_r;
    const float rx = (0.f + d.cos_r * vx) + ns * vy;
    const float ry = (0.f + d.sin_r * vx) + d.cos_r * vy;
    const float ox = (rx + d.half_w) + d.tl_x;
    const float oy = (ry + d.half_h) + d.tl_y;
    const float fx = std::round(ox - 0.5f), fy = std::round(oy - 0.5f);
    if (fx < 0.f || fy < 0.f || std::ceil(fx) >= 4294967296.f || std::ceil(fy) >= 4294967296.f) return 0u;
    const uint32_t ix = (uint32_t)std::round(fx), iy = (uint32_t)std::round(fy);
    if (ix >= img.width || iy >= img.height) return 0u;
    uint32_t v;
    std::memcpy(&v, img.rgba + (uint64_t)iy * img.row_stride + (uint64_t)ix * 4, 4);
    return v;
}
}  // namespace

std::vector<uint8_t> EyeRefiner::mirrored_crop(const Image &img, const RotatedRect &eye, float grow) const {
    if (img.on_device || !img.rgba) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the eye refiner takes a host image");
    const int in_w = (int)est_.cnn().input_width(), in_h = (int)est_.cnn().input_height();
    const zr_view v = to_zr_view(eye_crop_view(eye, img.width, img.height, grow, est_.aspect()));
    zr_view_desc d;
    check(zr_view_describe(&v, 1, 0, &d));
    std::vector<uint8_t> out((size_t)in_w * in_h * 4);
    for (int y = 0; y < in_h; y++)
        for (int x = 0; x < in_w; x++) {
            const uint32_t p = sample_pixel(d, img, in_w - 1 - x, y, in_w, in_h);
            std::memcpy(out.data() + ((size_t)y * in_w + x) * 4, &p, 4);
        }
    return out;
}

// `mapped`: the 76 points after the Estimator's map-out for `crop`
static RefinedEye finish_mapped(const float *mapped, const RotatedRect &crop) {
    RefinedEye e;
    e.landmarks = EyeLandmarks(mapped);
    std::vector<float> &p = e.landmarks.positions_mut();
    for (size_t j = 0; j < EYE_POINTS; j++) {  // tracker_update's map-out: x and y only
        const Vec2 o = crop.transform_out({p[3 * j], p[3 * j + 1]});
        p[3 * j] = o.x;
        p[3 * j + 1] = o.y;
    }
    e.iris_diameter = e.landmarks.iris_diameter();
    e.crop = crop;
    return e;
}

RefinedEye eye_map_out(const float *raw, bool right, const RotatedRect &crop, uint32_t in_w, AspectRatio aspect) {
    if (!raw || in_w == 0 || aspect.w == 0 || aspect.h == 0)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye_map_out: no positions, or a zero input width or aspect");
    EyeLandmarks lm(raw);
    if (right) lm.flip_horizontal_in_place(in_w);  // un-mirror before the map-out (eye.rs:121-125)
    const ze::Local local = ze::local_rect(crop.rect().width(), crop.rect().height(), (int)aspect.w, (int)aspect.h);
    std::vector<float> &p = lm.positions_mut();
    for (size_t j = 0; j < EYE_POINTS; j++) ze::map_point(&p[3 * j], local, (int)in_w);
    return finish_mapped(p.data(), crop);
}

RefinedEyes EyeRefiner::refine(const Image &img, const float *landmarks, size_t L, float grow) {
    if (img.on_device || !img.rgba) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the eye refiner takes a host image");
    const EyeRects rects = face_eye_rects(landmarks, L, 3);
    const uint32_t in_w = est_.cnn().input_width(), in_h = est_.cnn().input_height();
    const AspectRatio asp = est_.aspect();
    RefinedEyes out;
    if (rects.left) {
        // the existing Estimator path, unchanged
        const RotatedRect crop = eye_crop_rect(*rects.left, grow, asp);
        const Estimate &e = est_.estimate(img, ViewData::full(img.width, img.height).view(crop));
        out.left = finish_mapped(e.positions.data(), crop);
    }
    if (rects.right) {
        const RotatedRect crop = eye_crop_rect(*rects.right, grow, asp);
        // The mirrored network input as an image of its own, estimated on its full view.  That view
        // samples the identity: rotation 0 and size in_w x in_h make u * in_w = x and
        // round((x + 0.5 - in_w / 2) + in_w / 2 + 0 - 0.5) = x exact in f32 (likewise y), so the
        // tensor the network sees is the left-eye tensor of this crop with its columns reversed,
        // tensor'[c][y][x] = tensor[c][y][in_w - 1 - x], bit for bit.
        const std::vector<uint8_t> px = mirrored_crop(img, *rects.right, grow);
        Image mir;
        mir.rgba = px.data();
        mir.width = in_w;
        mir.height = in_h;
        mir.row_stride = (uint64_t)in_w * 4;
        const auto outs = est_.cnn().estimate(mir, {est_.network_view(ViewData::full(in_w, in_h), nullptr)});
        std::vector<const float *> ptrs;
        for (auto &o : outs) ptrs.push_back(o.data());
        Estimate raw;
        extract_landmarks(est_.network(), ptrs.data(), raw, in_w, in_h);
        out.right = eye_map_out(raw.positions.data(), true, crop, in_w, asp);
    }
    return out;
}

}  // namespace zh
