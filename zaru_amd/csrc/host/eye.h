// eye.h -- iris and eye-contour refinement of a face mesh: crates/zaru/src/face/eye.rs
// (EyeNetwork, EyeLandmarks) joined to FaceMeshV1::left_eye / right_eye
// (face/landmark/mediapipe.rs:162-192; V2: 315-343, the same indices).  The reference ships the two
// halves and leaves the middle -- crop each eye, mirror the right one, un-mirror its landmarks, map
// them back -- to the caller; this is that middle, restated on the host.  DeviceMultiTracker builds
// the same on the device (kernels/eye.hip), bit for bit.
//
// For a face with landmarks lm (frame px):
//     angle = signed_angle_to(lm[263].xy - lm[33].xy, +X)                  (estimate_angle)
//     left  = RotatedRect::bounding(angle, {lm[145], lm[33], lm[133], lm[159]})
//     right = RotatedRect::bounding(angle, {lm[374], lm[362], lm[263], lm[386]})
//     crop  = rect.grow_rel(grow).grow_to_fit_aspect(eye network aspect)
// An eye is valid when the x and y of its four points and of points 33 / 263 are finite and the
// ungrown rect has width > 0 and height > 0 (the reference's grow_to_fit_aspect panics on 0).
// The left eye is Estimator("eye").estimate(image, ViewData::full(W, H).view(crop)) followed by
// crop.transform_out on every point's x and y (tracker_update's map-out; z stays as the Estimator
// scaled it).  The right eye is the same with the network seeing the horizontally mirrored input,
// and the raw positions un-mirrored before the map-out (EyeLandmarks::flip_horizontal_in_place with
// the input resolution).  grow defaults to 0.65: not the reference's number (it ships no caller) but
// MediaPipe's iris RoI, 2.3 x the corner-to-corner box, expressed through grow_rel (1 + 2 * 0.65).
#pragma once
#include <array>
#include <optional>
#include <vector>

#include "landmark.h"

namespace zh {

constexpr float EYE_CROP_GROW = 0.65f;
constexpr size_t EYE_POINTS = 76;
constexpr uint32_t EYE_INPUT = 64;  // iris_landmark.onnx: 64 x 64

struct EyeRects {
    std::optional<RotatedRect> left, right;  // nullopt: invalid
};
// `landmarks`: L >= 387 points of `stride` floats (x, y first; frame px).  Needs no device.
EyeRects face_eye_rects(const float *landmarks, size_t L, size_t stride = 3);

// rect.grow_rel(grow).grow_to_fit_aspect(aspect)
RotatedRect eye_crop_rect(const RotatedRect &eye, float grow = EYE_CROP_GROW, AspectRatio aspect = AspectRatio{1, 1});
// The view of the whole image the eye network samples for an eye rect: the crop taken as a view
// of the image, ViewData::full(w, h).view(crop), as Estimator::estimate samples it -- its own
// aspect fit of the view's local rect and the second ViewData::view (landmark.rs:320-323), which
// moves no pixel for a crop that already has the aspect but rounds the corner once more.  Needs no
// device; zr_view_describe of it is what zr_eye_select_async writes.
ViewData eye_crop_view(const RotatedRect &eye, uint32_t image_w, uint32_t image_h, float grow = EYE_CROP_GROW,
                       AspectRatio aspect = AspectRatio{1, 1});

class EyeLandmarks {  // eye.rs:67-125
  public:
    static constexpr size_t NUM_LANDMARKS = EYE_POINTS;
    EyeLandmarks() : p_(3 * EYE_POINTS, 0.f) {}
    explicit EyeLandmarks(const float *positions) : p_(positions, positions + 3 * EYE_POINTS) {}
    const std::vector<float> &positions() const { return p_; }
    std::vector<float> &positions_mut() { return p_; }
    std::array<float, 3> iris_center() const { return {p_[0], p_[1], p_[2]}; }
    std::vector<float> iris_contour() const { return std::vector<float>(p_.begin() + 3, p_.begin() + 15); }  // 4 x 3
    std::vector<float> eye_contour() const { return std::vector<float>(p_.begin() + 15, p_.end()); }         // 71 x 3
    float iris_diameter() const;
    void flip_horizontal_in_place(uint32_t full_width);

  private:
    std::vector<float> p_;
};

struct RefinedEye {
    EyeLandmarks landmarks;  // frame px
    float iris_diameter = 0.f;
    RotatedRect crop;
};
struct RefinedEyes {
    std::optional<RefinedEye> left, right;
};

// What follows the network for one eye: `raw` are the 76 extracted points in network px (the iris
// first); a right eye's are un-mirrored, then the Estimator's map-out for `crop`
// (landmark.rs:336-345), crop.transform_out on x and y, and the diameter.  Needs no device.
RefinedEye eye_map_out(const float *raw, bool right, const RotatedRect &crop, uint32_t in_w = EYE_INPUT,
                       AspectRatio aspect = AspectRatio{1, 1});

class EyeRefiner {
  public:
    explicit EyeRefiner(int device = 0);
    // `img`: a host image; `landmarks`: the face's L >= 387 points of 3 floats, in its pixels
    RefinedEyes refine(const Image &img, const float *landmarks, size_t L, float grow = EYE_CROP_GROW);
    // what the network saw of a right eye: the mirrored in_w x in_h RGBA crop (tests)
    std::vector<uint8_t> mirrored_crop(const Image &img, const RotatedRect &eye, float grow = EYE_CROP_GROW) const;
    uint32_t input_width() const { return est_.input_width(); }

  private:
    Estimator est_;
};

}  // namespace zh
