// procrustes.h -- ProcrustesAnalyzer (crates/zaru/src/procrustes.rs) on the host: the similarity
// transform that maps a reference point set onto a data set, e.g. the head pose of a face mesh
// against the canonical face mesh (face/landmark/mediapipe.rs:508-522,589-600).  The arithmetic
// is kernels/procrustes_math.h, shared with the device kernel (kernels/procrustes.hip): both
// produce the same bits.  The caller supplies the reference points; the product ships no mesh.
#pragma once
#include <array>
#include <cstddef>
#include <vector>

#include "runtime.h"

namespace zh {

// AnalysisResult (procrustes.rs:197-251)
struct AnalysisResult {
    std::array<float, 3> centroid{};      // of the analysed data; rotation and scaling happen around it
    std::array<float, 3> ref_centroid{};
    std::array<float, 3> translation{};   // with the rotated, scaled reference centroid taken out
    float scale = 0.f;                    // data scale / reference scale
    std::array<float, 4> rotation{};      // unit quaternion {i, j, k, w}, sign not normalised
    std::array<float, 9> rotation_matrix{};  // row-major; what `rotation` was converted from
    // the recovered transform of the reference data, row-major 4x4 (procrustes.rs:245-250):
    // x -> centroid + scale * R * (x - ref_centroid)
    std::array<float, 16> transform() const;
    // roll, pitch, yaw about x, y, z (radians): atan2(R21, R22), -asin(R20), atan2(R10, R00),
    // libm on the host only (R20 clamped to [-1, 1])
    std::array<float, 3> euler_angles() const;
    zr_pose pose() const;  // the same values as the device record
};

class ProcrustesAnalyzer {
  public:
    // `reference`: n x 3 floats; throws on fewer than 2 points
    ProcrustesAnalyzer(const float *reference, size_t n);
    size_t size() const { return n_; }
    const std::array<float, 3> &reference_centroid() const { return ref_centroid_; }
    float reference_scale() const { return ref_scale_; }
    // `points`: exactly size() x 3 floats (throws otherwise); flip_y: a point is (x, -y, z)
    AnalysisResult analyze(const float *points, size_t n, bool flip_y = false);

  private:
    size_t n_ = 0;
    std::array<float, 3> ref_centroid_{};
    float ref_scale_ = 0.f;
    std::vector<float> q_, work_;  // the normalised reference; scratch of one analysis
};

}  // namespace zh
