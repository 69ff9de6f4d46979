// procrustes.cpp -- see procrustes.h.
#include "procrustes.h"

#include <cmath>
#include <cstring>

#include "../kernels/procrustes_math.h"

namespace zh {

namespace pm = zr::procrustes;
static_assert(sizeof(zr_pose) == sizeof(pm::Pose), "zr_pose layout");

std::array<float, 16> AnalysisResult::transform() const {
    std::array<float, 16> t{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) t[4 * r + c] = rotation_matrix[3 * r + c] * scale;
        t[4 * r + 3] = translation[r];
    }
    t[15] = 1.f;
    return t;
}

std::array<float, 3> AnalysisResult::euler_angles() const {
    const auto &R = rotation_matrix;
    float s = R[6];
    if (s > 1.f) s = 1.f;
    if (s < -1.f) s = -1.f;
    return {std::atan2(R[7], R[8]), -std::asin(s), std::atan2(R[3], R[0])};
}

zr_pose AnalysisResult::pose() const {
    zr_pose p{};
    std::memcpy(p.centroid, centroid.data(), 12);
    p.scale = scale;
    std::memcpy(p.translation, translation.data(), 12);
    p.valid = 1;
    std::memcpy(p.quat, rotation.data(), 16);
    std::memcpy(p.rot, rotation_matrix.data(), 36);
    return p;
}

ProcrustesAnalyzer::ProcrustesAnalyzer(const float *reference, size_t n) : n_(n) {
    if (!reference || n < 2) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "need at least 2 points for procrustes analysis");
    if (n > (size_t)INT32_MAX / 3) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "too many reference points");
    q_.assign(reference, reference + 3 * n);
    work_.resize(3 * n);
    pm::normalise(q_.data(), (int)n, ref_centroid_.data(), &ref_scale_);
}

AnalysisResult ProcrustesAnalyzer::analyze(const float *points, size_t n, bool flip_y) {
    if (!points || n != n_)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "`analyze` called on data of different length than the reference");
    pm::Pose p;
    pm::analyze(points, (int)n, flip_y, q_.data(), ref_centroid_.data(), ref_scale_, work_.data(), &p);
    AnalysisResult r;
    std::memcpy(r.centroid.data(), p.centroid, 12);
    r.ref_centroid = ref_centroid_;
    std::memcpy(r.translation.data(), p.translation, 12);
    r.scale = p.scale;
    std::memcpy(r.rotation.data(), p.quat, 16);
    std::memcpy(r.rotation_matrix.data(), p.rot, 36);
    return r;
}

}  // namespace zh
