// align.cpp -- see align.h.
#include "align.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "../kernels/align_math.h"

namespace zr_internal {
int set_error(int code, const std::string &msg);  // runtime/session.cpp: the C ABI's thread-local error
}

namespace za = zr::align;

static_assert(sizeof(zr_align_cfg) == sizeof(za::Cfg) && offsetof(zr_align_cfg, tmpl) == offsetof(za::Cfg, tmpl) &&
                  offsetof(zr_align_cfg, group) == offsetof(za::Cfg, group) &&
                  offsetof(zr_align_cfg, max_residual) == offsetof(za::Cfg, max_residual),
              "zr_align_cfg layout");
static_assert(sizeof(zr_face_alignment) == sizeof(za::Record) && sizeof(zr_face_alignment) == 16,
              "zr_face_alignment layout");
static_assert(sizeof(zr_view_desc) == sizeof(za::View), "zr_view_desc layout");
static_assert(ZR_ALIGN_ALIGNED == za::ALIGNED && ZR_ALIGN_FALLBACK == za::FALLBACK &&
                  ZR_ALIGN_FAIL_DEGENERATE == za::FAIL_DEGENERATE && ZR_ALIGN_FAIL_RESIDUAL == za::FAIL_RESIDUAL,
              "alignment flags");

int zr_internal::align_check(const zr_align_cfg *cfg, size_t L) {
    if (!cfg) return set_error(ZR_ERR_INVALID_ARGUMENT, "null argument");
    if (L < 1 || L > (size_t)INT32_MAX) return set_error(ZR_ERR_INVALID_ARGUMENT, "num_landmarks must be >= 1");
    if (cfg->num_points < 2 || cfg->num_points > za::MAX_POINTS)
        return set_error(ZR_ERR_INVALID_ARGUMENT, "num_points must be 2..8");
    if (cfg->ow < 1 || cfg->oh < 1) return set_error(ZR_ERR_INVALID_ARGUMENT, "the grid must be at least 1 x 1");
    if (cfg->max_residual != cfg->max_residual) return set_error(ZR_ERR_INVALID_ARGUMENT, "a NaN max_residual");
    for (int p = 0; p < cfg->num_points; p++) {
        if (!std::isfinite(cfg->tmpl[p][0]) || !std::isfinite(cfg->tmpl[p][1]))
            return set_error(ZR_ERR_INVALID_ARGUMENT, "a template coordinate is not finite");
        if (cfg->group[p][0] < 0) return set_error(ZR_ERR_INVALID_ARGUMENT, "an empty landmark group");
        for (int j = 0; j < za::MAX_GROUP; j++) {
            const int32_t idx = cfg->group[p][j];
            if (idx < -1 || (idx >= 0 && (size_t)idx >= L))
                return set_error(ZR_ERR_INVALID_ARGUMENT, "a landmark index outside [-1, num_landmarks)");
            if (idx < 0) break;
        }
    }
    za::Cfg c;
    std::memcpy(&c, cfg, sizeof c);
    float tx[za::MAX_POINTS], ty[za::MAX_POINTS], mx, my;
    const float den = za::center_template(c, tx, ty, mx, my);
    if (!(den > 0.f) || !std::isfinite(den))
        return set_error(ZR_ERR_INVALID_ARGUMENT, "the template points coincide (den == 0), or their spread overflows");
    return ZR_OK;
}

extern "C" int zr_face_align_host(const zr_align_cfg *cfg, const float *landmarks, size_t num_landmarks,
                                  size_t stride, uint32_t frame_w, uint32_t frame_h, uint32_t frame,
                                  zr_view_desc *view, zr_face_alignment *out) {
    try {
        if (!cfg || !landmarks || !view || !out) return zr_internal::set_error(ZR_ERR_INVALID_ARGUMENT, "null argument");
        if (stride < 2 || stride > (size_t)INT32_MAX) return zr_internal::set_error(ZR_ERR_INVALID_ARGUMENT, "stride must be >= 2");
        if (int rc = zr_internal::align_check(cfg, num_landmarks)) return rc;
        za::Cfg c;
        std::memcpy(&c, cfg, sizeof c);
        za::Crop crop;
        za::Record rec;
        if (za::fit(c, landmarks, (int)stride, crop, rec)) {
            za::View v;
            za::crop_view(v, crop, frame_w, frame_h, frame);
            std::memcpy(view, &v, sizeof v);
        }
        std::memcpy(out, &rec, sizeof rec);
        return ZR_OK;
    } catch (...) {
        return zr_internal::set_error(ZR_ERR_DEVICE, "out of host memory");
    }
}
