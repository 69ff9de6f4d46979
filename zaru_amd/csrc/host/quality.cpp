// quality.cpp -- see quality.h.
#include "quality.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../kernels/quality_math.h"

namespace zr_internal {
int set_error(int code, const std::string &msg);  // runtime/session.cpp: the C ABI's thread-local error
}

namespace {

namespace zq = zr::quality;

uint32_t sat_u32(float f) {  // Rust `f as u32`
    if (!(f > 0.f)) return 0u;
    if (f >= 4294967296.f) return 0xFFFFFFFFu;
    return (uint32_t)f;
}

// sample.h's sample_offset: the byte offset of the frame pixel that grid pixel (x, y) samples, -1 outside
int64_t sample_offset(const zr_view_desc &d, const zr_frame &f, int x, int y, int ow, int oh) {
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
    if (fx < 0.f || fy < 0.f || std::ceil(fx) >= 4294967296.f || std::ceil(fy) >= 4294967296.f) return -1;
    const uint32_t ix = (uint32_t)std::round(fx), iy = (uint32_t)std::round(fy);
    if (ix >= f.width || iy >= f.height) return -1;
    return (int64_t)((uint64_t)iy * f.row_stride + (uint64_t)ix * 4);
}

}  // namespace

extern "C" int zr_face_quality_host(const zr_quality_cfg *cfg, const zr_frame *frame, const zr_view_desc *view,
                                    const zr_pose *pose, zr_face_quality *out) {
    try {
        if (!cfg || !frame || !view || !out) return zr_internal::set_error(ZR_ERR_INVALID_ARGUMENT, "null argument");
        if (!frame->rgba || frame->width == 0 || frame->height == 0)
            return zr_internal::set_error(ZR_ERR_INVALID_ARGUMENT, "empty frame");
        if (cfg->ow < 1 || cfg->oh < 1 || (int64_t)cfg->ow * cfg->oh > ZR_QUALITY_MAX_PIXELS)
            return zr_internal::set_error(ZR_ERR_INVALID_ARGUMENT, "the grid must be 1 x 1 .. 16384 pixels");
        zq::Tier embed, learn;
        std::memcpy(&embed, &cfg->embed, sizeof(embed));
        std::memcpy(&learn, &cfg->learn, sizeof(learn));
        for (const zq::Tier *t : {&embed, &learn})
            if (t->min_size != t->min_size || t->min_inside != t->min_inside || t->min_sharpness != t->min_sharpness ||
                t->min_frontal != t->min_frontal)
                return zr_internal::set_error(ZR_ERR_INVALID_ARGUMENT, "a NaN minimum");
        const int ow = cfg->ow, oh = cfg->oh;
        std::vector<int16_t> grid((size_t)ow * oh);
        uint32_t n_in = 0;
        for (int y = 0; y < oh; y++)
            for (int x = 0; x < ow; x++) {
                const int64_t off = sample_offset(*view, *frame, x, y, ow, oh);
                int16_t v = -1;
                if (off >= 0) {
                    uint32_t px;
                    std::memcpy(&px, frame->rgba + off, 4);
                    v = (int16_t)zq::luma(px);
                    n_in++;
                }
                grid[(size_t)y * ow + x] = v;
            }
        uint32_t n = 0;
        int64_t s1 = 0;
        uint64_t s2 = 0;
        for (int y = 1; y <= oh - 2; y++)
            for (int x = 1; x <= ow - 2; x++) {
                const int16_t *g = grid.data() + (size_t)y * ow + x;
                const int c = g[0], l = g[-1], r = g[1], u = g[-ow], d = g[ow];
                if ((c | l | r | u | d) < 0) continue;
                const int lap = zq::laplacian(c, l, r, u, d);
                n++;
                s1 += lap;
                s2 += (uint64_t)((int64_t)lap * lap);
            }
        zq::Record r;
        r.size = zq::shorter_side(view->view_w, view->view_h);
        r.inside = zq::inside_fraction(n_in, ow, oh);
        r.sharpness = zq::variance(n, s1, s2);
        r.frontal = pose && pose->valid != 0 ? pose->rot[8] : zq::quiet_nan();
        r.samples = n;
        zq::judge(r, embed, learn, 0u);
        std::memcpy(out, &r, sizeof(r));
        return ZR_OK;
    } catch (...) {
        return zr_internal::set_error(ZR_ERR_DEVICE, "out of host memory");
    }
}
