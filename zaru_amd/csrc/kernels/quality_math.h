// quality_math.h -- the arithmetic of the face quality gate that is not the view lookup: the luma of
// a sampled pixel, the Laplacian, the variance from the three integer sums, the tiers and the flags.
// One definition for both sides: the same source compiles for the host (g++: host/quality.cpp) and
// for gfx950 (kernels/quality.hip).
//
// Everything before the one f64 division is integer arithmetic, so the measurement does not depend
// on the order the pixels are summed in, and host and device agree bit for bit by construction.
// The sampled pixel itself is sample.h's lookup (host/quality.cpp restates it, as host/eye.cpp does).
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
namespace quality {

// Layout mirrored by zr_face_quality / zr_quality_tier in include/zaru_hip.h.
struct Record {
    float size, inside, sharpness, frontal;
    uint32_t flags, rejected, samples, reserved;
};
struct Tier {
    float min_size, min_inside, min_sharpness, min_frontal;
};
enum : uint32_t {
    MEASURED = 1,
    EMBED = 2,
    LEARN = 4,
    FAIL_SIZE = 16,
    FAIL_INSIDE = 32,
    FAIL_SHARPNESS = 64,
    FAIL_FRONTAL = 128,
};
enum { MAX_PIXELS = 16384 };  // ow * oh: n * s2 stays below 2^53, and the grid fits LDS as int16

ZR_HD float quiet_nan() { return __builtin_bit_cast(float, (uint32_t)0x7fc00000u); }

// integer luma of an RGBA8 pixel (r in the lowest byte), 0..255
ZR_HD int luma(uint32_t rgba) {
    const int r = (int)(rgba & 0xffu), g = (int)((rgba >> 8) & 0xffu), b = (int)((rgba >> 16) & 0xffu);
    return (77 * r + 150 * g + 29 * b + 128) >> 8;
}

// the 4-neighbour Laplacian of lumas, |Lap| <= 1020
ZR_HD int laplacian(int c, int l, int r, int u, int d) { return 4 * c - l - r - u - d; }

// the variance of the Laplacian over n pixels from s1 = sum Lap and s2 = sum Lap^2: num and den are
// exact in int64 (below 2^53 for n <= MAX_PIXELS), so the f64 quotient is one rounding and the f32
// conversion another, whatever order the sums were made in
ZR_HD float variance(uint32_t n, int64_t s1, uint64_t s2) {
    if (n == 0) return 0.f;
    const int64_t num = (int64_t)n * (int64_t)s2 - s1 * s1;
    const int64_t den = (int64_t)n * (int64_t)n;
    return (float)((double)num / (double)den);
}

ZR_HD float inside_fraction(uint32_t n_in, int ow, int oh) { return (float)n_in / (float)(ow * oh); }
ZR_HD float shorter_side(float view_w, float view_h) { return __builtin_fminf(view_w, view_h); }

// a minimum of -inf skips its criterion; otherwise value >= min, so a NaN value fails
ZR_HD bool passes(float value, float min) { return min == -__builtin_inff() || value >= min; }

// the FAIL_* bits of the criteria of `t` that r misses
ZR_HD uint32_t failures(const Tier &t, const Record &r) {
    uint32_t f = 0;
    if (!passes(r.size, t.min_size)) f |= FAIL_SIZE;
    if (!passes(r.inside, t.min_inside)) f |= FAIL_INSIDE;
    if (!passes(r.sharpness, t.min_sharpness)) f |= FAIL_SHARPNESS;
    if (!passes(r.frontal, t.min_frontal)) f |= FAIL_FRONTAL;
    return f;
}

// flags and the rejection count of a measured record; `rejected_before` is the incoming record's
ZR_HD void judge(Record &r, const Tier &embed, const Tier &learn, uint32_t rejected_before) {
    const uint32_t fail = failures(embed, r);
    if (fail) {
        r.flags = MEASURED | fail;
        r.rejected = rejected_before == 0xffffffffu ? rejected_before : rejected_before + 1u;
    } else {
        r.flags = MEASURED | EMBED | (failures(learn, r) ? 0u : (uint32_t)LEARN);
        r.rejected = 0;
    }
    r.reserved = 0;
}

}  // namespace quality
}  // namespace zr
