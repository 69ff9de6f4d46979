// procrustes_math.h -- the arithmetic of ProcrustesAnalyzer (crates/zaru/src/procrustes.rs):
// the similarity transform (scale, rotation, translation) that maps a reference point set onto
// a data set of the same size, i.e. the head pose of a face mesh against the canonical mesh.
// One definition for both sides: the same source compiles for the host (g++: host/procrustes.cpp,
// runtime/session.cpp, tests/native/procrustes_check.cpp) and for gfx950 (kernels/procrustes.hip),
// and both produce the same bits for the whole result record.
//
// f32 only; nothing but + - * / sqrt, comparisons and sign.  The build forbids contraction
// (-ffp-contract=off) and rounds division and sqrt correctly
// (-fhip-fp32-correctly-rounded-divide-sqrt), so every operation below is one IEEE rounding.
//
// Operation order, per set of N >= 2 points (flip_y: a point is (x, -y, z), applied on load):
//   centroid     three running sums from 0 over the points in index order, each / (float)N,
//                then p[k] -= centroid                                  (remove_translation, :165-175)
//   scale        s += (x*x + y*y) + z*z in index order from 0; s /= (float)N; s = sqrt(s);
//                p[k] /= s per component (a division)                        (remove_scale, :182-195)
//                -- these two loops are plain Rust in the reference, so centroid and scale are
//                bit-exact with the reference itself.
//   covariance   M[r][c] = sum_k p[k][r] * q[k][c], k ascending from 0, product and sum rounded
//                separately; q is the reference set after the same two steps.  (The reference
//                multiplies with nalgebra's GEMM, whose order is unspecified: this order is ours.)
//   rotation     R = U diag(1, 1, d) V^T, d = sign(det(V^T U)), from an SVD of M (:138-161).
//                The SVD is a cyclic one-sided Jacobi (Hestenes) on the three columns of M:
//                SWEEPS sweeps over the pairs (0,1) (0,2) (1,2), each pair rotated so that its
//                columns become orthogonal, the same rotation accumulated in V.  Every loop has
//                a fixed trip count: NaN or all-zero input falls through the same sweeps.  The
//                columns are then ordered by norm (descending); u1, u2 and v1, v2 are
//                orthonormalised (Gram-Schmidt), and the third column of U and of V is the cross
//                product of the first two.  That makes det U = det V = +1, which is the
//                diag(1, 1, d) of the reference folded in (a flip lands on the smallest singular
//                value), and it survives a vanishing third singular value.
//                If the data scale == 0 the rotation is the identity (:108-112).
//   quaternion   UnitQuaternion::from_rotation_matrix's four branches on tr = R00 + R11 + R22,
//                stored {i, j, k, w}; the sign is not normalised.
//   result       scale = data_scale / ref_scale;
//                translation = centroid - (R * ref_centroid) * scale, row dot products left to
//                right (:116-136).  The reference rotates by the quaternion; here R is used.
// Finally every float of the record is canonicalised: any NaN becomes the quiet NaN 0x7fc00000
// (an integer test of the bits), because x86 and gfx950 generate and propagate different NaN
// payloads; the record of a non-finite set is then the same bytes on both sides.
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
namespace procrustes {

enum { SWEEPS = 5 };

// the result record; mirrored by zr_pose in include/zaru_hip.h
struct Pose {
    float centroid[3];
    float scale;
    float translation[3];
    uint32_t valid;
    float quat[4];  // i, j, k, w
    float rot[9];   // row-major
};

ZR_HD float canon(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;
    return __builtin_bit_cast(float, u);
}
ZR_HD float quiet_nan() { return __builtin_bit_cast(float, (uint32_t)0x7fc00000u); }

ZR_HD float sq_len(float x, float y, float z) { return (x * x + y * y) + z * z; }
ZR_HD float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
ZR_HD float abs1(float x) { return x < 0.f ? -x : x; }
ZR_HD void cross3(const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// remove_translation + remove_scale in place on n points (xyz interleaved)
ZR_HD void normalise(float *p, int n, float centroid[3], float *scale) {
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int k = 0; k < n; k++) {
        cx += p[3 * k];
        cy += p[3 * k + 1];
        cz += p[3 * k + 2];
    }
    const float fn = (float)n;
    cx /= fn;
    cy /= fn;
    cz /= fn;
    float s = 0.f;
    for (int k = 0; k < n; k++) {
        p[3 * k] -= cx;
        p[3 * k + 1] -= cy;
        p[3 * k + 2] -= cz;
        s += sq_len(p[3 * k], p[3 * k + 1], p[3 * k + 2]);
    }
    s /= fn;
    s = __builtin_sqrtf(s);
    for (int i = 0; i < 3 * n; i++) p[i] /= s;
    centroid[0] = cx;
    centroid[1] = cy;
    centroid[2] = cz;
    *scale = s;
}

// M[r][c] = sum_k p[k][r] * q[k][c]
ZR_HD void covariance(const float *p, const float *q, int n, float M[9]) {
    for (int e = 0; e < 9; e++) {
        const int r = e / 3, c = e - 3 * r;
        float m = 0.f;
        for (int k = 0; k < n; k++) m += p[3 * k + r] * q[3 * k + c];
        M[e] = m;
    }
}

// a (3 vectors of 3, vector-major) <- a unit a[0] and a unit a[1] orthogonal to it
ZR_HD void orthonormal_pair(float *a0, float *a1) {
    const float n0 = dot3(a0, a0);
    if (n0 > 0.f) {
        const float l = __builtin_sqrtf(n0);
        a0[0] /= l;
        a0[1] /= l;
        a0[2] /= l;
    } else if (n0 == 0.f) {  // (NaN stays NaN)
        a0[0] = 1.f;
        a0[1] = 0.f;
        a0[2] = 0.f;
    }
    const float d = dot3(a1, a0);
    float w[3] = {a1[0] - d * a0[0], a1[1] - d * a0[1], a1[2] - d * a0[2]};
    float nw = dot3(w, w);
    if (nw == 0.f) {  // no second direction: any unit vector orthogonal to a0
        const float ax = abs1(a0[0]), ay = abs1(a0[1]), az = abs1(a0[2]);
        float e[3] = {0.f, 0.f, 0.f};
        if (ax <= ay && ax <= az) e[0] = 1.f;
        else if (ay <= az) e[1] = 1.f;
        else e[2] = 1.f;
        cross3(a0, e, w);
        nw = dot3(w, w);
    }
    const float l = __builtin_sqrtf(nw);
    a1[0] = w[0] / l;
    a1[1] = w[1] / l;
    a1[2] = w[2] / l;
}

// R = U diag(1, 1, d) V^T of M's SVD (see the header comment); M and R row-major
ZR_HD void rotation(const float M[9], float R[9]) {
    // columns of A (= M) and of V, column-major: a[j] is column j
    float a[3][3], v[3][3];
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) {
            a[j][i] = M[3 * i + j];
            v[j][i] = i == j ? 1.f : 0.f;
        }
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
        for (int pair = 0; pair < 3; pair++) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
            const float alpha = dot3(a[p], a[p]), beta = dot3(a[q], a[q]), gamma = dot3(a[p], a[q]);
            float c = 1.f, s = 0.f;
            if (gamma != 0.f) {
                const float zeta = (beta - alpha) / (2.f * gamma);
                const float t = (zeta >= 0.f ? 1.f : -1.f) / (abs1(zeta) + __builtin_sqrtf(1.f + zeta * zeta));
                c = 1.f / __builtin_sqrtf(1.f + t * t);
                s = c * t;
            }
            for (int i = 0; i < 3; i++) {
                const float ap = a[p][i], aq = a[q][i];
                a[p][i] = c * ap - s * aq;
                a[q][i] = s * ap + c * aq;
                const float vp = v[p][i], vq = v[q][i];
                v[p][i] = c * vp - s * vq;
                v[q][i] = s * vp + c * vq;
            }
        }
    }
    // order the columns by norm, descending: compare-exchange (0,1) (1,2) (0,1)
    float n[3] = {dot3(a[0], a[0]), dot3(a[1], a[1]), dot3(a[2], a[2])};
    for (int step = 0; step < 3; step++) {
        const int lo = step == 1 ? 1 : 0, hi = lo + 1;
        if (n[lo] < n[hi]) {
            for (int i = 0; i < 3; i++) {
                float t = a[lo][i];
                a[lo][i] = a[hi][i];
                a[hi][i] = t;
                t = v[lo][i];
                v[lo][i] = v[hi][i];
                v[hi][i] = t;
            }
            const float t = n[lo];
            n[lo] = n[hi];
            n[hi] = t;
        }
    }
    orthonormal_pair(a[0], a[1]);
    orthonormal_pair(v[0], v[1]);
    cross3(a[0], a[1], a[2]);
    cross3(v[0], v[1], v[2]);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[3 * r + c] = (a[0][r] * v[0][c] + a[1][r] * v[1][c]) + a[2][r] * v[2][c];
}

// UnitQuaternion::from_rotation_matrix (nalgebra): {i, j, k, w}
ZR_HD void quaternion(const float R[9], float q[4]) {
    const float m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7],
                m22 = R[8];
    const float tr = (m00 + m11) + m22;
    if (tr > 0.f) {
        const float denom = __builtin_sqrtf(tr + 1.f) * 2.f;
        q[3] = 0.25f * denom;
        q[0] = (m21 - m12) / denom;
        q[1] = (m02 - m20) / denom;
        q[2] = (m10 - m01) / denom;
    } else if (m00 > m11 && m00 > m22) {
        const float denom = __builtin_sqrtf(((1.f + m00) - m11) - m22) * 2.f;
        q[3] = (m21 - m12) / denom;
        q[0] = 0.25f * denom;
        q[1] = (m01 + m10) / denom;
        q[2] = (m02 + m20) / denom;
    } else if (m11 > m22) {
        const float denom = __builtin_sqrtf(((1.f + m11) - m00) - m22) * 2.f;
        q[3] = (m02 - m20) / denom;
        q[0] = (m01 + m10) / denom;
        q[1] = 0.25f * denom;
        q[2] = (m12 + m21) / denom;
    } else {
        const float denom = __builtin_sqrtf(((1.f + m22) - m00) - m11) * 2.f;
        q[3] = (m10 - m01) / denom;
        q[0] = (m02 + m20) / denom;
        q[1] = (m12 + m21) / denom;
        q[2] = 0.25f * denom;
    }
}

// the record of a set from its centroid, data scale and covariance against the reference
ZR_HD void finish(const float centroid[3], float data_scale, const float M[9], const float ref_centroid[3],
                  float ref_scale, Pose *out) {
    float R[9];
    rotation(M, R);
    if (data_scale == 0.f) {  // collapsed onto a point: the rotation cannot be recovered
        for (int e = 0; e < 9; e++) R[e] = (e == 0 || e == 4 || e == 8) ? 1.f : 0.f;
    }
    float q[4];
    quaternion(R, q);
    const float scale = data_scale / ref_scale;
    for (int r = 0; r < 3; r++) {
        const float rc = (R[3 * r] * ref_centroid[0] + R[3 * r + 1] * ref_centroid[1]) + R[3 * r + 2] * ref_centroid[2];
        out->translation[r] = canon(centroid[r] - rc * scale);
        out->centroid[r] = canon(centroid[r]);
    }
    out->scale = canon(scale);
    out->valid = 1u;
    for (int e = 0; e < 4; e++) out->quat[e] = canon(q[e]);
    for (int e = 0; e < 9; e++) out->rot[e] = canon(R[e]);
}

// the record of a set that is not analysed: valid = 0, NaN in every float
ZR_HD void invalid(Pose *out) {
    const float nan = quiet_nan();
    for (int r = 0; r < 3; r++) out->centroid[r] = out->translation[r] = nan;
    out->scale = nan;
    out->valid = 0u;
    for (int e = 0; e < 4; e++) out->quat[e] = nan;
    for (int e = 0; e < 9; e++) out->rot[e] = nan;
}

// One whole set, sequentially (the host mirror; the kernel runs the same operations with the
// per-point work spread over a wavefront).  `work` holds 3n floats; q is the normalised reference.
ZR_HD void analyze(const float *points, int n, bool flip_y, const float *q, const float ref_centroid[3],
                   float ref_scale, float *work, Pose *out) {
    for (int k = 0; k < n; k++) {
        work[3 * k] = points[3 * k];
        work[3 * k + 1] = flip_y ? -points[3 * k + 1] : points[3 * k + 1];
        work[3 * k + 2] = points[3 * k + 2];
    }
    float centroid[3], scale, M[9];
    normalise(work, n, centroid, &scale);
    covariance(work, q, n, M);
    finish(centroid, scale, M, ref_centroid, ref_scale, out);
}

}  // namespace procrustes
}  // namespace zr
