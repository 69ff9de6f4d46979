// procrustes_check.cpp -- kernels/procrustes_math.h on the CPU, stand-alone: the transforms of
// tests/golden/procrustes_cases.json (the reference's unit tests, procrustes.rs:348-441) plus the
// degenerate and non-finite sets, meant to be built with -fsanitize=address,undefined and run
// directly (tests/test_procrustes_cpu.py does that).
//   procrustes_check <procrustes_cases.json>
// Exit status 0 and a last line "ok <cases>" when every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zaru_amd/csrc/kernels/procrustes_math.h"

namespace pm = zr::procrustes;

// every number after `"key"` up to the bracket that closes its array
static std::vector<float> numbers_after(const std::string &txt, size_t key_pos) {
    std::vector<float> out;
    size_t i = txt.find('[', key_pos);
    if (i == std::string::npos) return out;
    int depth = 0;
    for (; i < txt.size(); i++) {
        const char ch = txt[i];
        if (ch == '[') {
            depth++;
        } else if (ch == ']') {
            if (--depth == 0) break;
        } else if (ch == '-' || ch == '+' || (ch >= '0' && ch <= '9')) {
            char *end = nullptr;
            out.push_back(std::strtof(txt.c_str() + i, &end));
            i = (size_t)(end - txt.c_str()) - 1;
        }
    }
    return out;
}

static int failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            failures++;                   \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
        }                                 \
    } while (0)

struct Analyzer {
    std::vector<float> q, work;
    float rc[3], rs;
    int n;
    explicit Analyzer(const std::vector<float> &ref) : q(ref), work(ref.size()), n((int)ref.size() / 3) {
        pm::normalise(q.data(), n, rc, &rs);
    }
    pm::Pose run(const std::vector<float> &pts, bool flip = false) {
        pm::Pose p;
        pm::analyze(pts.data(), n, flip, q.data(), rc, rs, work.data(), &p);
        return p;
    }
};

static bool special_orthogonal(const float *R, float eps) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            float d = 0.f;
            for (int k = 0; k < 3; k++) d += R[3 * r + k] * R[3 * c + k];
            if (!(std::fabs(d - (r == c ? 1.f : 0.f)) <= eps)) return false;
        }
    const float det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                      R[2] * (R[3] * R[7] - R[4] * R[6]);
    return std::fabs(det - 1.f) <= eps;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: procrustes_check <procrustes_cases.json>\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::string txt;
    char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) txt.append(buf, n);
    std::fclose(f);

    const std::vector<float> ref = numbers_after(txt, txt.find("\"points\""));
    if (ref.size() < 6 || ref.size() % 3) {
        std::fprintf(stderr, "no points in %s\n", argv[1]);
        return 2;
    }
    const int n = (int)ref.size() / 3;
    Analyzer an(ref);
    int cases = 0;

    // test_recover_transform: every entry of the recovered 4x4 within 1e-5 (MAX_DELTA)
    for (size_t pos = txt.find("\"matrix\""); pos != std::string::npos; pos = txt.find("\"matrix\"", pos + 1)) {
        const std::vector<float> m = numbers_after(txt, pos);
        if (m.size() != 16) {
            std::fprintf(stderr, "a matrix has %zu entries\n", m.size());
            return 2;
        }
        std::vector<float> pts(ref.size());
        for (int k = 0; k < n; k++)
            for (int r = 0; r < 3; r++)
                pts[3 * k + r] = ((m[4 * r] * ref[3 * k] + m[4 * r + 1] * ref[3 * k + 1]) + m[4 * r + 2] * ref[3 * k + 2]) +
                                 m[4 * r + 3];
        const pm::Pose p = an.run(pts);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++)
                EXPECT(std::fabs(p.rot[3 * r + c] * p.scale - m[4 * r + c]) <= 1e-5f, "matrix %d entry (%d, %d): %g vs %g",
                       cases, r, c, p.rot[3 * r + c] * p.scale, m[4 * r + c]);
            EXPECT(std::fabs(p.translation[r] - m[4 * r + 3]) <= 1e-5f, "matrix %d translation %d: %g vs %g", cases, r,
                   p.translation[r], m[4 * r + 3]);
        }
        EXPECT(p.valid == 1u, "matrix %d valid", cases);
        cases++;
    }
    EXPECT(cases >= 15, "only %d matrices", cases);

    // all points equal: scale 0, identity rotation, finite translation
    {
        std::vector<float> pts(ref.size());
        for (int k = 0; k < n; k++) {
            pts[3 * k] = 3.f;
            pts[3 * k + 1] = -2.f;
            pts[3 * k + 2] = 0.5f;
        }
        const pm::Pose p = an.run(pts);
        EXPECT(p.scale == 0.f, "collapsed: scale %g", p.scale);
        EXPECT(p.quat[0] == 0.f && p.quat[1] == 0.f && p.quat[2] == 0.f && p.quat[3] == 1.f, "collapsed: quaternion");
        for (int r = 0; r < 3; r++) EXPECT(std::isfinite(p.translation[r]), "collapsed: translation %d", r);
        cases++;
    }
    // a NaN point: NaN out (the canonical quiet NaN), after the same fixed number of sweeps
    {
        std::vector<float> pts(ref);
        pts[4] = std::nanf("");
        const pm::Pose p = an.run(pts);
        uint32_t bits;
        std::memcpy(&bits, &p.quat[3], 4);
        EXPECT(bits == 0x7fc00000u, "NaN set: quaternion w bits %08x", bits);
        EXPECT(std::isnan(p.scale) && std::isnan(p.rot[0]), "NaN set: scale / rotation");
        cases++;
    }
    // an infinite point and an all-zero covariance fall through as well
    {
        std::vector<float> pts(ref);
        pts[0] = INFINITY;
        (void)an.run(pts);
        pm::Pose p;
        const float zero[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
        pm::finish(c, 1.f, zero, c, 1.f, &p);
        EXPECT(special_orthogonal(p.rot, 1e-3f), "zero covariance: rotation");
        cases++;
    }
    // mirrored (x -> -x): still a proper rotation (procrustes.rs:114)
    {
        std::vector<float> pts(ref);
        for (int k = 0; k < n; k++) pts[3 * k] = -pts[3 * k];
        const pm::Pose p = an.run(pts);
        EXPECT(special_orthogonal(p.rot, 1e-3f), "mirrored: rotation is not special-orthogonal");
        cases++;
    }
    // flip_y is (x, -y, z) on load
    {
        std::vector<float> pts(ref), flipped(ref);
        for (int k = 0; k < n; k++) flipped[3 * k + 1] = -flipped[3 * k + 1];
        const pm::Pose a = an.run(flipped, true), b = an.run(pts, false);
        EXPECT(std::memcmp(&a, &b, sizeof a) == 0, "flip_y");
        cases++;
    }
    // two points: the smallest set
    {
        const std::vector<float> two = {0.f, 0.f, 0.f, 1.f, 2.f, 3.f};
        Analyzer a2(two);
        const pm::Pose p = a2.run({1.f, 1.f, 1.f, 3.f, 5.f, 7.f});
        EXPECT(p.scale == 2.f, "two points: scale %g", p.scale);
        cases++;
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok %d\n", cases);
    return 0;
}
