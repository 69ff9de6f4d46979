// eye.hip -- iris and eye-contour refinement of the tracked faces inside the multi-object loop
// (host/device_multi_tracker.cpp): the reference has the two halves of the cascade --
// FaceMeshV1::left_eye / right_eye (face/landmark/mediapipe.rs:162-192) and EyeNetwork on a cropped
// left eye, a right eye by flipping image and landmarks (face/eye.rs:24-27) -- and this is the
// middle, with no host decision between frames.  Entry 2i is row i's left eye, 2i + 1 its right eye.
//   eye_select_kernel   one lane per entry: the eye's RotatedRect at the face's angle, the crop
//                       around it, and the view the eye network samples of it
//   eye_crop_kernel     one workgroup per entry: the packed entry's network-input-sized RGBA crop,
//                       mirrored for a right eye, into its cell of the atlas the eye network runs on
//   eye_commit_kernel   one wavefront per entry: extract, un-mirror, map-out, transform_out, diameter
// (the packing between the first two is identity_compact_kernel, identity.hip).  The arithmetic is
// the host's, operation for operation (host/eye.cpp; eye_math.h is shared; f32, -ffp-contract=off),
// and the sampling is sample.h's, so a cell holds the bits the stem kernel would have sampled.
#include "../runtime/zr_track.h"
#include "eye_math.h"
#include "geom_dev.h"
#include "sample.h"

namespace zr {

using namespace geo;

// grid: one lane per entry, past one wavefront for n > 32
__global__ __launch_bounds__(64) void eye_select_kernel(const EyeSelectParams P) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= 2 * P.n) return;
    const int i = e >> 1, right = e & 1;
    const float *lm = P.lm + (int64_t)i * P.L * 3;
    bool ok = P.state[i].tracked != 0;
    ok = ok && eye::points_finite(lm, 3, right);
    RRect r = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) {
        // rotation_radians (mediapipe.rs:146-160), RotatedRect::bounding (rect.rs:287-325)
        const float *a = lm + 3 * eye::CORNER_RIGHT, *b = lm + 3 * eye::CORNER_LEFT;
        const float angle = signed_angle_to({a[0] - b[0], a[1] - b[1]}, {1.f, 0.f});
        const float c = glibc::cosf(-angle), s = glibc::sinf(-angle), ns = -s;
        float mnx = 3.40282347e38f, mny = 3.40282347e38f, mxx = -3.40282347e38f, mxy = -3.40282347e38f;
        for (int k = 0; k < 4; k++) {
            const float *p = lm + 3 * eye::rect_point(right, k);
            const float rx = (0.f + c * p[0]) + ns * p[1], ry = (0.f + s * p[0]) + c * p[1];
            mnx = fminf(mnx, rx);
            mny = fminf(mny, ry);
            mxx = fmaxf(mxx, rx);
            mxy = fmaxf(mxy, ry);
        }
        const V2 ctr = rot_ccw({(mnx + mxx) * 0.5f, (mny + mxy) * 0.5f}, angle);
        r = {ctr.x, ctr.y, mxx - mnx, mxy - mny, angle};
        ok = r.w > 0.f && r.h > 0.f;  // the reference's grow_to_fit_aspect panics on 0
    }
    P.valid[e] = ok ? 1 : 0;
    if (!ok) return;
    // crop = rect.grow_rel(g).grow_to_fit_aspect(aspect); the view of it the Estimator samples
    // (landmark.rs:320-323: ViewData::view twice, as track.hip's next_view)
    const RRect crop = grow_to_fit_aspect(grow_rel(r, P.grow), P.asp_w, P.asp_h);
    const RRect full = from_top_left(0.f, 0.f, (float)P.state[i].frame_w, (float)P.state[i].frame_h, 0.f);
    const RRect view = view_of(full, crop);
    const RRect local = grow_to_fit_aspect(from_top_left(0.f, 0.f, view.w, view.h, 0.f), P.asp_w, P.asp_h);
    view_desc(P.views[e], view_of(view, local), i / P.K);
    float *o = P.crop + (int64_t)e * 5;
    o[0] = crop.cx;
    o[1] = crop.cy;
    o[2] = crop.w;
    o[3] = crop.h;
    o[4] = crop.rad;
}

const char *launch_eye_select(const EyeSelectParams &p, hipStream_t s) {
    hipLaunchKernelGGL(eye_select_kernel, dim3((2 * p.n + 63) / 64), dim3(64), 0, s, p);
    return "eye_select_kernel";
}

// grid: one 64 x 4 workgroup per entry; an entry that was not packed does nothing, so cells at and
// past *count are not written.  The frame table travels in the kernel arguments, EYE_CROP_FRAMES
// frames a launch: nothing is allocated or copied per step, and a launch crops its frames' views.
// Lane x holds its column's half of the sample (sample_col of the mirrored column for a right eye)
// across the rows.
__global__ __launch_bounds__(256) void eye_crop_kernel(const EyeCropParams P) {
    const int e = blockIdx.x;
    const int k = P.due_of[e];
    const int count = min(*P.count, P.entries);
    if (k < 0 || k >= count) return;  // whole workgroup
    const ViewDesc d = P.due_views[k];
    // as frame_of (sample.h): an index past the table samples a 0 x 0 frame through a valid pointer
    const bool held = d.frame < (uint32_t)P.nframes;
    const int64_t at = held ? (int64_t)d.frame - P.base : (P.base == 0 ? 0 : -1);
    if (at < 0 || at >= EYE_CROP_FRAMES) return;  // another launch's frame (whole workgroup)
    FrameDesc f = P.frames[at];
    if (!held) f.w = f.h = 0;
    const bool right = (e & 1) != 0;
    uint32_t *cell = P.atlas + (int64_t)k * P.in_h * P.in_w;
    for (int x = threadIdx.x; x < P.in_w; x += 64) {
        const float2 col = sample_col(d, right ? P.in_w - 1 - x : x, P.in_w);
        for (int y = threadIdx.y; y < P.in_h; y += 4)
            cell[(int64_t)y * P.in_w + x] = load_pixel(f, sample_join(d, f, col, sample_row(d, y, P.in_h)));
    }
}

const char *launch_eye_crop(const EyeCropParams &p, hipStream_t s) {
    hipLaunchKernelGGL(eye_crop_kernel, dim3(p.entries), dim3(64, 4), 0, s, p);
    return "eye_crop_kernel";
}

namespace {
// point j of packed cell k in frame px: EyeNetwork::extract (eye.rs:47-64: the iris from output 1
// first, then the contour from output 0), the un-mirroring of a right eye, the Estimator's map-out
// and the crop's transform_out on x and y (tracker_update's)
__device__ __forceinline__ void eye_point(const EyeCommitParams &P, int k, int j, bool right, const eye::Local &local,
                                          const RRect &crop, float *p) {
    const float *src = j < eye::IRIS_POINTS ? P.out1 + k * P.stride1 + 3 * j
                                            : P.out0 + k * P.stride0 + 3 * (j - eye::IRIS_POINTS);
    p[0] = src[0];
    p[1] = src[1];
    p[2] = src[2];
    if (right) p[0] = eye::flip_x(p[0], P.in_w);
    eye::map_point(p, local, P.in_w);
    const V2 o = transform_out(crop, {p[0], p[1]});
    p[0] = o.x;
    p[1] = o.y;
}
}  // namespace

// grid: one 64-lane workgroup per entry
__global__ __launch_bounds__(64) void eye_commit_kernel(const EyeCommitParams P) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const int k = P.due_of[e];
    const bool held = k >= 0 && k < 2 * P.n;
    float *out = P.lm + (int64_t)e * eye::POINTS * 3;
    if (!held) {
        for (int j = lane; j < eye::POINTS * 3; j += 64) out[j] = 0.f;
        if (lane == 0) {
            P.diam[e] = 0.f;
            P.valid[e] = 0;
        }
        return;
    }
    const float *c = P.crop + (int64_t)e * 5;
    const RRect crop = {c[0], c[1], c[2], c[3], c[4]};
    const eye::Local local = eye::local_rect(crop.w, crop.h, P.asp_w, P.asp_h);
    const bool right = (e & 1) != 0;
    for (int j = lane; j < eye::POINTS; j += 64) {
        float p[3];
        eye_point(P, k, j, right, local, crop, p);
        out[3 * j] = p[0];
        out[3 * j + 1] = p[1];
        out[3 * j + 2] = p[2];
    }
    if (lane != 0) return;
    float iris[3 * eye::IRIS_POINTS];
    for (int j = 0; j < eye::IRIS_POINTS; j++) eye_point(P, k, j, right, local, crop, iris + 3 * j);
    P.diam[e] = eye::iris_diameter(iris);
    P.valid[e] = 1;
}

const char *launch_eye_commit(const EyeCommitParams &p, hipStream_t s) {
    hipLaunchKernelGGL(eye_commit_kernel, dim3(2 * p.n), dim3(64), 0, s, p);
    return "eye_commit_kernel";
}

}  // namespace zr
