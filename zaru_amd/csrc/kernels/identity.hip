// identity.hip -- recognition of the tracked faces inside the multi-object loop
// (host/device_multi_tracker.cpp): which objects are embedded this step, their crops, and what
// the match means for each object, with no host decision between frames.
//   identity_select_kernel   one wavefront per slot: the object's identity state and embedding
//                            gathered from the slot it held before (src), the schedule (never
//                            embedded, or now >= next), and for a due object the crop the example
//                            takes of a face (eval_face_recognition.rs:82-91) around the bounding
//                            rect of its landmarks (Rect::bounding, rect.rs:49-68)
//   identity_compact_kernel  the due slots packed in slot order (one workgroup, fixed order)
//   identity_commit_kernel   the match of packed image k written back to its object
// The crop is the host's, operation for operation (host/recognition.cpp landmark_crop_view; f32,
// -ffp-contract=off).  min / max are exact whatever the order, so the wave reduction equals the
// host's fold over the points.
#include "../runtime/zr_track.h"
#include "geom_dev.h"

namespace zr {
namespace {

using namespace geo;

__device__ __forceinline__ IdentityState default_identity() {
    IdentityState d;
    d.row = -1;
    d.distance = __builtin_inff();
    d.embeddings = 0;
    d.flags = 0;
    d.next_ms = 0.0;
    return d;
}

}  // namespace

// grid: one 64-lane workgroup per row; every branch below is uniform over the wave
__global__ __launch_bounds__(64) void identity_select_kernel(const IdentitySelectParams P) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int s0 = (i / P.K) * P.K;
    const bool tracked = P.state[i].tracked != 0;
    const int src = tracked ? P.src[i] : -1;
    const bool known = src >= 0 && src < P.K;  // the object held slot src when its state was written
    const IdentityState st = known ? P.in[s0 + src] : default_identity();
    float2 e = make_float2(0.f, 0.f);
    if (known) e = reinterpret_cast<const float2 *>(P.emb_in + (int64_t)(s0 + src) * IDENTITY_DIM)[lane];
    reinterpret_cast<float2 *>(P.emb_out + (int64_t)i * IDENTITY_DIM)[lane] = e;

    const bool scheduled = tracked && (st.embeddings == 0 || P.now >= st.next_ms);
    const float inf = __builtin_inff();
    float x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
    bool finite = true;
    if (scheduled) {
        const float *lm = P.lm + (int64_t)i * P.L * 3;
        for (int j = lane; j < P.L; j += 64) {  // L is rarely a multiple of 64: idle lanes keep +-inf
            const float x = lm[3 * j], y = lm[3 * j + 1];
            finite = finite && isfinite(x) && isfinite(y);
            x0 = fminf(x0, x);
            y0 = fminf(y0, y);
            x1 = fmaxf(x1, x);
            y1 = fmaxf(y1, y);
        }
    }
    const bool due = scheduled && __all(finite);
    x0 = wave_min(x0);
    y0 = wave_min(y0);
    x1 = wave_max(x1);
    y1 = wave_max(y1);
    if (lane != 0) return;
    P.out[i] = st;
    P.due[i] = due ? 1 : 0;
    if (!due) return;
    // Rect::bounding -> span -> from_top_left; grow_rel(grow); grow_to_fit_aspect; the crop as a
    // view of the whole frame (ViewData::full(w, h).view(crop)); make_view (session.cpp)
    const RRect box = from_top_left(x0, y0, x1 - x0, y1 - y0, 0.f);
    const RRect crop = grow_to_fit_aspect(grow_rel(box, P.grow), P.asp_w, P.asp_h);
    const RRect full = from_top_left(0.f, 0.f, (float)P.state[i].frame_w, (float)P.state[i].frame_h, 0.f);
    view_desc(P.views[i], view_of(full, crop), i / P.K);
}

const char *launch_identity_select(const IdentitySelectParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_select_kernel, dim3(p.n), dim3(64), 0, s, p);
    return "identity_select_kernel";
}

// one workgroup: a block-wide exclusive scan of the due flags per 1024-row chunk (ballots within
// a wave, the 16 wave sums through LDS), as due_compact_kernel (track.hip)
__global__ __launch_bounds__(1024) void identity_compact_kernel(const IdentityCompactParams P) {
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int base = 0;
    for (int c0 = 0; c0 < P.n; c0 += 1024) {  // (n <= 2^24: no overflow)
        const int i = c0 + t;
        const bool req = i < P.n && P.due[i] != 0;
        const uint64_t m = __ballot(req);
        const int in_wave = (int)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = (int)__popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < 16; ++k) {
            before += k < w ? wsum[k] : 0;
            total += wsum[k];
        }
        if (i < P.n) {
            const int k = base + before + in_wave;
            if (req) P.due_views[k] = P.views[i];
            P.due_of[i] = req ? k : -1;
        }
        base += total;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    for (int k = t; k < P.n; k += 1024) P.due_valid[k] = k < base ? 1 : 0;
    if (t == 0) {
        *P.ndue = base;
        if (P.total) *P.total += (uint64_t)base;
    }
}

const char *launch_identity_compact(const IdentityCompactParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_compact_kernel, dim3(1), dim3(1024), 0, s, p);
    return "identity_compact_kernel";
}

// grid: one 64-lane workgroup per row; rows that were not due keep what select wrote
__global__ __launch_bounds__(64) void identity_commit_kernel(const IdentityCommitParams P) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int k = P.due_of[i];
    if (k < 0 || k >= P.n) return;
    reinterpret_cast<float2 *>(P.emb_out + (int64_t)i * IDENTITY_DIM)[lane] =
        reinterpret_cast<const float2 *>(P.dense_emb + (int64_t)k * IDENTITY_DIM)[lane];
    if (lane != 0) return;
    IdentityState st = P.out[i];
    const int best = P.best_idx[k];
    const float dist = P.best_dist[k];
    st.row = best >= 0 && dist <= P.threshold ? best : -1;  // (a NaN distance or threshold: unknown)
    st.distance = dist;
    st.embeddings += 1;
    st.next_ms = P.now + P.interval;
    P.out[i] = st;
}

const char *launch_identity_commit(const IdentityCommitParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_commit_kernel, dim3(p.n), dim3(64), 0, s, p);
    return "identity_commit_kernel";
}

}  // namespace zr
