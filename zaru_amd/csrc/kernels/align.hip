// align.hip -- the aligned identity crop of the recognition leg inside the multi-object loop
// (host/multi_stages.cpp, MultiAlign), between identity_select_kernel and the quality gate / the
// compaction: a due row's bounding crop replaced by the five-point similarity crop the embedder was
// trained on, with no host decision between frames.
//   identity_align_kernel   one lane per row: the row's P <= 8 face points gathered from <= 32 of its
//                           landmarks, the fit, the crop as a view of the row's frame, the record.  A
//                           row that falls back keeps the view select wrote; a row that is not due
//                           is not touched at all.
// The arithmetic is align_math.h's, shared with host/align.cpp (f32, -ffp-contract=off).  The counters
// are integers, one atomic per wavefront and counter.
#include "../runtime/zr_align.h"

namespace zr {

static_assert(sizeof(align::View) == sizeof(ViewDesc), "align::View is a ViewDesc");

// grid: 256 lanes a workgroup, past one wavefront for n > 64
__global__ __launch_bounds__(256) void identity_align_kernel(const AlignParams P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool aligned = false, fallback = false;
    if (i < P.n && P.due[i] != 0) {
        align::Crop crop;
        align::Record rec;
        aligned = align::fit(P.cfg, P.lm + (int64_t)i * P.L * 3, 3, crop, rec);
        fallback = !aligned;
        if (aligned) {
            align::View v;
            // the frame index is the one select wrote for this row
            align::crop_view(v, crop, P.state[i].frame_w, P.state[i].frame_h, P.views[i].frame);
            *reinterpret_cast<align::View *>(&P.views[i]) = v;
        }
        P.recs[i] = rec;
    }
    if (!P.totals) return;  // (uniform)
    const uint64_t ma = __ballot(aligned), mf = __ballot(fallback);
    if ((threadIdx.x & 63) != 0) return;
    if (ma != 0) atomicAdd(P.totals, (unsigned long long)__popcll(ma));
    if (mf != 0) atomicAdd(P.totals + 1, (unsigned long long)__popcll(mf));
}

const char *launch_identity_align(const AlignParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_align_kernel, dim3((p.n + 255) / 256), dim3(256), 0, s, p);
    return "identity_align_kernel";
}

}  // namespace zr
