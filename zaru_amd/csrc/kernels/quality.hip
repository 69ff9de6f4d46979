// quality.hip -- the face quality gate of the recognition leg inside the multi-object loop
// (host/multi_stages.cpp, MultiQuality): what the embedder is about to see of every due object,
// measured before it is embedded, with no host decision between frames.
//   quality_measure_kernel     one 256-thread workgroup per row: the object's record gathered from the
//                              slot it held before (src, as identity_select_kernel gathers its state);
//                              a due row's crop sampled once on the embedder's ow x oh grid into LDS
//                              as lumas, the Laplacian taken from LDS, three integer sums reduced, the
//                              tiers applied; a row that misses the embed tier leaves the due list
//   quality_learn_mask_kernel  one lane per row: the due list the enrolment and the refinement read,
//                              without the rows that were embedded but missed the learn tier
// The lookup is sample.h's (sample_col / sample_row / sample_join: the stem's, bit for bit), the rest
// quality_math.h's, shared with host/quality.cpp.  The sums are integers, so the reduction order
// does not matter; no float is accumulated, atomically or otherwise.  Every branch that returns or
// meets a barrier is uniform over the workgroup.
#include "../runtime/zr_track.h"
#include "quality_math.h"
#include "sample.h"

namespace zr {

namespace {

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ quality::Tier tier_of(const float *m) { return {m[0], m[1], m[2], m[3]}; }

}  // namespace

// dynamic LDS: 4 waves x 4 sums of 8 bytes, then the ow x oh grid as int16 (luma, -1 outside)
__global__ __launch_bounds__(256) void quality_measure_kernel(const QualityParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long *wsum = reinterpret_cast<long long *>(smem);
    int16_t *grid = reinterpret_cast<int16_t *>(smem + 128);
    const int i = blockIdx.x, t = threadIdx.x;
    const bool due = P.due[i] != 0;
    if (!due && P.base != 0) return;  // whole workgroup: the launch with base 0 copies the idle rows
    const int s0 = (i / P.K) * P.K;
    const int src = P.state[i].tracked != 0 ? P.src[i] : -1;
    const bool known = src >= 0 && src < P.K;  // the object held slot src when its record was written
    if (!due) {
        if (t == 0) {
            quality::Record r = {0.f, 0.f, 0.f, 0.f, 0u, 0u, 0u, 0u};
            if (known) r = P.in[s0 + src];
            P.out[i] = r;
        }
        return;
    }
    const ViewDesc d = P.views[i];
    // as eye_crop_kernel: an index past the table samples a 0 x 0 frame through a valid pointer
    const bool held = d.frame < (uint32_t)P.nframes;
    const int64_t at = held ? (int64_t)d.frame - P.base : (P.base == 0 ? 0 : -1);
    if (at < 0 || at >= QUALITY_FRAMES) return;  // another launch's frame (whole workgroup)
    FrameDesc f = P.frames[at];
    if (!held) f.w = f.h = 0;

    const int ow = P.ow, oh = P.oh, npx = ow * oh;  // <= quality::MAX_PIXELS: at most 64 a thread
    int n_in = 0;
    for (int p = t; p < npx; p += 256) {
        const int y = p / ow, x = p - y * ow;
        const int64_t off = sample_join(d, f, sample_col(d, x, ow), sample_row(d, y, oh));
        const uint32_t px = load_pixel(f, off);
        grid[p] = off >= 0 ? (int16_t)quality::luma(px) : (int16_t)-1;
        n_in += off >= 0 ? 1 : 0;
    }
    __syncthreads();
    // a thread's sums over its <= 64 pixels fit 32 bits: |Lap| <= 1020, Lap^2 <= 1,040,400
    int n = 0, s1 = 0;
    uint32_t s2 = 0;
    for (int p = t; p < npx; p += 256) {
        const int y = p / ow, x = p - y * ow;
        if (x < 1 || y < 1 || x > ow - 2 || y > oh - 2) continue;
        const int c = grid[p], l = grid[p - 1], r = grid[p + 1], u = grid[p - ow], dn = grid[p + ow];
        if ((c | l | r | u | dn) < 0) continue;  // a tap outside the frame
        const int lap = quality::laplacian(c, l, r, u, dn);
        n += 1;
        s1 += lap;
        s2 += (uint32_t)(lap * lap);
    }
    const long long w_in = wave_sum(n_in), w_n = wave_sum(n), w_s1 = wave_sum(s1), w_s2 = wave_sum((long long)s2);
    if ((t & 63) == 0) {
        long long *w = wsum + 4 * (t >> 6);
        w[0] = w_in;
        w[1] = w_n;
        w[2] = w_s1;
        w[3] = w_s2;
    }
    __syncthreads();
    if (t != 0) return;
    long long tot[4] = {0, 0, 0, 0};
    for (int w = 0; w < 4; ++w)
        for (int k = 0; k < 4; ++k) tot[k] += wsum[4 * w + k];
    quality::Record r;
    r.size = quality::shorter_side(d.view_w, d.view_h);
    r.inside = quality::inside_fraction((uint32_t)tot[0], ow, oh);
    r.sharpness = quality::variance((uint32_t)tot[1], tot[2], (uint64_t)tot[3]);
    r.frontal = quality::quiet_nan();
    if (P.pose) {
        const uint32_t *pose = P.pose + (int64_t)i * EXPORT_POSE_WORDS;
        if (pose[7] != 0) r.frontal = __builtin_bit_cast(float, pose[20]);  // valid; rot[8]
    }
    r.samples = (uint32_t)tot[1];
    quality::judge(r, tier_of(P.embed), tier_of(P.learn), known ? P.in[s0 + src].rejected : 0u);
    P.out[i] = r;
    const bool pass = (r.flags & quality::EMBED) != 0;
    if (!pass) P.due[i] = 0;
    if (P.measured_total) atomicAdd(P.measured_total, 1ull);
    if (P.rejected_total && !pass) atomicAdd(P.rejected_total, 1ull);
}

const char *launch_quality_measure(const QualityParams &p, hipStream_t s) {
    const size_t lds = 128 + (((size_t)p.ow * p.oh * sizeof(int16_t) + 15) & ~(size_t)15);
    hipLaunchKernelGGL(quality_measure_kernel, dim3(p.n), dim3(256), lds, s, p);
    return "quality_measure_kernel";
}

// grid: one lane per row, past one wavefront for n > 64; one atomic per wavefront that held a row back
__global__ __launch_bounds__(256) void quality_learn_mask_kernel(const QualityMaskParams P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool held = false;
    if (i < P.n) {
        const int k = P.due_of[i];
        const bool learn = (P.q[i].flags & quality::LEARN) != 0;
        P.due_of_learn[i] = k >= 0 && learn ? k : -1;
        held = k >= 0 && !learn;
    }
    const uint64_t m = __ballot(held);
    if (P.held_total && m != 0 && (threadIdx.x & 63) == 0) atomicAdd(P.held_total, (unsigned long long)__popcll(m));
}

const char *launch_quality_mask(const QualityMaskParams &p, hipStream_t s) {
    hipLaunchKernelGGL(quality_learn_mask_kernel, dim3((p.n + 255) / 256), dim3(256), 0, s, p);
    return "quality_learn_mask_kernel";
}

}  // namespace zr
