// lm_filter.hip -- Estimator's LandmarkFilter (crates/zaru/src/landmark.rs:142-202,330-333) on the
// device: each stream's extract, then one temporal filter per landmark and coordinate
// (crates/zaru/src/filter: ema.rs, alpha_beta.rs, one_euro.rs), so a filtered video loop keeps
// its state in HBM like the tracker's.  The result is the positions in network pixels that
// track_kernel's map-out then reads (TrackParams::pos).
//
// One thread per value (stream, landmark, coordinate); no reductions, nothing shared between
// lanes.  The filter state of a stream is a structure of arrays over its 3L values -- primed[],
// then x[] (EMA last / alpha-beta x / 1 euro prev.x), then v[] (alpha-beta v / 1 euro prev.dx) --
// so consecutive lanes touch consecutive words of every array and of `pos`.  Priming is per
// value: no lane reads a word another lane writes.  Zero words are the default state.
// f32 in the reference's operation order; the build forbids contraction and rounds division
// correctly, so every value equals the host restatement (host/filter.cpp) bit for bit.
#include "../runtime/zr_track.h"

namespace zr {
namespace {

// one_euro.rs:91-98
__device__ __forceinline__ float smoothing_factor(float t_e, float cutoff) {
    const float r = 6.2831855f * cutoff * t_e;  // 2.0 * PI * cutoff * t_e, left to right
    return r / (r + 1.f);
}
__device__ __forceinline__ float exponential_smoothing(float a, float x, float x_prev) {
    return a * x + (1.f - a) * x_prev;
}

__global__ __launch_bounds__(256) void lm_filter_kernel(const LmFilterParams P, int chunks) {
    const int i = blockIdx.x / chunks;  // stream
    const int nv = 3 * P.L;
    const int v = (blockIdx.x - i * chunks) * 256 + threadIdx.x;  // value 3j + c of the stream
    if (v >= nv) return;
    float *out = P.pos + (int64_t)i * nv + v;
    if (P.state && !P.state[i].active) {  // no estimate ran for it: state untouched, lm_out's NaN
        *out = __builtin_nanf("");
        return;
    }
    // the kind's extract, as track_kernel's `mapped` before the scale
    float x;
    if (P.kind == 3) {  // multipie68.rs:71-80: relative (x, y) * input resolution, z = 0
        const int j = v / 3, c = v - 3 * j;
        x = c == 2 ? 0.f : P.lm[(int64_t)i * P.lm_stride + 2 * j + c] * (float)(c == 0 ? P.in_w : P.in_h);
    } else if (P.kind == 2) {  // eye.rs:47-64: 5 iris points (output 1), then the contour
        x = v < 15 ? P.flag[(int64_t)i * P.flag_stride + v] : P.lm[(int64_t)i * P.lm_stride + (v - 15)];
    } else {
        x = P.lm[(int64_t)i * P.lm_stride + v];
    }
    if (P.filter != 0) {
        uint32_t *primed = P.fstate + (int64_t)i * (P.filter == 1 ? 2 : 3) * nv + v;
        float *sx = reinterpret_cast<float *>(primed + nv);
        if (!*primed) {  // the first value passes through and primes the state (v / dx stay 0)
            *primed = 1u;
            *sx = x;
        } else if (P.filter == 1) {  // ema.rs:41
            x = P.p0 * x + (1.f - P.p0) * *sx;
            *sx = x;
        } else if (P.filter == 2) {  // alpha_beta.rs:52-58
            float *sv = sx + nv;
            const float vel = *sv;
            const float prediction = *sx + vel * P.elapsed;
            const float residual = x - prediction;
            x = prediction + P.p0 * residual;
            *sx = x;
            *sv = vel + P.p1 * residual / P.elapsed;
        } else {  // one_euro.rs:74-85
            float *sv = sx + nv;
            const float px = *sx;
            const float a_d = smoothing_factor(P.elapsed, P.p2);
            const float dx = (x - px) / P.elapsed;
            const float dx_hat = exponential_smoothing(a_d, dx, *sv);
            const float cutoff = P.p0 + P.p1 * __builtin_fabsf(dx_hat);
            const float a = smoothing_factor(P.elapsed, cutoff);
            x = exponential_smoothing(a, x, px);
            *sx = x;
            *sv = dx_hat;
        }
    }
    *out = x;
}

}  // namespace

const char *launch_lm_filter(const LmFilterParams &p, hipStream_t s) {
    const int chunks = (3 * p.L + 255) / 256;
    hipLaunchKernelGGL(lm_filter_kernel, dim3((unsigned)(p.n * chunks)), dim3(256), 0, s, p, chunks);
    return "lm_filter_kernel";
}

}  // namespace zr
