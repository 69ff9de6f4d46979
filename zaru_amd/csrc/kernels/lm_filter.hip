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

// One primed value's step: the filtered value (also the new x of the state), `v` updated in place
// (alpha-beta v / 1 euro prev.dx; EMA leaves it).  Shared by both kernels, so they agree bit for bit.
__device__ __forceinline__ float filter_primed(const LmFilterParams &P, float x, float sx, float &v) {
    if (P.filter == 1) return P.p0 * x + (1.f - P.p0) * sx;  // ema.rs:41
    if (P.filter == 2) {  // alpha_beta.rs:52-58
        const float prediction = sx + v * P.elapsed;
        const float residual = x - prediction;
        v = v + P.p1 * residual / P.elapsed;
        return prediction + P.p0 * residual;
    }
    // one_euro.rs:74-85
    const float a_d = smoothing_factor(P.elapsed, P.p2);
    const float dx = (x - sx) / P.elapsed;
    const float dx_hat = exponential_smoothing(a_d, dx, v);
    const float cutoff = P.p0 + P.p1 * __builtin_fabsf(dx_hat);
    const float a = smoothing_factor(P.elapsed, cutoff);
    v = dx_hat;
    return exponential_smoothing(a, x, sx);
}

// the kind's extract of value v of image `img`, as track_kernel's `mapped` before the scale
__device__ __forceinline__ float extract_value(const LmFilterParams &P, int64_t img, int v) {
    if (P.kind == 3) {  // multipie68.rs:71-80: relative (x, y) * input resolution, z = 0
        const int j = v / 3, c = v - 3 * j;
        return c == 2 ? 0.f : P.lm[img * P.lm_stride + 2 * j + c] * (float)(c == 0 ? P.in_w : P.in_h);
    }
    if (P.kind == 2)  // eye.rs:47-64: 5 iris points (output 1), then the contour
        return v < 15 ? P.flag[img * P.flag_stride + v] : P.lm[img * P.lm_stride + (v - 15)];
    return P.lm[img * P.lm_stride + v];
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
    float x = extract_value(P, i, v);
    if (P.filter != 0) {
        uint32_t *primed = P.fstate + (int64_t)i * (P.filter == 1 ? 2 : 3) * nv + v;
        float *sx = reinterpret_cast<float *>(primed + nv);
        if (!*primed) {  // the first value passes through and primes the state (v / dx stay 0)
            *primed = 1u;
            *sx = x;
        } else if (P.filter == 1) {
            float unused = 0.f;
            *sx = x = filter_primed(P, x, *sx, unused);
        } else {
            float *sv = sx + nv;
            float vel = *sv;
            *sx = x = filter_primed(P, x, *sx, vel);
            *sv = vel;
        }
    }
    *out = x;
}

// The multi-object loop's form (DeviceMultiTracker): a filter state belongs to an object, and the
// bookkeeping (hand_manage_kernel) moves objects between the slots of their stream.  Row i's
// estimate is image index[i] (slot_compact's dense_of; null: image i), its incoming state is row
// src[i] of its stream in `fin` (hand_manage's src; outside [0, slots): a new object, the all-zero
// default state), and its new state goes to row i of `fout`: the gather is fused, the state is
// read and written once.  fin != fout, since a row is read by another workgroup than the one that
// writes it.  Every row of fout and pos is written: a row with nothing to filter (not active, or
// no estimate) gets the default state and NaN positions.  active, index[i] and src[i] are the
// same for the whole workgroup (scalar loads); the state rows stay coalesced.
__global__ __launch_bounds__(256) void lm_filter_indexed_kernel(const LmFilterParams P, int chunks, int slots,
                                                                const int32_t *__restrict__ index,
                                                                const int32_t *__restrict__ src,
                                                                const uint32_t *__restrict__ fin,
                                                                uint32_t *__restrict__ fout) {
    const int i = blockIdx.x / chunks;  // row: stream i / slots, slot i % slots
    const int nv = 3 * P.L;
    const int v = (blockIdx.x - i * chunks) * 256 + threadIdx.x;  // value 3j + c of the row
    if (v >= nv) return;
    const int arrays = P.filter == 0 ? 0 : P.filter == 1 ? 2 : 3;
    float *out = P.pos + (int64_t)i * nv + v;
    // the row's three table entries, asked for together: one scalar-load latency instead of three in
    // a chain.  Both tables hold n entries; an idle slot's are loaded and not looked at.
    const uint32_t active = P.state[i].active;
    const int at = index ? index[i] : i;
    const int from = P.filter != 0 ? src[i] : -1;
    const int64_t img = active ? at : -1;
    if (img < 0 || img >= P.n) {
        *out = __builtin_nanf("");
        for (int a = 0; a < arrays; ++a) fout[((int64_t)i * arrays + a) * nv + v] = 0u;
        return;
    }
    float x = extract_value(P, img, v);
    if (P.filter != 0) {
        uint32_t primed = 0u;
        float sx = 0.f, sv = 0.f;
        if (from >= 0 && from < slots) {
            const uint32_t *si = fin + ((int64_t)(i / slots) * slots + from) * arrays * nv + v;
            primed = si[0];
            sx = __uint_as_float(si[nv]);
            if (arrays == 3) sv = __uint_as_float(si[2 * (int64_t)nv]);
        }
        if (!primed) {  // the first value passes through and primes the state (v / dx stay 0)
            sx = x;
            sv = 0.f;
        } else {
            sx = x = filter_primed(P, x, sx, sv);
        }
        uint32_t *so = fout + (int64_t)i * arrays * nv + v;  // primed, then x, then v
        so[0] = 1u;
        so[nv] = __float_as_uint(sx);
        if (arrays == 3) so[2 * (int64_t)nv] = __float_as_uint(sv);
    }
    *out = x;
}

}  // namespace

const char *launch_lm_filter_indexed(const LmFilterIndexedParams &p, hipStream_t s) {
    const int chunks = (3 * p.base.L + 255) / 256;
    hipLaunchKernelGGL(lm_filter_indexed_kernel, dim3((unsigned)(p.base.n * chunks)), dim3(256), 0, s, p.base, chunks,
                       p.slots, p.index, p.src, p.fstate_in, p.base.fstate);
    return "lm_filter_indexed_kernel";
}

const char *launch_lm_filter(const LmFilterParams &p, hipStream_t s) {
    const int chunks = (3 * p.L + 255) / 256;
    hipLaunchKernelGGL(lm_filter_kernel, dim3((unsigned)(p.n * chunks)), dim3(256), 0, s, p, chunks);
    return "lm_filter_kernel";
}

}  // namespace zr
