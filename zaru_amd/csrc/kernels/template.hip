// template.hip -- identities that learn: two running means kept on the device, between the
// embedding network and the enrolment of a step (host/device_multi_tracker.cpp).
//   identity_blend_kernel    the object's template: the stored embedding select carried, moved
//                            towards this step's network output (zr_identity_blend_async, before the
//                            match; the match and the commit then read the blended rows)
//   identity_refine_kernel   the gallery row of every known object moved towards the object's raw
//                            sample (zr_identity_refine_async, after the commit, before the enrolment)
// One update of a vector m by a sample e with the divisor w is, per float and each operation rounded
// to f32 on its own (-ffp-contract=off, a correctly rounded divide),
//     m' = m + (e - m) / (float)w
// Both kernels are one wavefront per slot row, a float2 per lane for the 128 floats, so float f of
// a mean lives in one lane from its load to its one store.
//
// The refinement is sequential per gallery row: the contributors of row r update it in row order.
// A row i is a candidate when it was due, its state names a row r inside the gallery and its
// distance is within the threshold: all of that is its packed image and two words of its state, so
// every wavefront can tell every other's.  The first candidate of r (no candidate of r before it) is r's leader: it
// takes the row and its update count into registers, walks the candidates of r from itself on, 64
// rows to a ballot, applies each one whose 128 sample floats are finite, and stores row and count
// once.  Every other candidate returns.  So no two workgroups write one gallery row, no float is
// ever added atomically, and the chain's order never depends on scheduling.  A launch costs every
// candidate one pass over the states before it, and every leader one pass over those behind it.
#include "../runtime/zr_track.h"

namespace zr {
namespace {

constexpr int REFINE_AHEAD = 4;  // samples a leader loads ahead of its chain

__device__ __forceinline__ bool finite2(const float2 v) { return isfinite(v.x) && isfinite(v.y); }

// m + (e - m) / w, no contraction whatever the flags
__device__ __forceinline__ float toward(const float m, const float e, const float w) {
    return __fadd_rn(m, __fdiv_rn(__fsub_rn(e, m), w));
}

}  // namespace

// grid: one 64-lane workgroup per row; every branch is uniform over the wave
__global__ __launch_bounds__(64) void identity_blend_kernel(const IdentityBlendParams P) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int k = P.due_of[i];
    if (k < 0 || k >= P.n) return;
    const uint32_t c = P.out[i].embeddings;
    const float2 t = reinterpret_cast<const float2 *>(P.emb_out + (int64_t)i * IDENTITY_DIM)[lane];
    const float2 e = reinterpret_cast<const float2 *>(P.dense_emb + (int64_t)k * IDENTITY_DIM)[lane];
    float2 q = e;  // verbatim: a move keeps -0 and a NaN's payload
    if (c != 0 && __all(finite2(t) && finite2(e))) {
        const uint64_t w64 = (uint64_t)c + 1u;  // (c = 0xffffffff: no wrap)
        const float w = (float)(w64 < P.template_cap ? (uint32_t)w64 : P.template_cap);
        q.x = toward(t.x, e.x, w);
        q.y = toward(t.y, e.y, w);
    }
    reinterpret_cast<float2 *>(P.query + (int64_t)k * IDENTITY_DIM)[lane] = q;
}

const char *launch_identity_blend(const IdentityBlendParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_blend_kernel, dim3(p.n), dim3(64), 0, s, p);
    return "identity_blend_kernel";
}

// the gallery row row j contributes to, -1: none.  `rows` is min(count, capacity), clamped at 0
__device__ __forceinline__ int refine_target(const IdentityRefineParams &P, const int j, const int rows) {
    const int k = P.due_of[j];
    if (k < 0 || k >= P.n) return -1;
    const int r = P.out[j].row;
    if (r < 0 || r >= rows) return -1;
    return P.out[j].distance <= P.threshold ? r : -1;  // (a NaN on either side: no)
}

// grid: one 64-lane workgroup per row; every branch is uniform over the wave
__global__ __launch_bounds__(64) void identity_refine_kernel(const IdentityRefineParams P) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int rows = min(max(*P.count, 0), P.capacity);
    const int r = refine_target(P, i, rows);
    if (r < 0) return;
    for (int c0 = 0; c0 < i; c0 += 64) {  // an earlier candidate of r is, or follows, r's leader
        const int j = c0 + lane;
        if (__any(j < i && refine_target(P, j, rows) == r)) return;
    }
    float2 m = reinterpret_cast<const float2 *>(P.rows + (int64_t)r * IDENTITY_DIM)[lane];
    uint32_t u = P.updates[r];
    const uint32_t u0 = u;
    uint64_t applied = 0;
    for (int c0 = i & ~63; c0 < P.n; c0 += 64) {  // (n <= 2^24: no overflow)
        const int j = c0 + lane;
        const bool mine = j >= i && j < P.n && refine_target(P, j, rows) == r;
        const int kj = mine ? P.due_of[j] : 0;
        unsigned long long todo = __ballot(mine);
        while (todo) {
            // the next REFINE_AHEAD samples in flight before the chain takes them one by one: a link
            // then costs its arithmetic, not a trip to memory
            float2 e[REFINE_AHEAD];
            bool have[REFINE_AHEAD];
#pragma unroll
            for (int a = 0; a < REFINE_AHEAD; ++a) {
                have[a] = todo != 0;
                const int b = have[a] ? __builtin_ctzll(todo) : 0;
                todo &= todo - 1;  // (0 stays 0)
                // in [0, n): refine_target checked a contributor's; an idle lane's kj is 0, and row 0
                // is read and not used
                const int k = __shfl(kj, b);
                e[a] = reinterpret_cast<const float2 *>(P.dense_emb + (int64_t)k * IDENTITY_DIM)[lane];
            }
#pragma unroll
            for (int a = 0; a < REFINE_AHEAD; ++a) {
                if (!have[a] || !__all(finite2(e[a]))) continue;
                const uint64_t w64 = (uint64_t)u + 2u;  // (u = 0xffffffff: no wrap)
                const float w = (float)(w64 < P.max_samples ? (uint32_t)w64 : P.max_samples);
                m.x = toward(m.x, e[a].x, w);
                m.y = toward(m.y, e[a].y, w);
                u = u == 0xffffffffu ? u : u + 1u;
                ++applied;
            }
        }
    }
    if (!applied) return;  // every candidate's sample was not finite: the row keeps its bytes
    reinterpret_cast<float2 *>(P.rows + (int64_t)r * IDENTITY_DIM)[lane] = m;
    if (lane != 0) return;
    if (u != u0) P.updates[r] = u;
    if (P.refined_total) atomicAdd(reinterpret_cast<unsigned long long *>(P.refined_total), (unsigned long long)applied);
}

const char *launch_identity_refine(const IdentityRefineParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_refine_kernel, dim3(p.n), dim3(64), 0, s, p);
    return "identity_refine_kernel";
}

}  // namespace zr
