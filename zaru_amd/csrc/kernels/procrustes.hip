// procrustes.hip -- ProcrustesAnalyzer::analyze (crates/zaru/src/procrustes.rs:88-136) over a
// batch of point sets on the device: the head pose of every face mesh of a video loop against
// the canonical mesh, without copying n x 468 x 3 floats to the host each frame.
//
// One wavefront (one 64-thread workgroup) per set.  The set's first n_ref points and the
// normalised reference are loaded coalesced into LDS (flip_y applied there).  The arithmetic is
// procrustes_math.h, whose sums have a defined order, so they run as sequential chains over LDS
// on a few lanes while every lane does the per-point work:
//   lanes 0-2   the three centroid chains                 all lanes   p -= centroid, |p|^2 -> d[]
//   lane 0      the scale chain over d[]                  all lanes   p /= scale
//   lanes 0-8   the nine covariance chains                lane 0      the 3x3 work, the record
// The chains fetch their terms in batches of 16 (chain_sum), so a chain pays the add latency per
// term and the LDS latency per batch; every workgroup of a 1,024-set batch is resident at once.
// Every value equals the host mirror (host/procrustes.cpp) bit for bit.
//
// LDS: (7 n_ref + 16) floats: p[3 n] | q[3 n] | d[n] | centroid[3], scale, M[9].  Stride-3 word
// accesses across the lanes are conflict-free (3 is coprime to the bank count).
#include "../runtime/zr_track.h"
#include "procrustes_math.h"

namespace zr {
namespace {

// A sum in index order from 0 over n terms read from LDS, term(k) the k-th: the terms of a batch
// are fetched together, so their LDS reads are in flight at once instead of one read latency per
// term, then added one by one in order -- the same additions as the plain loop.
template <typename Term>
__device__ __forceinline__ float chain_sum(int n, Term term) {
    constexpr int U = 16;
    float acc = 0.f;
    int k = 0;
    for (; k + U <= n; k += U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = term(k + u);
#pragma unroll
        for (int u = 0; u < U; u++) acc += v[u];
    }
    for (; k < n; k++) acc += term(k);
    return acc;
}

__global__ __launch_bounds__(64) void procrustes_kernel(const ProcrustesParams P) {
    extern __shared__ float lds[];
    const int set = blockIdx.x, lane = threadIdx.x;
    const int n = P.n_ref, nv = 3 * n;
    procrustes::Pose *out = P.out + set;
    // uniform over the workgroup: no barrier is skipped by part of it
    const bool valid = P.valid ? P.valid[set] != 0 : P.state ? P.state[set].tracked != 0 : true;
    if (!valid) {
        if (lane == 0) {
            procrustes::Pose r;
            procrustes::invalid(&r);
            *out = r;
        }
        return;
    }
    float *p = lds, *q = lds + nv, *d = q + nv, *sh = d + n;
    const float *src = P.points + (int64_t)set * P.stride;
    for (int i = lane; i < nv; i += 64) {
        const float x = src[i];
        p[i] = (P.flip_y && i % 3 == 1) ? -x : x;
        q[i] = P.q[i];
    }
    __syncthreads();
    const float fn = (float)n;
    if (lane < 3) {  // remove_translation: running sums in index order
        sh[lane] = chain_sum(n, [&](int k) { return p[3 * k + lane]; }) / fn;
    }
    __syncthreads();
    for (int k = lane; k < n; k += 64) {
        const float x = p[3 * k] - sh[0], y = p[3 * k + 1] - sh[1], z = p[3 * k + 2] - sh[2];
        p[3 * k] = x;
        p[3 * k + 1] = y;
        p[3 * k + 2] = z;
        d[k] = procrustes::sq_len(x, y, z);
    }
    __syncthreads();
    if (lane == 0) {  // remove_scale
        const float s = chain_sum(n, [&](int k) { return d[k]; }) / fn;
        sh[3] = __builtin_sqrtf(s);
    }
    __syncthreads();
    const float s = sh[3];
    for (int i = lane; i < nv; i += 64) p[i] /= s;
    __syncthreads();
    if (lane < 9) {  // M[r][c] = sum_k p[k][r] * q[k][c]
        const int r = lane / 3, c = lane - 3 * r;
        sh[4 + lane] = chain_sum(n, [&](int k) { return p[3 * k + r] * q[3 * k + c]; });
    }
    __syncthreads();
    if (lane == 0) {
        const float centroid[3] = {sh[0], sh[1], sh[2]}, ref_centroid[3] = {P.ref_cx, P.ref_cy, P.ref_cz};
        float M[9];
        for (int e = 0; e < 9; e++) M[e] = sh[4 + e];
        procrustes::Pose r;
        procrustes::finish(centroid, s, M, ref_centroid, P.ref_scale, &r);
        *out = r;
    }
}

}  // namespace

size_t procrustes_lds(int n_ref) { return ((size_t)7 * n_ref + 16) * sizeof(float); }

const char *launch_procrustes(const ProcrustesParams &p, hipStream_t s) {
    hipLaunchKernelGGL(procrustes_kernel, dim3((unsigned)p.n_sets), dim3(64), procrustes_lds(p.n_ref), s, p);
    return "procrustes_kernel";
}

}  // namespace zr
