// detmerge.hip -- tiled detection's merge: a stream's per-tile detection lists (det_post's output,
// already in frame pixels) joined in tile order and put through NonMaxSuppression::process
// (detection/nms.rs:59-145) once more.  One wave per due stream; host/detection.cpp's restatement
// (TiledDetector::detect) is matched bit for bit, with det_post_kernel's scheme:
//   * the union takes tile t's first min(count, tile_cap) records, t = 0 .. T-1;
//   * the order is ascending total_cmp of the confidence, ties in union order (the host's stable
//     sort, = Rust's sort_unstable on <= 20 elements; `ties` reports the candidate and tied counts
//     as det_post does), seeds popped from the top;
//   * Average: confidence of the seed, every other field the confidence-weighted sum over
//     [seed] + group in retained order over the summed confidence; Remove: the seed as it is;
//   * a NaN IoU decides as the comparisons do (Remove drops the candidate, Average leaves it).
// Confidence, rect, order and group lists live in LDS; the 20-float records stay in global memory
// and are read during the averaging, where field f of the output belongs to lane f: each
// accumulator is summed by one lane in the sequential order.  No contraction, IEEE division.
#include "../runtime/zr_track.h"
#include "geom_dev.h"

namespace zr {
namespace {

using namespace geo;

__device__ __forceinline__ int32_t total_key(float f) {  // f32::total_cmp (zaru-image/src/num.rs:7-27)
    const int32_t i = (int32_t)glibc::asuint(f);
    return i ^ (int32_t)(((uint32_t)(i >> 31)) >> 1);
}

__global__ __launch_bounds__(64) void det_merge_kernel(const DetMergeParams P) {
    extern __shared__ float lds_dm[];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= min(max(*P.ndue, 0), P.S)) return;  // (whole wave)
    const int s = P.due[blockIdx.x];
    if (s < 0 || s >= P.S) return;
    const int T = P.T, cap = P.tile_cap, M = T * cap;
    int *src = (int *)lds_dm;             // candidate -> record of the stream's [T][cap] block  [M]
    float *cc = lds_dm + M;               // their confidences                                  [M]
    int *ord = (int *)(lds_dm + 2 * M);   // candidate ids in NMS order                          [M]
    float *cr = lds_dm + 3 * M;           // their rects (cx, cy, w, h)                          [4M]
    int *grp = (int *)(lds_dm + 7 * M);   // the current group                                   [M]
    const float *recs = P.tile_dets + (int64_t)s * M * 20;

    // 1. the union, in tile order
    int n = 0, dropped = 0;
    for (int t = 0; t < T; ++t) {
        const int raw = P.tile_count[(int64_t)s * T + t];
        const int c = min(max(raw, 0), cap);
        dropped += raw > cap ? raw - cap : 0;
        for (int j = lane; j < c; j += 64) {
            const int r = t * cap + j;
            const float *b = recs + (int64_t)r * 20;
            src[n + j] = r;
            cc[n + j] = b[0];
            cr[4 * (n + j)] = b[2];
            cr[4 * (n + j) + 1] = b[3];
            cr[4 * (n + j) + 2] = b[4];
            cr[4 * (n + j) + 3] = b[5];
        }
        n += c;
    }
    // 2. the ascending stable order: rank = #smaller keys + #equal keys before
    __shared__ int s_tied;
    if (lane == 0) s_tied = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const int32_t ki = total_key(cc[i]);
        int r = 0, eq = 0;
        for (int j = 0; j < n; ++j) {
            const int32_t kj = total_key(cc[j]);
            r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
            eq += (kj == ki && j != i) ? 1 : 0;
        }
        ord[r] = i;
        if (eq) atomicAdd(&s_tied, 1);
    }
    __syncthreads();

    // 3. NMS: pop the most confident, group everything within the IoU threshold (keeping order)
    const int nf = 6 + 2 * P.nkp;  // the record's fields in use
    int rem = n, out = 0;
    while (rem > 0) {
        const int seed = ord[--rem];
        const float sx = cr[4 * seed], sy = cr[4 * seed + 1], sw = cr[4 * seed + 2], sh = cr[4 * seed + 3];
        int ng = 0, nk = 0;
        for (int i0 = 0; i0 < rem; i0 += 64) {
            const int i = i0 + lane;
            int id = 0;
            bool in = false;
            if (i < rem) {
                id = ord[i];
                const float v = iou(sx, sy, sw, sh, cr[4 * id], cr[4 * id + 1], cr[4 * id + 2], cr[4 * id + 3]);
                // Remove retains a candidate only while iou < thresh (nms.rs:73); Average groups on >=
                in = P.mode == 1 ? !(v < P.iou) : v >= P.iou;
            }
            const uint64_t mg = __ballot(i < rem && in), mk = __ballot(i < rem && !in);
            const uint64_t below = (1ull << lane) - 1ull;
            __syncthreads();  // every lane has read ord[i0 .. i0 + 63] before the in-place compaction
            if (i < rem) {
                if (in) grp[ng + (int)__popcll(mg & below)] = id;
                else ord[nk + (int)__popcll(mk & below)] = id;  // retain: order kept, nk <= i
            }
            ng += (int)__popcll(mg);
            nk += (int)__popcll(mk);
            __syncthreads();
        }
        rem = nk;
        float v = 0.f;
        if (P.mode == 1) {
            // SuppressionMode::Remove (nms.rs:70-76): the group is dropped, the seed kept
            if (lane < nf) v = recs[(int64_t)src[seed] * 20 + lane];
        } else {
            // field `lane` over [seed] + group, summed in that order; lane 0 sums the divisor
            float acc = 0.f;
            if (lane < nf)
                for (int g = -1; g < ng; ++g) {
                    const int id = g < 0 ? seed : grp[g];
                    const float c = cc[id];
                    acc += lane == 0 ? c : recs[(int64_t)src[id] * 20 + lane] * c;
                }
            const float divisor = __shfl(acc, 0);
            if (lane < nf) v = lane == 0 ? cc[seed] : acc / divisor;
        }
        if (lane < 20 && out < P.dcap) P.dets[((int64_t)s * P.dcap + out) * 20 + lane] = v;
        ++out;
    }
    if (lane == 0) {
        P.count[s] = out;
        if (P.ties) {
            P.ties[2 * s] = n;
            P.ties[2 * s + 1] = s_tied;
        }
        if (P.tile_dropped) P.tile_dropped[s] = dropped;
    }
}

}  // namespace

size_t det_merge_lds(int tiles, int tile_cap) { return sizeof(float) * 8 * (size_t)tiles * (size_t)tile_cap; }

const char *launch_det_merge(const DetMergeParams &p, hipStream_t s) {
    hipLaunchKernelGGL(det_merge_kernel, dim3(p.S), dim3(64), det_merge_lds(p.T, p.tile_cap), s, p);
    return "det_merge_kernel";
}

}  // namespace zr
