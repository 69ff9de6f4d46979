// export.hip -- every stream's tracked objects as one packed batch (host/device_multi_tracker.cpp:
// snapshot / objects_packed).  DeviceMultiTracker::objects(s) restated on the device for all
// streams at once: slot j < clamp(nobjects[s], 0, K) of stream s is exported iff r = src[s K + j]
// lies in [0, K) (an object the last bookkeeping started has no result yet); id, roi and
// confidence are slot j's, landmarks, pose, identity and eyes slot r's -- the bookkeeping moved the
// objects, not their results.
//   export_scan_kernel   one workgroup: the streams' exported objects counted and scanned per
//                        1024-stream chunk (slot_compact_kernel's scan), so record k is the k-th
//                        exported object in stream-then-slot order whatever the scheduling; writes
//                        count, stream offsets and the records' headers
//   export_copy_kernel   one workgroup per record: finds its source through the header the scan
//                        wrote and copies the payload, every lane on consecutive dwords
// Two launches, not one: the scan has to be one workgroup to fix the order, and the payload
// (about 8 KB a record with a face mesh, pose, identity and eyes) wants the whole device.  Fused,
// every copying workgroup would either scan all the counts again or wait for the scanning one
// inside the launch; the second launch on the same stream costs a few microseconds and needs
// neither.  Plain vector stores only; nothing is placed with atomics.
#include "../runtime/zr_track.h"

namespace zr {

namespace {
__device__ __forceinline__ bool exported(int r, int K) { return r >= 0 && r < K; }
}  // namespace

// each thread owns a stream of the chunk: counts its exported slots, takes its place from the
// block-wide exclusive scan, then walks its slots again and writes their headers
__global__ __launch_bounds__(1024) void export_scan_kernel(const ExportParams P) {
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int base = 0;
    for (int64_t c0 = 0; c0 < P.S; c0 += 1024) {  // (64-bit: S may be within 1024 of 2^31)
        const int64_t s = c0 + t;
        const int no = s < P.S ? min(max(P.nobjects[s], 0), P.K) : 0;
        const int64_t slot0 = s * P.K;
        int c = 0;
        for (int j = 0; j < no; ++j) c += exported(P.src[slot0 + j], P.K) ? 1 : 0;
        int inc = c;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < 16; ++i) {
            before += i < w ? wsum[i] : 0;
            total += wsum[i];
        }
        if (s < P.S) {
            int k = base + before + (inc - c);
            P.offsets[s] = k;
            for (int j = 0; j < no; ++j) {
                const int r = P.src[slot0 + j];
                if (!exported(r, P.K)) continue;
                const int64_t from = slot0 + r;
                uint32_t flags = (P.pose ? EXPORT_POSE : 0) | (P.quality ? EXPORT_QUALITY : 0);
                if (P.ist && P.ist[from].embeddings != 0) flags |= EXPORT_IDENTITY;
                if (P.eye_valid) {
                    if (P.eye_valid[2 * from] != 0) flags |= EXPORT_EYE_LEFT;
                    if (P.eye_valid[2 * from + 1] != 0) flags |= EXPORT_EYE_RIGHT;
                }
                ExportHeader h;
                h.id = P.ids[slot0 + j];
                h.stream = (int32_t)s;
                h.slot = j;
                for (int i = 0; i < 5; ++i) h.roi[i] = P.roi[(slot0 + j) * 5 + i];
                h.confidence = P.state[slot0 + j].confidence;
                h.flags = flags;
                h.reserved = 0;
                P.header[k++] = h;
            }
        }
        base += total;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    if (t == 0) {
        P.offsets[P.S] = base;
        *P.count = base;
    }
}

namespace {
// n dwords from src to dst (src == nullptr: zeros), the workgroup's lanes on consecutive dwords,
// or on consecutive 16-byte quads when the caller knows both rows are 16-byte aligned and n % 4 == 0
template <bool V4>
__device__ __forceinline__ void copy_words(uint32_t *dst, const uint32_t *src, int n) {
    const int t = threadIdx.x, T = blockDim.x;
    if (V4) {
        uint4 *d = reinterpret_cast<uint4 *>(dst);
        const uint4 *q = reinterpret_cast<const uint4 *>(src);
        for (int i = t; i < n / 4; i += T) d[i] = src ? q[i] : make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (int i = t; i < n; i += T) dst[i] = src ? src[i] : 0u;
    }
}
}  // namespace

// grid: workgroups stride over the records; one whose record is at or past *count returns at once,
// so nothing past the count is written
template <bool V4>
__global__ __launch_bounds__(256) void export_copy_kernel(const ExportParams P) {
    const int64_t rows = (int64_t)P.S * P.K;
    const int64_t count = min((int64_t)max(*P.count, 0), rows);
    for (int64_t k = blockIdx.x; k < count; k += gridDim.x) {
        const ExportHeader h = P.header[k];
        const int64_t slot0 = (int64_t)h.stream * P.K;
        if (h.stream < 0 || h.stream >= P.S || h.slot < 0 || h.slot >= P.K) continue;  // (the scan's own values)
        const int r = P.src[slot0 + h.slot];
        if (!exported(r, P.K)) continue;
        const int64_t from = slot0 + r;
        const int W = 3 * P.L;
        copy_words<V4>(P.out_lm + k * W, P.lm + from * W, W);
        if (P.pose) copy_words<false>(P.out_pose + k * EXPORT_POSE_WORDS, P.pose + from * EXPORT_POSE_WORDS, EXPORT_POSE_WORDS);
        if (P.ist) {
            const bool present = (h.flags & EXPORT_IDENTITY) != 0;
            if (threadIdx.x == 0) {
                ExportIdentity o = {0, 0.f, 0u, 0u};
                if (present) {
                    const IdentityState is = P.ist[from];
                    o.row = is.row;
                    o.distance = is.distance;
                    o.embeddings = is.embeddings;
                    o.flags = is.flags;
                }
                P.out_ist[k] = o;
            }
            copy_words<V4>(P.out_emb + k * IDENTITY_DIM, present ? P.emb + from * IDENTITY_DIM : nullptr, IDENTITY_DIM);
        }
        if (P.quality)
            copy_words<false>(P.out_quality + k * EXPORT_QUALITY_WORDS, P.quality + from * EXPORT_QUALITY_WORDS,
                              EXPORT_QUALITY_WORDS);
        if (P.eye_valid) {
            for (int side = 0; side < 2; ++side) {
                const bool present = (h.flags & (side ? EXPORT_EYE_RIGHT : EXPORT_EYE_LEFT)) != 0;
                const int64_t e = 2 * from + side, o = 2 * k + side;
                if (threadIdx.x == 0) {
                    P.out_eye_valid[o] = present ? 1 : 0;
                    P.out_eye_diam[o] = present ? P.eye_diam[e] : 0u;
                }
                copy_words<false>(P.out_eye_crop + o * 5, present ? P.eye_crop + e * 5 : nullptr, 5);
                copy_words<V4>(P.out_eye_lm + o * EXPORT_EYE_WORDS, present ? P.eye_lm + e * EXPORT_EYE_WORDS : nullptr,
                               EXPORT_EYE_WORDS);
            }
        }
    }
}

const char *launch_export(const ExportParams &p, hipStream_t s) {
    hipLaunchKernelGGL(export_scan_kernel, dim3(1), dim3(1024), 0, s, p);
    // a record of a small landmark set (a hand: 63 dwords) is one wavefront's work
    const int64_t rows = (int64_t)p.S * p.K;
    const unsigned grid = (unsigned)(rows < (1 << 20) ? rows : (1 << 20));
    const unsigned block = 3 * (int64_t)p.L > 256 ? 256 : 64;
    if (p.vec4)
        hipLaunchKernelGGL(export_copy_kernel<true>, dim3(grid), dim3(block), 0, s, p);
    else
        hipLaunchKernelGGL(export_copy_kernel<false>, dim3(grid), dim3(block), 0, s, p);
    return "export_copy_kernel";
}

}  // namespace zr
