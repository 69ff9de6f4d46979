// enrol.hip -- identity_enrol_kernel: the unknown objects of a step become gallery rows, on the
// device (zr_identity_enrol_async, after identity_commit_kernel in host/device_multi_tracker.cpp).
//
// The rule is sequential: whether candidate c is appended depends on what every earlier candidate
// of the step did (two unknown objects of one step may be the same person).  So one workgroup of
// 256 threads walks the rows in row order, 256 rows at a time:
//   scan     every thread looks at one row: a due row that is known gets EVER_KNOWN; a row that is
//            due, unknown, never known, embedded often enough and finite is a candidate.  The
//            candidates of the chunk are four ballots in LDS.
//   decide   the workgroup takes the ballots' bits in order.  The candidate's embedding goes to LDS;
//            every thread takes the rows this call has appended so far, 256 apart, and computes
//            match.hip's distance to each (subtract, multiply and add rounded on their own, k in
//            order, a correctly rounded sqrt); the nearest is an unsigned 64-bit minimum over
//            (distance bits << 32) | row in LDS, which does not depend on the order of its
//            operands.  At or below the threshold the candidate is that row; otherwise its 128
//            floats are appended by 128 threads, or, with the gallery full, it is counted as dropped.
// Every branch of the walk is uniform over the workgroup: the ballots and the minimum are read from
// LDS after a barrier, and count / next id / the counters are kept by every thread alike and stored
// once, by thread 0, at the end.  A step without a candidate costs the scan alone.
// Rows appended by earlier candidates are read back through global memory by other threads of this
// workgroup: the barrier between append and read orders them at workgroup scope.
#include "../runtime/zr_track.h"

namespace zr {

constexpr int ET = 256;  // the workgroup's width
constexpr unsigned long long ENROL_NONE = ~0ull;

__global__ __launch_bounds__(ET) void identity_enrol_kernel(const IdentityEnrolParams P) {
    __shared__ __attribute__((aligned(16))) float emb[IDENTITY_DIM];
    __shared__ unsigned long long cand[ET / 64];
    __shared__ unsigned long long best;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int count0 = min(max(*P.count, 0), P.capacity);
    int count = count0;
    uint64_t next_id = *P.next_id, appended = 0, dropped = 0;
    for (int c0 = 0; c0 < P.n; c0 += ET) {  // (n <= 2^24: no overflow)
        const int i = c0 + t;
        bool is_cand = false;
        if (i < P.n && P.due_of[i] >= 0) {
            const IdentityState st = P.out[i];
            if (st.row >= 0) {
                if (!(st.flags & IDENTITY_EVER_KNOWN)) P.out[i].flags = st.flags | IDENTITY_EVER_KNOWN;
            } else if (st.row == -1 && !(st.flags & IDENTITY_EVER_KNOWN) && st.embeddings >= P.min_embeddings) {
                const float2 *e = reinterpret_cast<const float2 *>(P.emb_out + (int64_t)i * IDENTITY_DIM);
                bool finite = true;
                for (int k = 0; k < IDENTITY_DIM / 2; ++k) {
                    const float2 v = e[k];
                    finite = finite && isfinite(v.x) && isfinite(v.y);
                }
                is_cand = finite;
            }
        }
        const unsigned long long m = __ballot(is_cand);
        if (lane == 0) cand[w] = m;
        __syncthreads();
        for (int cw = 0; cw < ET / 64; ++cw) {
            unsigned long long todo = cand[cw];
            while (todo) {
                const int r = c0 + 64 * cw + __builtin_ctzll(todo);  // < n: only rows below n are candidates
                todo &= todo - 1;
                if (t < IDENTITY_DIM) emb[t] = P.emb_out[(int64_t)r * IDENTITY_DIM + t];
                if (t == 0) best = ENROL_NONE;
                __syncthreads();
                unsigned long long key = ENROL_NONE;
                for (int g = count0 + t; g < count; g += ET) {  // count <= capacity: inside the gallery
                    const float4 *row = reinterpret_cast<const float4 *>(P.rows + (int64_t)g * IDENTITY_DIM);
                    float4 r4[IDENTITY_DIM / 4];  // the whole row in flight before the sum, which is one chain
#pragma unroll
                    for (int k4 = 0; k4 < IDENTITY_DIM / 4; ++k4) r4[k4] = row[k4];
                    float s = 0.f;
#pragma unroll
                    for (int k4 = 0; k4 < IDENTITY_DIM / 4; ++k4) {
                        const float b[4] = {r4[k4].x, r4[k4].y, r4[k4].z, r4[k4].w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float d = __fsub_rn(emb[4 * k4 + j], b[j]);
                            s = __fadd_rn(s, __fmul_rn(d, d));
                        }
                    }
                    const float dist = sqrtf(s);  // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt)
                    if (dist == dist) {
                        const unsigned long long kk = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)g;
                        key = kk < key ? kk : key;
                    }
                }
                if (key != ENROL_NONE) atomicMin(&best, key);
                __syncthreads();
                const unsigned long long b = best;
                const float dist = __uint_as_float((unsigned)(b >> 32));
                if (b != ENROL_NONE && dist <= P.threshold) {  // (a NaN threshold: never)
                    if (t == 0) {
                        IdentityState st = P.out[r];
                        st.row = (int)(unsigned)(b & 0xffffffffull);
                        st.distance = dist;
                        st.flags |= IDENTITY_EVER_KNOWN;
                        P.out[r] = st;
                    }
                } else if (count < P.capacity) {
                    if (t < IDENTITY_DIM) P.rows[(int64_t)count * IDENTITY_DIM + t] = emb[t];
                    if (t == 0) {
                        P.ids[count] = next_id;
                        IdentityState st = P.out[r];
                        st.row = count;
                        st.distance = 0.f;
                        st.flags |= IDENTITY_EVER_KNOWN | IDENTITY_ENROLLED;
                        P.out[r] = st;
                    }
                    ++count;
                    ++next_id;
                    ++appended;
                } else {
                    ++dropped;
                }
                __syncthreads();  // emb and best are rewritten; the appended row is read by the next candidate
            }
        }
        __syncthreads();  // cand is rewritten by the next chunk
    }
    if (t == 0 && (appended | dropped)) {
        *P.count = count;
        *P.next_id = next_id;
        *P.enrolled_total += appended;
        *P.dropped += dropped;
    }
}

const char *launch_identity_enrol(const IdentityEnrolParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_enrol_kernel, dim3(1), dim3(ET), 0, s, p);
    return "identity_enrol_kernel";
}

}  // namespace zr
