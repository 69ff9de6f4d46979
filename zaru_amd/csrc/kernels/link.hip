// link.hip -- duplicate gallery rows joined from track evidence, on the device
// (zr_identity_link_async, last in the identity leg: host/multi_stages.cpp).  One continuously
// tracked object is one person: when its nearest row was p at its previous look and is b now, p and
// b are one person, unless another object of the same frame holds either identity.  Rows are never
// moved: every row has a GalleryLink whose alias is the canonical row of its person.
//
// identity_link_walk_kernel   pass 1.  The rule is sequential: whether a pair is still two people
//          depends on the merges earlier rows made.  So, as in enrol.hip, one workgroup of 256 threads
//          walks the rows in row order, 256 at a time:
//   scan     every thread tests one row for eligibility and evidence: p, b inside the gallery, both
//            distances within the threshold, and two aliases that differ now.  Merges only ever make
//            aliases equal, so a row that is no evidence here is none later in the call; the common
//            object, whose nearest row did not change, never reaches the serial part.  The chunk's
//            evidence rows are four ballots in LDS.
//   decide   the workgroup takes the ballots' bits in order.  Every thread reads the row's p and b
//            and their aliases as they are now; every wavefront takes the veto's ballot over the
//            stream's at most 64 slots for itself (the same loads, the same answer, no exchange);
//            then a barrier, since the record read here is written next.  A merge's relabel is
//            spread over all threads, the gallery's rows 256 apart; a barrier ends the evidence row.
// Every branch of the walk is uniform over the workgroup; the counters are kept by every thread
// alike and stored once, by thread 0.  The veto reads the states from global memory, so a stream
// whose slots straddle two chunks is no special case.  Records written by earlier evidence rows are
// read back through global memory by other threads of this workgroup: the barrier orders them at
// workgroup scope.
// identity_link_canon_kernel  pass 2, a launch of its own behind pass 1 on the stream: one thread per
//          row, d_out[i].row becomes its alias; only rows that change are written.
#include "../runtime/zr_track.h"

namespace zr {

constexpr int LT = 256;  // the workgroup's width

// the canonical row of r (0 <= r < G); a stored alias outside [0, r] reads as r, so the result is in [0, r]
__device__ __forceinline__ int link_alias(const GalleryLink *links, int r) {
    const int a = links[r].alias;
    return a < 0 || a > r ? r : a;
}

__global__ __launch_bounds__(LT) void identity_link_walk_kernel(const IdentityLinkParams P) {
    __shared__ unsigned long long evid[LT / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int G = min(max(*P.count, 0), P.capacity);
    uint64_t merged = 0, vetoed = 0, observed = 0;
    for (int c0 = 0; c0 < P.n; c0 += LT) {  // (n <= 2^24: no overflow)
        const int i = c0 + t;
        bool ev = false;
        if (i < P.n) {
            const int d = P.due_of[i], sr = P.src[i];
            if (d >= 0 && d < P.n && P.state[i].tracked != 0 && sr >= 0 && sr < P.K) {
                const IdentityState was = P.in[i / P.K * P.K + sr], now = P.out[i];
                ev = was.row >= 0 && was.row < G && now.row >= 0 && now.row < G && was.distance <= P.threshold &&
                     now.distance <= P.threshold &&  // (a NaN threshold: never)
                     link_alias(P.links, was.row) != link_alias(P.links, now.row);
            }
        }
        const unsigned long long m = __ballot(ev);
        if (lane == 0) evid[w] = m;
        __syncthreads();
        for (int cw = 0; cw < LT / 64; ++cw) {
            unsigned long long todo = evid[cw];
            while (todo) {
                const int r = c0 + 64 * cw + __builtin_ctzll(todo);  // < n, eligible: src[r] in [0, K)
                todo &= todo - 1;
                const int base = r / P.K * P.K;
                const int ap = link_alias(P.links, P.in[base + P.src[r]].row);  // both rows are in [0, G)
                const int ab = link_alias(P.links, P.out[r].row);
                const int lo = min(ap, ab), hi = max(ap, ab);
                const GalleryLink rec = P.links[hi];
                bool other = false;
                if (lane < P.K && base + lane != r && P.state[base + lane].tracked != 0) {
                    const int orow = P.out[base + lane].row;
                    if (orow >= 0 && orow < G) {
                        const int ao = link_alias(P.links, orow);
                        other = ao == lo || ao == hi;
                    }
                }
                const bool veto = __ballot(other) != 0;
                __syncthreads();  // every read of the table above comes before the writes below
                if (ap != ab) {
                    if (veto) {
                        if (t == 0) P.links[hi] = GalleryLink{hi, -1, 0u, 0u};
                        ++vetoed;
                    } else {
                        ++observed;
                        const uint32_t seen = rec.partner == lo ? rec.seen + 1u : 1u;
                        if (seen >= P.min_observations) {
                            // (hi itself is among them; thread 0's fields below are other dwords)
                            for (int g = t; g < G; g += LT)
                                if (link_alias(P.links, g) == hi) P.links[g].alias = lo;
                            if (t == 0) {
                                P.links[hi].partner = -1;
                                P.links[hi].seen = 0u;
                            }
                            ++merged;
                        } else if (t == 0) {
                            P.links[hi].partner = lo;
                            P.links[hi].seen = seen;
                        }
                    }
                }
                __syncthreads();  // the next evidence row reads the table as this one left it
            }
        }
        __syncthreads();  // evid is rewritten by the next chunk, whose scan reads the table as this one left it
    }
    if (t == 0 && P.counts && (merged | vetoed | observed)) {
        P.counts[0] += merged;
        P.counts[1] += vetoed;
        P.counts[2] += observed;
    }
}

__global__ __launch_bounds__(LT) void identity_link_canon_kernel(const IdentityLinkParams P) {
    const int i = blockIdx.x * LT + threadIdx.x;
    if (i >= P.n) return;
    const int G = min(max(*P.count, 0), P.capacity);
    const int r = P.out[i].row;
    if (r < 0 || r >= G) return;
    const int a = link_alias(P.links, r);
    if (a != r) P.out[i].row = a;
}

const char *launch_identity_link_walk(const IdentityLinkParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_link_walk_kernel, dim3(1), dim3(LT), 0, s, p);
    return "identity_link_walk_kernel";
}

const char *launch_identity_link_canon(const IdentityLinkParams &p, hipStream_t s) {
    hipLaunchKernelGGL(identity_link_canon_kernel, dim3((p.n + LT - 1) / LT), dim3(LT), 0, s, p);
    return "identity_link_canon_kernel";
}

}  // namespace zr
