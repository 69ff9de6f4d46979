// match.hip -- embed_match_kernel: the reference's Embedding::difference
// (crates/zaru/examples/eval_face_recognition.rs:31-42) of Q query embeddings against a
// device-resident gallery of G embeddings of D floats, and each query's nearest gallery row.
//
// Arithmetic, bit for bit the Rust:  s = 0;  for k in 0..D { d = a[k] - b[k];  s = s + d * d }
// with the subtract, the multiply and the add each rounded on its own, k in order, then a
// correctly rounded sqrt.  That order rules out the Gram-matrix form (|a|^2 + |b|^2 - 2 a.b on
// the MFMA units), so this is a VALU kernel: a workgroup takes a 64 x 64 tile of pairs, stages 32
// dimensions of both sides in LDS transposed ([k][row], row stride 68 floats), and every thread
// walks k over a 4 x 4 block of pairs held in registers.  Per k a thread reads two 16-byte
// vectors: the 16 lanes that differ in tq read 64 consecutive floats, the lanes that differ only
// in tg read the same address (a broadcast), so the reads are conflict-free (tools/lds_banks.py).
//
// Nearest row: the key (distance bits << 32) | row orders like (distance, row) as an unsigned
// integer because a distance is never negative.  Threads fold their pairs into a per-query key in
// LDS with an unsigned 64-bit atomic min (a minimum does not depend on the order of its operands),
// and every workgroup stores its tile's keys to keys[gallery tile][query] with plain stores.  A
// NaN distance takes no part.  match_finish_kernel, a second pass, takes each query's minimum
// over the gallery tiles and unpacks it; a query that met no candidate (G = 0, masked out, or NaN
// everywhere) gets row -1 at +inf.  The keys are scratch in plain hipMalloc memory, kept per
// stream by the caller (runtime/session.cpp).
//
// Counted form (MatchParams::gcount, zr_embed_match_count_async): the gallery's size is read from
// the device, clamped to [0, G]; G is then the capacity the grid covers.  A tile at or past the
// count returns before it reads a row or writes a key, and the second pass folds only the tiles
// below the count, so the result is the plain form's at G = the count, bit for bit.
#include "../runtime/zr_kernels.h"

namespace zr {

constexpr int MT = 64;        // tile: MT queries x MT gallery rows
constexpr int MKC = 32;       // dimensions staged per pass
constexpr int MS = MT + 4;    // LDS row stride (floats): keeps 16-B alignment, spreads the staging writes
constexpr unsigned long long MATCH_NONE = ~0ull;

__global__ __launch_bounds__(256) void embed_match_kernel(const MatchParams P, int gtiles) {
    __shared__ __attribute__((aligned(16))) float qs[MKC][MS];
    __shared__ __attribute__((aligned(16))) float gs[MKC][MS];
    __shared__ unsigned long long best[MT];
    const int qt = blockIdx.x / gtiles, gt = blockIdx.x - qt * gtiles;
    const int q0 = qt * MT, g0 = gt * MT;
    const int G = P.gcount ? min(max(*P.gcount, 0), P.G) : P.G;
    if (g0 >= G) return;  // (counted form only: the plain grid has no such tile)
    const int tq = threadIdx.x & 15, tg = threadIdx.x >> 4;
    if (threadIdx.x < MT) best[threadIdx.x] = MATCH_NONE;
    float s[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[i][j] = 0.f;
    for (int k0 = 0; k0 < P.D; k0 += MKC) {
        __syncthreads();  // the previous pass is consumed (first pass: best[] is initialised)
        for (int i = threadIdx.x; i < MT * MKC; i += 256) {
            const int r = i / MKC, k = i - r * MKC;  // lanes along k: 128-B runs of a row
            const bool kin = k0 + k < P.D;
            qs[k][r] = (kin && q0 + r < P.Q) ? P.q[(int64_t)(q0 + r) * P.D + k0 + k] : 0.f;
            gs[k][r] = (kin && g0 + r < G) ? P.g[(int64_t)(g0 + r) * P.D + k0 + k] : 0.f;
        }
        __syncthreads();
        const int kn = min(MKC, P.D - k0);
#pragma unroll 4
        for (int k = 0; k < kn; ++k) {
            const float4 a4 = *reinterpret_cast<const float4 *>(&qs[k][4 * tq]);
            const float4 b4 = *reinterpret_cast<const float4 *>(&gs[k][4 * tg]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = __fsub_rn(a[i], b[j]);
                    s[i][j] = __fadd_rn(s[i][j], __fmul_rn(d, d));
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = q0 + 4 * tq + i;
        if (q >= P.Q) continue;
        const bool on = !P.valid || P.valid[q] != 0;
        unsigned long long key = MATCH_NONE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = g0 + 4 * tg + j;
            if (g >= G) continue;
            const float dist = sqrtf(s[i][j]);  // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt)
            if (P.dist) P.dist[(int64_t)q * G + g] = on ? dist : __builtin_inff();
            if (on && dist == dist) {
                const unsigned long long kk = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)g;
                key = kk < key ? kk : key;
            }
        }
        if (key != MATCH_NONE) atomicMin(&best[4 * tq + i], key);
    }
    __syncthreads();
    // keys is [gtiles][qtiles * MT]: every slot of this tile is written, padding queries included
    const int64_t qpad = (int64_t)(gridDim.x / gtiles) * MT;
    if (threadIdx.x < MT) P.keys[(int64_t)gt * qpad + q0 + threadIdx.x] = best[threadIdx.x];
}

__global__ __launch_bounds__(256) void match_finish_kernel(const MatchParams P, int gtiles, int64_t qpad) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P.Q) return;
    unsigned long long key = MATCH_NONE;
    if (P.gcount) gtiles = (min(max(*P.gcount, 0), P.G) + MT - 1) / MT;  // the tiles that took part
    for (int gt = 0; gt < gtiles; ++gt) {
        const unsigned long long k = P.keys[(int64_t)gt * qpad + q];
        key = k < key ? k : key;
    }
    P.best_idx[q] = key == MATCH_NONE ? -1 : (int)(unsigned)(key & 0xffffffffull);
    P.best_dist[q] = key == MATCH_NONE ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32));
}

size_t embed_match_scratch(int Q, int G) {
    const size_t qtiles = ((size_t)Q + MT - 1) / MT, gtiles = ((size_t)G + MT - 1) / MT;
    return qtiles * MT * gtiles * sizeof(unsigned long long);
}

// keys: embed_match_scratch(Q, G) bytes, contents irrelevant
const char *launch_embed_match(const MatchParams &p, hipStream_t s) {
    const int qtiles = (p.Q + MT - 1) / MT, gtiles = (p.G + MT - 1) / MT;
    if (p.G > 0) hipLaunchKernelGGL(embed_match_kernel, dim3((unsigned)(qtiles * gtiles)), dim3(256), 0, s, p, gtiles);
    hipLaunchKernelGGL(match_finish_kernel, dim3((p.Q + 255) / 256), dim3(256), 0, s, p, gtiles, (int64_t)qtiles * MT);
    return "embed_match_kernel";
}

}  // namespace zr
