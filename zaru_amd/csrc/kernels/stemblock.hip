// stemblock.hip -- the face networks' stem conv and their first BlazeBlock in one launch (form
// "stemblock"): the dense KxK stride-2 stem (Cin = 3, + bias, activation) of an output tile plus
// the block's one-pixel depthwise halo is computed into LDS, and the 3x3 stride-1 depthwise ->
// 1x1 block (residual = its own input, i.e. the stem tile's centre tap) runs from there.  Unfused,
// stem_kernel writes the stem tensor to HBM and dwpw_vres_kernel reads it straight back (FaceMesh
// V1: 96^2 x 16, BlazeFace short range: 64^2 x 24 f32 per image); nothing else ever reads it.
// Reference: the first Conv / PRelu (Relu) / depthwise Conv / Conv / Add nodes of
// face_landmark.onnx and face_detection_short_range.onnx that ORT / tract execute at
// crates/zaru/src/nn/mod.rs:483-533, with the image -> tensor map of nn/mod.rs:54-73 in front.
//
// A 256-thread workgroup owns an 8 x 32 output tile of one image:
//   phase 1: the 3-channel input patch of the 10 x 34 stem region, sampled from the RGBA frame
//            through the image's view (PRE, every gather issued before the first is used; the
//            lookup's divisions and rounds once per patch row and column, sample.h) or read from
//            the f32 tensor, staged with even and odd columns apart so the stride-2 tap reads of
//            neighbouring lanes fall into neighbouring banks;
//   phase 2: the stem over the region.  Each of the 4 waves computes one half of the output
//            channels over one half of the 340 region positions, three positions per lane: the
//            channel group is uniform in a wave, so the weights come through the scalar cache,
//            once per tap for the three positions, one kernel row per step of a rolled loop
//            (DESIGN 5.10).  That is 1.5x the stem's FMAs (one position per thread with every
//            channel would take two lock-step passes, 2x).  Region
//            positions outside the stem's output plane hold 0.f: they are the block's zero
//            padding;
//   phase 3: dwpw_vres_kernel's arithmetic from the LDS tile: per channel the depthwise (bias,
//            fmaf over the taps in (ky, kx) order), the residual from the centre tap (channels
//            >= r_C zero), the 1x1 accumulated with v_pk_fma_f32 in channel order, then bias,
//            pre-activation, + residual, post-activation and one coalesced store per channel.
// Every output value comes from the same fmaf chain in the same order as the two launches
// (stem: c, ky, kx from +0, then + bias; block: as above), so the form changes no output bit
// (tests/test_gpu_stemblock.py, tests/test_gpu_forms.py).
#include "../runtime/zr_kernels.h"
#include "act.h"
#include "sample.h"

namespace zr {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int SB_TH = 8, SB_TW = 32, SB_RH = SB_TH + 2, SB_RW = SB_TW + 2, SB_NPOS = SB_RH * SB_RW;

// KS x KS stride-SS stem to CS channels, 3x3 stride-1 block CS -> (<= CO) channels; GC: stem
// output channels per wave
template <int KS, int SS, int CS, int CO, bool PRE>
__global__ __launch_bounds__(256) void stem_dwpw_kernel(const StemParams P, const DwPwParams D, int tiles_x, int tpi,
                                                        int ntiles) {
    static_assert(SS == 2, "the patch is staged for stride 2");
    constexpr int PR = (SB_RH - 1) * SS + KS, PC = (SB_RW - 1) * SS + KS, PH = (PC + 1) / 2;
    constexpr int GC = CS / 2, HALF = SB_NPOS / 2, NPL = (HALF + 63) / 64;
    constexpr int CP = 32;  // stem_cpad(CS)
    static_assert(GC % 2 == 0 && SB_NPOS % 2 == 0 && CS <= CO && CS <= CP, "stemblock layout");
    __shared__ float patch[3][PR][2][PH];         // [channel][row][column parity][column / 2]
    __shared__ float sS[CS][SB_RH][SB_RW];        // stem region (zero outside the stem's plane)
    __shared__ float2 sCol[PRE ? PC : 1], sRow[PRE ? PR : 1];  // the view lookup per column / row
    const GemmParams &G = D.g;
    const int cpx = gridDim.x >> 3;  // gridDim.x is a multiple of 8: consecutive tiles share an XCD
    const int tile = (blockIdx.x & 7) * cpx + (blockIdx.x >> 3);
    if (tile >= ntiles) return;  // whole workgroup, before any barrier
    const int n = tile / tpi, tt = tile - n * tpi;
    if (P.nact && n >= *P.nact) return;  // (the same)
    const int ty0 = (tt / tiles_x) * SB_TH, tx0 = (tt % tiles_x) * SB_TW;
    const int tid = threadIdx.x;
    // the region starts one stem pixel above / left of the tile
    const int iy0 = (ty0 - 1) * SS - P.pad_t, ix0 = (tx0 - 1) * SS - P.pad_l;

    // ---- phase 1: the input patch
    if constexpr (PRE) {
        // the view lookup's per-column and per-row halves once (sample.h), then every gather of
        // this thread issued before the first is used
        constexpr int NP = (PR * PC + 255) / 256;
        const ViewDesc d = P.pre.views[n];
        const FrameDesc f = frame_of(P.pre, d);
        for (int i = tid; i < PC + PR; i += 256) {
            if (i < PC) sCol[i] = sample_col(d, ix0 + i, P.IW);
            else sRow[i - PC] = sample_row(d, iy0 + i - PC, P.IH);
        }
        __syncthreads();
        uint32_t px[NP];
        bool pad[NP];
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int i = min(tid + 256 * u, PR * PC - 1);
            const int r = i / PC, x = i - r * PC;
            const int iy = iy0 + r, ix = ix0 + x;
            // outside the network input: the ONNX zero padding of the f32 tensor
            pad[u] = !(iy >= 0 && iy < P.IH && ix >= 0 && ix < P.IW);
            px[u] = load_pixel(f, pad[u] ? -1 : sample_join(d, f, sCol[x], sRow[r]));
        }
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int i = tid + 256 * u;
            if (i >= PR * PC) break;
            const int r = i / PC, x = i - r * PC;
            patch[0][r][x & 1][x >> 1] = pad[u] ? 0.f : color_map(px[u], 0, P.pre.adjust, P.pre.lo);
            patch[1][r][x & 1][x >> 1] = pad[u] ? 0.f : color_map(px[u], 1, P.pre.adjust, P.pre.lo);
            patch[2][r][x & 1][x >> 1] = pad[u] ? 0.f : color_map(px[u], 2, P.pre.adjust, P.pre.lo);
        }
    } else {
        // (every load of this thread issued before the first is stored)
        constexpr int NF = (3 * PR * PC + 255) / 256;
        const float *src = P.in.p + (int64_t)n * P.in.sN;
        float pv[NF];
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const int i = min(tid + 256 * u, 3 * PR * PC - 1);
            const int c = i / (PR * PC), rem = i - c * (PR * PC);
            const int r = rem / PC, x = rem - r * PC;
            const int iy = iy0 + r, ix = ix0 + x;
            const bool ok = iy >= 0 && iy < P.IH && ix >= 0 && ix < P.IW;
            const float v = src[(int64_t)c * P.in.sC + (ok ? (int64_t)iy * P.IW + ix : 0)];
            pv[u] = ok ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const int i = tid + 256 * u;
            if (i >= 3 * PR * PC) break;
            const int c = i / (PR * PC), rem = i - c * (PR * PC);
            const int r = rem / PC, x = rem - r * PC;
            patch[c][r][x & 1][x >> 1] = pv[u];
        }
    }
    __syncthreads();

    // ---- phase 2: the stem over the region.  Wave (g, h) computes channels g * GC .. + GC of
    // region half h, NPL positions per lane: a tap's weights are loaded once for all of them
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const int c0 = (wave >> 1) * GC, pbase = (wave & 1) * HALF;  // uniform in the wave
        int poff[NPL];
        f32x2 acc[NPL][GC / 2];
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int pc = pbase + min(lane + 64 * j, HALF - 1);
            const int ry = pc / SB_RW, rx = pc - ry * SB_RW;
            poff[j] = ry * SS * 2 * PH + rx;
#pragma unroll
            for (int o = 0; o < GC / 2; ++o) acc[j][o] = (f32x2)(0.f);
        }
        // One kernel row per step, the loops over rows kept rolled: a row's KS x GC weights
        // (scalar loads) and KS x NPL patch values are requested together and waited for once,
        // then the row's FMAs run.  (Scalar loads return out of order and share the LDS counter,
        // so every wait drains both: unrolled, the compiler waits once per tap, in front of 4
        // FMAs, or hoists every row's reads to the top and runs out of registers.)
        const float *pf = &patch[0][0][0][0];
#pragma unroll 1
        for (int c = 0; c < 3; ++c)
#pragma unroll 1
            for (int ky = 0; ky < KS; ++ky) {
                // weights [3][K][K][CP]: uniform, so scalar loads feeding v_pk_fma_f32
                const __attribute__((address_space(4))) f32x2 *wp =
                    (const __attribute__((address_space(4))) f32x2 *)(P.w + (c * KS + ky) * KS * CP + c0);
                const float *pt = pf + (c * PR + ky) * 2 * PH;
                f32x2 w[KS][GC / 2];
                float v[KS][NPL];
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
#pragma unroll
                    for (int o = 0; o < GC / 2; ++o) w[kx][o] = wp[kx * (CP / 2) + o];
#pragma unroll
                    for (int j = 0; j < NPL; ++j) v[kx][j] = pt[(kx & 1) * PH + (kx >> 1) + poff[j]];
                }
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                    for (int j = 0; j < NPL; ++j)
#pragma unroll
                        for (int o = 0; o < GC / 2; ++o)
                            acc[j][o] = __builtin_elementwise_fma(w[kx][o], (f32x2)(v[kx][j]), acc[j][o]);
            }
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            float vo[GC];
#pragma unroll
            for (int o = 0; o < GC / 2; ++o) {
                vo[2 * o] = acc[j][o].x + ldc(P.bias, c0 + 2 * o);
                vo[2 * o + 1] = acc[j][o].y + ldc(P.bias, c0 + 2 * o + 1);
            }
            apply_act_n<GC>(P.act, vo, [c0](int o) { return c0 + o; });
            const int pl = lane + 64 * j, pc = pbase + min(pl, HALF - 1);
            const int ry = pc / SB_RW, rx = pc - ry * SB_RW;
            const int sy = ty0 - 1 + ry, sx = tx0 - 1 + rx;
            const bool in = sy >= 0 && sy < P.OH && sx >= 0 && sx < P.OW;
            if (pl < HALF) {
#pragma unroll
                for (int o = 0; o < GC; ++o) sS[c0 + o][ry][rx] = in ? vo[o] : 0.f;
            }
        }
    }
    __syncthreads();

    // ---- phase 3: the block, output (ty0 + ty, tx0 + tx)
    const int ty = tid / SB_TW, tx = tid - ty * SB_TW;
    f32x2 acc[CO / 2];
#pragma unroll
    for (int i = 0; i < CO / 2; ++i) acc[i] = (f32x2)(0.f);
    // CB channels per step of a rolled loop, requested and waited for together as in phase 2
    constexpr int CB = CO <= 16 ? 2 : 1;
    static_assert(CS % CB == 0, "stemblock channel steps");
#pragma unroll 1
    for (int cb = 0; cb < CS; cb += CB) {
        float t[CB][9], wk[CB][10];
        f32x2 w2[CB][CO / 2];
#pragma unroll
        for (int g = 0; g < CB; ++g) {
            const int ch = cb + g;
            const float *t0 = &sS[0][0][0] + (ch * SB_RH + ty) * SB_RW + tx;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) t[g][ky * 3 + kx] = t0[ky * SB_RW + kx];
#pragma unroll
            for (int k = 0; k < 9; ++k) wk[g][k] = ldc(D.dw_w, ch * 9 + k);
            wk[g][9] = ldc(D.dw_b, ch);
            const __attribute__((address_space(4))) f32x2 *wp =
                (const __attribute__((address_space(4))) f32x2 *)(G.wt + (size_t)ch * G.Mpad);  // [Kpad][Mpad]
#pragma unroll
            for (int i = 0; i < CO / 2; ++i) w2[g][i] = wp[i];
        }
#pragma unroll
        for (int g = 0; g < CB; ++g) {
            float d = wk[g][9];
#pragma unroll
            for (int k = 0; k < 9; ++k) d = __builtin_fmaf(wk[g][k], t[g][k], d);
#pragma unroll
            for (int i = 0; i < CO / 2; ++i) acc[i] = __builtin_elementwise_fma(w2[g][i], (f32x2)(d), acc[i]);
        }
    }
    const int oy = ty0 + ty, ox = tx0 + tx;
    if (oy >= P.OH || ox >= P.OW) return;
    float v[CO];
#pragma unroll
    for (int i = 0; i < CO / 2; ++i) {
        v[2 * i] = acc[i].x + G.bias[2 * i];
        v[2 * i + 1] = acc[i].y + G.bias[2 * i + 1];
    }
    auto chan = [](int m) { return m; };
    apply_act_n<CO>(G.pre, v, chan);
    // the residual: the block's input at this position, the centre tap (channels >= r_C zero)
#pragma unroll
    for (int m = 0; m < CO; ++m) v[m] += m < CS && m < G.r_C ? sS[m < CS ? m : 0][ty + 1][tx + 1] : 0.f;
    apply_act_n<CO>(G.post, v, chan);
    const uint32_t q = (uint32_t)(oy * P.OW + ox);
    const uint32_t ob = (uint32_t)n * (uint32_t)G.o_sN + q * (uint32_t)G.o_sP;
#pragma unroll
    for (int m = 0; m < CO; ++m)
        if (m < G.M) G.out[ob + (uint32_t)m * (uint32_t)G.o_sC] = v[m];
}

namespace {

template <int KS, int SS, int CS, int CO>
const char *stem_dwpw_go(const StemParams &p, bool pre, const DwPwParams &d, hipStream_t s) {
    const int tiles_x = (p.OW + SB_TW - 1) / SB_TW, tpi = tiles_x * ((p.OH + SB_TH - 1) / SB_TH);
    const int ntiles = tpi * p.N;
    dim3 grid((ntiles + 7) / 8 * 8);
    if (pre) hipLaunchKernelGGL((stem_dwpw_kernel<KS, SS, CS, CO, true>), grid, dim3(256), 0, s, p, d, tiles_x, tpi, ntiles);
    else hipLaunchKernelGGL((stem_dwpw_kernel<KS, SS, CS, CO, false>), grid, dim3(256), 0, s, p, d, tiles_x, tpi, ntiles);
    return kernel_name("stem_dwpw_kernel<%d,%d,%d,%d,%s>", KS, SS, CS, CO, pre ? "true" : "false");
}

}  // namespace

// The fused form applies to a stem whose output only the next step reads (plan.cpp
// mark_stem_blocks) when that step would run as dwpw_vres_kernel's stride-1 case -- a 3x3
// depthwise without activation over the whole stem plane, the residual its own input, forms
// valu / valu_db / vres on -- with plain CNHW stem storage; instances: the 3x3 stride-2 stem to
// 16 channels with a block of <= 16 outputs (FaceMesh V1) and the 5x5 stride-2 stem to 24
// channels with a block of 17..32 outputs (BlazeFace short range).  Everything else: nullptr,
// and the caller runs the two launches.
const char *launch_stem_dwpw(const StemParams &p, bool pre, const DwPwParams &d, hipStream_t s) {
    const GemmParams &g = d.g;
    if (!form_on(FORM_STEMBLOCK) || !dwpw_is_vres1(d) || p.stride != 2 || d.k != 3 || g.K != p.Cout ||
        d.in.p != p.out || d.in.sN != p.o_sN || d.in.sC != p.o_sC || d.in.H != p.OH || d.in.W != p.OW ||
        g.P != p.OH * p.OW || g.ncols != p.N * g.P || g.nact != p.nact || g.Mpad % 2 != 0 ||
        ((uintptr_t)g.wt | (uintptr_t)p.w) % 8 != 0)
        return nullptr;
    if (p.k == 3 && p.Cout == 16 && g.M <= 16) return stem_dwpw_go<3, 2, 16, 16>(p, pre, d, s);
    if (p.k == 5 && p.Cout == 24 && g.M > 16 && g.M <= 32) return stem_dwpw_go<5, 2, 24, 32>(p, pre, d, s);
    return nullptr;
}

}  // namespace zr
