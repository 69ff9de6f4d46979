// gdc.hip -- gdc_kernel: a depthwise conv whose kernel is its whole input plane (pad 0, stride
// 1), MobileFaceNet's "global depthwise conv" (7x7 on the 7^2 plane, 512 channels), which turns
// the last feature map into one vector per image:
//     out(n, c) = act(bias[c] + sum over (ky, kx) in row-major order of w[c][ky][kx] * x(n, c, ky, kx))
// with the multiply and the add rounded separately and the taps summed in exactly that order.
//
// Memory-bound: 4*C*H*W bytes in and 4*C bytes out per image.  The shape is dwgap_lane_kernel's
// (misc.hip): a workgroup takes one channel of 256 images -- in CNHW those planes are one
// contiguous run -- stages it in LDS with 16-byte loads, and every lane then owns one plane.  A
// lane's plane starts HW floats after its neighbour's; HW = 49 is odd, so the 64 lanes of a
// read hit distinct banks.  The channel is uniform over the workgroup: its HW weights and its
// bias come through the scalar cache, and the taps are static indices.
// Reference: the Conv node the ONNX runtime executes at crates/zaru/src/nn/mod.rs:483-533.
#include "../runtime/zr_kernels.h"
#include "act.h"

namespace zr {

constexpr int GDC_NB = 256;  // images (planes of one channel) per workgroup, one per lane

// HWT: the plane size when known at compile time (0: read from P, taps in a counted loop)
template <int HWT>
__global__ __launch_bounds__(GDC_NB) void gdc_kernel(const DwParams P, int vec) {
    extern __shared__ __attribute__((aligned(16))) float pl[];  // GDC_NB planes of HW floats
    const int HW = HWT ? HWT : P.in.H * P.in.W;
    const int c = blockIdx.y, n0 = blockIdx.x * GDC_NB;
    const int nb = min(GDC_NB, P.N - n0);
    const float *src = P.in.p + (int64_t)c * P.in.sC + (int64_t)n0 * P.in.sN;
    if (vec) {  // the planes are contiguous (sN = HW) and the run starts 16-B aligned
        const int n4 = (nb * HW) >> 2;
        for (int i = threadIdx.x; i < n4; i += GDC_NB)
            reinterpret_cast<float4 *>(pl)[i] = reinterpret_cast<const float4 *>(src)[i];
        for (int i = 4 * n4 + threadIdx.x; i < nb * HW; i += GDC_NB) pl[i] = src[i];
    } else {
        for (int i = threadIdx.x; i < nb * HW; i += GDC_NB) {
            const int n = i / HW, q = i - n * HW;
            pl[i] = src[(int64_t)n * P.in.sN + q];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x >= nb) return;
    const float *x = pl + threadIdx.x * HW;
    const float *w = P.w + (int64_t)c * HW;
    float acc = P.bias[c];
    if constexpr (HWT != 0) {
#pragma unroll
        for (int t = 0; t < HWT; ++t) acc = __fadd_rn(acc, __fmul_rn(w[t], x[t]));
    } else {
        for (int t = 0; t < HW; ++t) acc = __fadd_rn(acc, __fmul_rn(w[t], x[t]));
    }
    P.out[(int64_t)(n0 + threadIdx.x) * P.o_sN + (int64_t)c * P.o_sC] = apply_act(P.act, acc, c);
}

template <int HWT>
static void gdc_go(const DwParams &p, int hw, int vec, hipStream_t s) {
    static const bool attr = hipFuncSetAttribute((const void *)gdc_kernel<HWT>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    (void)attr;
    const dim3 grid((p.N + GDC_NB - 1) / GDC_NB, p.in.C);
    hipLaunchKernelGGL((gdc_kernel<HWT>), grid, dim3(GDC_NB), sizeof(float) * GDC_NB * hw, s, p, vec);
}

const char *launch_gdc(const DwParams &p, hipStream_t s) {
    const int hw = p.in.H * p.in.W;  // gdc_supported(): <= 64, so GDC_NB planes fit 64 KB of LDS
    const int vec = p.in.sN == hw && p.in.sC % 4 == 0 && (GDC_NB * hw) % 4 == 0 && (uintptr_t)p.in.p % 16 == 0;
    if (hw == 49) {
        gdc_go<49>(p, hw, vec, s);
        return "gdc_kernel<49>";
    }
    gdc_go<0>(p, hw, vec, s);
    return "gdc_kernel<0>";
}

}  // namespace zr
