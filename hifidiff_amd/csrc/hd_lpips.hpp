// hd_lpips.hpp — the kernels of LPIPS-AlexNet v0.1 (Zhang et al. 2018) that are not convolutions: the input preparation, the max-pool
// without padding and the distance over the five tapped layers.  The contract is in include/hifidiff_hip.h (hd_lpips); the five
// convolutions are launches of the shared GEMM family (hd_lpips.hip).  The two images of a pair travel through the network as faces f and
// B + f of one batch of 2B: the same launches, row-independent arithmetic, hence the same bits for equal inputs.
//   lpips_input_kernel: steps 1-4 for both tensors (bicubic resampling while loading, min-max normalisation, 2x - 1, scaling layer) into
//     channels-last bf16 with 8 channels per pixel, the upper five zero: the gather source of the first convolution.
//   maxpool3x3s2_valid_bf16_kernel: MaxPool2d(3, 2) on channels-last bf16, eight channels per thread.
//   lpips_distance_kernel: one launch for all five layers.  A wave owns a position of a face in a layer; lane l holds channels l, l + 64,
//     ... of fa and fb.  Two wave reductions give the squared norms, a third the weighted squared difference of the unit vectors; four
//     positions are in flight per wave.  The wave adds its positions in fp64, the workgroup its waves by index, and writes one fp64 partial.
//   lpips_combine_kernel: per face, the partials of each layer in index order, divided by the position count; the total.
// No atomics: a score has the same bits from call to call and at every slot of a batch.
#pragma once
#include <hip/hip_runtime.h>
#include "hd_internal.hpp"
#include "hd_metrics.hpp"

namespace hd {

constexpr int LP_LAYERS = 5;
constexpr int LP_THREADS = 256;                                   // distance kernel: four waves
constexpr int LP_POS_PER_WG = 64;                                 // positions of one (layer, face) per workgroup: 16 per wave

// Per layer: the two feature maps are fa = feat[face] and fb = feat[B + face], [2B][P][C] bf16; w [C] fp32; wg0: the layer's first
// workgroup in a face's row of the grid (wg0[5] = the row's length)
struct LpDistP {
    const unsigned short* feat[LP_LAYERS];
    const float* w[LP_LAYERS];
    int C[LP_LAYERS], P[LP_LAYERS], wg0[LP_LAYERS + 1];
    int B;
    double* partial;                                              // [B][wg0[5]]
};

// grid (ceil(2B * Rb^2 / 256)).  in8 [2B][Rb][Rb] pixels of 8 bf16.
static __global__ __launch_bounds__(256) void lpips_input_kernel(const float* __restrict__ images, int R, const float* __restrict__ ref, int Rb, int B,
                                                                 int unit_range, const float* __restrict__ images_range,
                                                                 const float* __restrict__ ref_range, LpScale sc, uint4* __restrict__ in8) {
    const size_t npix = (size_t)Rb * Rb, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * (size_t)B * npix) return;
    const size_t f2 = i / npix;
    const int rem = (int)(i - f2 * npix), gy = rem / Rb, gx = rem - gy * Rb;
    const bool is_ref = f2 >= (size_t)B;
    const size_t face = is_ref ? f2 - B : f2;
    const int Rs = is_ref ? Rb : R;
    const float* __restrict__ src = (is_ref ? ref : images) + face * 3 * Rs * Rs;
    const float* __restrict__ rng = is_ref ? (ref_range ? ref_range + face * 2 : nullptr) : (images_range ? images_range + face * 2 : nullptr);
    const float scale = (float)Rs / (float)Rb;
    float v[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float x = mt_normalise(mt_fetch(src, ch, Rs, Rb, scale, gy, gx), rng);
        if (unit_range) x = __fsub_rn(__fmul_rn(2.f, x), 1.f);
        v[ch] = __fdiv_rn(__fsub_rn(x, sc.shift[ch]), sc.scale[ch]);
    }
    in8[i] = make_uint4(pack2(v[0], v[1]), pack2(v[2], 0.f), 0u, 0u);
}

// MaxPool2d(3, stride 2), no padding, channels-last bf16: Ho = (H - 3) / 2 + 1.  One thread per (pixel, 8 channels); C % 8 == 0.
static __global__ __launch_bounds__(256) void maxpool3x3s2_valid_bf16_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out,
                                                                             int N, int H, int C) {
    const int Ho = (H - 3) / 2 + 1, C8 = C / 8;
    const size_t total = (size_t)N * Ho * Ho * C8;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    size_t r = i / C8;
    const int ox = (int)(r % Ho); r /= Ho;
    const int oy = (int)(r % Ho);
    const size_t b = r / Ho;
    float m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = -3.402823466e38f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {                          // 2 * (Ho - 1) + 2 <= H - 1: every tap is inside the image
            const int y = oy * 2 + ky, x = ox * 2 + kx;
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(in + ((b * H + y) * H + x) * C + c8 * 8), v);
#pragma unroll
            for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], v[k]);
        }
    *reinterpret_cast<uint4*>(out + i * 8) = pack8(m);
}

constexpr int LP_UNROLL = 4;                                      // positions a wave has in flight

// The positions pos0, pos0 + 4, ... (< p1, at most 16) of a layer of NJ * 64 channels, as one wave: per position
//   sum_c w_c (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2,
// the norms and the sum by wave reduction on the DPP path (hd_gemm.hpp wave_sum: a fixed order, the same value for every lane), added
// up in fp64 in position order.  Four positions are in flight so that their loads and reductions overlap; a position past p1 is
// loaded from the last valid one and not added (wave-uniform).  Spelled out in intrinsics: swapping fa and fb, or making them equal,
// must not change how anything is rounded.
template <int NJ>
__device__ __forceinline__ double lp_wave_positions(const unsigned short* __restrict__ fa, const unsigned short* __restrict__ fb,
                                                    const float* __restrict__ w, int pos0, int p1, int lane) {
    constexpr int C = NJ * 64, STEP = LP_THREADS / 64;
    float wv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) wv[j] = w[lane + 64 * j];
    double acc = 0.0;
    for (int g = 0; g < LP_POS_PER_WG / (STEP * LP_UNROLL); ++g) {
        const int base = pos0 + g * STEP * LP_UNROLL;
        if (base >= p1) break;
        float a[LP_UNROLL][NJ], b[LP_UNROLL][NJ], d[LP_UNROLL];
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u) {
            const size_t at = (size_t)min(base + u * STEP, p1 - 1) * C + lane;
#pragma unroll
            for (int j = 0; j < NJ; ++j) { a[u][j] = bf16_bits_to_f32(fa[at + 64 * j]); b[u][j] = bf16_bits_to_f32(fb[at + 64 * j]); }
        }
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u) {
            float na = 0.f, nb = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) { na = __fmaf_rn(a[u][j], a[u][j], na); nb = __fmaf_rn(b[u][j], b[u][j], nb); }
            const float da = __fadd_rn(__fsqrt_rn(wave_sum(na)), 1e-10f), db = __fadd_rn(__fsqrt_rn(wave_sum(nb)), 1e-10f);
            float e2 = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float e = __fsub_rn(__fdiv_rn(a[u][j], da), __fdiv_rn(b[u][j], db));
                e2 = __fmaf_rn(wv[j], __fmul_rn(e, e), e2);
            }
            d[u] = wave_sum(e2);
        }
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u)
            if (base + u * STEP < p1) acc += (double)d[u];
    }
    return acc;
}

// grid (wg0[5], B).  Workgroup j of layer k covers positions [64 j, 64 j + 64) of the layer, wave w every fourth of them.
static __global__ __launch_bounds__(LP_THREADS) void lpips_distance_kernel(LpDistP p) {
    __shared__ double red[LP_THREADS / 64];
    int k = 0;
#pragma unroll
    for (int q = 1; q < LP_LAYERS; ++q) if ((int)blockIdx.x >= p.wg0[q]) k = q;
    const int j = blockIdx.x - p.wg0[k], C = p.C[k], P = p.P[k];
    const size_t face = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned short* __restrict__ fa = p.feat[k] + face * P * C;
    const unsigned short* __restrict__ fb = p.feat[k] + (face + p.B) * P * C;
    const float* __restrict__ w = p.w[k];
    const int pos0 = j * LP_POS_PER_WG + wave, p1 = min(P, (j + 1) * LP_POS_PER_WG);      // j * 64 < P: p1 - 1 is a position of this workgroup
    double acc;
    if (C == 64) acc = lp_wave_positions<1>(fa, fb, w, pos0, p1, lane);
    else if (C == 192) acc = lp_wave_positions<3>(fa, fb, w, pos0, p1, lane);
    else if (C == 384) acc = lp_wave_positions<6>(fa, fb, w, pos0, p1, lane);
    else acc = lp_wave_positions<4>(fa, fb, w, pos0, p1, lane);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < LP_THREADS / 64; ++q) s += red[q];
        p.partial[face * p.wg0[LP_LAYERS] + blockIdx.x] = s;
    }
}

// grid (B), 64 threads.  out [B]; layers_out [B][5] or NULL.
static __global__ __launch_bounds__(64) void lpips_combine_kernel(LpDistP p, double* __restrict__ out, double* __restrict__ layers_out) {
    __shared__ double lay[LP_LAYERS];
    const size_t face = blockIdx.x;
    const int k = threadIdx.x;
    if (k < LP_LAYERS) {
        const double* __restrict__ q = p.partial + face * p.wg0[LP_LAYERS];
        double s = 0.0;
        for (int i = p.wg0[k]; i < p.wg0[k + 1]; ++i) s += q[i];
        lay[k] = s / (double)p.P[k];
        if (layers_out) layers_out[face * LP_LAYERS + k] = lay[k];
    }
    __syncthreads();
    if (k == 0) {
        double s = 0.0;
        for (int i = 0; i < LP_LAYERS; ++i) s += lay[i];
        out[face] = s;
    }
}

}  // namespace hd
