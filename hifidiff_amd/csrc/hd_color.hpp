// hd_color.hpp — colour correction of decoded faces against a reference image, the step restoration stacks apply after
// vae.decode (StableSR's wavelet_color_fix / adain_color_fix).  The reference project has no such step: like guidance, masks and
// previews it is an addition around its loop (include/hifidiff_hip.h: hd_color_fix).  Planes are NCHW fp32; c is a decoded plane
// [R,R], s the reference plane [Rr,Rr], w the face's weight.
//   wavelet, n levels:  out = c + w * B_n(s' - c),  B_n = blur_{n-1} o ... o blur_0,  blur_i = the 3x3 binomial kernel
//                       [1/4 1/2 1/4]^T [1/4 1/2 1/4] with dilation 2^i and replicate padding, s' = s resampled to R x R with
//                       F.interpolate(mode="bicubic", align_corners=False) when Rr != R.  StableSR's high(c) + low(s) telescopes
//                       to c - B_n(c) + B_n(s), and every blur_i is linear.
//   AdaIN:              out = c + w * (a - c),  a = (c - mean(c)) * std(s) / std(c) + mean(s),  std = sqrt(var_unbiased + 1e-5),
//                       the statistics of s at its own resolution.
// vae_range: s is first mapped to clamp(s, 0, 1) * 2 - 1 (to_vae_range, as hd_vae_encode).  w == 0 stores c bit for bit.
// Neither kernel uses global scratch; out must not overlap images or ref (the tiled kernel reads its neighbours' c).
#pragma once
#include <hip/hip_runtime.h>
#include "hd_bicubic.hpp"

namespace hd {

constexpr int CF_TILE = 64;                                       // output tile side
constexpr int CF_MAX_LEVELS = 5;                                  // halo 2^n - 1 <= 31
constexpr int CF_MAX_SIDE = CF_TILE + 2 * ((1 << CF_MAX_LEVELS) - 1);   // 126: a tile with its full halo
constexpr int CF_THREADS = 1024;
constexpr size_t CF_MAX_SMEM = (size_t)2 * CF_MAX_SIDE * CF_MAX_SIDE * sizeof(float);   // 127008 B of gfx950's 160 KiB

__device__ __forceinline__ float cf_ref_value(float v, int vae_range) {
    return vae_range ? fminf(fmaxf(v, 0.f), 1.f) * 2.f - 1.f : v;
}

// s'(oy, ox): bicubic_resize_kernel's arithmetic (cubic_coeffs, taps clamped to the border) for one output pixel of an R x R grid
__device__ __forceinline__ float cf_bicubic_tap(const float* __restrict__ src, int Rr, float scale, int oy, int ox, int vae_range) {
    const float fy = (oy + 0.5f) * scale - 0.5f, fx = (ox + 0.5f) * scale - 0.5f;
    const int iy = (int)floorf(fy), ix = (int)floorf(fx);
    float wy[4], wx[4];
    cubic_coeffs(fy - (float)iy, wy); cubic_coeffs(fx - (float)ix, wx);
    int xs[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) xs[b] = min(max(ix - 1 + b, 0), Rr - 1);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int yy = min(max(iy - 1 + a, 0), Rr - 1);
        float r = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) r += wx[b] * cf_ref_value(src[(size_t)yy * Rr + xs[b]], vae_range);
        acc += wy[a] * r;
    }
    return acc;
}

// One workgroup per (plane, 64 x 64 output tile).  d = s' - c of the tile and its 2^n - 1 halo, clipped to the image, is staged in
// LDS; the 2n separable passes (horizontal then vertical per level) run between two LDS planes; the tile's interior gets
// c + w * d_n.  Taps are clamped to the staged region: where its edge is an image edge that is the replicate padding, where it is
// not, the wrong values move inwards 2^i per level, 2^n - 1 in all, and stop at the interior.  Each pass therefore only computes
// what the interior still depends on (margin 2^n - 2^(i+1) after level i), and a pixel's bits do not depend on the tiling: every
// value the interior reads is the same expression of the same image values in every tile.
static __global__ __launch_bounds__(CF_THREADS) void wavelet_fix_kernel(const float* __restrict__ images, const float* __restrict__ ref,
                                                                         float* __restrict__ out, const float* __restrict__ weight,
                                                                         int R, int Rr, int vae_range, int levels) {
    extern __shared__ __attribute__((aligned(16))) float cf_smem[];
    const int tiles = R / CF_TILE;
    const int tx = blockIdx.x % tiles, ty = blockIdx.x / tiles;
    const size_t plane = blockIdx.y;
    const int t = threadIdx.x;
    const float* __restrict__ c = images + plane * R * R;
    float* __restrict__ o = out + plane * R * R;
    const float w = weight ? weight[plane / 3] : 1.f;
    const int oy0 = ty * CF_TILE, ox0 = tx * CF_TILE;             // the interior in image coordinates
    if (w == 0.f) {                                               // the face keeps its image, bit for bit
        for (int i = t; i < CF_TILE * CF_TILE; i += CF_THREADS) {
            const size_t g = (size_t)(oy0 + (i >> 6)) * R + ox0 + (i & 63);
            o[g] = c[g];
        }
        return;
    }
    const int halo = (1 << levels) - 1;
    const int gy0 = max(oy0 - halo, 0), gy1 = min(oy0 + CF_TILE + halo, R);   // the staged region in image coordinates
    const int gx0 = max(ox0 - halo, 0), gx1 = min(ox0 + CF_TILE + halo, R);
    const int rh = gy1 - gy0, rw = gx1 - gx0;                     // <= 126 each
    const int iy0 = oy0 - gy0, ix0 = ox0 - gx0;                   // the interior in region coordinates
    const int plane_elems = rh * rw;
    // thread layout of every pass: lanes along x (LDS and global accesses of a wave are consecutive), rows strided
    const int lx = t & 127, ly = t >> 7;                          // 128 x 8

    constexpr int RS = CF_THREADS / 128;                          // row stride of the layout
    if (lx < rw) {   // stage d = s' - c
        const float* __restrict__ s = ref + plane * Rr * Rr;
        const float scale = (float)Rr / (float)R;
        const int gx = gx0 + lx;
        for (int y = ly; y < rh; y += RS) {
            const int gy = gy0 + y;
            const float sv = Rr == R ? cf_ref_value(s[(size_t)gy * R + gx], vae_range) : cf_bicubic_tap(s, Rr, scale, gy, gx, vae_range);
            cf_smem[y * rw + lx] = sv - c[(size_t)gy * R + gx];
        }
    }
    __syncthreads();

    const int src = 0, dst = plane_elems;
    for (int lv = 0; lv < levels; ++lv) {
        const int r = 1 << lv;
        const int m_cur = (1 << levels) - r, m_next = m_cur - r;  // margins still needed before / after this level
        const int xa = max(ix0 - m_next, 0), xb = min(ix0 + CF_TILE + m_next, rw);
        const int x = xa + lx;
        if (x < xb) {   // horizontal: the rows the vertical pass of this level will read
            const int ya = max(iy0 - m_cur, 0), yb = min(iy0 + CF_TILE + m_cur, rh);
            const int xl = max(x - r, 0), xr = min(x + r, rw - 1);
            for (int y = ya + ly; y < yb; y += RS) {
                const int row = src + y * rw;
                cf_smem[dst + y * rw + x] = 0.5f * cf_smem[row + x] + 0.25f * (cf_smem[row + xl] + cf_smem[row + xr]);
            }
        }
        __syncthreads();
        if (x < xb) {   // vertical
            const int ya = max(iy0 - m_next, 0), yb = min(iy0 + CF_TILE + m_next, rh);
            for (int y = ya + ly; y < yb; y += RS) {
                const int col = dst + x;
                cf_smem[src + y * rw + x] = 0.5f * cf_smem[col + y * rw] + 0.25f * (cf_smem[col + max(y - r, 0) * rw] + cf_smem[col + min(y + r, rh - 1) * rw]);
            }
        }
        __syncthreads();
    }
    // the blurred difference of the interior is in the first plane again
    for (int i = t; i < CF_TILE * CF_TILE; i += CF_THREADS) {
        const int y = i >> 6, x = i & 63;
        const size_t g = (size_t)(oy0 + y) * R + ox0 + x;
        o[g] = c[g] + w * cf_smem[src + (iy0 + y) * rw + ix0 + x];
    }
}

// One workgroup per plane: sum and sum of squares of c and of s in fp64 (per thread, then across the workgroup through LDS, in a
// fixed order), then the apply pass over the plane.  No partial leaves the workgroup, so nothing is kept in global memory.
static __global__ __launch_bounds__(CF_THREADS) void adain_fix_kernel(const float* __restrict__ images, const float* __restrict__ ref,
                                                                       float* __restrict__ out, const float* __restrict__ weight,
                                                                       int R, int Rr, int vae_range) {
    __shared__ double red[4][CF_THREADS / 64];
    __shared__ float coef[3];
    const size_t plane = blockIdx.x;
    const int t = threadIdx.x;
    const int n = R * R, nr = Rr * Rr;                            // multiples of 4096
    const float4* __restrict__ c4 = reinterpret_cast<const float4*>(images + plane * n);
    float4* __restrict__ o4 = reinterpret_cast<float4*>(out + plane * n);
    const float w = weight ? weight[plane / 3] : 1.f;
    if (w == 0.f) {
        for (int i = t; i < n / 4; i += CF_THREADS) o4[i] = c4[i];
        return;
    }
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(ref + plane * nr);
    double a[4] = {0.0, 0.0, 0.0, 0.0};                           // sum c, sum c^2, sum s, sum s^2
    for (int i = t; i < n / 4; i += CF_THREADS) {
        const float4 v = c4[i];
        const double x = v.x, y = v.y, z = v.z, q = v.w;
        a[0] += (x + y) + (z + q); a[1] += (x * x + y * y) + (z * z + q * q);
    }
    for (int i = t; i < nr / 4; i += CF_THREADS) {
        const float4 v = s4[i];
        const double x = cf_ref_value(v.x, vae_range), y = cf_ref_value(v.y, vae_range), z = cf_ref_value(v.z, vae_range), q = cf_ref_value(v.w, vae_range);
        a[2] += (x + y) + (z + q); a[3] += (x * x + y * y) + (z * z + q * q);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = a[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((t & 63) == 0) red[k][t >> 6] = v;
    }
    __syncthreads();
    if (t == 0) {
        double sum[4];
        for (int k = 0; k < 4; ++k) {
            double v = 0.0;
            for (int j = 0; j < CF_THREADS / 64; ++j) v += red[k][j];
            sum[k] = v;
        }
        const double mc = sum[0] / n, ms = sum[2] / nr;
        const double vc = fmax((sum[1] - sum[0] * mc) / (n - 1), 0.0), vs = fmax((sum[3] - sum[2] * ms) / (nr - 1), 0.0);
        coef[0] = (float)mc; coef[1] = (float)(sqrt(vs + 1e-5) / sqrt(vc + 1e-5)); coef[2] = (float)ms;
    }
    __syncthreads();
    const float mc = coef[0], ratio = coef[1], ms = coef[2];
    for (int i = t; i < n / 4; i += CF_THREADS) {
        const float4 v = c4[i];
        float4 r;
        r.x = v.x + w * (((v.x - mc) * ratio + ms) - v.x);
        r.y = v.y + w * (((v.y - mc) * ratio + ms) - v.y);
        r.z = v.z + w * (((v.z - mc) * ratio + ms) - v.z);
        r.w = v.w + w * (((v.w - mc) * ratio + ms) - v.w);
        o4[i] = r;
    }
}

}  // namespace hd
