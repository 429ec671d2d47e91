// hd_metrics.hpp — per-face MSE (for PSNR) and SSIM of images against a reference, the last step of the reference's evaluation loop
// (test_refiner.py:113-122: F.interpolate to the target's size, min-max normalise, pyiqa's psnr and ssim).  pyiqa is absent: the
// formulas of include/hifidiff_hip.h (hd_image_metrics, hd_image_range) are the contract.  Images are NCHW fp32; a = images resampled to
// the reference's side Rb, b = the reference, both optionally normalised with a per-face (lo, hi) and reduced to luma.
//   metrics_kernel: one workgroup per (64 x 64 tile, scored plane, face).  The tile's 74 x 74 region of a' and b' (64 + the 10 further
//     rows and columns the 11-tap window reaches) is staged in LDS once, resampled, normalised and converted during that load.  Thread
//     (column x, strip of 16 rows) then walks down its column: the horizontal window sums of the five moments a, b, a^2, b^2, ab of one row
//     go into a ring of 11 register rows, and every row past the tenth closes one map value from the ring.  The moment maps never leave
//     the registers.  A map value is the same expression of the same pixels wherever its face stands in the batch.
//   metrics_combine_kernel: one thread per face adds the face's tile partials (fp64) in index order.
//   range_kernel: one workgroup per face, min and max over the three channels.
// Sums over a face are fp64 and combined in a fixed order (lanes by shuffle, waves and tiles by index): no atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include "hd_color.hpp"

namespace hd {

constexpr int MT_TILE = 64;                                       // map positions (and owned pixels) per tile side
constexpr int MT_WIN = 11;                                        // window taps
constexpr int MT_SIDE = MT_TILE + MT_WIN - 1;                     // 74: the staged region
constexpr int MT_STRIP = 16;                                      // map rows per thread
constexpr int MT_THREADS = MT_TILE * (MT_TILE / MT_STRIP);        // 256: one wave per strip, lanes along x
constexpr int MT_RANGE_THREADS = 1024;

struct MtWindow { float g[MT_WIN]; };                             // the normalised Gaussian, rounded from float64

__device__ __forceinline__ float mt_normalise(float v, const float* __restrict__ range) {
    if (!range) return v;
    const float lo = range[0], hi = range[1];
    return hi > lo ? __fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo)) : 0.f;
}

// one pixel of plane `ch` of a face at the scored resolution Rb
__device__ __forceinline__ float mt_fetch(const float* __restrict__ face, int ch, int R, int Rb, float scale, int gy, int gx) {
    const float* __restrict__ p = face + (size_t)ch * R * R;
    return R == Rb ? p[(size_t)gy * R + gx] : cf_bicubic_tap(p, R, scale, gy, gx, 0);
}

// the scored value: normalised, then the plane itself (rgb) or the BT.601 studio luma of the three (y)
template <int LUMA>
__device__ __forceinline__ float mt_value(const float* __restrict__ face, int plane, int R, int Rb, float scale, int gy, int gx,
                                          const float* __restrict__ range, float L) {
    if (!LUMA) return mt_normalise(mt_fetch(face, plane, R, Rb, scale, gy, gx), range);
    const float r = mt_normalise(mt_fetch(face, 0, R, Rb, scale, gy, gx), range);
    const float g = mt_normalise(mt_fetch(face, 1, R, Rb, scale, gy, gx), range);
    const float b = mt_normalise(mt_fetch(face, 2, R, Rb, scale, gy, gx), range);
    // spelled out in intrinsics: both images take the same roundings however the compiler contracts the code around each of the two uses
    // (equal inputs must give a' == b' bit for bit)
    const float s = __fmaf_rn(24.966f, b, __fmaf_rn(128.553f, g, __fmul_rn(65.481f, r)));
    return __fdiv_rn(__fadd_rn(s, __fmul_rn(16.f, L)), 255.f);
}

// grid (tiles^2, P, B).  partial [B][P * tiles^2][2] (fp64): the tile's sum of (a' - b')^2 over its 64 x 64 pixels and of the map over
// its valid positions.  ssim_map [B][P][Rb-10][Rb-10] or NULL.
template <int LUMA>
static __global__ __launch_bounds__(MT_THREADS) void metrics_kernel(const float* __restrict__ images, int R, const float* __restrict__ ref, int Rb,
                                                                    float L, const float* __restrict__ images_range, const float* __restrict__ ref_range,
                                                                    MtWindow win, double* __restrict__ partial, float* __restrict__ ssim_map) {
    __shared__ float sa[MT_SIDE * MT_SIDE], sb[MT_SIDE * MT_SIDE];
    __shared__ double red[MT_THREADS / 64][2];
    const int tiles = Rb / MT_TILE;
    const int tx = blockIdx.x % tiles, ty = blockIdx.x / tiles;
    const int plane = blockIdx.y, P = gridDim.y;
    const size_t face = blockIdx.z;
    const int t = threadIdx.x;
    const int oy0 = ty * MT_TILE, ox0 = tx * MT_TILE;             // the region's origin: image and map coordinates coincide
    const int V = Rb - (MT_WIN - 1);                              // side of the valid map
    {   // stage a' and b'; past the image (last tile row / column) zeros, read only by map positions that are not stored
        const float* __restrict__ fa = images + face * 3 * R * R;
        const float* __restrict__ fb = ref + face * 3 * Rb * Rb;
        const float* __restrict__ ra = images_range ? images_range + face * 2 : nullptr;
        const float* __restrict__ rb = ref_range ? ref_range + face * 2 : nullptr;
        const float scale = (float)R / (float)Rb;
        for (int i = t; i < MT_SIDE * MT_SIDE; i += MT_THREADS) {
            const int y = i / MT_SIDE, x = i - y * MT_SIDE;
            const int gy = oy0 + y, gx = ox0 + x;
            float av = 0.f, bv = 0.f;
            if (gy < Rb && gx < Rb) {
                av = mt_value<LUMA>(fa, plane, R, Rb, scale, gy, gx, ra, L);
                bv = mt_value<LUMA>(fb, plane, Rb, Rb, 1.f, gy, gx, rb, L);
            }
            sa[i] = av; sb[i] = bv;
        }
    }
    __syncthreads();

    const int x = t & (MT_TILE - 1), y0 = (t >> 6) * MT_STRIP;     // this thread's column and first map row, in tile coordinates
    const int nrows = min(MT_STRIP, V - (oy0 + y0));              // valid map rows of the strip: 16, or 6 in the last tile row
    const bool col_ok = ox0 + x < V;
    const float C1 = (0.01f * L) * (0.01f * L), C2 = (0.03f * L) * (0.03f * L);
    float* __restrict__ mp = ssim_map ? ssim_map + ((face * P + plane) * V + (oy0 + y0)) * V + ox0 + x : nullptr;
    float h[MT_WIN][5];                                           // ring: the horizontal sums of row r live in slot r % 11
    double mse = 0.0, ssim = 0.0;
#pragma unroll
    for (int r = 0; r < MT_STRIP + MT_WIN - 1; ++r) {
        if (r < nrows + MT_WIN - 1) {                             // wave-uniform; nrows + 10 >= 16, so every owned pixel is visited
            const int row = (y0 + r) * MT_SIDE + x;
            float ha = 0.f, hb = 0.f, haa = 0.f, hbb = 0.f, hab = 0.f;
#pragma unroll
            for (int k = 0; k < MT_WIN; ++k) {
                const float av = sa[row + k], bv = sb[row + k], gk = win.g[k];
                if (k == 0 && r < MT_STRIP) {                     // the pixel (y0 + r, x) itself is one of the tile's 64 x 64
                    const float d = av - bv;
                    mse += (double)(d * d);
                }
                ha += gk * av; hb += gk * bv;
                haa += gk * (av * av); hbb += gk * (bv * bv); hab += gk * (av * bv);
            }
            constexpr int NW = MT_WIN;
            const int slot = r % NW;
            h[slot][0] = ha; h[slot][1] = hb; h[slot][2] = haa; h[slot][3] = hbb; h[slot][4] = hab;
            if (r >= NW - 1) {                                    // rows r-10 .. r are in the ring: map row r - 10
                float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    const int s = (r + 1 + k) % NW;               // slot of row r - 10 + k
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] += win.g[k] * h[s][q];
                }
                const float mua = m[0], mub = m[1];
                const float va = m[2] - mua * mua, vb = m[3] - mub * mub, cab = m[4] - mua * mub;
                const float v = ((2.f * mua * mub + C1) * (2.f * cab + C2)) / ((mua * mua + mub * mub + C1) * (va + vb + C2));
                if (col_ok) {
                    ssim += (double)v;
                    if (mp) mp[(size_t)(r - (NW - 1)) * V] = v;
                }
            }
        }
    }
    // lanes by shuffle, then the four waves by index
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { mse += __shfl_down(mse, off, 64); ssim += __shfl_down(ssim, off, 64); }
    if ((t & 63) == 0) { red[t >> 6][0] = mse; red[t >> 6][1] = ssim; }
    __syncthreads();
    if (t == 0) {
        double a = 0.0, b = 0.0;
        for (int j = 0; j < MT_THREADS / 64; ++j) { a += red[j][0]; b += red[j][1]; }
        double* __restrict__ o = partial + ((face * P + plane) * gridDim.x + blockIdx.x) * 2;
        o[0] = a; o[1] = b;
    }
}

// out [B][2] (fp64): mse, ssim.  n = P * tiles^2 partials per face, added in index order.
static __global__ void metrics_combine_kernel(const double* __restrict__ partial, int batch, int n, double inv_pixels, double inv_positions,
                                              double* __restrict__ out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= batch) return;
    const double* __restrict__ p = partial + (size_t)f * n * 2;
    double a = 0.0, b = 0.0;
    for (int i = 0; i < n; ++i) { a += p[2 * i]; b += p[2 * i + 1]; }
    out[2 * f] = a * inv_pixels; out[2 * f + 1] = b * inv_positions;
}

// range_out [B][2]: min and max over the three channels of face blockIdx.x at side Ro.  R == Ro: the 3 R^2 values as float4 (R^2 is a
// multiple of 4096), eight loads in flight per thread.
static __global__ __launch_bounds__(MT_RANGE_THREADS) void range_kernel(const float* __restrict__ images, int R, int Ro, float* __restrict__ range_out) {
    __shared__ float red[2][MT_RANGE_THREADS / 64];
    const size_t face = blockIdx.x;
    const int t = threadIdx.x;
    const float* __restrict__ src = images + face * 3 * R * R;
    float lo = INFINITY, hi = -INFINITY;
    if (R == Ro) {
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
        const int n4 = 3 * R * R / 4;
        int i = t;
        for (; i + 7 * MT_RANGE_THREADS < n4; i += 8 * MT_RANGE_THREADS) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = s4[i + j * MT_RANGE_THREADS];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lo = fminf(lo, fminf(fminf(v[j].x, v[j].y), fminf(v[j].z, v[j].w)));
                hi = fmaxf(hi, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
            }
        }
        for (; i < n4; i += MT_RANGE_THREADS) {
            const float4 v = s4[i];
            lo = fminf(lo, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
            hi = fmaxf(hi, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
    } else {
        const float scale = (float)R / (float)Ro;
        const int n = Ro * Ro;
        for (int ch = 0; ch < 3; ++ch) {
            const float* __restrict__ p = src + (size_t)ch * R * R;
            for (int i = t; i < n; i += MT_RANGE_THREADS) {
                const int y = i / Ro, x = i - y * Ro;
                const float v = cf_bicubic_tap(p, R, scale, y, x, 0);
                lo = fminf(lo, v); hi = fmaxf(hi, v);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo = fminf(lo, __shfl_down(lo, off, 64)); hi = fmaxf(hi, __shfl_down(hi, off, 64)); }
    if ((t & 63) == 0) { red[0][t >> 6] = lo; red[1][t >> 6] = hi; }
    __syncthreads();
    if (t == 0) {
        for (int j = 1; j < MT_RANGE_THREADS / 64; ++j) { lo = fminf(lo, red[0][j]); hi = fmaxf(hi, red[1][j]); }
        range_out[face * 2] = lo; range_out[face * 2 + 1] = hi;
    }
}

}  // namespace hd
