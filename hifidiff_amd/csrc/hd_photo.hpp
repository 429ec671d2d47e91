// hd_photo.hpp — the two ends that touch a photograph: head boxes of uint8 photos in (the reference's ln_face, dataset_kface.py:86-98:
// crop -> resize((lr, lr), BICUBIC) -> resize((res, res), BICUBIC) -> to_tensor) and restored faces back out (resize to the box, feathered
// blend).  Both are Pillow's 8-bit two-pass antialiased bicubic resize; include/hifidiff_hip.h (hd_face_ingest, hd_face_paste) states the
// rule and is the contract.  The weights are 22-bit integers made from float64 coefficients, the sums are int32, so results equal
// Pillow's byte for byte -- as long as the float64 code below is not contracted into fused multiply-adds (one fma in ph_bicubic or in
// `center` moves a weight by one): every function that touches a double carries `#pragma clang fp contract(off)`.
//
// One kernel does every resize: a workgroup owns a band of PH_MAX_ROWS or fewer output rows by PH_MAX_COLS or fewer output columns of one
// face (ph_tile; integer arithmetic shared with the host, which sizes the grid with it), computes the weights of its columns and rows
// in fp64 into LDS, runs the horizontal pass over the source rows its band needs into a uint8 LDS intermediate (clipped and rounded, as
// Pillow's), then the vertical pass from LDS, then the epilogue.  Nothing but integers depends on the tiling, so a face's bytes do not.
// The host's boxes reach the kernel as launch arguments, PH_CHUNK faces per launch: no table in global memory, no host memory read
// after the call returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hd {

constexpr int PH_THREADS = 256;
constexpr int PH_CHUNK = 64;              // faces per launch: 64 * sizeof(PhJob) = 3 KiB of launch arguments
constexpr int PH_BITS = 22;               // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int PH_MAX_SIDE = 2048;
constexpr int PH_MAX_COLS = 512, PH_MAX_ROWS = 32;
constexpr int PH_HT_INTS = 4608;          // horizontal weights of a band (>= the 2049 taps of 512 -> 1)
constexpr int PH_VT_INTS = 2304;          // vertical weights of a band (likewise)
constexpr int PH_INTER_BYTES = 32768;     // the band's intermediate rows (>= 2048 rows of one pixel)

struct PhJob {
    long long src_off;                    // bytes from the source base to the region's first pixel (HWC, 3 bytes a pixel)
    long long dst_off;                    // likewise in the uint8 destination
    int src_stride, dst_stride;           // bytes per row
    int iw, ih, ow, oh;
    int face, pad;                        // the face's index in the fp32 output
};
struct PhChunk { PhJob j[PH_CHUNK]; };

struct PhTile { int ksh, ksv, C, R, nrows; };

// an upper bound of the taps of one output sample: Pillow's ksize = 2 * ceil(support) + 1, support = 2 * max(in / out, 1)
__host__ __device__ inline int ph_ksize(int in, int out) {
    if (in == out) return 1;                                          // a skipped pass: one tap of weight 1
    const int m = in > out ? in : out;
    return 2 * ((2 * m + out - 1) / out) + 1;
}
// source rows that R consecutive output rows can touch, at most
__host__ __device__ inline int ph_rows(int ih, int oh, int ksv, int R) {
    const int n = ksv + 1 + ((R - 1) * ih + oh - 1) / oh;
    return n < ih ? n : ih;
}
__host__ __device__ inline int ph_min(int a, int b) { return a < b ? a : b; }
// the band a workgroup owns: C columns by R rows, sized so that the weights and the intermediate fit their LDS arrays
__host__ __device__ inline PhTile ph_tile(int iw, int ih, int ow, int oh) {
    PhTile t;
    t.ksh = ph_ksize(iw, ow); t.ksv = ph_ksize(ih, oh);
    t.C = ph_min(ph_min(ow, PH_MAX_COLS), ph_min(PH_HT_INTS / t.ksh, PH_INTER_BYTES / (3 * ph_rows(ih, oh, t.ksv, 1))));
    t.R = ph_min(ph_min(oh, PH_MAX_ROWS), PH_VT_INTS / t.ksv);
    while (t.R > 1 && ph_rows(ih, oh, t.ksv, t.R) * t.C * 3 > PH_INTER_BYTES) --t.R;
    t.nrows = ph_rows(ih, oh, t.ksv, t.R);
    return t;
}
__host__ __device__ inline int ph_blocks(int iw, int ih, int ow, int oh) {
    const PhTile t = ph_tile(iw, ih, ow, oh);
    return ((ow + t.C - 1) / t.C) * ((oh + t.R - 1) / t.R);
}

__device__ __forceinline__ double ph_bicubic(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output sample xx of an axis: K[0..n) are the weights of source samples
// xmin .. xmin + n - 1
__device__ __forceinline__ void ph_coeffs(int in, int out, int xx, int* K, int& xmin_out, int& n_out) {
#pragma clang fp contract(off)
    if (in == out) { K[0] = 1 << PH_BITS; xmin_out = xx; n_out = 1; return; }
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += ph_bicubic((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < n; ++x) {
        double k = ph_bicubic((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) k /= ww;
        K[x] = (int)(k * (double)(1 << PH_BITS) + (k < 0 ? -0.5 : 0.5));
    }
    xmin_out = xmin; n_out = n;
}

__device__ inline int ph_clip8(int acc) {
    const int v = acc >> PH_BITS;
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// BLEND = false: the band's bytes go to dst8 (if given) and, as byte / 255, to plane c of face j.face of dstf [B,3,oh,ow] (if given).
// BLEND = true:  they are blended into dst8 with the feathered edge weight of hd_face_paste.
template <bool BLEND>
__global__ __launch_bounds__(PH_THREADS) void photo_resize_kernel(const PhChunk jobs, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst8,
                                                                   float* __restrict__ dstf, int feather) {
    __shared__ int ht[PH_HT_INTS];
    __shared__ int vt[PH_VT_INTS];
    __shared__ int hb[2 * PH_MAX_COLS];
    __shared__ int vb[2 * PH_MAX_ROWS];
    __shared__ uint8_t inter[PH_INTER_BYTES];
    const PhJob& j = jobs.j[blockIdx.y];
    const int iw = j.iw, ih = j.ih, ow = j.ow, oh = j.oh;
    const PhTile t = ph_tile(iw, ih, ow, oh);
    const int ncb = (ow + t.C - 1) / t.C, nrb = (oh + t.R - 1) / t.R;
    if ((int)blockIdx.x >= ncb * nrb) return;                          // the grid is sized for the chunk's largest face
    const int cb = blockIdx.x % ncb, rb = blockIdx.x / ncb;
    const int x0 = cb * t.C, nx = ph_min(t.C, ow - x0);
    const int y0 = rb * t.R, ny = ph_min(t.R, oh - y0);
    const int tid = threadIdx.x;

    for (int i = tid; i < nx + ny; i += PH_THREADS) {
        int first, n;
        if (i < nx) { ph_coeffs(iw, ow, x0 + i, ht + i * t.ksh, first, n); hb[2 * i] = first; hb[2 * i + 1] = n; }
        else { const int r = i - nx; ph_coeffs(ih, oh, y0 + r, vt + r * t.ksv, first, n); vb[2 * r] = first; vb[2 * r + 1] = n; }
    }
    __syncthreads();
    const int ylo = vb[0];
    int yhi = ylo;
    for (int r = 0; r < ny; ++r) { const int e = vb[2 * r] + vb[2 * r + 1]; yhi = e > yhi ? e : yhi; }
    const int nr = ph_min(yhi - ylo, t.nrows);                         // ph_rows bounds it; the clamp keeps LDS writes inside `inter` regardless

    const uint8_t* s = src + j.src_off;
    for (int i = tid; i < nr * nx; i += PH_THREADS) {
        const int r = i / nx, x = i - r * nx;
        const int n = hb[2 * x + 1];
        const int* K = ht + x * t.ksh;
        const uint8_t* p = s + (long long)(ylo + r) * j.src_stride + hb[2 * x] * 3;
        int a0 = 1 << (PH_BITS - 1), a1 = a0, a2 = a0;
        for (int k = 0; k < n; ++k) {
            const int w = K[k];
            a0 += p[3 * k] * w; a1 += p[3 * k + 1] * w; a2 += p[3 * k + 2] * w;
        }
        uint8_t* q = inter + i * 3;
        q[0] = (uint8_t)ph_clip8(a0); q[1] = (uint8_t)ph_clip8(a1); q[2] = (uint8_t)ph_clip8(a2);
    }
    __syncthreads();

    for (int i = tid; i < ny * nx; i += PH_THREADS) {
        const int r = i / nx, x = i - r * nx;
        const int ymin = vb[2 * r] - ylo;
        const int n = ph_min(vb[2 * r + 1], nr - ymin);
        const int* K = vt + r * t.ksv;
        const uint8_t* p = inter + (ymin * nx + x) * 3;
        int a0 = 1 << (PH_BITS - 1), a1 = a0, a2 = a0;
        for (int k = 0; k < n; ++k) {
            const int w = K[k];
            a0 += p[0] * w; a1 += p[1] * w; a2 += p[2] * w;
            p += nx * 3;
        }
        const int v[3] = {ph_clip8(a0), ph_clip8(a1), ph_clip8(a2)};
        const int X = x0 + x, Y = y0 + r;
        if (BLEND) {
            int m = 256;
            if (feather > 0) {
                const int d = ph_min(ph_min(X, ow - 1 - X), ph_min(Y, oh - 1 - Y));
                m = ph_min(256, ((2 * d + 1) * 256) / (2 * feather));
            }
            uint8_t* o = dst8 + j.dst_off + (long long)Y * j.dst_stride + X * 3;
            for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((o[c] * (256 - m) + v[c] * m + 128) >> 8);
        } else {
            if (dst8) {
                uint8_t* o = dst8 + j.dst_off + (long long)Y * j.dst_stride + X * 3;
                for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
            }
            if (dstf) {
                float* o = dstf + ((long long)j.face * 3 * oh + Y) * ow + X;
                for (int c = 0; c < 3; ++c) o[(long long)c * oh * ow] = (float)v[c] / 255.0f;      // to_tensor: a true fp32 division
            }
        }
    }
}

// faces fp32 [B,3,R,R] -> uint8 [B,R,R,3]: torchvision save_image's clamp(floor(x * 255 + 0.5), 0, 255), the multiply and the add rounded
// separately; NaN -> 0
__global__ __launch_bounds__(PH_THREADS) void photo_quantize_kernel(const float* __restrict__ faces, uint8_t* __restrict__ q8, int res, long long npix) {
    const long long i = (long long)blockIdx.x * PH_THREADS + threadIdx.x;
    if (i >= npix) return;
    const long long plane = (long long)res * res, f = i / plane, p = i - f * plane;
    for (int c = 0; c < 3; ++c) {
        const float x = faces[(f * 3 + c) * plane + p];
        const float v = floorf(__fadd_rn(__fmul_rn(x, 255.0f), 0.5f));
        q8[i * 3 + c] = (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);    // fmaxf(NaN, 0) = 0
    }
}

}  // namespace hd
