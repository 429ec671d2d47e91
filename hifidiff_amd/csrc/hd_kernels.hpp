// hd_kernels.hpp — the non-GEMM kernels of the refiner path (gfx950).  All activations are
// channels-last fp32 [rows = (face, y, x)][C] unless stated; see DESIGN.md for the buffer map.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hd_gemm.hpp"

namespace hd {

// Device-resident loop state read by the captured per-step graph (so one graph serves every step).
struct StepState {
    int step;                 // index into the schedule; incremented by the first kernel of a step
    int n_steps;              // length of the schedule (0: single evaluation)
    const float* noise;       // [n_steps][n_elems] or NULL -> Philox
    unsigned long long seed;
    // multistep schedules (hd_sample_multistep): this chain's x0 history [B_chain,4,L,L] and the [n_steps] table of the
    // history coefficient c7.  NULL: single-step schedule (hd_sample) -- the update reads and writes nothing more.
    float* x0_hist;
    const float* c7;
    // per-face schedule positions (hd_sample_rows*): this chain's [B_chain] start rows r_f; face f is evaluated at row r_f + step
    // and held (nothing written) from row n_steps on.  hist_first: a face's first row is first-order (no history before it: h := x0).
    // NULL for hd_sample / hd_sample_multistep, whose launches never read these fields.
    const int* start_rows;
    int hist_first;
    // per-face keys and resumption (hd_sample_faces*; NULL for every other entry): this chain's [B_chain] Philox keys -- face f's z at
    // row k, element e of the face is Philox(face_seeds[f]; k, e) -- and [B_chain] first-order flags that replace hist_first per face.
    const unsigned long long* face_seeds;
    const int* face_first;
    // masked sampling (hd_mask_faces; NULL while no face of the batch has a mask): this chain's [B_chain,L,L] masks m in [0,1] (1: resample,
    // 0: keep), the [B_chain,4,L,L] known latents and their fixed noise, and [B_chain] flags -- only a face whose flag is set is blended
    const float* mask;
    const float* mask_known;
    const float* mask_noise;
    const int* mask_on;
    // per-face schedule spans (hd_sample_spans; NULL: 0 and n_steps for every face): this chain's [B_chain] rows begin_f / end_f.  Face f's
    // schedule is rows [begin_f, end_f) of the table: it is held from row end_f on, its FiLM row and its mask blend stop there, and its
    // Philox counter is k - begin_f.  Read by the per-face launches only.
    const int* begin_rows;
    const int* end_rows;
    // progress previews (hd_preview_config; all NULL / 0 while previews are off): this chain's [B_chain,4,L,L] plane of the latest denoised
    // estimate p = x0 (a masked face: m*x0 + (1 - m)*known), pv_snaps snapshot planes with a stride of pv_batch faces -- row j of a face's
    // own schedule (j = k - begin_f) with (j + 1) % pv_every == 0 also goes to plane (j + 1)/pv_every - 1 -- and the rows: pv_row[f] is the
    // table row k of face f's latest estimate, pv_row[(1 + s)*pv_batch + f] that of its snapshot s.  A held face writes none of them.
    float* pv_x0;
    int* pv_row;
    float* pv_snap;
    int pv_every, pv_snaps, pv_batch;
    // low-pass fidelity guidance (hd_guide_faces; all NULL while guidance is off or no face of the batch is guided): this chain's
    // [B_chain,4,L,L] stored LP_N(g_f) and, per face, the weight w_f (0: not guided), the block size N_f and the window [j0_f, j1_f) of rows
    // of the face's own schedule (j = k - begin_f) on which it is guided.  A guided row's latent update is left to guided_update_kernel.
    const float* gd_lp;
    const float* gd_w;
    const int* gd_n;
    const int* gd_j0;
    const int* gd_j1;
};

// ----------------------------------------------------------------------------------- weight packing
// fp32 conv/linear weight [N][Cin][KH][KW] -> bf16 MFMA B-fragment order [nt][kstep][lane][8] with
// k = tap*Cin_pad + c, optional per-output-channel scale (folded BatchNorm), optional centre-tap
// slice (3x3 conv on a 1x1 map: only the centre tap ever sees data), optional output permutation
// n' = pos*Cg + c  <-  n = c*S2 + pos  (idc_conv: (B,2048*s*s,1,1) viewed as (B,2048,s,s), model.py:246).
struct PackP {
    const float* src; uint4* dst;
    int N, Cin, Cin_pad, KH, KW, ntaps, centre_only, S2, Kp, nt_total;
    const float* nscale;
};
static __global__ void pack_weight_kernel(const PackP p) {
    const int ksteps = p.Kp >> 4;
    const size_t total = (size_t)p.nt_total * ksteps * 64;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e & 63);
        const size_t tk = e >> 6;
        const int ks = (int)(tk % ksteps), nt = (int)(tk / ksteps);
        const int np = nt * 32 + (lane & 31);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = ks * 16 + 8 * (lane >> 5) + j;
            const int tap = k / p.Cin_pad, c = k - tap * p.Cin_pad;
            float x = 0.f;
            if (np < p.N && tap < p.ntaps && c < p.Cin) {
                int n = np;
                if (p.S2 > 1) { const int cg = p.N / p.S2; n = (np % cg) * p.S2 + np / cg; }
                int ky, kx;
                if (p.centre_only) { ky = p.KH >> 1; kx = p.KW >> 1; }
                else { ky = tap / p.KW; kx = tap - ky * p.KW; }
                x = p.src[(((size_t)n * p.Cin + c) * p.KH + ky) * p.KW + kx];
                if (p.nscale) x *= p.nscale[n];
            }
            v[j] = x;
        }
        p.dst[e] = pack8(v);
    }
}

// 1x1 conv weight [N][K] fp32 -> bf16 in the A-operand order of v_mfma_f32_16x16x32_bf16 (hd_xcd2.hpp: the WEIGHTS are the A operand,
// 16 output channels x 32 k per fragment): dst[(mb * K/32 + ks) * 64 + lane] = W[mb*16 + (lane & 15)][ks*32 + 8*(lane >> 4) .. + 7]
static __global__ void pack_weight16_kernel(const float* __restrict__ src, uint4* __restrict__ dst, int N, int K) {
    const int ksteps = K >> 5;
    const size_t total = (size_t)(N >> 4) * ksteps * 64;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e & 63);
        const size_t tk = e >> 6;
        const int ks = (int)(tk % ksteps), mb = (int)(tk / ksteps);
        const float* q = src + (size_t)(mb * 16 + (lane & 15)) * K + ks * 32 + 8 * (lane >> 4);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = q[j];
        dst[e] = pack8(v);
    }
}

// depthwise weights [2C][9] -> tap-major [9][2C]: the fused conv1 epilogue reads them with one coalesced load per tap
static __global__ void dw_weight_layout_kernel(const float* __restrict__ w, float* __restrict__ wT, int n2c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2c * 9) return;
    const int ch = i / 9, t = i - ch * 9;
    wT[(size_t)t * n2c + ch] = w[i];
}

// ----------------------------------------------------------------------------------- intro / ending
// intro: Conv2d(4,128,3,pad 1) on the NCHW latent -> channels-last fp32 + bf16 copy + LayerNorm partial
// (models/denoiser/model.py:159-167,235).  fp32 FMA (K = 36 is too small for MFMA).  One wave per run of 16
// pixels of an image row, lanes over output channels (co = lane, lane + 64): the lane's 72 weights stay in
// registers (wT is the weight re-laid as [ci*9 + tap][co]: coalesced loads), the 3 x 18 x 4 latent patch of
// the run sits in LDS and is read as broadcasts.  The first thread also advances the loop's step counter.
static __global__ void intro_weight_layout_kernel(const float* __restrict__ w, float* __restrict__ wT) {    // w[co][36] -> wT[36][co]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 128 * 36) return;
    const int co = i / 36;
    wT[(i - co * 36) * 128 + co] = w[i];
}
// PXS: pixels per wave.  One wave per run of 16 pixels gave one wave per SIMD at the benchmark batch (1024 waves): a serial
// chain of LDS reads, FMAs, DPP reductions and stores with nothing to overlap it; runs of 8 put two waves on a SIMD
// (measured per launch, runs of 16 / 8 / 4 / 2: intro 13.4 / 9.5 / 9.5 / 10.8 us, ending 11.8 / 8.8 / 9.8 / 12.8 us).  From
// kLongRunRows rows on (latent 32 at batch 64) runs of 16 already give four waves per SIMD and re-read fewer halo columns.
constexpr int kIntroPx = 8, kEndingPx = 8, kLongRunRows = 32768;
template <int PXS>
__global__ __launch_bounds__(256) void intro_conv_kernel(const float* __restrict__ lat, const float* __restrict__ wT,
                                                          const float* __restrict__ b, float* __restrict__ out,
                                                          unsigned short* __restrict__ out16, float2* __restrict__ stats, int B, int L,
                                                          StepState* st, int advance) {
    __shared__ float patch[4][4][3][PXS + 4];                            // [wave][ci][row][x0-1 .. x0+PXS] (+pad)
    if (advance && blockIdx.x == 0 && threadIdx.x == 0) st->step += 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nseg = B * L * (L / PXS);
    const int seg = blockIdx.x * 4 + wave;
    if (seg >= nseg) return;                                             // whole wave; no block-wide barrier below
    const int spr = L / PXS;
    const int bb = seg / (L * spr), rem = seg - bb * L * spr, y = rem / spr, x0 = (rem - y * spr) * PXS;
    for (int i = lane; i < 4 * 3 * (PXS + 2); i += 64) {
        const int ci = i / (3 * (PXS + 2)), r = (i - ci * 3 * (PXS + 2)) / (PXS + 2), xx = i - ci * 3 * (PXS + 2) - r * (PXS + 2);
        const int yy = y + r - 1, x = x0 + xx - 1;
        patch[wave][ci][r][xx] = (yy >= 0 && yy < L && x >= 0 && x < L) ? lat[((size_t)(bb * 4 + ci) * L + yy) * L + x] : 0.f;
    }
    float wl[36][2];
#pragma unroll
    for (int r = 0; r < 36; ++r) { wl[r][0] = wT[r * 128 + lane]; wl[r][1] = wT[r * 128 + lane + 64]; }
    const float b0 = b[lane], b1 = b[lane + 64];
    __builtin_amdgcn_wave_barrier();
    const size_t row0 = ((size_t)bb * L + y) * L + x0;
#pragma unroll
    for (int px = 0; px < PXS; ++px) {
        float a0 = b0, a1 = b1;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float v = patch[wave][ci][r][px + k];
                    a0 += v * wl[ci * 9 + r * 3 + k][0];
                    a1 += v * wl[ci * 9 + r * 3 + k][1];
                }
        const size_t o = (row0 + px) * 128;
        out[o + lane] = a0; out[o + lane + 64] = a1;
        out16[o + lane] = f32_to_bf16_bits(a0); out16[o + lane + 64] = f32_to_bf16_bits(a1);
        // LayerNorm statistics of the 128-channel row for the first block's norm1: (mean, M2), one partial
        const float s1 = wave_sum(a0 + a1), s2 = wave_sum(a0 * a0 + a1 * a1);
        const float mean = s1 * (1.0f / 128.0f);
        if (lane == 0) stats[row0 + px] = make_float2(mean, fmaxf(s2 - s1 * mean, 0.f));
    }
}

// ending: Conv2d(128,4,3,pad 1) channels-last fp32 -> NCHW eps (models/denoiser/model.py:168-176,261), and --
// in the sampling loop -- the scheduler update of the same elements (sched_update below) plus the staging of
// the next step's FiLM row, so the step ends with this launch.
// One wave per run of 16 pixels of an image row; lanes over input channels (ci = lane, lane + 64).  The lane's
// 72 weights stay in registers for the whole run (wT is the weight re-laid as [tap][co][ci], so these are
// coalesced loads) and the 3x3 window slides along x (one new column = 6 loads per pixel).  The 64 per-lane
// partial sums (16 pixels x 4 outputs) are reduced over the wave with DPP.
struct SchedArgs {
    float* lat;                   // chain-local latents x_t -> x_{t-1} (NULL: plain eps evaluation)
    const float* coef;            // [n_steps][7]
    const StepState* st;
    int elem0, n_total;           // position of this chain's elements inside the whole batch (noise indexing)
    const float* film_table; float* film_cur; int film_total;
};
__device__ __forceinline__ float philox_normal(unsigned long long seed, unsigned step, unsigned idx);
// x0 = clamp((x - c0*eps)/c1, +-c2);  x <- c3*x0 + c4*x + c5*eps + c6*z      (hd_schedule in the C-ABI)
// and, with a history (st->x0_hist != NULL, hd_schedule_ms):  x <- ... + c7*h;  h <- x0.  gi: element index in the whole
// batch (noise), li: in this chain (latents, history).  h is read only when c7 != 0, so an unwritten history never enters
// step 0; lane-private (same element read and written by one lane).
// PF (per-face rows, hd_sample_rows*): `step` is the face's row k, and `first` (k == r_f with StepState::hist_first) makes that row
// first-order (h := x0, see below).  PF = false is the code of hd_sample / hd_sample_multistep.
// face f's start row (the pointer is read from device memory: a global pointer, as in sched_update)
__device__ __forceinline__ int st_row(const StepState* st, int f) { return ((const __attribute__((address_space(1))) int*)st->start_rows)[f]; }
// face f's span of the table (hd_sample_spans), or the whole table: the row its noise counter starts from, and the row it is held from
__device__ __forceinline__ int st_begin(const StepState* st, int f) { return st->begin_rows ? ((const __attribute__((address_space(1))) int*)st->begin_rows)[f] : 0; }
__device__ __forceinline__ int st_end(const StepState* st, int f) { return st->end_rows ? ((const __attribute__((address_space(1))) int*)st->end_rows)[f] : st->n_steps; }
// is face f's row k its first-order row: k == r_f and (per face, hd_sample_faces_multistep) face_first[f] or (hd_sample_rows*) hist_first
__device__ __forceinline__ bool st_first(const StepState* st, int f, int k, int r) {
    return k == r && (st->face_first ? ((const __attribute__((address_space(1))) int*)st->face_first)[f] != 0 : st->hist_first != 0);
}
// f is the chain-local face and ef the element's index inside the face (PF: the per-face Philox key's counter, hd_sample_faces*)
// Masked faces (st->mask != NULL and mask_on[f], hd_mask_faces; ll = L*L): the inpainting blend of the updated value r with the known latent
// re-noised to the next row, x <- m*r + (1 - m)*(b0*known + b1*nz), (b0, b1) = (c1, c0) of row step + 1 -- the row's signal and noise scale
// -- and (1, 0) on the last row.  In this order m == 1 gives r and m == 0 gives kn exactly, contracted or not.  The history keeps the
// unblended x0.  f is uniform over the wave (a run lies in one face), so the branch is too.
// PF with spans (hd_sample_spans): the last row is that of the face's span (step + 1 >= end_f), and the Philox counter is the row inside the
// span, step - begin_f -- a request's z does not depend on where its schedule sits in the table; an explicit noise tensor keeps the absolute row.
// Previews (st->pv_x0 != NULL, hd_preview_config): the estimate p -- x0, blended with the known latent of a masked face in the order of the
// blend above, so m == 1 gives x0 and m == 0 gives known exactly -- is stored as one more output (StepState::pv_*).  NULL: nothing is read or written.
// is face f guided on row j of its own schedule (hd_guide_faces): uniform over a run, a workgroup of the fused ending launch and a plane
__device__ __forceinline__ bool st_guided(const StepState* st, int f, int j) {
    if (!st->gd_w) return false;
    if (((const __attribute__((address_space(1))) float*)st->gd_w)[f] == 0.f) return false;
    return j >= ((const __attribute__((address_space(1))) int*)st->gd_j0)[f] && j < ((const __attribute__((address_space(1))) int*)st->gd_j1)[f];
}
// The update in two halves.  sched_x0: the denoised estimate of the element.  sched_from_x0: everything after it -- the new latent from an
// x0 (the row's own, or the guided x0g of guided_update_kernel), the history, the mask blend and the preview store.  sched_update is the
// two in a row: what the ending kernels run for every face that is not guided on this row.
__device__ __forceinline__ float sched_x0(float xv, float e, const float* c) {
    float x0 = (xv - c[0] * e) / c[1];
    x0 = fminf(fmaxf(x0, -c[2]), c[2]);
    return x0;
}
template <bool PF = false>
__device__ __forceinline__ float sched_from_x0(float x0, float xv, float e, const float* c, const StepState* st, int step, size_t gi, int n_total,
                                              size_t li, bool first, int f, unsigned ef, int ll) {
    float c3 = c[3];
    // a face's first row of a multistep call has no history: the row is taken first-order, h := x0 -- the x0 coefficient becomes c3 + c7
    // (c3 = g (1 + k'), c7 = -g k' in a second-order row: their sum is the first-order g)
    if (PF && first && st->x0_hist) c3 += ((const __attribute__((address_space(1))) float*)st->c7)[step];
    float r = c3 * x0 + c[4] * xv + c[5] * e;
    if (c[6] != 0.f) {
        // (the pointer is read from device memory: say that it is a global pointer, or the load is a flat load with a full wait)
        float z;
        if (st->noise) z = ((const __attribute__((address_space(1))) float*)st->noise)[(size_t)step * n_total + gi];
        else if (PF && st->face_seeds) z = philox_normal(((const __attribute__((address_space(1))) unsigned long long*)st->face_seeds)[f], (unsigned)(step - st_begin(st, f)), ef);
        else z = philox_normal(st->seed, (unsigned)(PF ? step - st_begin(st, f) : step), (unsigned)gi);
        r += c[6] * z;
    }
    if (st->x0_hist) {
        __attribute__((address_space(1))) float* h = (__attribute__((address_space(1))) float*)st->x0_hist;
        float c7 = ((const __attribute__((address_space(1))) float*)st->c7)[step];
        if (PF && first) c7 = 0.f;
        if (c7 != 0.f) r += c7 * h[li];
        h[li] = x0;
    }
    if (st->mask && ((const __attribute__((address_space(1))) int*)st->mask_on)[f] != 0) {
        const bool last = step + 1 >= (PF ? st_end(st, f) : st->n_steps);
        const float b0 = last ? 1.f : c[7 + 1], b1 = last ? 0.f : c[7 + 0];
        const float m = ((const __attribute__((address_space(1))) float*)st->mask)[(size_t)f * ll + (ef & (unsigned)(ll - 1))];
        const float kn = b0 * ((const __attribute__((address_space(1))) float*)st->mask_known)[li] +
                         b1 * ((const __attribute__((address_space(1))) float*)st->mask_noise)[li];
        r = m * r + (1.f - m) * kn;
    }
    if (st->pv_x0) {                                       // previews on: uniform over the launch
        float p = x0;
        if (st->mask && ((const __attribute__((address_space(1))) int*)st->mask_on)[f] != 0) {
            const float m = ((const __attribute__((address_space(1))) float*)st->mask)[(size_t)f * ll + (ef & (unsigned)(ll - 1))];
            p = m * x0 + (1.f - m) * ((const __attribute__((address_space(1))) float*)st->mask_known)[li];
        }
        ((__attribute__((address_space(1))) float*)st->pv_x0)[li] = p;
        const int j1 = step - (PF ? st_begin(st, f) : 0) + 1, s = j1 / st->pv_every - 1;      // wave-uniform
        const bool snap = j1 % st->pv_every == 0 && s < st->pv_snaps;
        if (snap) ((__attribute__((address_space(1))) float*)st->pv_snap)[(size_t)s * st->pv_batch * 4 * ll + li] = p;
        if (ef == 0) {                                     // one lane of the face
            __attribute__((address_space(1))) int* rows = (__attribute__((address_space(1))) int*)st->pv_row;
            rows[f] = step;
            if (snap) rows[(size_t)(1 + s) * st->pv_batch + f] = step;
        }
    }
    return r;
}
template <bool PF = false>
__device__ __forceinline__ float sched_update(float xv, float e, const float* c, const StepState* st, int step, size_t gi, int n_total,
                                             size_t li, bool first, int f, unsigned ef, int ll) {
    return sched_from_x0<PF>(sched_x0(xv, e, c), xv, e, c, st, step, gi, n_total, li, first, f, ef, ll);
}

// Low-pass fidelity guidance (hd_guide_faces).  LP_N of one L x L plane: the mean over each of the P x P blocks of N x N elements (P = L/N),
// upsampled bilinearly back to L x L with align_corners = False -- for output index i in either axis s = max((i + 0.5)/N - 0.5, 0),
// i0 = floor(s), i1 = min(i0 + 1, P - 1), frac = s - i0.  N = 1 returns the plane bit for bit (frac = 0), N = L its mean everywhere.
// lp_block_means: the plane sits in LDS (pl); rs [L][P] takes the sums of the N-runs of every row, bm [P][P] the block means (a block's
// N row sums in row order).  Called by the whole workgroup; bm is complete when it returns.
__device__ __forceinline__ void lp_block_means(const float* pl, float* rs, float* bm, int L, int N) {
    const int P = L / N;
    for (int i = threadIdx.x; i < L * P; i += blockDim.x) {
        const int y = i / P, bx = i - y * P;
        float s = 0.f;
        for (int k = 0; k < N; ++k) s += pl[y * L + bx * N + k];
        rs[i] = s;
    }
    __syncthreads();
    const float inv = 1.f / (float)(N * N);
    for (int i = threadIdx.x; i < P * P; i += blockDim.x) {
        const int by = i / P, bx = i - by * P;
        float s = 0.f;
        for (int k = 0; k < N; ++k) s += rs[(by * N + k) * P + bx];
        bm[i] = s * inv;
    }
    __syncthreads();
}
__device__ __forceinline__ float lp_bilinear(const float* bm, int P, int N, int y, int x) {
    const float sy = fmaxf(((float)y + 0.5f) / (float)N - 0.5f, 0.f), sx = fmaxf(((float)x + 0.5f) / (float)N - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx, y1 = min(y0 + 1, P - 1), x1 = min(x0 + 1, P - 1);
    const float fy = sy - (float)y0, fx = sx - (float)x0;
    const float top = (1.f - fx) * bm[y0 * P + x0] + fx * bm[y0 * P + x1];
    const float bot = (1.f - fx) * bm[y1 * P + x0] + fx * bm[y1 * P + x1];
    return (1.f - fy) * top + fy * bot;
}
constexpr int kGuideMaxL = 64;                            // a plane of 64 x 64 fp32 is 16 KB: plane + row sums + block means = 48 KB of LDS
inline size_t guide_lds_bytes(int L) { return (size_t)3 * L * L * sizeof(float); }

// The guided half of a step, launched right after the ending launch while guidance is switched on (hd_guide_config): one workgroup per
// (chain-local face, channel) plane.  The ending launch has stored eps and left the latents of a face that is guided on this row alone;
// here x0 of the plane goes to LDS, is low-passed, pulled towards the stored LP_N(g) by w -- x0g = x0 + w (LP_N(g) - LP_N(x0)) -- and the
// "from x0" half of the update runs on x0g with the element indices of the ending kernels (gi, li, ef, the Philox counters).  eps is
// re-derived from x0g (e' = (x - c1 x0g)/c0) where the row uses it (c5 != 0).  A workgroup whose face is not guided on this row, or is
// held, exits at once; a plane belongs to one workgroup, so nothing is synchronised across workgroups.  The step counter has been advanced
// by the intro.  PF: the per-face form (hd_sample_rows* / _faces* / _spans).
struct GuideArgs {
    float* lat; const float* eps;     // chain-local [B_chain,4,L,L]
    const float* coef;                // [n_steps][7]
    const StepState* st;
    int elem0, n_total, L;
};
template <bool PF>
__global__ __launch_bounds__(256) void guided_update_kernel(const GuideArgs g) {
    extern __shared__ float guide_lds[];
    const StepState* st = g.st;
    if (!st->gd_w) return;
    const int f = blockIdx.x >> 2, L = g.L, ll = L * L;
    const int step = st->step;
    int k = step, r = 0, j = step;
    if (PF) {
        r = st_row(st, f); k = r + step;
        if (k >= st_end(st, f)) return;                   // held
        j = k - st_begin(st, f);
    }
    if (!st_guided(st, f, j)) return;
    const float w = ((const __attribute__((address_space(1))) float*)st->gd_w)[f];
    const int N = ((const __attribute__((address_space(1))) int*)st->gd_n)[f], P = L / N;
    const __attribute__((address_space(1))) float* lpg = (const __attribute__((address_space(1))) float*)st->gd_lp;
    const float* c = g.coef + (size_t)k * 7;
    float *pl = guide_lds, *rs = pl + ll, *bm = rs + ll;
    const size_t o0 = (size_t)blockIdx.x * ll;            // (f * 4 + channel) * L * L: NCHW
    for (int i = threadIdx.x; i < ll; i += blockDim.x) pl[i] = sched_x0(g.lat[o0 + i], g.eps[o0 + i], c);
    __syncthreads();
    lp_block_means(pl, rs, bm, L, N);
    const bool first = PF ? st_first(st, f, k, r) : false;
    for (int i = threadIdx.x; i < ll; i += blockDim.x) {
        const size_t o = o0 + i;
        const int y = i / L, x = i - y * L;
        const float xv = g.lat[o];
        float e = g.eps[o];
        const float x0g = pl[i] + w * (lpg[o] - lp_bilinear(bm, P, N, y, x));
        if (c[5] != 0.f) e = (xv - c[1] * x0g) / c[0];
        g.lat[o] = sched_from_x0<PF>(x0g, xv, e, c, st, k, (size_t)g.elem0 + o, g.n_total, o, first, f, (unsigned)(o - (size_t)f * 4 * ll), ll);
    }
}
static __global__ void ending_weight_layout_kernel(const float* __restrict__ w, float* __restrict__ wT) {   // w[co][ci][tap] -> wT[tap][co][ci]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * 128 * 9) return;
    const int co = i / (128 * 9), r = i - co * 128 * 9, ci = r / 9, tap = r - ci * 9;
    wT[(tap * 4 + co) * 128 + ci] = w[i];
}
// PF (hd_sample_rows*): film_cur is the chain's [B][film_total] staging buffer and every face has its own row (StepState::start_rows);
// the trailing workgroups stage ceil(film_total / 1024) float4 pieces of 256 threads x 4 per face (film_stage_pieces): grid = conv workgroups
// + B * film_stage_pieces(film_total).
__host__ __device__ constexpr int film_stage_pieces(int film_total) { return (film_total / 4 + 1023) / 1024; }
template <int PXS, bool PF = false>
__global__ __launch_bounds__(256) void ending_conv_kernel(const float* __restrict__ X, const float* __restrict__ wT,
                                                           const float* __restrict__ b, float* __restrict__ eps,
                                                           int B, int L, const SchedArgs sa) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nseg = B * L * (L / PXS);                                  // runs of PXS pixels (L is a multiple of 16)
    const int nb_conv = (nseg + 3) >> 2;
    if (PF && (int)blockIdx.x >= nb_conv) {
        // per face: row r_f + step + 1 of the table while the face's schedule has it (a held face keeps its last row: its eps is discarded)
        const int t = (int)blockIdx.x - nb_conv, np = film_stage_pieces(sa.film_total), f = t / np, piece = t - f * np;
        if (f >= B) return;
        const int row = st_row(sa.st, f) + sa.st->step + 1;
        if (row >= st_end(sa.st, f)) return;
        const float4* src = reinterpret_cast<const float4*>(sa.film_table + (size_t)row * sa.film_total);
        float4* dst = reinterpret_cast<float4*>(sa.film_cur + (size_t)f * sa.film_total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = piece * 1024 + j * 256 + (int)threadIdx.x;
            if (i < sa.film_total / 4) dst[i] = src[i];
        }
        return;
    }
    if (!PF && (int)blockIdx.x >= nb_conv) {
        // trailing workgroups: stage the NEXT step's FiLM row at a fixed address, so that no LayerNorm loader of
        // the next replay has to chase the step index through memory before it can fetch its gain/bias
        const int step = sa.st->step;
        if (step + 1 >= sa.st->n_steps) return;
        const float4* src = reinterpret_cast<const float4*>(sa.film_table + (size_t)(step + 1) * sa.film_total);
        const int i = ((int)blockIdx.x - nb_conv) * 256 + (int)threadIdx.x;
        if (i < sa.film_total / 4) reinterpret_cast<float4*>(sa.film_cur)[i] = src[i];
        return;
    }
    const int seg = blockIdx.x * 4 + wave;
    if (seg >= nseg) return;                                             // whole wave; no block-wide barrier below
    const int spr = L / PXS;                                             // runs per image row
    const int bb = seg / (L * spr), rem = seg - bb * L * spr, y = rem / spr, x0 = (rem - y * spr) * PXS;
    float wl[9][4][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int co = 0; co < 4; ++co) {
            wl[tap][co][0] = wT[(tap * 4 + co) * 128 + lane];
            wl[tap][co][1] = wT[(tap * 4 + co) * 128 + lane + 64];
        }
    // column loader: the three rows y-1, y, y+1 at image column x (zeros outside the image)
    const float* face = X + (size_t)bb * L * L * 128;
    auto load_col = [&](int x, float (&c)[3][2]) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int yy = y + r - 1;
            const bool in = yy >= 0 && yy < L && x >= 0 && x < L;      // wave-uniform
            const float* q = face + ((size_t)(in ? yy : y) * L + (in ? x : x0)) * 128;
            const float v0 = q[lane], v1 = q[lane + 64];
            c[r][0] = in ? v0 : 0.f; c[r][1] = in ? v1 : 0.f;
        }
    };
    float cl[3][2], cc[3][2], cr[3][2];
    load_col(x0 - 1, cl);
    load_col(x0, cc);
    float part[PXS][4];
#pragma unroll
    for (int px = 0; px < PXS; ++px) {
        load_col(x0 + px + 1, cr);
#pragma unroll
        for (int co = 0; co < 4; ++co) {
            float a = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                a += cl[r][0] * wl[r * 3 + 0][co][0] + cl[r][1] * wl[r * 3 + 0][co][1];
                a += cc[r][0] * wl[r * 3 + 1][co][0] + cc[r][1] * wl[r * 3 + 1][co][1];
                a += cr[r][0] * wl[r * 3 + 2][co][0] + cr[r][1] * wl[r * 3 + 2][co][1];
            }
            part[px][co] = a;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) { cl[r][0] = cc[r][0]; cl[r][1] = cc[r][1]; cc[r][0] = cr[r][0]; cc[r][1] = cr[r][1]; }
    }
    // wave reduction of the 4 PXS partial sums; lane j keeps value j = (pixel j >> 2, output j & 3)
    float mine = 0.f;
#pragma unroll
    for (int px = 0; px < PXS; ++px)
#pragma unroll
        for (int co = 0; co < 4; ++co) {
            const float t = wave_sum(part[px][co]);
            if (lane == px * 4 + co) mine = t;
        }
    if (lane >= 4 * PXS) return;
    const int co = lane & 3, x = x0 + (lane >> 2);
    const size_t o = (((size_t)bb * 4 + co) * L + y) * L + x;           // NCHW
    const float e = mine + b[co];
    eps[o] = e;
    if (sa.lat) {
        const int step = sa.st->step;
        if constexpr (PF) {
            const int r = st_row(sa.st, bb), k = r + step;          // the wave's run lies in one face: k is wave-uniform
            if (k < st_end(sa.st, bb) && !st_guided(sa.st, bb, k - st_begin(sa.st, bb)))
                sa.lat[o] = sched_update<true>(sa.lat[o], e, sa.coef + (size_t)k * 7, sa.st, k, (size_t)sa.elem0 + o, sa.n_total, o,
                                               st_first(sa.st, bb, k, r), bb, (unsigned)(o - (size_t)bb * 4 * L * L), L * L);
        } else if (!st_guided(sa.st, bb, step)) {
            sa.lat[o] = sched_update(sa.lat[o], e, sa.coef + (size_t)step * 7, sa.st, step, (size_t)sa.elem0 + o, sa.n_total, o, false, bb,
                                     (unsigned)(o - (size_t)bb * 4 * L * L), L * L);
        }
    }
}

// first FiLM rows of the per-face form: film_pf[f] = film_table[min(r_f, end_f - 1)] (a face that starts held reads a valid row);
// ends == NULL: end_f = n
static __global__ void film_rows_gather_kernel(float* __restrict__ film_pf, const float* __restrict__ film_table, const int* __restrict__ rows,
                                               const int* __restrict__ ends, int n, int film_total) {
    const int f = blockIdx.y;
    const int row = max(min(rows[f], (ends ? ends[f] : n) - 1), 0);
    const float4* src = reinterpret_cast<const float4*>(film_table + (size_t)row * film_total);
    float4* dst = reinterpret_cast<float4*>(film_pf + (size_t)f * film_total);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < film_total / 4; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// hd_mask_faces: face j (< n = gridDim.y) of mask [n,L,L] / known / noise [n,4,L,L] goes to slot slots[j] (slots == NULL: j) of the batch's
// mask buffers and the slot's flag is set; mask == NULL clears the flag and leaves the buffers.  ll = L*L.
struct MaskScatterP {
    const float *mask, *known, *noise;
    float *dmask, *dknown, *dnoise;
    int* on;
    const int* slots;
    int ll;
};
static __global__ void mask_scatter_kernel(const MaskScatterP p) {
    const int j = blockIdx.y, slot = p.slots ? p.slots[j] : j;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.on[slot] = p.mask ? 1 : 0;
    if (!p.mask) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 4 * p.ll; i += gridDim.x * blockDim.x) {
        if (i < p.ll) p.dmask[(size_t)slot * p.ll + i] = p.mask[(size_t)j * p.ll + i];
        p.dknown[(size_t)slot * 4 * p.ll + i] = p.known[(size_t)j * 4 * p.ll + i];
        p.dnoise[(size_t)slot * 4 * p.ll + i] = p.noise[(size_t)j * 4 * p.ll + i];
    }
}

// hd_guide_faces: plane (j, channel) of target [n,4,L,L] (grid (4, n)) is low-passed with N = scale[j] and stored for slot slots[j]
// (slots == NULL: j), and the slot's weight, block size and row window are set from the call's staged arrays; target == NULL sets the
// slot's weight to 0 (not guided) and leaves the rest.
struct GuideScatterP {
    const float* target;
    float *lp, *w;
    int *n, *j0, *j1;
    const int* slots;
    const float* weight; const int *scale, *row_from, *row_to;   // the call's [n] arrays, on the device
    int L;
};
static __global__ __launch_bounds__(256) void guide_scatter_kernel(const GuideScatterP p) {
    extern __shared__ float guide_lds[];
    const int j = blockIdx.y, ch = blockIdx.x, slot = p.slots ? p.slots[j] : j;
    if (ch == 0 && threadIdx.x == 0) {
        p.w[slot] = p.target ? p.weight[j] : 0.f;
        if (p.target) { p.n[slot] = p.scale[j]; p.j0[slot] = p.row_from[j]; p.j1[slot] = p.row_to[j]; }
    }
    if (!p.target) return;
    const int L = p.L, ll = L * L, N = p.scale[j], P = L / N;
    float *pl = guide_lds, *rs = pl + ll, *bm = rs + ll;
    const float* src = p.target + ((size_t)j * 4 + ch) * ll;
    float* dst = p.lp + ((size_t)slot * 4 + ch) * ll;
    for (int i = threadIdx.x; i < ll; i += blockDim.x) pl[i] = src[i];
    __syncthreads();
    lp_block_means(pl, rs, bm, L, N);
    for (int i = threadIdx.x; i < ll; i += blockDim.x) dst[i] = lp_bilinear(bm, P, N, i / L, i - (i / L) * L);
}

// Progress previews (hd_preview_config).  ll4 = 4*L*L.  preview_reset_kernel (hd_prepare_slots): slot slots[j] (j < n = gridDim.y) has no
// estimate -- its latest plane and its `snaps` snapshot planes are zeroed and their rows set to -1.  preview_gather_kernel (hd_preview_read):
// face slots[j] (NULL: j) of one plane and its row go to out[j] / rows_out[j] (rows_out may be NULL).
struct PreviewP { float *x0, *snap; int* rows; const int* slots; int B, snaps, ll4; };
static __global__ void preview_reset_kernel(const PreviewP p) {
    const int slot = p.slots[blockIdx.y];
    for (int pl = 0; pl <= p.snaps; ++pl) {
        float* d = (pl ? p.snap + (size_t)(pl - 1) * p.B * p.ll4 : p.x0) + (size_t)slot * p.ll4;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.ll4; i += gridDim.x * blockDim.x) d[i] = 0.f;
        if (blockIdx.x == 0 && threadIdx.x == 0) p.rows[(size_t)pl * p.B + slot] = -1;
    }
}
struct PreviewReadP { const float* plane; const int* rows; const int* slots; float* out; int* rows_out; int ll4; };
static __global__ void preview_gather_kernel(const PreviewReadP p) {
    const int j = blockIdx.y, slot = p.slots ? p.slots[j] : j;
    if (p.rows_out && blockIdx.x == 0 && threadIdx.x == 0) p.rows_out[j] = p.rows[slot];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.ll4; i += gridDim.x * blockDim.x) p.out[(size_t)j * p.ll4 + i] = p.plane[(size_t)slot * p.ll4 + i];
}

// The one copy of per-face conditioning (hd_prepare_slots, hd_pool_prepare, hd_pool_commit).  A face's conditioning is kSlotBufs buffers --
// 5 priors NHWC, 5 w_c, 5 w_s, the idc term and id_emb -- each face-contiguous with sz[b] floats per face (1 float: w_s of a 1 x 1 level;
// 32768 S^2: prior 4).  Face j (< n) of the call is read from face src_idx[j] of src (src_idx NULL: face j -- the staging chain's n
// faces in order) and written to dst_idx[j]: with faces_per_chain > 0 a slot of the batch (chain dst_idx[j] / faces_per_chain, face
// dst_idx[j] % faces_per_chain of that chain), with faces_per_chain == 0 an entry of the conditioning pool (dst[0]).  grid (x, n,
// kSlotBufs); the lists are checked on the host (in range; destinations distinct).  16 bytes per lane where the per-face size and both
// face addresses allow it; the small gates (sizes that are no multiple of 4) take the scalar loop.
constexpr int kSlotBufs = 17, kSlotChains = 8;
struct CondCopyP {
    const float* src[kSlotBufs];
    float* dst[kSlotChains][kSlotBufs];
    int sz[kSlotBufs];
    const int* src_idx;
    const int* dst_idx;
    int faces_per_chain;
};
static __global__ __launch_bounds__(256) void cond_copy_kernel(const CondCopyP p) {
    const int j = blockIdx.y, b = blockIdx.z, sz = p.sz[b];
    const int from = p.src_idx ? p.src_idx[j] : j, to = p.dst_idx[j];
    const int ch = p.faces_per_chain ? to / p.faces_per_chain : 0, f = to - ch * p.faces_per_chain;
    const float* __restrict__ src = p.src[b] + (size_t)from * sz;
    float* __restrict__ dst = p.dst[ch][b] + (size_t)f * sz;
    const int t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    if ((sz & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
        for (int i = t; i < sz / 4; i += nt) d4[i] = s4[i];
    } else {
        for (int i = t; i < sz; i += nt) dst[i] = src[i];
    }
}

// ----------------------------------------------------------------------- depthwise 3x3 + gate + pool
// conv2 (depthwise 3x3, pad 1) -> SimpleGate -> G (bf16) and the SCA global average pool
// (conditional_naf.py:116-119 / naf.py:109-112).  T1 is the fp32 conv1 output [rows][2C].
// grid (C/32, faces); a workgroup owns one face x 32 gate channels, so the pooled mean is complete
// without atomics.
// Unfused form (faces too large for the fused conv1 epilogue: side > 16).  grid (C/32, faces, bands): a workgroup
// owns 32 gate channels x a band of 8 image rows of one face; each of its 8 row workers slides a 3x3 window along
// its row (6 new values per pixel per gate half instead of 18).  Band sums go to pool_part[face][band][C]; the
// mean over the face is finished by dwconv_pool_finish_kernel in band order (no atomics: reproducible).
static __global__ __launch_bounds__(256) void dwconv_gate_pool_kernel(const float* __restrict__ T1, const float* __restrict__ w2,
                                                                const float* __restrict__ b2,
                                                                unsigned short* __restrict__ G, float* __restrict__ pool_part,
                                                                int H, int W, int C) {
    __shared__ float red[8][32];
    const int j = blockIdx.x * 32 + (threadIdx.x & 31);
    const int rw = threadIdx.x >> 5;
    const int face = blockIdx.y, band = blockIdx.z, nbands = gridDim.z;
    const int HW = H * W, C2 = 2 * C;
    float wa[9], wb[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) { wa[t] = w2[(size_t)j * 9 + t]; wb[t] = w2[(size_t)(j + C) * 9 + t]; }
    const float ba = b2[j], bb = b2[j + C];
    const float* base = T1 + (size_t)face * HW * C2;
    const int y = band * 8 + rw;
    float sum = 0.f;
    if (y < H) {
        // column x of the three rows y-1, y, y+1 for both gate halves (zeros outside the image)
        auto load_col = [&](int x, float (&a)[3], float (&b)[3]) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int yy = y + r - 1;
                const bool in = yy >= 0 && yy < H && x >= 0 && x < W;
                const float* q = base + (size_t)(in ? yy * W + x : 0) * C2;
                const float va = q[j], vb = q[j + C];
                a[r] = in ? va : 0.f; b[r] = in ? vb : 0.f;
            }
        };
        float la[3], lb[3], ca[3], cb[3], ra[3], rb[3];
        load_col(-1, la, lb);
        load_col(0, ca, cb);
        for (int x = 0; x < W; ++x) {
            load_col(x + 1, ra, rb);
            float u1 = ba, u2 = bb;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                u1 += wa[r * 3] * la[r] + wa[r * 3 + 1] * ca[r] + wa[r * 3 + 2] * ra[r];
                u2 += wb[r * 3] * lb[r] + wb[r * 3 + 1] * cb[r] + wb[r * 3 + 2] * rb[r];
            }
            const float g = u1 * u2;
            G[((size_t)face * HW + y * W + x) * C + j] = f32_to_bf16_bits(g);
            sum += g;
#pragma unroll
            for (int r = 0; r < 3; ++r) { la[r] = ca[r]; lb[r] = cb[r]; ca[r] = ra[r]; cb[r] = rb[r]; }
        }
    }
    red[rw][threadIdx.x & 31] = sum;
    __syncthreads();
    if (rw == 0) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += red[i][threadIdx.x];
        pool_part[((size_t)face * nbands + band) * C + j] = s;
    }
}
static __global__ void dwconv_pool_finish_kernel(const float* __restrict__ pool_part, float* __restrict__ pooled, int faces, int nbands, int C, float inv_hw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= faces * C) return;
    const int face = i / C, j = i - face * C;
    float s = 0.f;
    for (int b = 0; b < nbands; ++b) s += pool_part[((size_t)face * nbands + b) * C + j];
    pooled[i] = s * inv_hw;
}

// -------------------------------------------------------------------------------------- FiLM path
// sinusoidal embedding: [sin(t f_k), cos(t f_k)], k < 64 (models/denoiser/model.py:22-29).
// f_k comes from the host (expf in fp32, like torch.exp on a float32 tensor).
static __global__ void time_embed_kernel(const float* __restrict__ t, const float* __restrict__ freq, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 64) return;
    const int r = i >> 6, k = i & 63;
    const float a = t[r] * freq[k];
    out[(size_t)r * 128 + k] = sinf(a);
    out[(size_t)r * 128 + 64 + k] = cosf(a);
}

// out[m][n] = bias[n] + sum_k in'[m][k] W[n][k], in' = in[m][k]*in[m][k+K] when GATE_IN (SimpleGate on
// the input).  fp32 FMA: time_mlp and the per-block FiLM Linear(256,4C) stay in fp32
// (models/denoiser/model.py:152-157, conditional_naf.py:18-22).  64x64 tile, 4x4 per thread.
template <bool GATE_IN>
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ in, int ldin, const float* __restrict__ Wt,
                                                          const float* __restrict__ bias, float* __restrict__ out, int ldo,
                                                          int M, int N, int K) {
    __shared__ float sa[16][65];
    __shared__ float sb[16][65];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            const int r = i >> 4, kk = i & 15;
            float a = 0.f, b = 0.f;
            if (m0 + r < M && k0 + kk < K) {
                a = in[(size_t)(m0 + r) * ldin + k0 + kk];
                if (GATE_IN) a *= in[(size_t)(m0 + r) * ldin + K + k0 + kk];
            }
            if (n0 + r < N && k0 + kk < K) b = Wt[(size_t)(n0 + r) * K + k0 + kk];
            sa[kk][r] = a; sb[kk][r] = b;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = sa[kk][ty * 4 + i]; b[i] = sb[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
            if (m < M && n < N) out[(size_t)m * ldo + n] = acc[i][j] + bias[n];
        }
}

// Fold LayerNorm2d's affine into FiLM, in place on the raw Linear output of one block:
//   raw  = [shift_att, scale_att, shift_ffn, scale_ffn]            (conditional_naf.py:110)
//   out  = [b1*(1+scale_att)+shift_att, w1*(1+scale_att), b2*(1+scale_ffn)+shift_ffn, w2*(1+scale_ffn)]
// ln holds [b1, w1, b2, w2] at the same offsets.  grid (ceil(C/256), n_blocks, rows).
struct FilmBlock { int off, C; };
static __global__ void film_fold_kernel(float* __restrict__ film, const float* __restrict__ ln, const FilmBlock* __restrict__ blocks,
                                 int film_total) {
    const FilmBlock fb = blocks[blockIdx.y];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= fb.C) return;
    float* f = film + (size_t)blockIdx.z * film_total + fb.off;
    const float* l = ln + fb.off;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float shift = f[2 * h * fb.C + c], scale = f[(2 * h + 1) * fb.C + c];
        const float lb = l[2 * h * fb.C + c], lw = l[(2 * h + 1) * fb.C + c];
        f[2 * h * fb.C + c] = lb * (scale + 1.0f) + shift;
        f[(2 * h + 1) * fb.C + c] = lw * (scale + 1.0f);
    }
}

// ------------------------------------------------------------------------------------- scheduler
// Philox4x32-10 (Salmon et al. 2011), counter (elem, step, 0, 0), key (seed lo, seed hi); two
// Box-Muller normals per call, the first is used.  Restated identically in tests (numpy).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned* o) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ float philox_normal(unsigned long long seed, unsigned step, unsigned elem) {
    unsigned o[4];
    philox4x32_10(elem, step, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), o);
    const float u1 = ((float)(o[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);      // (0, 1]
    const float u2 = (float)(o[1] >> 8) * (1.0f / 16777216.0f);               // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// The sampling loop applies the scheduler update inside ending_conv_kernel (sched_update); this kernel serves
// hd_scheduler_step (hist NULL) and hd_scheduler_step_multistep (hist: read for the c7 term when c7 != 0, then <- x0).
struct Coef7 { float c[7]; };
static __global__ void sched_step_direct_kernel(float* __restrict__ x, const float* __restrict__ eps, const Coef7 k,
                                         const float* __restrict__ noise, unsigned long long seed, int step, long long n,
                                         float* __restrict__ hist, float c7) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float xv = x[i], e = eps[i];
    float x0 = (xv - k.c[0] * e) / k.c[1];
    x0 = fminf(fmaxf(x0, -k.c[2]), k.c[2]);
    float r = k.c[3] * x0 + k.c[4] * xv + k.c[5] * e;
    if (k.c[6] != 0.f) r += k.c[6] * (noise ? noise[i] : philox_normal(seed, (unsigned)step, (unsigned)i));
    if (hist) {
        if (c7 != 0.f) r += c7 * hist[i];
        hist[i] = x0;
    }
    x[i] = r;
}

// A persistent stage of this call gave up a hand-off wait (abort word set): everything computed since is invalid, so the
// call's result buffer is filled with NaN -- the caller sees the failure in the very tensors it gets back, whatever it does
// with the return code (hd_check() reports it after a synchronisation).  One launch per hd_eps / hd_sample call.
static __global__ void poison_if_abort_kernel(const unsigned* __restrict__ abort_dev, float* __restrict__ out, size_t n) {
    if (*abort_dev == 0u) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __builtin_nanf("");
}

// ------------------------------------------------------------------------------- pooling / layout
// channels-last fp32 -> NCHW fp32 (priors handed out by hd_fpg)
static __global__ void nhwc_to_nchw_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int HW, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int p = (int)(i % HW);
    const size_t r = i / HW;
    const int c = (int)(r % C);
    const size_t b = r / C;
    out[i] = in[(b * HW + p) * C + c];
}

// avg + max pool over the face: HCA channel gate input (models/fpg/hca.py:34-36).  X fp32 [B][HW][C].
// The sum is taken in runs of kPoolRun pixels whose sums are then added: one running sum over the 4096 pixels of a 64 x 64 face was 2 ulp
// (4.7e-7) from float64, four times torch's fp32 error.  Faces of up to kPoolRun pixels (every level of latent 16) are one run: the same bits.
constexpr int kPoolRun = 256;
static __global__ void pool_avgmax_kernel(const float* __restrict__ X, float* __restrict__ out, int HW, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float* p = X + (size_t)blockIdx.y * HW * C + c;
    float s = 0.f, m = -3.402823466e38f;
    for (int i0 = 0; i0 < HW; i0 += kPoolRun) {
        const int i1 = min(i0 + kPoolRun, HW);
        float run = 0.f;
        for (int i = i0; i < i1; ++i) { const float v = p[(size_t)i * C]; run += v; m = fmaxf(m, v); }
        s = i0 ? s + run : run;
    }
    out[(size_t)blockIdx.y * C + c] = s / (float)HW + m;
}

// out[row] = sigmoid(dot(Hd[row], w) + bias): spatial gate's Conv2d(C/2,1,1)+BN (folded)+Sigmoid
// (models/fpg/hca.py:16-18).  One wave per row, fp32.
static __global__ __launch_bounds__(256) void rowdot_sigmoid_kernel(const float* __restrict__ Hd, const float* __restrict__ w, float bias,
                                                              float* __restrict__ out, int M, int K) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += Hd[(size_t)row * K + k] * w[k];
    s = wave_sum(s);
    if (lane == 0) out[row] = 1.0f / (1.0f + expf(-(s + bias)));
}

// NCHW fp32 -> channels-last fp32 (priors handed in by hd_prepare_from_priors)
static __global__ void nchw_to_nhwc_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int HW, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t r = i / C;
    const int p = (int)(r % HW);
    const size_t b = r / HW;
    out[i] = in[(b * C + c) * HW + p];
}

// cr_face NCHW fp32 [B,3,H,W] -> channels-last bf16 padded to 8 channels (ResNet conv1 input)
static __global__ void nchw3_to_nhwc8_bf16_kernel(const float* __restrict__ in, uint4* __restrict__ out, int HW, size_t npix) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const size_t b = i / HW, p = i - b * HW;
    float v[8] = {in[(b * 3 + 0) * HW + p], in[(b * 3 + 1) * HW + p], in[(b * 3 + 2) * HW + p], 0, 0, 0, 0, 0};
    out[i] = pack8(v);
}

// MaxPool2d(3, stride 2, pad 1) on channels-last bf16 (models/idc/model.py:112,124)
static __global__ void maxpool3x3s2_bf16_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out,
                                         int B, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)B * Ho * Wo * C;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    size_t r = i / C;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m = -3.402823466e38f;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int y = oy * 2 - 1 + ky, x = ox * 2 - 1 + kx;
            if (y < 0 || y >= H || x < 0 || x >= W) continue;
            m = fmaxf(m, bf16_bits_to_f32(in[(((size_t)b * H + y) * W + x) * C + c]));
        }
    out[i] = f32_to_bf16_bits(m);
}

// AdaptiveAvgPool2d(1) on channels-last bf16 -> fp32 [B][C] (models/idc/model.py:131)
static __global__ void avgpool_bf16_kernel(const unsigned short* __restrict__ in, float* __restrict__ out, int HW, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const unsigned short* p = in + (size_t)blockIdx.y * HW * C + c;
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += bf16_bits_to_f32(p[(size_t)i * C]);
    out[(size_t)blockIdx.y * C + c] = s / (float)HW;
}

}  // namespace hd
