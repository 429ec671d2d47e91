// hd_image.hip -- the entry points on decoded face images that need no context: colour correction against a reference (hd_color_fix,
// hd_color.hpp) and the per-face value range, MSE and SSIM (hd_image_range, hd_image_metrics, hd_metrics.hpp).  The contract is in
// include/hifidiff_hip.h.  Errors go to hd_last_error(NULL), and every argument is checked before the first HIP call.
#include <cmath>

#include "hd_args.hpp"
#include "hd_color.hpp"
#include "hd_metrics.hpp"

using namespace hd;
using namespace hd_args;

extern "C" {

// Colour correction of decoded faces against a reference (hd_color.hpp).  No context: errors go to hd_last_error(NULL), and every
// argument is checked before the first HIP call.
int hd_color_fix(const float* images, float* out, int batch, int res, const float* ref, int ref_res, int ref_vae_range, int mode,
                 int levels, const float* weight, void* stream) {
    if (batch < 1) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: batch must be >= 1, got %d", batch);
    if (!res_ok(res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: res must be a multiple of 64 in [64, 512], got %d", res);
    if (!res_ok(ref_res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: ref_res must be a multiple of 64 in [64, 512], got %d", ref_res);
    if (mode != 1 && mode != 2) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: mode must be 1 (wavelet) or 2 (AdaIN), got %d", mode);
    if (mode == 1 && (levels < 1 || levels > CF_MAX_LEVELS)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: levels must be in [1, %d] in wavelet mode, got %d", CF_MAX_LEVELS, levels);
    if (ref_vae_range != 0 && ref_vae_range != 1) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: ref_vae_range must be 0 or 1, got %d", ref_vae_range);
    if (!images) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: images is NULL");
    if (!out) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: out is NULL");
    if (!ref) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: ref is NULL");
    const uintptr_t pi = (uintptr_t)images, po = (uintptr_t)out, pr = (uintptr_t)ref;
    if ((pi | po | pr | (uintptr_t)weight) % sizeof(float)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: images, out, ref and weight must be aligned to 4 bytes");
    if (mode == 2 && (pi | po | pr) % 16) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: images, out and ref must be aligned to 16 bytes in AdaIN mode");
    const size_t nimg = (size_t)batch * 3 * res * res * sizeof(float), nref = (size_t)batch * 3 * ref_res * ref_res * sizeof(float);
    const ByteRange dst = {"out", out, nimg};
    if (overlap(dst, {"images", images, nimg})) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: out overlaps images (the tiled kernel reads its neighbours' pixels)");
    if (overlap(dst, {"ref", ref, nref})) HD_ARG_FAIL(HD_ERR_INVALID, "hd_color_fix: out overlaps ref");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int planes = batch * 3;
    hipError_t e;
    if (mode == 1) {
        const int tiles = res / CF_TILE, halo = (1 << levels) - 1;
        const int side = CF_TILE + (tiles == 1 ? 0 : tiles == 2 ? halo : 2 * halo);   // the largest staged region of any tile
        const size_t smem = (size_t)2 * side * side * sizeof(float);
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wavelet_fix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CF_MAX_SMEM);
        if (e != hipSuccess) HD_ARG_FAIL(HD_ERR_HIP, "hd_color_fix: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
        hipLaunchKernelGGL(wavelet_fix_kernel, dim3(tiles * tiles, planes), dim3(CF_THREADS), smem, s, images, ref, out, weight, res, ref_res, ref_vae_range, levels);
    } else {
        hipLaunchKernelGGL(adain_fix_kernel, dim3(planes), dim3(CF_THREADS), 0, s, images, ref, out, weight, res, ref_res, ref_vae_range);
    }
    e = hipGetLastError();
    if (e != hipSuccess) HD_ARG_FAIL(HD_ERR_HIP, "hd_color_fix: launch failed: %s", hipGetErrorString(e));
    return HD_OK;
}
// Per-face MSE / SSIM of images against a reference and the per-face value range (hd_metrics.hpp).  No context, as hd_color_fix:
// errors go to hd_last_error(NULL) and every argument is checked before the first HIP call.
int64_t hd_image_metrics_workspace(int batch, int ref_res, int channels) {
    if (batch < 1 || batch > 65535) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics_workspace: batch must be in [1, 65535], got %d", batch);
    if (!res_ok(ref_res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics_workspace: ref_res must be a multiple of 64 in [64, 512], got %d", ref_res);
    if (channels != 1 && channels != 2) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics_workspace: channels must be 1 (rgb) or 2 (y), got %d", channels);
    const int tiles = ref_res / MT_TILE;
    return (int64_t)batch * (channels == 1 ? 3 : 1) * tiles * tiles * 2 * (int64_t)sizeof(double);
}

int hd_image_range(const float* images, int batch, int res, int out_res, float* range_out, void* stream) {
    if (batch < 1) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: batch must be >= 1, got %d", batch);
    if (!res_ok(res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: res must be a multiple of 64 in [64, 512], got %d", res);
    if (!res_ok(out_res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: out_res must be a multiple of 64 in [64, 512], got %d", out_res);
    if (!images) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: images is NULL");
    if (!range_out) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: range_out is NULL");
    const uintptr_t pi = (uintptr_t)images, po = (uintptr_t)range_out;
    if (res == out_res && pi % 16) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: images must be aligned to 16 bytes when out_res == res (vector loads)");
    if (pi % sizeof(float)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: images must be aligned to 4 bytes");
    if (po % sizeof(float)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: range_out must be aligned to 4 bytes");
    if (overlap({"range_out", range_out, (size_t)batch * 2 * sizeof(float)}, {"images", images, (size_t)batch * 3 * res * res * sizeof(float)}))
        HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_range: range_out overlaps images");
    hipLaunchKernelGGL(range_kernel, dim3(batch), dim3(MT_RANGE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), images, res, out_res, range_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) HD_ARG_FAIL(HD_ERR_HIP, "hd_image_range: launch failed: %s", hipGetErrorString(e));
    return HD_OK;
}

int hd_image_metrics(const float* images, int res, const float* ref, int ref_res, int batch, int channels, float data_range,
                     const float* images_range, const float* ref_range, double* out, float* ssim_map_out, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    if (batch < 1 || batch > 65535) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: batch must be in [1, 65535], got %d", batch);
    if (!res_ok(res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: res must be a multiple of 64 in [64, 512], got %d", res);
    if (!res_ok(ref_res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: ref_res must be a multiple of 64 in [64, 512], got %d", ref_res);
    if (channels != 1 && channels != 2) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: channels must be 1 (rgb) or 2 (y), got %d", channels);
    if (!(data_range > 0.f) || !std::isfinite(data_range)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: data_range must be finite and > 0, got %g", (double)data_range);
    if (!images) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: images is NULL");
    if (!ref) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: ref is NULL");
    if (!out) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: out is NULL");
    if (!workspace) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: workspace is NULL (hd_image_metrics_workspace gives its size)");
    const int P = channels == 1 ? 3 : 1, tiles = ref_res / MT_TILE, V = ref_res - (MT_WIN - 1);
    const int64_t need = (int64_t)batch * P * tiles * tiles * 2 * (int64_t)sizeof(double);
    if (workspace_bytes < need)
        HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: workspace_bytes is %lld, this call needs %lld (hd_image_metrics_workspace)", (long long)workspace_bytes, (long long)need);
    const uintptr_t pi = (uintptr_t)images, pr = (uintptr_t)ref, pir = (uintptr_t)images_range, prr = (uintptr_t)ref_range;
    const uintptr_t po = (uintptr_t)out, pm = (uintptr_t)ssim_map_out, pw = (uintptr_t)workspace;
    if ((pi | pr | pir | prr | pm) % sizeof(float))
        HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: images, ref, images_range, ref_range and ssim_map_out must be aligned to 4 bytes");
    if ((po | pw) % sizeof(double)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: out and workspace must be aligned to 8 bytes");
    const size_t nimg = (size_t)batch * 3 * res * res * sizeof(float), nref = (size_t)batch * 3 * ref_res * ref_res * sizeof(float);
    const size_t nrange = (size_t)batch * 2 * sizeof(float), nout = (size_t)batch * 2 * sizeof(double);
    const size_t nmap = (size_t)batch * P * V * V * sizeof(float);
    const ByteRange outs[3] = {{"out", out, nout}, {"ssim_map_out", ssim_map_out, nmap}, {"workspace", workspace, (size_t)need}},
                    ins[4] = {{"images", images, nimg}, {"ref", ref, nref}, {"images_range", images_range, nrange}, {"ref_range", ref_range, nrange}};
    const ByteRange *a, *b;
    if (first_overlap(outs, 3, ins, 4, &a, &b)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_image_metrics: %s overlaps %s", a->name, b->name);
    MtWindow win;
    {   // g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), normalised in float64
        double g[MT_WIN], sum = 0.0;
        for (int k = 0; k < MT_WIN; ++k) { g[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
        for (int k = 0; k < MT_WIN; ++k) win.g[k] = (float)(g[k] / sum);
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    const dim3 grid(tiles * tiles, P, batch);
    if (channels == 1)
        hipLaunchKernelGGL(metrics_kernel<0>, grid, dim3(MT_THREADS), 0, s, images, res, ref, ref_res, data_range, images_range, ref_range, win, partial, ssim_map_out);
    else
        hipLaunchKernelGGL(metrics_kernel<1>, grid, dim3(MT_THREADS), 0, s, images, res, ref, ref_res, data_range, images_range, ref_range, win, partial, ssim_map_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) HD_ARG_FAIL(HD_ERR_HIP, "hd_image_metrics: launch failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(metrics_combine_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, partial, batch, P * tiles * tiles,
                       1.0 / ((double)P * ref_res * ref_res), 1.0 / ((double)P * V * V), out);
    e = hipGetLastError();
    if (e != hipSuccess) HD_ARG_FAIL(HD_ERR_HIP, "hd_image_metrics: launch failed: %s", hipGetErrorString(e));
    return HD_OK;
}

}  // extern "C"
