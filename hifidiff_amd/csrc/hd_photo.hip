// hd_photo.hip -- hd_face_ingest / hd_face_paste and their workspace queries: argument checks, the per-face jobs of hd_photo.hpp's resize
// kernel and its launches.  The contract is in include/hifidiff_hip.h.  No context: errors go to hd_last_error(NULL), and every argument
// is checked before the first HIP call.
#include <vector>

#include "hd_args.hpp"
#include "hd_photo.hpp"

using namespace hd;
using hd_args::res_ok;

namespace {

constexpr int PH_MAX_BATCH = 4096, PH_MAX_PHOTO_SIDE = 16384, PH_MAX_FEATHER = 256;

bool ph_lr_ok(int lr) { return lr == 0 || (lr >= 8 && lr <= 64); }

// what both calls check of the photos and the boxes
int ph_check_boxes(const char* fn, const void* photos, int n_photos, int height, int width, const int32_t* boxes, const int32_t* photo_index, int batch) {
    if (!photos) HD_ARG_FAIL(HD_ERR_INVALID, "%s: photos is NULL", fn);
    if (!boxes) HD_ARG_FAIL(HD_ERR_INVALID, "%s: boxes is NULL", fn);
    if (n_photos < 1) HD_ARG_FAIL(HD_ERR_INVALID, "%s: n_photos must be >= 1, got %d", fn, n_photos);
    if (height < 1 || height > PH_MAX_PHOTO_SIDE) HD_ARG_FAIL(HD_ERR_INVALID, "%s: height must be in [1, %d], got %d", fn, PH_MAX_PHOTO_SIDE, height);
    if (width < 1 || width > PH_MAX_PHOTO_SIDE) HD_ARG_FAIL(HD_ERR_INVALID, "%s: width must be in [1, %d], got %d", fn, PH_MAX_PHOTO_SIDE, width);
    if (batch < 1 || batch > PH_MAX_BATCH) HD_ARG_FAIL(HD_ERR_INVALID, "%s: batch must be in [1, %d], got %d", fn, PH_MAX_BATCH, batch);
    for (int i = 0; i < batch; ++i) {
        const int l = boxes[4 * i], t = boxes[4 * i + 1], w = boxes[4 * i + 2], h = boxes[4 * i + 3];
        if (w < 1 || w > PH_MAX_SIDE || h < 1 || h > PH_MAX_SIDE)
            HD_ARG_FAIL(HD_ERR_INVALID, "%s: boxes[%d]: sides must be in [1, %d], got %d x %d", fn, i, PH_MAX_SIDE, w, h);
        if (l < 0 || t < 0 || l > width - w || t > height - h)
            HD_ARG_FAIL(HD_ERR_INVALID, "%s: boxes[%d] = (%d, %d, %d, %d) does not lie inside the %d x %d photo", fn, i, l, t, w, h, width, height);
        if (photo_index && (photo_index[i] < 0 || photo_index[i] >= n_photos))
            HD_ARG_FAIL(HD_ERR_INVALID, "%s: photo_index[%d] = %d is outside [0, %d)", fn, i, photo_index[i], n_photos);
    }
    return HD_OK;
}

// one resize of every face, PH_CHUNK faces per launch; job(f) describes face f
template <bool BLEND, class JobFn>
hipError_t ph_launch(int batch, JobFn job, const uint8_t* src, uint8_t* dst8, float* dstf, int feather, hipStream_t s) {
    for (int f0 = 0; f0 < batch; f0 += PH_CHUNK) {
        PhChunk ch = {};
        const int n = batch - f0 < PH_CHUNK ? batch - f0 : PH_CHUNK;
        int blocks = 1;
        for (int i = 0; i < n; ++i) {
            ch.j[i] = job(f0 + i);
            const int b = ph_blocks(ch.j[i].iw, ch.j[i].ih, ch.j[i].ow, ch.j[i].oh);
            blocks = b > blocks ? b : blocks;
        }
        hipLaunchKernelGGL(photo_resize_kernel<BLEND>, dim3(blocks, n), dim3(PH_THREADS), 0, s, ch, src, dst8, dstf, feather);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

extern "C" {

int64_t hd_face_ingest_workspace(int batch, int lr, int res) {
    if (batch < 1 || batch > PH_MAX_BATCH) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest_workspace: batch must be in [1, %d], got %d", PH_MAX_BATCH, batch);
    if (!ph_lr_ok(lr)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest_workspace: lr must be 0 or in [8, 64], got %d", lr);
    if (!res_ok(res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest_workspace: res must be a multiple of 64 in [64, 512], got %d", res);
    return (int64_t)batch * lr * lr * 3;
}

int64_t hd_face_paste_workspace(int batch, int res) {
    if (batch < 1 || batch > PH_MAX_BATCH) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste_workspace: batch must be in [1, %d], got %d", PH_MAX_BATCH, batch);
    if (!res_ok(res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste_workspace: res must be a multiple of 64 in [64, 512], got %d", res);
    return (int64_t)batch * res * res * 3;
}

int hd_face_ingest(const uint8_t* photos, int n_photos, int height, int width, const int32_t* boxes, const int32_t* photo_index, int batch,
                   int lr, int res, float* out, uint8_t* out_u8, void* workspace, int64_t workspace_bytes, void* stream) {
    if (const int rc = ph_check_boxes("hd_face_ingest", photos, n_photos, height, width, boxes, photo_index, batch)) return rc;
    if (!ph_lr_ok(lr)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest: lr must be 0 or in [8, 64], got %d", lr);
    if (!res_ok(res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest: res must be a multiple of 64 in [64, 512], got %d", res);
    if (!out) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest: out is NULL");
    if ((uintptr_t)out % sizeof(float)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest: out must be aligned to 4 bytes");
    const int64_t need = (int64_t)batch * lr * lr * 3;
    if (need && !workspace) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest: workspace is NULL (hd_face_ingest_workspace gives its size)");
    if (workspace_bytes < need)
        HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_ingest: workspace_bytes is %lld, this call needs %lld (hd_face_ingest_workspace)", (long long)workspace_bytes, (long long)need);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* mid = static_cast<uint8_t*>(workspace);
    const int side = lr ? lr : res;                               // the first resize's target
    const auto crop = [=](int f) {
        const int l = boxes[4 * f], t = boxes[4 * f + 1], w = boxes[4 * f + 2], h = boxes[4 * f + 3], p = photo_index ? photo_index[f] : 0;
        PhJob j = {};
        j.src_off = (((long long)p * height + t) * width + l) * 3; j.src_stride = width * 3;
        j.dst_off = (long long)f * side * side * 3; j.dst_stride = side * 3;
        j.iw = w; j.ih = h; j.ow = side; j.oh = side; j.face = f;
        return j;
    };
    hipError_t e;
    if (lr) {
        e = ph_launch<false>(batch, crop, photos, mid, nullptr, 0, s);
        if (e == hipSuccess) {
            const auto up = [=](int f) {
                PhJob j = {};
                j.src_off = (long long)f * lr * lr * 3; j.src_stride = lr * 3;
                j.dst_off = (long long)f * res * res * 3; j.dst_stride = res * 3;
                j.iw = lr; j.ih = lr; j.ow = res; j.oh = res; j.face = f;
                return j;
            };
            e = ph_launch<false>(batch, up, mid, out_u8, out, 0, s);
        }
    } else {
        e = ph_launch<false>(batch, crop, photos, out_u8, out, 0, s);
    }
    if (e != hipSuccess) HD_ARG_FAIL(HD_ERR_HIP, "hd_face_ingest: launch failed: %s", hipGetErrorString(e));
    return HD_OK;
}

int hd_face_paste(uint8_t* photos, int n_photos, int height, int width, const float* faces, int res, const int32_t* boxes,
                  const int32_t* photo_index, int batch, int feather, void* workspace, int64_t workspace_bytes, void* stream) {
    if (const int rc = ph_check_boxes("hd_face_paste", photos, n_photos, height, width, boxes, photo_index, batch)) return rc;
    if (!res_ok(res)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste: res must be a multiple of 64 in [64, 512], got %d", res);
    if (feather < 0 || feather > PH_MAX_FEATHER) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste: feather must be in [0, %d], got %d", PH_MAX_FEATHER, feather);
    if (!faces) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste: faces is NULL");
    if ((uintptr_t)faces % sizeof(float)) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste: faces must be aligned to 4 bytes");
    for (int i = 0; i < batch; ++i)
        for (int k = i + 1; k < batch; ++k) {
            if ((photo_index ? photo_index[i] : 0) != (photo_index ? photo_index[k] : 0)) continue;
            const int32_t *a = boxes + 4 * i, *b = boxes + 4 * k;
            if (a[0] < b[0] + b[2] && b[0] < a[0] + a[2] && a[1] < b[1] + b[3] && b[1] < a[1] + a[3])
                HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste: boxes[%d] and boxes[%d] overlap in photo %d", i, k, photo_index ? photo_index[i] : 0);
        }
    const int64_t need = (int64_t)batch * res * res * 3;
    if (!workspace) HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste: workspace is NULL (hd_face_paste_workspace gives its size)");
    if (workspace_bytes < need)
        HD_ARG_FAIL(HD_ERR_INVALID, "hd_face_paste: workspace_bytes is %lld, this call needs %lld (hd_face_paste_workspace)", (long long)workspace_bytes, (long long)need);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* q8 = static_cast<uint8_t*>(workspace);
    const long long npix = (long long)batch * res * res;
    hipLaunchKernelGGL(photo_quantize_kernel, dim3((unsigned)((npix + PH_THREADS - 1) / PH_THREADS)), dim3(PH_THREADS), 0, s, faces, q8, res, npix);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        const auto box = [=](int f) {
            const int l = boxes[4 * f], t = boxes[4 * f + 1], w = boxes[4 * f + 2], h = boxes[4 * f + 3], p = photo_index ? photo_index[f] : 0;
            PhJob j = {};
            j.src_off = (long long)f * res * res * 3; j.src_stride = res * 3;
            j.dst_off = (((long long)p * height + t) * width + l) * 3; j.dst_stride = width * 3;
            j.iw = res; j.ih = res; j.ow = w; j.oh = h; j.face = f;
            return j;
        };
        e = ph_launch<true>(batch, box, q8, photos, nullptr, feather, s);
    }
    if (e != hipSuccess) HD_ARG_FAIL(HD_ERR_HIP, "hd_face_paste: launch failed: %s", hipGetErrorString(e));
    return HD_OK;
}

}  // extern "C"
