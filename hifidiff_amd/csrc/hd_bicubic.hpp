// hd_bicubic.hpp -- the bicubic weights that the VAE boundary's resize (hd_vae.hpp) and the colour fix and the metrics (hd_color.hpp,
// hd_metrics.hpp) share, on their own so that the image entry points do not compile the GEMM family.
#pragma once
#include <hip/hip_runtime.h>

namespace hd {

// ---- F.interpolate(x, R, mode="bicubic", align_corners=False) (ATen upsample_bicubic2d: A = -0.75,
// source index (dst + 0.5) * scale - 0.5, taps clamped to the border) ----
__device__ __forceinline__ void cubic_coeffs(float t, float* w) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

}  // namespace hd
