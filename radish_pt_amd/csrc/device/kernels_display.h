// radish_pt_amd/csrc/device/kernels_display.h — the step AFTER the path: image → RGBA8 for the preview PBO.
//
// Restates sendImageToPBO's four overloads (/root/reference/src/pathtrace.cu:32-118) and the tone-mapping helpers
// Math::filmic / ACES / gammaCorrection (/root/reference/src/mathUtil.h:110-126).  Elementwise, HBM-bound: 12 B read +
// 4 B written per pixel.  The reference's gamma is glm::pow(c, 1/2.2) = CUDA libdevice powf, whose bits no other
// platform reproduces; both this file and the oracle evaluate pow_gamma_det below (binary32 operations in this order
// only, ~2e-7 relative), so the RGBA8 output is bit-identical between them.  Float → int follows CUDA's conversion
// (NaN → 0, saturating), which is what the reference's glm::ivec3(color * 255.f) compiles to on its GPU.
#pragma once
#include "display_math.h"

namespace rd {

// kind 0: vec3 image (tone mapping + scale, pathtrace.cu:32-59); 1: vec2 (:61-78); 2: float (:80-97);
// 3: int pixel index shown as normalised coordinates (:99-118)
__global__ __launch_bounds__(256) void k_send_image_to_pbo(uint32_t *__restrict__ pbo, const void *__restrict__ image, int width,
                                                           int height, int kind, int toneMapping, float scale) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)width * height) return;
    v3 color;
    if (kind == 0) {
        const float *img = static_cast<const float *>(image);
        color = mk3(img[3 * idx], img[3 * idx + 1], img[3 * idx + 2]) * scale;
        if (toneMapping == 1) color = filmic(color);
        else if (toneMapping == 2) color = ACES(color);
    } else if (kind == 1) {
        const float *img = static_cast<const float *>(image);
        color = mk3(img[2 * idx], img[2 * idx + 1], 0.f);
    } else if (kind == 2) {
        float g = static_cast<const float *>(image)[idx];
        color = mk3(g, g, g);
    } else {
        int v = static_cast<const int *>(image)[idx];
        int px = v % width, py = v / width;
        color = mk3(float(px) / float(width), float(py) / float(height), 0.f);
    }
    pbo[idx] = packRGBA(color);
}

}  // namespace rd
