// radish_pt_amd/csrc/device/kernels_textures.h — textures and the environment map edited on the device (rdh_scene_set_texture,
// rdh_scene_env_power).
//
// A plain texture is a device-to-device copy into texData, ordered on the stream (no kernel).  The environment map also feeds the
// pixel alias table and, through its total power, the last entry of the light sampler.  The kernels below repeat
// rdh_build_envmap_pdf (host/scene_build.cpp) operation for operation — the library is built with -ffp-contract=off like the
// host's — and leave the rest to kernels_lights.h:
//
//   k_env_weights      one lane per pixel: luminance * rowSin[row], the value rdh_build_envmap_pdf hands to the alias construction.
//                      rowSin[i] = sinf((.5f + i) / height * PI) comes from the host (glibc's sinf is not the device's)
//   k_light_power_dev  k_light_power with the environment entry read from device memory: the sum k_alias_classify left
//
// Every launch is ordered by the stream; nothing is handed over between workgroups inside a kernel.
#pragma once
#include "kernels_lights.h"

namespace rd {

// pdf[i * width + j] = (0.2126f * r + 0.7152f * g + 0.0722f * b) * rowSin[i]; n = width * height pixels.
__global__ __launch_bounds__(256) void k_env_weights(const float *__restrict__ texels, const float *__restrict__ rowSin, int width, int n,
                                                     float *__restrict__ pdf) {
    const int idx = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= n) return;
    const float *c = texels + 3 * (size_t)idx;
    const float lum = 0.2126f * c[0] + 0.7152f * c[1] + 0.0722f * c[2];
    pdf[idx] = lum * rowSin[idx / width];
}

// The aperture mask's weights (rdh_set_lens): weight[k] = luminance(texel k), texel order, n = width * height texels.
__global__ __launch_bounds__(256) void k_lens_weights(const float *__restrict__ texels, int n, float *__restrict__ weight) {
    const int idx = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= n) return;
    weight[idx] = luminance(texel(texels, idx));
}

// k_light_power for an environment power that never left the device (rdh_scene_set_texture): entries numLights .. n - 1 = *envPower.
__global__ __launch_bounds__(256) void k_light_power_dev(const LightRec *__restrict__ lights, int numLights, int n,
                                                         const float *__restrict__ envPower, float *__restrict__ power) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (i >= numLights) {
        power[i] = *envPower;
        return;
    }
    const float4 A = lights[i].a, B = lights[i].b, C = lights[i].c;
    power[i] = emitterPower(mk3(A.x, A.y, A.z), mk3(A.w, B.x, B.y), mk3(B.z, B.w, C.x), C.y, C.z, C.w);
}

}  // namespace rd
