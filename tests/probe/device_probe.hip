// tests/probe/device_probe.hip — TEST INFRASTRUCTURE ONLY: one tiny kernel around each small __device__ function of the
// kernel-free device headers, so that tests/test_gpu_device_functions.py can feed a function millions of chosen inputs and
// compare every output with the oracle's copy of that function, bit by bit.
//
// Built by radish_pt_amd/_build.py:build_probe with exactly the product's HIP_FLAGS (plus hidden visibility) into
// tests/probe/libradish_probe.so.  The product never loads it and api.EXPORTS does not list it.
//
// What this pins and what it does not:
//   * It pins each function's SOURCE TEXT under the product's compiler flags.  It does not pin each inlined copy of the function
//     inside a hot kernel (the compiler may schedule and select instructions differently there).  The frame, ray-batch and
//     G-buffer tests remain that pin.
//   * Functions that need a DScene (lights.h, texSample, the tree walks) and cameraSample stay with the scene-level tests.
//   * Reservoir::W (restir.h:31-40) has no device function of its own: k_reservoir_w below restates the two lines of
//     restirFinish (kernels_restir.h) that compute it, from the same functions.  It is the only arithmetic written here, and
//     it pins materialBSDF / satDot / length in that combination, not restirFinish's own copy.
//
// Every entry is  int probe_<name>(const void *d_in, void *d_out, long long n, void *stream):
// d_in / d_out are device pointers to n fixed-size records of 32-bit words (layout above each kernel; `f` float, `i` int32,
// `u` uint32), one lane per record, 256 lanes per workgroup, bounds-checked, plain vector loads and stores.  Returns 0, or
// -1 for a null pointer or n <= 0 (nothing is launched), or -2 when the launch itself fails.
#include <hip/hip_runtime.h>

#include "bsdf.h"
#include "denoise_math.h"
#include "display_math.h"
#include "layouts.h"
#include "reservoir.h"
#include "rmath.h"
#include "traverse.h"

using namespace rd;

#define PROBE_API extern "C" __attribute__((visibility("default")))

namespace {

__device__ __forceinline__ v3 ld3(const float *p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ void st3(float *p, v3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
__device__ __forceinline__ long long laneRecord() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }

// in  12 f: box pMin.xyz, pMax.xyz, ray origin.xyz, direction.xyz
// out  9  : i hit(aabbIntersect), i hit(aabbFast), i hit(aabbFastPk), i hit(boxTest), f tMin of the same four, i cls
//           The two fast tests are evaluated only when cls == 0; otherwise their flags are -1 and their tMin 0.
__global__ __launch_bounds__(256) void k_box(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const float *p = in + 12 * i;
    const v3 lo = ld3(p), hi = ld3(p + 3);
    const RaySlab rs = makeRaySlab(Ray{ld3(p + 6), ld3(p + 9)});
    const float4 lo4 = make_float4(lo.x, lo.y, lo.z, 0.f), hi4 = make_float4(hi.x, hi.y, hi.z, 0.f);
    float tLit = 0.f, tFast = 0.f, tPk = 0.f, tDisp = 0.f;
    int hLit = aabbIntersect(lo, hi, rs, tLit) ? 1 : 0, hFast = -1, hPk = -1;
    if (rs.cls == 0) {
        hFast = aabbFast(lo4, hi4, rs, tFast) ? 1 : 0;
        hPk = aabbFastPk(lo4, hi4, packSlab(rs), tPk) ? 1 : 0;
    }
    int hDisp = boxTest(lo4, hi4, rs, tDisp) ? 1 : 0;
    float *o = out + 9 * i;
    o[0] = __int_as_float(hLit);
    o[1] = __int_as_float(hFast);
    o[2] = __int_as_float(hPk);
    o[3] = __int_as_float(hDisp);
    o[4] = tLit;
    o[5] = tFast;
    o[6] = tPk;
    o[7] = tDisp;
    o[8] = __int_as_float(rs.cls);
}

// in  15 f: ray origin.xyz, direction.xyz, v0.xyz, v1.xyz, v2.xyz
// out  4  : i hit, f bary.x, f bary.y, f dist
__global__ __launch_bounds__(256) void k_triangle(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const float *p = in + 15 * i;
    const RaySlab rs = makeRaySlab(Ray{ld3(p), ld3(p + 3)});
    v2 bary = {0.f, 0.f};
    float dist = 0.f;
    const bool hit = intersectTriangle(rs, ld3(p + 6), ld3(p + 9), ld3(p + 12), bary, dist);
    float *o = out + 4 * i;
    o[0] = __int_as_float(hit ? 1 : 0);
    o[1] = bary.x;
    o[2] = bary.y;
    o[3] = dist;
}

// in  6 f: position.xyz, direction.xyz
// out 8  : i getMTBVHId(direction), i getMTBVHId(-direction), f makeOffsetedRay(position, direction).o.xyz, .d.xyz
__global__ __launch_bounds__(256) void k_ray(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const float *p = in + 6 * i;
    const v3 pos = ld3(p), dir = ld3(p + 3);
    const Ray r = makeOffsetedRay(pos, dir);
    float *o = out + 8 * i;
    o[0] = __int_as_float(getMTBVHId(dir));
    o[1] = __int_as_float(getMTBVHId(-dir));
    st3(o + 2, r.o);
    st3(o + 5, r.d);
}

// in 1 u: a;  out 1 u: utilhash(a)
__global__ __launch_bounds__(256) void k_utilhash(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    out[i] = utilhash(in[i]);
}

// in 1 f: x;  out 2 f: sin, cos of sincos_det(x)
__global__ __launch_bounds__(256) void k_sincos(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    float s, c;
    sincos_det(in[i], s, c);
    out[2 * i] = s;
    out[2 * i + 1] = c;
}

// in 2 f: y, x;  out 1 f: atan2_det(y, x)
__global__ __launch_bounds__(256) void k_atan2(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    out[i] = atan2_det(in[2 * i], in[2 * i + 1]);
}

// in 2 f: uv;  out 3 f: toSphere(uv)
__global__ __launch_bounds__(256) void k_to_sphere(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    st3(out + 3 * i, toSphere(mk2(in[2 * i], in[2 * i + 1])));
}

// in 3 f: v;  out 2 f: toPlane(v)
__global__ __launch_bounds__(256) void k_to_plane(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const v2 r = toPlane(ld3(in + 3 * i));
    out[2 * i] = r.x;
    out[2 * i + 1] = r.y;
}

// in 2 f: f, g;  out 1 f: powerHeuristic(f, g)
__global__ __launch_bounds__(256) void k_power_heuristic(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    out[i] = powerHeuristic(in[2 * i], in[2 * i + 1]);
}

// in  20 : i type, f baseColor.xyz, f metallic, f roughness, f ior, f n.xyz, f wo.xyz, f wi.xyz, f r.xyz, 1 unused
// out 12 : f materialBSDF(n, wo, wi).xyz, f materialPdf(n, wo, wi), then materialSample(n, wo, r) into a zeroed BSDFSample:
//          f dir.xyz, f bsdf.xyz, f pdf, u type
__global__ __launch_bounds__(256) void k_material(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const float *p = in + 20 * i;
    const Material m{__float_as_int(p[0]), ld3(p + 1), p[4], p[5], p[6]};
    const v3 nrm = ld3(p + 7), wo = ld3(p + 10), wi = ld3(p + 13), r = ld3(p + 16);
    float *o = out + 12 * i;
    st3(o, materialBSDF(m, nrm, wo, wi));
    o[3] = materialPdf(m, nrm, wo, wi);
    BSDFSample s;
    s.dir = mk3(0.f);
    s.bsdf = mk3(0.f);
    s.pdf = 0.f;
    s.type = 0u;
    materialSample(m, nrm, wo, r, s);
    st3(o + 4, s.dir);
    st3(o + 7, s.bsdf);
    o[10] = s.pdf;
    o[11] = __uint_as_float(s.type);
}

// in 2 f: uv (finite);  out 3 f: proceduralTexture(uv)
__global__ __launch_bounds__(256) void k_procedural_texture(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    st3(out + 3 * i, proceduralTexture(mk2(in[2 * i], in[2 * i + 1])));
}

// in: a 4-word header {i width, i height, 0, 0}, then n records of 2 f: uv (finite), then width*height texels of 3 f.
// out 3 f: linearSample(texels, uv, width, height).  Nothing is masked here: the caller sends finite uv only (the function's texel
// index is int(NaN) otherwise: 0 on gfx950, still inside the array) and width, height >= 1.
__global__ __launch_bounds__(256) void k_linear_sample(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const int width = __float_as_int(in[0]), height = __float_as_int(in[1]);
    const float *uvs = in + 4, *texels = in + 4 + 2 * n;
    const v2 uv = mk2(uvs[2 * i], uvs[2 * i + 1]);
    st3(out + 3 * i, linearSample(texels, uv, width, height));
}

// in 1 f: x;  out 1 f: pow_gamma_det(x)
__global__ __launch_bounds__(256) void k_pow_gamma(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    out[i] = pow_gamma_det(in[i]);
}

// in 3 f: colour;  out 1 u: packRGBA(colour)
__global__ __launch_bounds__(256) void k_pack_rgba(const float *__restrict__ in, uint32_t *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    out[i] = packRGBA(ld3(in + 3 * i));
}

// in 3 f: colour;  out 6 f: filmic(colour).xyz, ACES(colour).xyz
__global__ __launch_bounds__(256) void k_tonemap(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const v3 c = ld3(in + 3 * i);
    st3(out + 6 * i, filmic(c));
    st3(out + 6 * i + 3, ACES(c));
}

// in 2 f: x, y;  out 6 f: exp_det(x), exp_det(y), exp_det2({x, y}).x, .y, pow_det(x, y), 0
__global__ __launch_bounds__(256) void k_exp_pow(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const float x = in[2 * i], y = in[2 * i + 1];
    const f2v e2 = exp_det2(f2v{x, y});
    float *o = out + 6 * i;
    o[0] = exp_det(x);
    o[1] = exp_det(y);
    o[2] = e2.x;
    o[3] = e2.y;
    o[4] = pow_det(x, y);
    o[5] = 0.f;
}

// in  20 : reservoir r (9 words: f Li.xyz, f wi.xyz, f dist, i numSamples, f weight), reservoir rhs (9 words), f rnd, i M
// out 45 : five reservoirs of 9 words, each starting from r: resvUpdate(rhs.sample, rhs.weight, rnd, faithful = true),
//          the same with faithful = false, resvMerge(rhs, rnd), resvPreClampedMerge(rhs, rnd, M), resvCheckValidity()
__global__ __launch_bounds__(256) void k_reservoir(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const float *p = in + 20 * i;
    const Reservoir r0 = loadReservoir(p, 0), rhs = loadReservoir(p, 1);
    const float rnd = p[18];
    const int M = __float_as_int(p[19]);
    float *o = out + 45 * i;
    Reservoir r = r0;
    resvUpdate(r, rhs.sample, rhs.weight, rnd, true);
    storeReservoir(o, 0, r);
    r = r0;
    resvUpdate(r, rhs.sample, rhs.weight, rnd, false);
    storeReservoir(o, 1, r);
    r = r0;
    resvMerge(r, rhs, rnd);
    storeReservoir(o, 2, r);
    r = r0;
    resvPreClampedMerge(r, rhs, rnd, M);
    storeReservoir(o, 3, r);
    r = r0;
    resvCheckValidity(r);
    storeReservoir(o, 4, r);
}

// in  24 : reservoir (9 words, as above), i type, f baseColor.xyz, f metallic, f roughness, f ior, f n.xyz, f wo.xyz, 2 unused
// out  1 f: W = weight / (|pHat| * numSamples), pHat = Li * materialBSDF(n, wo, sample.wi) * satDot(n, sample.wi), the two
//           statements of restirFinish (kernels_restir.h; restir.h:31-40) word for word
__global__ __launch_bounds__(256) void k_reservoir_w(const float *__restrict__ in, float *__restrict__ out, long long n) {
    const long long i = laneRecord();
    if (i >= n) return;
    const float *p = in + 24 * i;
    const Reservoir reservoir = loadReservoir(p, 0);
    const Material material{__float_as_int(p[9]), ld3(p + 10), p[13], p[14], p[15]};
    const v3 norm = ld3(p + 16), wo = ld3(p + 19);
    LightLiSample smp = reservoir.sample;
    v3 pHat = smp.Li * materialBSDF(material, norm, wo, smp.wi) * satDot(norm, smp.wi);  // restir.h:31-35
    float Wgt = reservoir.weight / (length(pHat) * static_cast<float>(reservoir.numSamples));  // :37-40
    out[i] = Wgt;
}

template <typename TI, typename TO>
int launch(void (*k)(const TI *, TO *, long long), const void *d_in, void *d_out, long long n, void *stream) {
    if (!d_in || !d_out || n <= 0) return -1;
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const TI *)d_in, (TO *)d_out, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

#define PROBE_ENTRY(name, kernel) \
    PROBE_API int probe_##name(const void *d_in, void *d_out, long long n, void *stream) { return launch(kernel, d_in, d_out, n, stream); }

PROBE_ENTRY(box, k_box)
PROBE_ENTRY(triangle, k_triangle)
PROBE_ENTRY(ray, k_ray)
PROBE_ENTRY(utilhash, k_utilhash)
PROBE_ENTRY(sincos, k_sincos)
PROBE_ENTRY(atan2, k_atan2)
PROBE_ENTRY(to_sphere, k_to_sphere)
PROBE_ENTRY(to_plane, k_to_plane)
PROBE_ENTRY(power_heuristic, k_power_heuristic)
PROBE_ENTRY(material, k_material)
PROBE_ENTRY(procedural_texture, k_procedural_texture)
PROBE_ENTRY(linear_sample, k_linear_sample)
PROBE_ENTRY(pow_gamma, k_pow_gamma)
PROBE_ENTRY(pack_rgba, k_pack_rgba)
PROBE_ENTRY(tonemap, k_tonemap)
PROBE_ENTRY(exp_pow, k_exp_pow)
PROBE_ENTRY(reservoir, k_reservoir)
PROBE_ENTRY(reservoir_w, k_reservoir_w)
