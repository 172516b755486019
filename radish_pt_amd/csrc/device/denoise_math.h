// radish_pt_amd/csrc/device/denoise_math.h — the denoisers' fixed exp / pow recipes (scalar and packed), free of kernels so that
// kernels_denoise.h and the test-only probe (tests/probe/device_probe.hip) compile the same text.
#pragma once
#include "traverse.h"  // f2v

namespace rd {

// e^x: n = rint(x log2 e), r = x - n ln2 (two-term Cody-Waite), degree-6 polynomial on [-ln2/2, ln2/2], scale by 2^n.
RD_DEV float exp_det(float x) {
    if (!(x == x)) return x;
    if (x > 88.7f) return __builtin_inff();
    if (x < -87.3f) return 0.f;  // below the smallest normal: the reference's weights flush to ~0 there as well
    float n = __builtin_rintf(x * 1.44269504088896341f);
    float r = (x - n * 0.693359375f) - n * -2.12194440e-4f;
    float p = 1.f + r * (1.f + r * (0.5f + r * (0.166666671633720f + r * (0.0416666679084301f +
                  r * (0.00833333376795053f + r * 0.00138888892252f)))));
    return __uint_as_float(__float_as_uint(p) + ((uint32_t)(int)n << 23));
}
// x^y for x >= 0 (Math::satDot(...) ^ sigNormal): 0^y = 0 for y > 0, else 2^(y log2 x) with pow_gamma_det's log2 / exp2.
RD_DEV float pow_det(float x, float y) {
    if (!(x > 0.f)) return (x == 0.f && y > 0.f) ? 0.f : ((x == 0.f && y == 0.f) ? 1.f : __builtin_nanf(""));
    if (x == __builtin_inff()) return x;
    int eAdj = 0;
    if (x < 1.17549435e-38f) {
        x = x * 16777216.f;
        eAdj = -24;
    }
    uint32_t bits = __float_as_uint(x);
    int e = int((bits >> 23) & 0xffu) - 126 + eAdj;
    float m = __uint_as_float((bits & 0x007fffffu) | 0x3f000000u);
    if (m < 0.70710678118654752f) {
        m = m + m;
        e = e - 1;
    }
    float sN = (m - 1.f) / (m + 1.f);
    float z = sN * sN;
    float p = sN + sN * z * (0.333333333333f + z * (0.2f + z * (0.142857142857f + z * 0.111111111111f)));
    float l2 = p * 2.8853900817779268f;
    float t = (float(e) + l2) * y;
    if (t > 127.9f) return __builtin_inff();
    if (t < -125.9f) return 0.f;
    float n = __builtin_rintf(t);
    float f = t - n;
    float q = 1.f + f * (0.69314718056f + f * (0.240226506959f + f * (0.0555041086648f + f * (0.00961812910763f +
                  f * (0.00133335581464f + f * 0.000154035303934f)))));
    return __uint_as_float(__float_as_uint(q) + ((uint32_t)(int)n << 23));
}

RD_DEV f2v splat2(float v) { return f2v{v, v}; }
RD_DEV f2v exp_det2(f2v x) {  // exp_det on both halves
    f2v n = x * splat2(1.44269504088896341f);
    n = f2v{__builtin_rintf(n.x), __builtin_rintf(n.y)};
    const f2v r = (x - n * splat2(0.693359375f)) - n * splat2(-2.12194440e-4f);
    const f2v p = splat2(1.f) + r * (splat2(1.f) + r * (splat2(0.5f) + r * (splat2(0.166666671633720f) + r * (splat2(0.0416666679084301f) +
                  r * (splat2(0.00833333376795053f) + r * splat2(0.00138888892252f))))));
    float a = __uint_as_float(__float_as_uint(p.x) + ((uint32_t)(int)n.x << 23));
    float b = __uint_as_float(__float_as_uint(p.y) + ((uint32_t)(int)n.y << 23));
    a = (x.x < -87.3f) ? 0.f : a;
    b = (x.y < -87.3f) ? 0.f : b;
    a = (x.x > 88.7f) ? __builtin_inff() : a;
    b = (x.y > 88.7f) ? __builtin_inff() : b;
    a = (x.x == x.x) ? a : x.x;
    b = (x.y == x.y) ? b : x.y;
    return f2v{a, b};
}

}  // namespace rd
