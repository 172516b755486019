// radish_pt_amd/csrc/device/kernels_lights.h — the light sampler rebuilt on the device (rdh_scene_rebuild_lights,
// rdh_build_alias_table_device).
//
// rdh_build_alias_table (host/scene_build.cpp, after src/sampler.h:81-125) is Vose's construction with two LIFO piles.  A big entry
// that stays above 1 goes back on top of the `over` pile and is popped again at once; one that falls to <= 1 goes on top of the
// `under` pile and is the next small.  So neither pile is ever read below its top except to take the next ORIGINAL entry: the
// construction is one sweep over the two classified lists from the back, carrying one float.  The kernels below repeat the host's
// operations one for one (a strictly sequential binary32 sum, float(n) / sum, one multiply per value, r - (1.f - p) per step), so
// table and sum come out with the host's bits; the library is built with -ffp-contract=off like the host's.
//
//   k_light_power    one lane per light: rdh_build_light_list's power expression on the scene's current LightRecs
//   k_alias_classify one wave: sum, scale, and the order-keeping split into `over` (val > 1) and `under` as {id, val} records
//   k_alias_sweep    one wave: the recurrence, wave-uniform, both lists staged 64 records at a time in registers
//   k_light_precompute_dev   k_light_precompute with sumLightPowerInv read from device memory
//
// Every launch is ordered by the stream; nothing is handed over between workgroups inside a kernel.
#pragma once
#include "kernels_restir.h"

namespace rd {

struct AliasWork {
    int2 *over;    // n records {id, val bits}, ascending id: val > 1
    int2 *under;   // n records: the rest (val <= 1, NaN)
    float *sums;   // [0] sum, [1] 1.f / sum
    int *counts;   // [0] entries of over, [1] of under
};

RD_DEV int laneBelow(unsigned long long mask) {  // set bits of `mask` below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
RD_DEV float uniformF(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }
RD_DEV float laneF(float x, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane)); }

// rdh_build_light_list's power of one emissive triangle (scene_build.cpp), operation for operation.
RD_DEV float emitterPower(v3 v0, v3 v1, v3 v2_, float r, float g, float b) {
    const float lum = 0.2126f * r + 0.7152f * g + 0.0722f * b;
    const float powerUnitArea = lum * 2.f * 3.14159265358979323846264338327950288f;
    const v3 c = cross(v1 - v0, v2_ - v0);
    const float area = __builtin_sqrtf(dot(c, c)) * 0.5f;
    return powerUnitArea * area;
}

// power[i] = luminance(radiance) * 2 * pi * area of light i (scene_build.cpp, rdh_build_light_list); entries numLights .. n - 1 (the
// environment map's, at most one) = envPower.
__global__ __launch_bounds__(256) void k_light_power(const LightRec *__restrict__ lights, int numLights, int n, float envPower,
                                                     float *__restrict__ power) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (i >= numLights) {
        power[i] = envPower;
        return;
    }
    const float4 A = lights[i].a, B = lights[i].b, C = lights[i].c;
    power[i] = emitterPower(mk3(A.x, A.y, A.z), mk3(A.w, B.x, B.y), mk3(B.z, B.w, C.x), C.y, C.z, C.w);
}

// One wave.  The sum's order is fixed (index order), so a tile of 64 values is loaded in one coalesced load and added lane by lane
// from registers: 64 dependent adds per tile, every lane carrying the same sum.
__global__ __launch_bounds__(64) void k_alias_classify(const float *__restrict__ values, int n, AliasWork w) {
    const int lane = (int)threadIdx.x;
    float sum = 0.f;
    for (int base = 0; base < n; base += 64) {
        const int cnt = n - base < 64 ? n - base : 64;
        const float v = lane < cnt ? values[base + lane] : 0.f;
        if (cnt == 64) {
#pragma unroll
            for (int j = 0; j < 64; j++) sum += laneF(v, j);
        } else {
            for (int j = 0; j < cnt; j++) sum += laneF(v, j);
        }
    }
    sum = uniformF(sum);
    const float scale = static_cast<float>(n) / sum;
    int nOver = 0, nUnder = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n;
        const float val = in ? values[i] * scale : 0.f;
        const bool isOver = in && val > 1.f;
        const unsigned long long mOver = __ballot(isOver), mIn = __ballot(in);
        const unsigned long long mUnder = mIn & ~mOver;
        const int2 rec = make_int2(i, __builtin_bit_cast(int, val));
        if (isOver) w.over[nOver + laneBelow(mOver)] = rec;
        else if (in) w.under[nUnder + laneBelow(mUnder)] = rec;
        nOver += __popcll(mOver);
        nUnder += __popcll(mUnder);
    }
    if (lane == 0) {
        w.sums[0] = sum;
        w.sums[1] = 1.f / sum;
        w.counts[0] = nOver;
        w.counts[1] = nUnder;
    }
}

// One wave.  Both lists are read from the back; a finished entry {slot, prob, failId} is parked in lane nOut's registers and the 64
// of them leave with one vector store per lane.  State (wave-uniform): the current big (B, r) and a pending small (S, p) — a big
// that fell to <= 1.  Each step finalises one entry, so there are at most n - 1 steps whatever the values are.
__global__ __launch_bounds__(64) void k_alias_sweep(AliasWork w, AliasRec *__restrict__ table) {
    const int lane = (int)threadIdx.x;
    int oTop = __builtin_amdgcn_readfirstlane(w.counts[0]);  // unread entries of over: [0, oTop)
    int uTop = __builtin_amdgcn_readfirstlane(w.counts[1]);
    int2 oTile = make_int2(0, 0), uTile = make_int2(0, 0);   // lane L: record top - 1 - L of the list when the tile was staged
    int oPos = 64, uPos = 64;                                // next lane of the tile to take; 64 = stage another
    int outSlot = 0, outFail = 0, nOut = 0;
    float outProb = 0.f;
    bool haveBig = false, havePend = false;
    int B = 0, S = 0;
    float r = 0.f, p = 0.f;

    auto flush = [&]() {
        if (lane < nOut) table[outSlot] = AliasRec{outProb, outFail};
        nOut = 0;
    };
    auto emit = [&](int slot, float prob, int failId) {
        if (lane == nOut) {
            outSlot = slot;
            outProb = prob;
            outFail = failId;
        }
        if (++nOut == 64) flush();
    };

    for (;;) {
        if (!haveBig) {
            if (oTop == 0) break;
            if (oPos == 64) {
                if (lane < oTop) oTile = w.over[oTop - 1 - lane];
                oPos = 0;
            }
            B = __builtin_amdgcn_readlane(oTile.x, oPos);
            r = __builtin_bit_cast(float, __builtin_amdgcn_readlane(oTile.y, oPos));
            oPos++;
            oTop--;
            haveBig = true;
        }
        if (!havePend) {
            if (uTop == 0) break;
            if (uPos == 64) {
                if (lane < uTop) uTile = w.under[uTop - 1 - lane];
                uPos = 0;
            }
            S = __builtin_amdgcn_readlane(uTile.x, uPos);
            p = __builtin_bit_cast(float, __builtin_amdgcn_readlane(uTile.y, uPos));
            uPos++;
            uTop--;
        }
        havePend = false;
        emit(S, p, B);
        r = uniformF(r - (1.f - p));
        if (!(r > 1.f)) {  // also when r is NaN, as the host's `big.prob > 1.f ? over : under`
            S = B;
            p = r;
            havePend = true;
            haveBig = false;
        }
    }
    if (haveBig) emit(B, r, B);
    if (havePend) emit(S, p, S);
    flush();
    // whatever neither pile gave up keeps its own value and names itself
    for (int i = lane; i < oTop; i += 64) {
        const int2 e = w.over[i];
        table[e.x] = AliasRec{__builtin_bit_cast(float, e.y), e.x};
    }
    for (int i = lane; i < uTop; i += 64) {
        const int2 e = w.under[i];
        table[e.x] = AliasRec{__builtin_bit_cast(float, e.y), e.x};
    }
}

// k_light_precompute for a sumLightPowerInv that is still on its way to the host (rdh_scene_rebuild_lights).
__global__ __launch_bounds__(256) void k_light_precompute_dev(const LightRec *__restrict__ lights, LightPre *__restrict__ out, int n,
                                                              const float *__restrict__ sumLightPowerInv) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float inv = *sumLightPowerInv;
    const float4 A = lights[i].a, B = lights[i].b, C = lights[i].c;
    const v3 v0 = mk3(A.x, A.y, A.z), v1 = mk3(A.w, B.x, B.y), v2_ = mk3(B.z, B.w, C.x);
    const v3 normal = triangleNormal(v0, v1, v2_);
    const float area = triangleArea(v0, v1, v2_);
    const float power = luminance(mk3(C.y, C.z, C.w)) / (area * 2.f * PI_F);  // scene.h:489
    out[i].a = A;
    out[i].b = B;
    out[i].c = C;
    out[i].d = make_float4(normal.x, normal.y, normal.z, power * inv);
}

}  // namespace rd
