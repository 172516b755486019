// radish_pt_amd/csrc/device/reservoir.h — ReSTIR's reservoir record and its arithmetic (restir.h:10-99), free of kernels so that
// kernels_restir.h and the test-only probe (tests/probe/device_probe.hip) compile the same text.
#pragma once
#include "rmath.h"

namespace rd {

struct LightLiSample {  // restir.h:95-99
    v3 Li, wi;
    float dist;
};
struct Reservoir {  // restir.h:10-92, 36 B when stored
    LightLiSample sample;
    int numSamples;
    float weight;
};
RD_DEV Reservoir emptyReservoir() { return Reservoir{{mk3(0.f), mk3(0.f), 0.f}, 0, 0.f}; }
RD_DEV Reservoir loadReservoir(const float *buf, long long i) {
    const float *p = buf + 9 * i;
    Reservoir r;
    r.sample.Li = mk3(p[0], p[1], p[2]);
    r.sample.wi = mk3(p[3], p[4], p[5]);
    r.sample.dist = p[6];
    r.numSamples = __float_as_int(p[7]);
    r.weight = p[8];
    return r;
}
RD_DEV void storeReservoir(float *buf, long long i, const Reservoir &r) {
    float *p = buf + 9 * i;
    p[0] = r.sample.Li.x; p[1] = r.sample.Li.y; p[2] = r.sample.Li.z;
    p[3] = r.sample.wi.x; p[4] = r.sample.wi.y; p[5] = r.sample.wi.z;
    p[6] = r.sample.dist;
    p[7] = __int_as_float(r.numSamples);
    p[8] = r.weight;
}
RD_DEV void resvUpdate(Reservoir &r, const LightLiSample &s, float newWeight, float rnd, bool faithful) {  // restir.h:17-24
    r.weight += newWeight;
    r.numSamples++;
    // restir.h:21 tests a float for truthiness; the corrected form is the usual `rand*W < w`.
    bool take = faithful ? ((rnd * r.weight / newWeight) != 0.f) : (rnd * r.weight < newWeight);
    if (take) r.sample = s;
}
RD_DEV bool resvInvalid(const Reservoir &r) { return isNanOrInf(r.weight) || r.weight < 0.f; }  // :42
RD_DEV void resvCheckValidity(Reservoir &r) {  // :44-49 → clear() :26-29 (keeps the stale sample)
    if (resvInvalid(r)) {
        r.weight = 0.f;
        r.numSamples = 0;
    }
}
RD_DEV void resvMerge(Reservoir &r, const Reservoir &rhs, float rnd) {  // :51-58
    r.weight += rhs.weight;
    r.numSamples += rhs.numSamples;
    if (rnd * r.weight < rhs.weight) r.sample = rhs.sample;
}
RD_DEV void resvPreClampedMerge(Reservoir &r, Reservoir rhs, float rnd, int M) {  // :69-77
    if (rhs.numSamples > 0 && rhs.numSamples > (M - 1) * r.numSamples && r.numSamples > 0) {
        rhs.weight *= static_cast<float>(M - 1) * r.numSamples / rhs.numSamples;
        rhs.numSamples = (M - 1) * r.numSamples;
    }
    resvMerge(r, rhs, rnd);
}

}  // namespace rd
