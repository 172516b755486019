// radish_pt_amd/csrc/device/path_step.h — the path's shading step, written once.
//
// singleKernelPT (/root/reference/src/pathtrace.cu:149-291) shades a closest hit with four expressions: the NEE contribution, the MIS
// weight of an emitter that a BSDF sample hits, the MIS weight of the environment on a miss, and the throughput update after a BSDF
// sample.  They are here, each once.  k_path_trace_mega (kernels_pt.h) keeps the reference's control flow — it traces the shadow ray
// before it evaluates the BSDF — and calls them in place.  The kernels that trace a ray elsewhere and come back to shade its hit
// (k_pt_persistent, k_wf_shade) run the whole bounce body through pathStep below; they differ only in where a path's state lives, and
// each hands pathStep an accessor for it.
#pragma once
#include "lights.h"

namespace rd {

// `c` of pathtrace.cu:201-207: what an unoccluded light sample adds (lightPdf > 0)
RD_DEV v3 neeContribution(const Material &material, const Surface &isec, v3 throughput, v3 radiance, v3 wi, float lightPdf) {
    float BSDFPdf = materialPdf(material, isec.norm, isec.wo, wi);
    return throughput * materialBSDF(material, isec.norm, isec.wo, wi) * radiance * satDot(isec.norm, wi) / lightPdf *
           powerHeuristic(lightPdf, BSDFPdf);
}
// MIS weight of the emitter `isec` that a non-specular BSDF sample of density samplePdf, drawn at prevPos, has hit (:257-266)
RD_DEV float emitterHitWeight(const DScene &s, v3 radiance, const Surface &isec, v3 prevPos, float samplePdf) {
    return powerHeuristic(samplePdf, pdfAreaToSolidAngle(luminance(radiance) * s.sumLightPowerInv * getPrimitiveArea(s, isec.primId),
                                                         prevPos, isec.pos, isec.norm));
}
// ... and of the environment map when such a sample leaves the scene along dir (:232-247)
RD_DEV float envMissWeight(const DScene &s, v3 dir, float samplePdf) { return powerHeuristic(samplePdf, environmentMapPdf(s, dir)); }
// the factor a valid BSDF sample puts on the throughput (:216-219)
RD_DEV v3 bsdfSampleWeight(const BSDFSample &sample, v3 norm) {
    return sample.bsdf / sample.pdf * ((sample.type & Specular) != 0 ? 1.f : absDot(norm, sample.dir));
}
// one accumulated sample as it enters the running mean: NaN/Inf scrub, then tone mapping (:279-286)
RD_DEV v3 finishSample(v3 v) {
    if (hasNanOrInf(v)) v = mk3(0.f);
    return HDRToLDR(v);
}

// What the caller has to schedule after pathStep.  Neither ray: the path has ended.
struct PathStepResult {
    bool shadow = false;     // a shadow ray shadowFrom -> shadowTo decides whether the contribution given to setNee is added
    bool extension = false;  // the path goes on along `ray` (given to setRay as well), after the shadow ray if there is one
    v3 shadowFrom, shadowTo;
    Ray ray;
    RD_DEV bool goesOn() const { return shadow || extension; }
};

// Hit k of a path (k = 0: the primary ray's): miss or emitter termination with the MIS weight, the depth bound, then bounce body
// k + 1 — normal flip, NEE pick and contribution, BSDF sample, throughput update and offset extension ray — in the megakernel's
// order of RNG draws and additions.  `prim` = -1 is a miss; `rayDir` is the direction of the ray that led here.
//
// PathState is the kernel's view of the path's state:
//   throughput() samplePdf() sampleDelta() prevPos()   of the BSDF sample that made this ray (asked for k > 0 only)
//   setDirect(v) addIndirect(v)                        the two accumulators
//   rng(s)                                             the path's sampler
//   setNee(c, w)                                       pending NEE contribution; w: 0 -> direct, 1 -> indirect, -1 -> nothing to add
//   setPrevPos(x)                                      the position the next rays leave from
//   setRay(ray, pdf, delta, throughput, rng)           the extension ray and everything that rides with it
// Every getter is called on the one branch that needs its value, so state that lives in memory is read only there, and nothing is
// written on a branch that ends the path beyond what that branch adds.  Where the two kernels' earlier copies differed, this is the
// wavefront's form: the sampler's state is stored with an extension ray only (it is dead when none follows), and a sample that
// yields no ray leaves the stored ray alone — a caller that asks its stored state later whether a ray is pending (k_pt_persistent,
// after the shadow ray) notes that from the result.
template <class PathState>
RD_DEV PathStepResult pathStep(const DScene &s, int k, int maxDepth, int prim, v2 bary, v3 rayDir, PathState &st) {
    PathStepResult r;
    if (prim == -1) {  // miss: pathtrace.cu:169-172 (primary), :232-247 (later)
        if (k == 0) {
            st.setDirect(mk3(1.f));
        } else if (hasEnvMap(s)) {
            v3 radiance = envLookup(s, rayDir) * st.throughput();
            float weight = st.sampleDelta() ? 1.f : envMissWeight(s, rayDir, st.samplePdf());
            st.addIndirect(radiance * weight);
        }
        return r;
    }
    Surface isec;
    fetchSurface(s, prim, bary, isec);
    Material material = texturedMaterial(s, isec);
    v3 throughput;
    if (k == 0) {
        material.baseColor = mk3(1.f);  // DENOISER_DEMODULATE (:175-178)
        if (material.type == Light) {   // :179-182
            st.setDirect(mk3(1.f));
            return r;
        }
        throughput = mk3(1.f);
    } else {
        throughput = st.throughput();
        if (material.type == Light) {  // :251-271
            if (dot(isec.norm, rayDir) < 0.f) return r;  // SCENE_LIGHT_SINGLE_SIDED (:252-256)
            v3 radiance = material.baseColor;
            float weight = st.sampleDelta() ? 1.f : emitterHitWeight(s, radiance, isec, st.prevPos(), st.samplePdf());
            st.addIndirect(radiance * throughput * weight);
            return r;
        }
    }
    const int depth = k + 1;
    if (depth > maxDepth) return r;  // loop bound of pathtrace.cu:187
    isec.wo = -rayDir;
    bool deltaBSDF = (material.type == Dielectric);
    if (material.type != Dielectric && dot(isec.norm, isec.wo) < 0.f) isec.norm = -isec.norm;
    Sampler rng = st.rng(s);
    if (!deltaBSDF) {  // NEE (:195-208); the caller has the shadow ray traced
        v4 r4 = sample4D(rng);
        if (s.lightSamplerLength != 0) {
            LightPick lp = pickLightPoint(s, isec.pos, r4);
            v3 radiance = mk3(0.f), wi = mk3(0.f);
            float lightPdf = lightPdfUnoccluded(s, isec.pos, lp, radiance, wi);
            v3 c = mk3(0.f);
            float nw = -1.f;
            if (lightPdf > 0.f) {
                c = neeContribution(material, isec, throughput, radiance, wi, lightPdf);
                nw = depth == 1 ? 0.f : 1.f;
            }
            st.setNee(c, nw);
            r.shadow = true;  // traced even when nothing can be added: sampleDirectLight tests occlusion before the single-sided
                              // rejection
            r.shadowFrom = isec.pos;
            r.shadowTo = lp.sampled;
        }
    }
    st.setPrevPos(isec.pos);
    BSDFSample sample;
    sample.pdf = 0.f;
    materialSample(material, isec.norm, isec.wo, sample3D(rng), sample);
    if (sample.type == Invalid) return r;
    else if (sample.pdf < 1e-8f) return r;
    throughput = throughput * bsdfSampleWeight(sample, isec.norm);
    r.ray = makeOffsetedRay(isec.pos, sample.dir);
    r.extension = true;
    st.setRay(r.ray, sample.pdf, (sample.type & Specular) != 0, throughput, rng);
    return r;
}

}  // namespace rd
