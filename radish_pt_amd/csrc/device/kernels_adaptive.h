// radish_pt_amd/csrc/device/kernels_adaptive.h — adaptive sampling: a per-pixel sample budget around the wavefront stages
// (rdh_path_trace_adaptive, rdh_adaptive_plan).
//
// k_wf_trace and k_wf_shade work on path slots and never look at a pixel (kernels_wave.h), so an uneven frame needs a new front end
// and a new back end only: a dense list of the requested (pixel, sample) pairs in front of stage 0, and a fold of every pixel's own
// slots behind the last stage.  The list is an ORDERED compaction of the request plane, as the light list is of the triangles
// (kernels_materials.h): three launches ordered by the stream, no atomic decides a slot, so the list repeats exactly.
//
//   k_ad_count     one lane per pixel in PixelMap's 8x8-block order: the request, checked, summed per wave and per 256-pixel workgroup
//   k_ad_scan      one workgroup: the exclusive prefix of the workgroup totals (scanBlockTotals) and the slot total T
//   k_ad_scatter   the request again; first slot of the pixel = workgroup offset + waves before (LDS) + lanes before (wave scan);
//                  every one of its r slots receives its owner, (pixel work index << 4) | sample number j
//   k_ad_raygen    one lane per slot: k_wf_raygen's body, seeded with the owner's row (looper + count + j) % 10000
//   ... k_wf_trace / k_wf_shade x (maxDepth + 1), untouched ...
//   k_ad_finish    the lane of a pixel's slot j = 0 folds the pixel's r slots in sample order and stores once
//
// Slot order: pixel-major inside block order.  A pixel's r slots are neighbours and a block's pixels follow each other, so the slot
// of a pixel's sample 0 is also the pixel's slotBase: no plane holds it, the owner list says it (j == 0), and a wave of stage 0
// carries the rays of one neighbourhood.  The images and counters do not depend on the order: the stages see slots only.
//
// k_ad_plan decides the requests from the running moments of the luminance; see there.
#pragma once
#include "kernels_wave.h"
#include "kernels_refit.h"

namespace rd {

constexpr int kAdaptiveMaxRequest = 16;  // RDH_ADAPTIVE_MAX_REQUEST: samples of one pixel in one pass, hence four bits of j
constexpr int kAdaptiveOwnerShift = 4;
constexpr long long kAdaptiveMaxWork = 1ll << 27;  // pixel work indices an owner can name; 16 slots each stay below 2^31

// The sum of v over the lanes up to and including this one (all 64 lanes must call it).
RD_DEV int waveInclusiveSum(int v) {
    const int lane = int(threadIdx.x & 63u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int x = __shfl_up(v, d, 64);
        if (lane >= d) v += x;
    }
    return v;
}

// Pixel work index -> pixel: the 8x8 block work >> 6 of this launch (mapPixel), lane work & 63.
RD_DEV Pix adaptivePixel(const PixelMap &pm, unsigned work) { return mapPixel(pm, work >> 6, work & 63u); }

// The head of the scan's scratch: what the host reads back in its one blocking copy.
struct AdaptiveHead {
    int err;    // a request outside 0..16, or a requested pixel's count negative or count + request beyond int32
    int total;  // T: the requested samples of the plane
};

// One lane per pixel.  A pixel without a request is not read beyond its request.
__global__ __launch_bounds__(256) void k_ad_count(PixelMap pm, const int *__restrict__ count, const int *__restrict__ request,
                                                  int *__restrict__ wgTotals, AdaptiveHead *head) {
    __shared__ int wsum[4];
    const unsigned work = blockIdx.x * 256u + threadIdx.x;
    const Pix px = adaptivePixel(pm, work);
    int r = 0;
    if (px.valid) {
        r = request[px.out];
        bool bad = r < 0 || r > kAdaptiveMaxRequest;
        if (!bad && r > 0) {
            const int c = count[px.out];
            bad = c < 0 || c > 0x7fffffff - r;
        }
        if (bad) {
            head->err = 1;  // every lane that gets here stores the same value
            r = 0;
        }
    }
    const int incl = waveInclusiveSum(r);
    if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x == 0) wgTotals[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Workgroup totals -> exclusive offsets in place, and T.
__global__ __launch_bounds__(256) void k_ad_scan(int *wgTotals, int nGroups, AdaptiveHead *head) {
    const int total = scanBlockTotals(wgTotals, nGroups);
    if (threadIdx.x == 0) head->total = total;
}

// Launched only for a plane that k_ad_count found valid.  `total` is the T the host read: nothing is written beyond it.
__global__ __launch_bounds__(256) void k_ad_scatter(PixelMap pm, const int *__restrict__ request, const int *__restrict__ wgOff, int total,
                                                    int *__restrict__ owner) {
    __shared__ int wsum[4];
    const unsigned work = blockIdx.x * 256u + threadIdx.x;
    const int wave = int(threadIdx.x >> 6);
    const Pix px = adaptivePixel(pm, work);
    int r = px.valid ? request[px.out] : 0;
    r = r < 0 ? 0 : (r > kAdaptiveMaxRequest ? kAdaptiveMaxRequest : r);
    const int incl = waveInclusiveSum(r);
    if ((threadIdx.x & 63u) == 63u) wsum[wave] = incl;
    __syncthreads();
    int base = wgOff[blockIdx.x] + incl - r;  // the pixel's slotBase
    for (int v = 0; v < wave; v++) base += wsum[v];
    for (int j = 0; j < r; j++)
        if (base + j < total) owner[base + j] = int(work << kAdaptiveOwnerShift) | j;
}

// ---- raygen from the list ---------------------------------------------------------------------------------------------------
// One lane per slot of the total padded to 64.  What it writes for a slot is what k_wf_raygen writes for the slot of that pixel and
// row: set 0 of the riding state, both accumulators zero, literal-class primary rays on stage 0's first list; the padding of the
// last 64-group gets -1 in rayq[0], and rayCount[0] is the padded total.
template <bool LENS>  // written once for k_ad_raygen and k_ad_raygen_lens, as wfRaygen (kernels_wave.h)
RD_DEV void adRaygen(const DScene &s, const DCamera &cam, const PixelMap &pm, const WaveWorkspace &w, int looper,
                     const int *__restrict__ count, const int *__restrict__ owner, int total, const DLens &lens) {
    unsigned wg;
    const unsigned nGroups = ((unsigned)total + 63u) >> 6;
    const bool wgValid = xcdSwizzle(blockIdx.x, (nGroups + 3u) >> 2, wg);
    const unsigned lane = threadIdx.x & 63u;
    const unsigned group = wgValid ? wg * 4u + (threadIdx.x >> 6) : 0xffffffffu / 64u;
    const bool inRange = wgValid && group < nGroups;
    const int p = int(group * 64u + lane);  // the path's home slot; its slot in stage 0 as well
    const bool valid = inRange && p < total;
    bool listed = false;
    if (valid) {
        const unsigned o = (unsigned)owner[p];
        const Pix px = adaptivePixel(pm, o >> kAdaptiveOwnerShift);
        const unsigned j = o & (unsigned)(kAdaptiveMaxRequest - 1);
        // the pixel's own row: count < 2^31, looper < 10000, j < 16, so the unsigned sum is exact
        const unsigned row = ((unsigned)looper + (unsigned)count[px.out] + j) % (unsigned)kSobolRows;
        Sampler rng = makeSeededRandomEngine(int(row), px.index, 0, s.sobol);
        Ray ray = cameraSample<LENS>(cam, px.x, px.y, sample4D(rng), lens);
        w.ro[0][p] = make_float4(ray.o.x, ray.o.y, ray.o.z, 0.f);
        w.rd[0][p] = make_float4(ray.d.x, ray.d.y, ray.d.z, 0.f);
        w.accD[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.accI[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.rng[0][p] = make_uint2(rng.scramble, (unsigned)rng.ptr);
        if (fabs_(ray.d.x) < 1.1e-6f || fabs_(ray.d.y) < 1.1e-6f || fabs_(ray.d.z) < 1.1e-6f) {  // (as k_wf_raygen)
            const int at = atomicAdd(&w.ctr->litCount[0].v, 1);
            if (at < w.litCap) {
                w.litq[0][at] = p;
                listed = true;
            }
        }
    }
    if (inRange) w.rayq[0][p] = valid ? (listed ? -2 - p : p) : -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) w.ctr->rayCount[0][0].v = int(nGroups) * 64;
}
__global__ __launch_bounds__(256) void k_ad_raygen(DScene s, DCamera cam, PixelMap pm, WaveWorkspace w, int looper,
                                                   const int *__restrict__ count, const int *__restrict__ owner, int total) {
    adRaygen<false>(s, cam, pm, w, looper, count, owner, total, DLens{});
}
__global__ __launch_bounds__(256) void k_ad_raygen_lens(DScene s, DCamera cam, PixelMap pm, WaveWorkspace w, int looper,
                                                        const int *__restrict__ count, const int *__restrict__ owner, int total,
                                                        DLens lens) {
    adRaygen<true>(s, cam, pm, w, looper, count, owner, total, lens);
}

// ---- finish -------------------------------------------------------------------------------------------------------------------
// One thread per pixel with a request: the lane of the pixel's slot j = 0 (the launch is one lane per slot, so its cost follows T
// like everything else).  The two means, the count and the moments are loaded once, the r slots folded in sample order, each with
// storeRunningMean's expression at its own iter c + j (foldRunningMean), and everything is stored once.  The moments are the
// running means of L and L * L, L = luminance(finishSample(accD) + finishSample(accI)), folded alike.  moments may be null.
__global__ __launch_bounds__(256) void k_ad_finish(PixelMap pm, WaveWorkspace w, const int *__restrict__ owner, int total,
                                                   int *__restrict__ count, const int *__restrict__ request,
                                                   float *__restrict__ directIllum, float *__restrict__ indirectIllum,
                                                   float *__restrict__ moments) {
    const int p = int(blockIdx.x * 256u + threadIdx.x);
    if (p >= total) return;
    const unsigned o = (unsigned)owner[p];
    if ((o & (unsigned)(kAdaptiveMaxRequest - 1)) != 0u) return;
    const Pix px = adaptivePixel(pm, o >> kAdaptiveOwnerShift);
    int r = request[px.out];
    r = r < total - p ? r : total - p;  // (the plane k_ad_scatter saw: never beyond the list)
    const int c = count[px.out];
    v3 direct = load3(directIllum, px.out), indirect = load3(indirectIllum, px.out);
    float m1 = 0.f, m2 = 0.f;
    if (moments) {
        m1 = moments[2 * px.out];
        m2 = moments[2 * px.out + 1];
    }
    for (int j = 0; j < r; j++) {
        const float4 aD = w.accD[p + j], aI = w.accI[p + j];
        const int n = c + j;
        direct = foldRunningMean(direct, aD, n);
        indirect = foldRunningMean(indirect, aI, n);
        const float L = luminance(finishSample(mk3(aD.x, aD.y, aD.z)) + finishSample(mk3(aI.x, aI.y, aI.z)));
        m1 = (m1 * float(n) + L) / float(n + 1);
        m2 = (m2 * float(n) + L * L) / float(n + 1);
    }
    store3(directIllum, px.out, direct);
    store3(indirectIllum, px.out, indirect);
    if (moments) {
        moments[2 * px.out] = m1;
        moments[2 * px.out + 1] = m2;
    }
    count[px.out] = c + r;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------
// One wave per 8x8 block (mapPixel), all float32, in exactly this order (tests/adaptive_model.py restates it in numpy):
//   a valid pixel WANTS samples if n < minSamples, or if err2 > tol * tol with
//       var = m2 - m1 * m1,  err2 = var / float(n),  tol = threshold * (m1 + 0.01f)
//   (false for NaN; a negative var needs no clamp).  A block is ACTIVE if any of its valid pixels wants: a pixel whose samples all
//   missed the lamp has variance 0 and must not be trusted on its own.  Every valid pixel of an active block with n < maxSamples
//   gets min(step, maxSamples - n), every other valid pixel 0.
// The three statistics are integer sums: one atomic each per wave that has something to add.
struct AdaptiveStats {  // == rdh_adaptive_stats
    long long samplesRequested;
    int activeBlocks, wantingPixels;
};
__global__ __launch_bounds__(256) void k_ad_plan(PixelMap pm, const int *__restrict__ count, const float *__restrict__ moments,
                                                 int *__restrict__ request, int minSamples, int maxSamples, int step, float threshold,
                                                 AdaptiveStats *stats) {
    const unsigned work = blockIdx.x * 256u + threadIdx.x;
    const Pix px = adaptivePixel(pm, work);
    bool wants = false;
    int n = 0;
    if (px.valid) {
        n = count[px.out];
        if (n < minSamples) {
            wants = true;
        } else {
            const float m1 = moments[2 * px.out], m2 = moments[2 * px.out + 1];
            const float var = m2 - m1 * m1;
            const float err2 = var / float(n);
            const float tol = threshold * (m1 + 0.01f);
            wants = err2 > tol * tol;
        }
    }
    const unsigned long long wantM = __ballot(wants);
    const bool active = wantM != 0ull;
    int req = 0;
    if (px.valid && active && n < maxSamples) {
        const long long room = (long long)maxSamples - (long long)n;
        req = room < (long long)step ? int(room) : step;
    }
    if (px.valid) request[px.out] = req;
    const int sum = waveInclusiveSum(req);
    if ((threadIdx.x & 63u) == 63u && active) {
        if (sum > 0) atomicAdd(reinterpret_cast<unsigned long long *>(&stats->samplesRequested), (unsigned long long)sum);
        atomicAdd(&stats->activeBlocks, 1);
        atomicAdd(&stats->wantingPixels, __popcll(wantM));
    }
}

}  // namespace rd
