// radish_pt_amd/csrc/device/kernels_gbuffer.h — renderGBuffer (gBuffer.cu:3-76) over the walk-only bodies of kernels_walk.h.
//
// k_gbuffer (kernels_pt.h) binds a pixel to a lane for the whole launch, so every wave waits for the longest of its 64
// primary rays (measured on the teapots scene: 2.97 ms for 2.07 M rays, a quarter of k_pt_persistent's rate).  The kernels here
// are the three walk-only bodies with a pixel as the item of work (PixelWork): its un-jittered centre ray goes in, its G-buffer
// record comes out.  Same centre ray, same walk, same record per pixel as k_gbuffer.
//   k_gbuffer_persistent   walkLanes: a lane whose ray has ended writes its record (batched: once 16 lanes wait) and takes the
//                          next pixel
//   k_gbuffer_packet       walkPacket: one 8x8 block per wave
//   k_gbuffer_literal      wgTraceItem: one workgroup per literal-class pixel listed by k_gbuffer_find_literal
#pragma once
#include "kernels_walk.h"

namespace rd {

#ifndef RD_PIX_REFILL_MIN
#define RD_PIX_REFILL_MIN 16
#endif
#ifndef RD_GB_FINISH_MIN
#define RD_GB_FINISH_MIN 16
#endif

// One pixel's G-buffer record (gBuffer.cu:28-67), from the primary ray's closest hit.
RD_DEV void gbufStore(const DScene &s, const DCamera &cam, const DCamera &lastCam, const GBufPtrs &gb, int idx, const RaySlab &rs,
                      int hitPrim, v2 hitBary) {
    if (hitPrim != -1) {
        Surface isec;
        fetchSurface(s, hitPrim, hitBary, isec);
        // first, while prim and bary are live anyway: kept to the end they cost k_gbuffer_packet its seventh wave (75 VGPRs for 72)
        gb.motion[idx] = gbufMotionIndex(cam, lastCam, gb, isec, hitBary);
        int matId = isec.matId;
        if (loadMaterial(s.mats, isec.matId).type == Light) matId = -2;  // NullPrimitive - 1 (gBuffer.cu:33-37)
        Material material = texturedMaterial(s, isec);                  // :44 (may perturb isec.norm)
        store3(gb.albedo, idx, material.baseColor);
        store3(gb.normal, idx, isec.norm);
        gb.primId[idx] = matId;
        gb.depth[idx] = length(rs.o - isec.pos);
    } else {
        store3(gb.albedo, idx, hasEnvMap(s) ? envLookup(s, rs.d) : mk3(0.f));  // :61-66
        store3(gb.normal, idx, mk3(0.f));
        gb.primId[idx] = -1;
        gb.depth[idx] = 1.f;
        gb.motion[idx] = 0;
    }
}

// The un-jittered centre ray of pixel (x, y) (gBuffer.cu:11-26).
RD_DEV Ray gbufPrimaryRay(const DCamera &cam, int x, int y) {
    float aspect = float(cam.resx) / float(cam.resy);
    v2 pixelsize = {1.f / float(cam.resx), 1.f / float(cam.resy)};
    v2 scr = mk2(float(x), float(y)) * pixelsize;
    v2 ruv = scr + pixelsize * mk2(0.5f, 0.5f);
    ruv = {1.f - ruv.x * 2.f, 1.f - ruv.y * 2.f};
    v3 pLens = mk3(0.f);
    v2 f = (ruv * mk2(aspect, 1.f)) * cam.tanFovY;
    v3 pFocus = mk3(f.x, f.y, 1.f) * cam.focalDist;
    v3 dir = pFocus - pLens;
    Ray ray;
    ray.o = cam.position + cam.right * pLens.x + cam.up * pLens.y;
    ray.d = normalize(mul(m3{cam.right, cam.up, cam.view}, dir));
    return ray;
}

// The work of the G-buffer kernels: the centre ray of a pixel, its record in the G-buffer's planes.  A chunk is an 8x8 pixel
// block, a slot a pixel of it (mapPixel); SWIZZLE: the chunk index is a position in the XCD-aware order of the blocks (workgroup-
// sized groups of 4, as in the one-shot kernels), padded to a multiple of 8 groups — a position in the padding holds no pixel.
template <bool SWIZZLE>
struct PixelWork {
    const DCamera &cam, &lastCam;
    const PixelMap *pm;  // the chunked form only
    const GBufPtrs &gb;
    int idx, x, y;  // the pixel taken last

    RD_DEV bool find(long long chunk, int slot) {
        unsigned blk = (unsigned)chunk;
        bool ok = true;
        if (SWIZZLE) {
            unsigned wgLogical;
            ok = xcdSwizzle(blk >> 2, (unsigned)(pm->numBlocks + 3) >> 2, wgLogical);
            blk = ok ? wgLogical * 4u + (blk & 3u) : 0xffffffffu / 64u;
        }
        const Pix px = mapPixel(*pm, blk, (unsigned)slot);
        if (!(px.valid && ok)) return false;
        idx = px.index;
        x = px.x;
        y = px.y;
        return true;
    }
    RD_DEV void findListed(int pixel) {
        idx = pixel;
        x = pixel % cam.resx;
        y = pixel / cam.resx;
    }
    RD_DEV Ray ray(float &tmax) const {
        tmax = 3.402823466e+38f;
        return gbufPrimaryRay(cam, x, y);
    }
    RD_DEV void store(const DScene &s, const RaySlab &rs, int hitPrim, v2 hitBary, float, bool) const {
        gbufStore(s, cam, lastCam, gb, idx, rs, hitPrim, hitBary);
    }
};

// PAIRS: the primary rays walk the sibling pairs (traverse.h, pairStep).  Coherent rays gain nothing from it while the threaded arrays
// sit in the caches (teapots, 201 k nodes: 0.78 ms either way) — the host picks it for trees whose six threaded arrays outgrow the
// Infinity Cache (radish_hip.hip, rdh_gbuffer_render).
template <bool COUNT, bool DEFER, bool PAIRS = false>
__global__ __launch_bounds__(64, PAIRS && !COUNT ? 4 : 1) void k_gbuffer_persistent(DScene s, DCamera cam, DCamera lastCam, PixelMap pm, GBufPtrs gb,
                                                           PersistCounters *pc, int2 *__restrict__ pairOvf = nullptr, int pairOvfDepth = 0) {
    __shared__ int2 sStack[PAIRS ? kPairLds * 64 : 1];  // PAIRS: the lanes' stacks (traverse.h, pairPush)
    int2 *const ovf = PAIRS ? pairOvf + (size_t)blockIdx.x * (size_t)pairOvfDepth * 64 : nullptr;
    // xcdSwizzle is a bijection on the group range padded to a multiple of 8: walk the padded range, skip the padding
    const int paddedBlocks = int((((unsigned)(pm.numBlocks + 3) / 4u + 7u) / 8u) * 8u * 4u);
    const bool deferAll = DEFER && pc->deferCount <= kDeferCap;  // written by k_gbuffer_find_literal, earlier in the stream
    PixelWork<true> work{cam, lastCam, &pm, gb, 0, 0, 0};
    walkLanes<COUNT, false, DEFER, PAIRS, RD_PIX_REFILL_MIN, RD_GB_FINISH_MIN>(s, pc, paddedBlocks, deferAll, sStack, ovf, work);
}

// ---- the primary rays of an 8x8 block walked as a PACKET ---------------------------------------------------------------------------
// Centre rays of neighbouring pixels make nearly the same walk (teapots camera: 89 visits per ray, 107 different nodes per block), so
// a wave takes one block, walks the union once with one uniform node load per visit, and writes its 64 records.  No lane refill,
// no persistent grid: a wave's work is one short walk.
template <bool COUNT, bool DEFER>
__global__ __launch_bounds__(256) void k_gbuffer_packet(DScene s, DCamera cam, DCamera lastCam, PixelMap pm, GBufPtrs gb, const PersistCounters *pc,
                                                        int budget) {
    const unsigned blk = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (blk >= (unsigned)pm.numBlocks) return;
    const bool deferAll = DEFER && pc->deferCount <= kDeferCap;  // written by k_gbuffer_find_literal, earlier in the stream
    PixelWork<false> work{cam, lastCam, &pm, gb, 0, 0, 0};
    walkPacket<COUNT, DEFER>(s, blk, deferAll, budget, work);
}

// Literal-class primary rays are traced apart, each by a whole 1 024-thread workgroup (wg_trace.h), in a launch that runs
// BESIDE k_gbuffer_persistent on a second stream: traced in place by one wave, one such ray takes 1.2 ms on the teapots scene,
// twice the rest of the pass.  The ray's class depends on the camera and the pixel only, so a first tiny kernel lists them;
// when there are more than kDeferCap (an axis-aligned camera makes a whole pixel row such rays) none is set aside — many
// one-wave traces in parallel are the better use of the chip then.
__global__ __launch_bounds__(256) void k_gbuffer_find_literal(DScene s, DCamera cam, PixelMap pm, PersistCounters *pc) {
    const int idx = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= cam.resx * cam.resy || s.bvhSize == 0) return;
    // on a tile partition only the rays of this rank's tiles (tile t belongs to rank t % world)
    if (pm.world > 1 && (((idx / cam.resx) / pm.tile) * pm.tilesX + (idx % cam.resx) / pm.tile) % pm.world != pm.rank) return;
    Ray ray = gbufPrimaryRay(cam, idx % cam.resx, idx / cam.resx);
    if (raySetAside(makeRaySlab(ray).cls)) {
        const int at = atomicAdd(&pc->deferCount, 1);
        if (at < kDeferCap) pc->deferred[at] = idx;
    }
}

template <bool COUNT>
__global__ __launch_bounds__(kWgTraceThreads) void k_gbuffer_literal(DScene s, DCamera cam, DCamera lastCam, GBufPtrs gb,
                                                                      const PersistCounters *pc) {
    __shared__ WgTraceShared sh;
    const int n = pc->deferCount;
    if (n > kDeferCap) return;  // k_gbuffer_persistent traces them all in place
    const PixelWork<false> work{cam, lastCam, nullptr, gb, 0, 0, 0};
    for (int i = int(blockIdx.x); i < n; i += int(gridDim.x)) wgTraceItem<COUNT, false>(s, pc->deferred[i], sh, work);
}

}  // namespace rd
