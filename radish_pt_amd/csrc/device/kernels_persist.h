// radish_pt_amd/csrc/device/kernels_persist.h — pathTrace as ONE persistent launch: a per-lane state machine with
// lane refill ("wavefront in registers").
//
// Why: node visits per ray are heavy-tailed on the reference's threaded BVH (Cornell stand-in: median 1, mean 34,
// p99 ≈ 950, max ≈ 2 800 dependent steps).  A kernel boundary per bounce (kernels_wave.h) makes every bounce wait for
// its longest ray (≈0.4–0.6 ms each, nine times per frame), and a one-lane-per-pixel megakernel makes every wave wait
// for its longest path.  Here a lane that finishes a ray shades it and carries on; a lane whose path ends takes the
// next pixel; the frame's critical path is the longest single PATH, and lanes stay busy until the frame runs dry.
//
// Every lane executes exactly singleKernelPT's sequence for its pixel (/root/reference/src/pathtrace.cu:149-291):
// primary ray → [NEE sample → shadow ray → BSDF sample → extension ray]* with the same RNG draws and the same order of
// additions (the bounce body is pathStep, path_step.h), so the result is bit-identical to the megakernel and to the queue pipeline.  Wave-level scheduling only
// decides WHEN a lane's next step runs:
//   box steps   while enough lanes are walking,
//   leaf tests  when >= 1/RD_PT_LEAF_DEN of the tracing lanes are parked on a leaf,
//   shading     when >= RD_SHADE_MIN 64ths of the busy lanes wait for it (or nothing else can run),
//   raygen      when >= RD_PT_REFILL_MIN lanes are idle and pixels remain.
// The three thresholds were re-tuned together at the end of round 1 (profiles/r01_f_experiment_thresholds.txt): 16 / 16 / 4
// -> 32 / 6 / 3 is 4.8 % on the Cornell frame (3.34 -> 3.18 ms) and on the teapots frame (10.24 -> 9.75 ms), +1 % on the
// 1-M-triangle 4K frame; one at a time each gave 1.5-2.4 %.  (Later shading batches are fuller and cost the same ~10 k clocks;
// idle lanes are refilled sooner; triangles are tested a little earlier.)
// Path state that is live only across phases (throughput, accumulators, the pending extension ray, …) sits in LDS,
// 84 B per lane, so the traversal loop runs on the walker's registers alone.
#pragma once
#include "kernels_pt.h"

namespace rd {

#ifndef RD_SHADE_MIN
#define RD_SHADE_MIN 32
#endif
#ifndef RD_PT_REFILL_MIN
#define RD_PT_REFILL_MIN 6
#endif
#ifndef RD_PT_LEAF_DEN  // k_pt_persistent only; the one-ray-per-lane kernels and the G-buffer keep RD_LEAF_NUM / RD_LEAF_DEN = 1 / 4
#define RD_PT_LEAF_DEN 3
#endif
// ... and once the pixel supply has ended (64ths of the busy lanes).  In the drain a wave serialises the shading calls of its
// remaining paths (≈10 k clocks each, whatever the lane count); with RD_SHADE_MIN at a quarter, waiting for half of them
// in the drain measured 1 % faster on the Cornell frame, 4 / 8 64ths 3 % / 1.5 % slower; with RD_SHADE_MIN = 32 the two coincide.
#ifndef RD_SHADE_MIN_DRAIN
#define RD_SHADE_MIN_DRAIN 32
#endif

constexpr int kDeferCap = 256;  // rays k_gbuffer_literal takes: one per workgroup, one round
struct PersistCounters {
    int blockHead;  // next 8x8 pixel block beyond the static first round (see k_pt_persistent)
    int deferCount;  // literal-class primary rays of the frame (k_gbuffer_find_literal); above kDeferCap none is set aside
#ifdef RD_PERSIST_STAMPS  // diagnostic build only: when each wave started, ran out of pixels, and ended (wall clock);
    // [3] wall-clock ticks it spent tracing literal-class rays whole, [4] how many such rays
    unsigned long long stamp[5][4096];
#endif
#ifdef RD_PERSIST_PHASES  // diagnostic build only: where the waves' time goes (s_memtime ticks summed over waves) and how full
    // the wave is in each phase: [0..5] ticks in raygen / literal+coop / box loop / leaf / retire / shade, [6] total;
    // [8] box wave-steps, [9] box lane-steps, [10] leaf calls, [11] leaf lanes, [12] shade calls, [13] shade lanes,
    // [14] raygen calls, [15] raygen lanes
    unsigned long long phase[16];
#endif
    int deferred[kDeferCap];  // pixel indices; NOT cleared between launches (the host clears up to here)
};

constexpr int PS_IDLE = 0, PS_TRACE = 1, PS_SHADE = 2;

// ---- longest-paths-first block order ---------------------------------------------------------------------------
// A persistent launch ends one path-latency after the pixel supply runs dry (measured: supply dry at ~1.9 ms, last
// wave out at ~3.8 ms on the Cornell frame), so the blocks holding long paths must start first.  Each launch records,
// per 8x8 block, the largest number of box steps any of its paths took; the next launch visits blocks in descending
// order of that figure (frames of an animation are coherent; the first frame uses plain order).  Pure scheduling:
// which lane renders a pixel, and when, cannot change its value.
constexpr int kCostBuckets = 64;
// One workgroup of 1 024 threads (a counting sort of ~32 000 blocks into 64 buckets).  The LDS counters are bumped once per
// wave and bucket, not once per block: neighbouring blocks cost about the same, so a wave's 64 blocks fall into a handful of
// buckets, and 64 lanes adding to ONE LDS word serialise (the first version did that from 256 threads: 104 us per frame, 3 %
// of the Cornell frame, on the stream between two persistent launches; this one: see profiles/).
// `ema`: running estimate of each block's cost over the frames so far (the per-launch figure is ONE sample of the longest of
// 64 random paths — noisy; blocks differ systematically by what they look at).  ema' = (RD_EMA_KEEP * ema + cost) / (RD_EMA_KEEP + 1).
#ifndef RD_EMA_KEEP
#define RD_EMA_KEEP 7
#endif
constexpr int kScheduleThreads = 1024;
__global__ __launch_bounds__(kScheduleThreads) void k_persist_schedule(unsigned *__restrict__ cost, unsigned *__restrict__ ema,
                                                                       int *__restrict__ order, int n) {
    __shared__ int hist[kCostBuckets], base[kCostBuckets];
    const int t = int(threadIdx.x);
    const int lane = t & 63;
    if (t < kCostBuckets) hist[t] = 0;
    __syncthreads();
    auto bucketOf = [](unsigned c) {  // quarter-octave buckets, descending: bucket 0 = most expensive
        int b = 0;
        if (c > 0) {
            int lg = 31 - __clz((int)c);                         // floor(log2 c)
            int frac = lg >= 2 ? int((c >> (lg - 2)) & 3u) : 0;  // next two bits
            b = lg * 4 + frac + 1;
        }
        if (b > kCostBuckets - 1) b = kCostBuckets - 1;
        return kCostBuckets - 1 - b;
    };
    // add `1` per lane of the wave to counter[bucket] with one atomic per distinct bucket; returns the lane's slot
    auto waveAdd = [&](int *counter, int bucket, bool valid) {
        int slot = 0;
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int L = __ffsll((long long)todo) - 1;
            const int b0 = __shfl(bucket, L, 64);
            const unsigned long long same = __ballot(valid && bucket == b0);
            int first = 0;
            if (lane == L) first = atomicAdd(&counter[b0], __popcll(same));
            first = __shfl(first, L, 64);
            if (valid && bucket == b0) slot = first + __popcll(same & ((1ull << lane) - 1ull));
            todo &= ~same;
        }
        return slot;
    };
    // four blocks per thread and round: the four pairs of loads are in flight together (one workgroup cannot hide a
    // dependent global load per round behind anything else)
    for (int i0 = 0; i0 < n; i0 += 4 * kScheduleThreads) {
        unsigned old[4], c[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = i0 + j * kScheduleThreads + t;
            old[j] = i < n ? ema[i] : 0u;
            c[j] = i < n ? cost[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = i0 + j * kScheduleThreads + t;
            const bool valid = i < n;
            const unsigned e = old[j] == 0u ? c[j] : (RD_EMA_KEEP * old[j] + c[j] + RD_EMA_KEEP / 2) / (RD_EMA_KEEP + 1);
            if (valid) {
                ema[i] = e;
                cost[i] = 0u;
            }
            waveAdd(hist, bucketOf(e), valid);
        }
    }
    __syncthreads();
    if (t < 64) {  // exclusive prefix sum of the 64 bucket sizes
        int v = hist[t], incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (t >= d) incl += up;
        }
        base[t] = incl - v;
    }
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 4 * kScheduleThreads) {  // order inside a bucket: ties are equally expensive
        unsigned e[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = i0 + j * kScheduleThreads + t;
            e[j] = i < n ? ema[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = i0 + j * kScheduleThreads + t;
            const bool valid = i < n;
            const int pos = waveAdd(base, bucketOf(e[j]), valid);
            if (valid) order[pos] = i;
        }
    }
}

#ifndef RD_PERSIST_WAVES
#define RD_PERSIST_WAVES 1
#endif
#ifdef RD_PERSIST_PHASES
#ifdef RD_PERSIST_PHASES_DRAIN  // count only what happens after this wave has found the pixel supply dry
#define PH_ON exhausted
#else
#define PH_ON true
#endif
#define PH_MARK(i) do { unsigned long long _n = __builtin_amdgcn_s_memtime(); if (PH_ON) phT[i] += _n - phLast; phLast = _n; } while (0)
#define PH_COUNT(i, mask) do { if (PH_ON) { phT[i] += 1ull; phT[(i) + 1] += (unsigned long long)__popcll(mask); } } while (0)
#else
#define PH_MARK(i) do { } while (0)
#define PH_COUNT(i, mask) do { } while (0)
#endif
// PAIRS: the per-lane walks go over the sibling pairs (DScene::pairs; traverse.h, pairStep) instead of the six threaded arrays:
// same triangle tests in the same order, same counters; chosen by the host for big scenes (radish_hip.hip, usePairs).
#ifndef RD_PERSIST_PAIR_WAVES
#define RD_PERSIST_PAIR_WAVES 3  // the pair variant is held to three waves per SIMD (173 VGPRs otherwise: two)
#endif
template <bool COUNT, bool PAIRS = false, bool LENS = false>
__global__ __launch_bounds__(64, PAIRS && !COUNT ? RD_PERSIST_PAIR_WAVES : RD_PERSIST_WAVES) void k_pt_persistent(DScene s, DCamera cam, PixelMap pm, int looper, int iter, int maxDepth,
                                                       float *__restrict__ directIllum, float *__restrict__ indirectIllum,
                                                       PersistCounters *pc, const int *__restrict__ blockOrder,
                                                       unsigned *__restrict__ blockCost, int2 *__restrict__ pairOvf = nullptr,
                                                       int pairOvfDepth = 0, DLens lens = DLens{}) {
    // ---- LDS-resident path state (SoA: lane-consecutive, conflict-free) ----
    // One wave per workgroup: nothing here needs a workgroup barrier, and a finished wave frees its CU slot at once
    // (with 4-wave workgroups the slot stays taken until the slowest of the four has drained its last path).
    __shared__ float sThr[3][64], sAccD[3][64], sAccI[3][64], sCur[3][64];
    __shared__ float sExtO[3][64], sExtD[3][64], sExtPdf[64], sNee[4][64];
    __shared__ int sFlags[64];  // bit0: extension ray pending, bit1: that sample was specular
    __shared__ int2 sStack[PAIRS ? kPairLds * 64 : 1];  // PAIRS: the lanes' stacks (traverse.h, pairPush)
    int2 *const ovf = PAIRS ? pairOvf + (size_t)blockIdx.x * (size_t)pairOvfDepth * 64 : nullptr;
    const int t = int(threadIdx.x);
    const int lane = t & 63;
    const int end = s.bvhSize;
    const int numBlocks = pm.numBlocks;
    // xcdSwizzle is a bijection on the group range padded to a multiple of 8: walk the padded range, skip the padding
    const int paddedBlocks = blockOrder ? numBlocks : int((((unsigned)(numBlocks + 3) / 4u + 7u) / 8u) * 8u * 4u);

    WalkStats ws{0, 0};
    unsigned nClosest = 0, nAny = 0, nHits = 0;
#ifdef RD_PERSIST_PHASES
    unsigned long long phT[16] = {0};
    unsigned long long phLast = __builtin_amdgcn_s_memtime();
    const unsigned long long phStart = phLast;
#endif
#ifdef RD_PERSIST_STAMPS
    const int gw = int(blockIdx.x);
    bool stampedDry = false;
    unsigned long long litTicks = 0, litRays = 0;
    if (lane == 0 && gw < 4096) pc->stamp[0][gw] = wall_clock64();
#endif

    // wave-uniform pixel reservation: one 8x8 block at a time; the first is static (wave g takes block g)
    int curBlock = int(blockIdx.x);
    int slotNext = 0;  // next unassigned pixel slot (0..63) of curBlock
    const int gridWavesN = int(gridDim.x);
    bool exhausted = curBlock >= paddedBlocks;

    // per-lane registers
    int state = PS_IDLE;
    int outIdx = 0;
    int myBlock = 0;         // 8x8 block this lane's pixel belongs to (index into blockCost)
    unsigned pathSteps = 0;  // box steps of the current path
    int k = 0;  // index of the hit the current extension ray leads to (0 = primary)
    uint32_t rngScramble = 0;
    int rngPtr = 0;
    // the ray being walked: origin / reciprocal direction as register pairs (packed slab test), direction, slab-test class
    RaySlabPk rp;
    rp.oxy = rp.ozw = rp.ixy = rp.izw = f2v{0.f, 0.f};
    v3 rayD = mk3(0.f);
    int rayCls = 0;
    auto slab = [&]() {  // the RaySlab view of it (same registers)
        RaySlab r;
        r.o = mk3(rp.oxy.x, rp.oxy.y, rp.ozw.x);
        r.d = rayD;
        r.inv = mk3(rp.ixy.x, rp.ixy.y, rp.izw.x);
        r.cls = rayCls;
        return r;
    };
    unsigned ordOfs = 0;  // byte offset of this ray's ordering inside the node allocation (layouts.h: one allocation)
    const char *nodeBase = reinterpret_cast<const char *>(s.nodes[0]);
    const unsigned ordStride = (unsigned)(s.bvhSize + 1) * (unsigned)sizeof(NodeRec);
    unsigned stepMark = 0, waveSteps = 0;  // wave-uniform count of box-loop iterations: the path's cost is how many it was in flight for
    int node = end, pending = -1;  // PAIRS: `node` is the pair to enter next (pairStep's `cur`), `ordOfs` the ordering itself
    PairStack stack{0, 0};
    float tmax = 0.f;
    int hitPrim = -1;
    v2 hitBary = mk2(0.f, 0.f);
    bool isShadow = false, occluded = false;
    // is this lane's walk over?  (threaded: the position has reached the end of the array; pairs: nothing to enter, nothing stacked)
    auto walkOver = [&]() { return PAIRS ? (node == kPairNone && stack.sp == 0) : (node == end); };

    auto startTrace = [&](const Ray &ray, float limit, bool shadow) {
        {
            const RaySlab r = makeRaySlab(ray);
            rp = packSlab(r);
            rayD = r.d;
            rayCls = r.cls;
        }
        ordOfs = (unsigned)getMTBVHId(-ray.d) * (PAIRS ? 1u : ordStride);
        stepMark = waveSteps;
        node = 0;
        pending = -1;
        hitPrim = -1;
        occluded = false;
        tmax = limit;
        isShadow = shadow;
        state = PS_TRACE;
        if (PAIRS) {
            stack = PairStack{0, 0};
            if (rayCls == 0 || end == 0) pairStart<COUNT>(s, slab(), limit, node, pending, ws);  // the root's box
            else node = kPairFresh;  // a literal-class ray: traced whole below
        }
    };
    auto startShadow = [&](v3 x, v3 y) {
        float limit;
        const Ray ray = shadowRay(x, y, limit);
        nAny++;
        startTrace(ray, limit, true);
    };
    auto finishPixel = [&]() {  // pathtrace.cu:279-290
        storeRunningMean(directIllum, outIdx, finishSample(mk3(sAccD[0][t], sAccD[1][t], sAccD[2][t])), iter);
        storeRunningMean(indirectIllum, outIdx, finishSample(mk3(sAccI[0][t], sAccI[1][t], sAccI[2][t])), iter);
        atomicMax(&blockCost[myBlock], pathSteps);
        state = PS_IDLE;
    };
    // this lane's path state as pathStep sees it (path_step.h): column t of the LDS arrays, the sampler's state in registers
    struct LanePath {
        const int t;
        uint32_t &scramble;
        int &ptr;
        RD_DEV v3 throughput() const { return mk3(sThr[0][t], sThr[1][t], sThr[2][t]); }
        RD_DEV float samplePdf() const { return sExtPdf[t]; }
        RD_DEV bool sampleDelta() const { return (sFlags[t] & 2) != 0; }
        RD_DEV v3 prevPos() const { return mk3(sCur[0][t], sCur[1][t], sCur[2][t]); }
        RD_DEV void setDirect(v3 v) { sAccD[0][t] = v.x; sAccD[1][t] = v.y; sAccD[2][t] = v.z; }
        RD_DEV void addIndirect(v3 v) { sAccI[0][t] += v.x; sAccI[1][t] += v.y; sAccI[2][t] += v.z; }
        RD_DEV Sampler rng(const DScene &sc) const { return Sampler{sc.sobol, scramble, ptr}; }
        RD_DEV void setNee(v3 c, float w) { sNee[0][t] = c.x; sNee[1][t] = c.y; sNee[2][t] = c.z; sNee[3][t] = w; }
        RD_DEV void setPrevPos(v3 x) { sCur[0][t] = x.x; sCur[1][t] = x.y; sCur[2][t] = x.z; }
        RD_DEV void setRay(const Ray &ray, float pdf, bool delta, v3 throughput, const Sampler &rng) {
            sExtO[0][t] = ray.o.x; sExtO[1][t] = ray.o.y; sExtO[2][t] = ray.o.z;
            sExtD[0][t] = ray.d.x; sExtD[1][t] = ray.d.y; sExtD[2][t] = ray.d.z;
            sExtPdf[t] = pdf;
            sThr[0][t] = throughput.x; sThr[1][t] = throughput.y; sThr[2][t] = throughput.z;
            sFlags[t] = 1 | (delta ? 2 : 0);
            scramble = rng.scramble;
            ptr = rng.ptr;
        }
    };
    auto startExtensionOrFinish = [&]() {
        if (sFlags[t] & 1) {
            Ray ray{mk3(sExtO[0][t], sExtO[1][t], sExtO[2][t]), mk3(sExtD[0][t], sExtD[1][t], sExtD[2][t])};
            nClosest++;
            startTrace(ray, 3.402823466e+38f, false);
        } else {
            finishPixel();
        }
    };

    for (;;) {
        // ---------------- raygen for idle lanes ----------------
        unsigned long long idleM = __ballot(state == PS_IDLE);
        int nIdle = __popcll(idleM);
        if (!exhausted && nIdle >= RD_PT_REFILL_MIN) {
            PH_COUNT(14, idleM);
            int myRank = __popcll(idleM & laneMaskLt());
            int taken = 0;
            while (taken < nIdle && !exhausted) {
                if (slotNext == 64) {
                    int b = 0;
                    if (lane == 0) b = atomicAdd(&pc->blockHead, 1);
                    curBlock = __shfl(b, 0, 64) + gridWavesN;
                    slotNext = 0;
                    if (curBlock >= paddedBlocks) {
                        exhausted = true;
                        break;
                    }
                }
                int avail = 64 - slotNext;
                int give = (nIdle - taken) < avail ? (nIdle - taken) : avail;
                if (state == PS_IDLE && myRank >= taken && myRank < taken + give) {
                    // block to render: the scheduled order if there is one, else XCD-aware plain order (workgroup-sized
                    // groups of 4 blocks, as in the one-shot kernels)
                    unsigned blk;
                    bool ok = true;
                    if (blockOrder) {
                        blk = (unsigned)blockOrder[curBlock];
                    } else {
                        unsigned wgLogical;
                        ok = xcdSwizzle((unsigned)curBlock >> 2, (unsigned)(numBlocks + 3) >> 2, wgLogical);
                        blk = ok ? wgLogical * 4u + ((unsigned)curBlock & 3u) : 0xffffffffu / 64u;
                    }
                    Pix px = mapPixel(pm, blk, (unsigned)(slotNext + (myRank - taken)));
                    if (px.valid && ok) {
                        outIdx = px.out;
                        myBlock = int(blk);
                        pathSteps = 0;
                        Sampler rng = makeSeededRandomEngine(looper, px.index, 0, s.sobol);
                        Ray ray = cameraSample<LENS>(cam, px.x, px.y, sample4D(rng), lens);
                        rngScramble = rng.scramble;
                        rngPtr = rng.ptr;
                        sAccD[0][t] = sAccD[1][t] = sAccD[2][t] = 0.f;
                        sAccI[0][t] = sAccI[1][t] = sAccI[2][t] = 0.f;
                        k = 0;
                        nClosest++;
                        startTrace(ray, 3.402823466e+38f, false);
#ifndef RD_NO_ROOT_SHORTCUT
                        if (PAIRS) {  // the root has been tested by startTrace
                            if (rayCls == 0 && end != 0 && node == kPairNone && pending < 0) {
                                sAccD[0][t] = sAccD[1][t] = sAccD[2][t] = 1.f;
                                finishPixel();
                            }
                        } else
                        // A primary ray that misses the root box is finished here and now: the walk would visit the root, miss
                        // it, follow its link to the end of the array, and the shading step would write direct = 1
                        // (pathtrace.cu:169-172).  More than half of the Cornell frame's pixels are such rays; taking them
                        // through the trace / shade phases costs the wave's other lanes two phase changes each.
                        if (rayCls == 0 && end != 0) {
                            const NodeRec *root = reinterpret_cast<const NodeRec *>(nodeBase + ordOfs);
                            const float4 lo = root->lo_prim, hi = root->hi_next;
                            float boundDist;
                            const bool boundHit = aabbFastPk(lo, hi, rp, boundDist);
                            if (!(boundHit && boundDist < tmax) && __float_as_int(hi.w) == end) {
                                if (COUNT) ws.nodes++;
                                sAccD[0][t] = sAccD[1][t] = sAccD[2][t] = 1.f;
                                finishPixel();
                            }
                        }
#endif
                    }
                }
                slotNext += give;
                taken += give;
            }
        }
        if (__ballot(state != PS_IDLE) == 0ull) {
            if (exhausted) break;
            continue;
        }
#ifdef RD_PERSIST_STAMPS
        if (exhausted && !stampedDry) {
            stampedDry = true;
            if (lane == 0 && gw < 4096) pc->stamp[1][gw] = wall_clock64();
        }
#endif

        PH_MARK(0);
        // ---------------- literal-class rays: traced whole by the whole wave (traverse.h, coopTraceWhole) ----------------
        {
            unsigned long long lit = __ballot(PAIRS ? (state == PS_TRACE && node == kPairFresh)
                                                    : (state == PS_TRACE && rayCls != 0 && node == 0 && pending < 0 && end != 0));
#ifdef RD_PERSIST_STAMPS
            const unsigned long long litT0 = wall_clock64();
            litRays += (unsigned long long)__popcll(lit);
#endif
            while (lit) {
                const int L = __ffsll((long long)lit) - 1;
                lit &= lit - 1ull;
                const bool shadowL = readlaneI(isShadow ? 1 : 0, L) != 0;
                const NodeRec *un = reinterpret_cast<const NodeRec *>(nodeBase + (unsigned)readlaneI((int)ordOfs, L) * (PAIRS ? ordStride : 1u));
                const RaySlab ur = readlaneRay(slab(), L);
                const float lim = readlaneF(tmax, L);
                CoopTrace ct = shadowL ? coopTraceWhole<true>(s, un, ur, lim) : coopTraceWhole<false>(s, un, ur, lim);
                if (lane == L) {
                    hitPrim = ct.hitPrim;
                    hitBary = ct.bary;
                    tmax = ct.tmax;
                    occluded = ct.found;
                    node = PAIRS ? kPairNone : end;
                    if (COUNT) {
                        ws.nodes += ct.nodes;
                        ws.tris += ct.tris;
                    }
                }
            }
#ifdef RD_PERSIST_STAMPS
            litTicks += wall_clock64() - litT0;
#endif
        }
        PH_MARK(1);
        // ---------------- box steps ----------------
        // Run until a quarter of the lanes that entered the loop have stopped walking (parked on a leaf or finished
        // their ray): one ballot + popcount per step is the whole scheduling cost.
        if (PAIRS) {
            bool busy = state == PS_TRACE && pending < 0 && !walkOver();
            const int nStart = __popcll(__ballot(busy));
            if (nStart > 0) {
                const int minWalk = (nStart * (RD_PT_LEAF_DEN - 1) + RD_PT_LEAF_DEN - 1) / RD_PT_LEAF_DEN;
                const RaySlab rs = slab();
                do {
                    PH_COUNT(8, __ballot(busy));
                    waveSteps++;
                    pairPopOne<COUNT>(sStack, lane, ovf, tmax, busy, node, stack, pending, ws);
                    if (busy && node >= 0) {
                        pairStep<COUNT>(s.pairs, sStack, lane, ovf, rs, tmax, (int)ordOfs, node, stack, pending, ws);
                        busy = pending < 0 && (node >= 0 || stack.sp > 0);
                    }
                } while (__popcll(ballotb(busy)) >= (minWalk > 1 ? minWalk : 1));
            }
        } else {
            bool walking = state == PS_TRACE && pending < 0 && node != end;
            int nStart = __popcll(__ballot(walking));
            if (nStart == 1) {
                // a lone walker (the drain of the frame): the whole wave tests 64 boxes ahead for it (coopWalk)
                const int L = __ffsll((long long)__ballot(walking)) - 1;
                CoopResult cr = coopWalk(reinterpret_cast<const NodeRec *>(nodeBase + (unsigned)readlaneI((int)ordOfs, L)),
                                         readlaneI(node, L), end, readlaneRay(slab(), L), readlaneF(tmax, L), RD_COOP_WINDOWS);
                waveSteps += 8u;
                if (lane == L) {
                    node = cr.node;
                    pending = cr.pending;
                    if (COUNT) ws.nodes += cr.visited;
                }
            } else if (nStart > 0) {
                const int minWalk = (nStart * (RD_PT_LEAF_DEN - 1) + RD_PT_LEAF_DEN - 1) / RD_PT_LEAF_DEN;
                do {
                    PH_COUNT(8, __ballot(walking));
                    waveSteps++;
                    if (walking) {
                        // one VALU for the address: base (SGPRs) + 32-bit byte offset
                        const NodeRec *rec = reinterpret_cast<const NodeRec *>(nodeBase + (ordOfs + ((unsigned)node << 5)));
                        float4 lo = rec->lo_prim;
                        float4 hi = rec->hi_next;
                        float boundDist;
                        if (COUNT) ws.nodes++;
                        bool boundHit = aabbFastPk(lo, hi, rp, boundDist);  // every walker here is of class 0 (the others were traced whole above)
                        if (boundHit && boundDist < tmax) {
                            pending = __float_as_int(lo.w);
                            node++;
                        } else {
                            node = __float_as_int(hi.w);
                        }
                        walking = pending < 0 && node != end;
                    }
                } while (__popcll(ballotb(walking)) >= (minWalk > 1 ? minWalk : 1));
                // (Requesting both successors ahead of the box test was measured and rejected: the L1 is busy ~80 % of
                //  the launch — TCP_GATE_EN — and doubling its requests cost 7 % in the bulk and gained nothing in the
                //  drain; DESIGN.md §7.  Round 3 tried the general form for SMALL launches — a rank's share of the frame on
                //  4-8 GPUs, where the launch lasts one path latency: 2 / 4 / 8 records of the threaded order per round trip,
                //  walked through without waiting again, bit-exact — and it lost there too (2.58 -> 3.38 / 3.53 / 6.41 ms per
                //  rank at 8 ranks, profiles/r03_c_*): a draining wave is bound by instruction issue shared with its SIMD's
                //  other waves, not by the round trip.)
            }
        }
        PH_MARK(2);
        // ---------------- leaf tests of parked lanes ----------------
        if (__ballot(state == PS_TRACE && pending >= 0) != 0ull) PH_COUNT(10, __ballot(state == PS_TRACE && pending >= 0));
        if (state == PS_TRACE && pending >= 0) {
            TriVerts tv = loadTri(s.tris, pending);
            float dist;
            v2 bary;
            if (COUNT) ws.tris++;
            bool hit = intersectTriangle(slab(), tv.a, tv.b, tv.c, bary, dist);
            if (hit && dist < tmax) {
                if (isShadow) {
                    occluded = true;
                    node = PAIRS ? kPairNone : end;
                    stack = PairStack{0, 0};
                } else {
                    hitPrim = pending;
                    tmax = dist;
                    hitBary = bary;
                }
            }
            pending = -1;
        }
        PH_MARK(3);
        // ---------------- retire finished traces ----------------
        if (state == PS_TRACE && pending < 0 && walkOver()) {
            pathSteps += waveSteps - stepMark;
            if (isShadow) {
                float nw = sNee[3][t];
                if (!occluded && nw >= 0.f) {  // the `+=` of pathtrace.cu:201-207
                    if (nw == 0.f) {
                        sAccD[0][t] += sNee[0][t]; sAccD[1][t] += sNee[1][t]; sAccD[2][t] += sNee[2][t];
                    } else {
                        sAccI[0][t] += sNee[0][t]; sAccI[1][t] += sNee[1][t]; sAccI[2][t] += sNee[2][t];
                    }
                }
                startExtensionOrFinish();
            } else {
                state = PS_SHADE;
            }
        }
        PH_MARK(4);
        // ---------------- shading ----------------
        unsigned long long shadeM = __ballot(state == PS_SHADE);
        if (shadeM != 0ull) {
            // Shade once a quarter of the busy lanes wait for it (16 of 64 in the bulk of the frame; in the drain, with a
            // handful of lanes left, a lane must not wait for every other lane's ray to end before it may continue).
            int nBusy = __popcll(__ballot(state != PS_IDLE));
            if (__popcll(shadeM) * 64 >= nBusy * (exhausted ? RD_SHADE_MIN_DRAIN : RD_SHADE_MIN)) {
                PH_COUNT(12, shadeM);
                if (state == PS_SHADE) {
                    if (hitPrim != -1) nHits++;
                    LanePath st{t, rngScramble, rngPtr};
                    const PathStepResult r = pathStep(s, k, maxDepth, hitPrim, hitBary, rayD, st);
                    if (r.goesOn()) {
                        k++;
                        if (!r.extension) sFlags[t] = 0;  // nothing is pending behind the shadow ray
                        if (r.shadow) startShadow(r.shadowFrom, r.shadowTo);
                        else startExtensionOrFinish();
                    } else {
                        finishPixel();
                    }
                }
            }
        }
        PH_MARK(5);
    }
#ifdef RD_PERSIST_PHASES
#ifdef RD_PERSIST_PHASES_DRAIN
    phT[6] = phT[0] + phT[1] + phT[2] + phT[3] + phT[4] + phT[5];
    (void)phStart;
#else
    phT[6] = __builtin_amdgcn_s_memtime() - phStart;
#endif
    if (lane == 0)
        for (int i = 0; i < 16; i++) atomicAdd(&pc->phase[i], phT[i]);
#endif
#ifdef RD_PERSIST_STAMPS
    if (lane == 0 && gw < 4096) {
        pc->stamp[2][gw] = wall_clock64();
        pc->stamp[3][gw] = litTicks;
        pc->stamp[4][gw] = litRays;
    }
#endif
    if (COUNT) flushCounters(s.counters, nClosest, nAny, nHits, ws);
}

}  // namespace rd
