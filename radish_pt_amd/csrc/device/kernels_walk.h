// radish_pt_amd/csrc/device/kernels_walk.h — the WALK-ONLY kernels: box steps, leaf tests, retire, and nothing else in their
// register allocation.  Three bodies, each written ONCE over a "work" type, and the ray-batch kernels around them; the G-buffer's
// kernels around the same bodies are in kernels_gbuffer.h.
//
//   walkLanes    the lane-refill walker: a lane whose ray has ended writes its record and takes the next item.  Items are handed
//                out in chunks of 64 (the first chunk of a wave is its index, further ones come from PersistCounters::blockHead).
//                k_trace_closest / k_trace_occluded (kernels_pt.h) give every ray a lane for the whole launch, so each wave waits
//                for its longest ray; here it does not.  DevScene::intersect (scene.h:262-301) / DevScene::testOcclusion
//                (:303-334) per lane, exactly as walkRay (traverse.h) performs them: same decisions, same counters.
//                Entries: k_walk_persistent (threaded arrays), k_walk_pair (sibling pairs), k_gbuffer_persistent.
//   walkPacket   one 64-item chunk per wave, walked as a packet (traverse.h, packetWalk).  k_walk_packet, k_gbuffer_packet.
//   wgTraceItem  one 1 024-thread workgroup per listed item (wg_trace.h).  k_trace_wg, k_trace_wg_list, k_gbuffer_literal.
//
// A work type is a plain struct that says where a lane's ray comes from and where its result goes; it remembers the item it
// handed out (a ray index, a pixel index) itself:
//   bool find(chunk, slot)    take the item in slot `slot` of chunk `chunk`; false: the slot holds none
//   void findListed(entry)    take the item a list entry names
//   Ray ray(float &tmax)      the ray of the item taken last, and how far it reaches
//   void store(s, RaySlab, hitPrim, hitBary, tmax, found)   the record of that item's finished walk
// BatchWork (below) is ray i of a float array with hits[i] / occluded[i]; PixelWork (kernels_gbuffer.h) is a pixel's centre ray
// with its G-buffer record.
#pragma once
#include "kernels_persist.h"
#include "wg_trace.h"

namespace rd {

#ifndef RD_WALK_REFILL_MIN
#define RD_WALK_REFILL_MIN 16  // refill once this many lanes are idle
#endif
#ifndef RD_WALK_FINISH_MIN
#define RD_WALK_FINISH_MIN 8  // retire once done lanes * 64 >= busy lanes * this
#endif

// Ray i of a batch (six floats a, b) as DevScene::intersect takes it — origin a, direction b, no limit — or, ANY, as
// testOcclusion(a, b) does (scene.h:303-315): the segment from a to b; its limit goes to tmax either way.
template <bool ANY>
RD_DEV Ray batchRay(const float *__restrict__ rays, long long i, float &tmax) {
    const v3 a = mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
    const v3 b = mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    if (ANY) return shadowRay(a, b, tmax);
    tmax = 3.402823466e+38f;
    return Ray{a, b};
}
// The record of a closest-hit ray that ended on triangle `prim` (-1: a miss) at `bary`, `t` along the ray.
RD_DEV int4 hitRecord(int prim, v2 bary, float t) {
    const bool hit = prim != -1;
    return make_int4(prim, __float_as_int(hit ? bary.x : 0.f), __float_as_int(hit ? bary.y : 0.f), __float_as_int(hit ? t : 3.402823466e+38f));
}

// The work of the ray-batch kernels: ray i of `rays`, its record in hits[i] (closest) or occluded[i] (ANY).
template <bool ANY>
struct BatchWork {
    const float *__restrict__ rays;
    long long n;
    int4 *__restrict__ hits;
    int *__restrict__ occluded;
    int slotList;
    long long i;  // the ray taken last

    RD_DEV bool find(long long chunk, int slot) {
        const long long k = chunk * 64 + slot;
        // slotList (ReSTIR's per-slot ray lists only): a NaN in the first float marks an EMPTY SLOT — no ray, no record,
        // nothing counted (the consumer, k_restir_resolve, does not read the record of such a slot either).  The public
        // ray-batch entries (rdh_trace_closest / rdh_trace_occluded) pass slotList = 0: a caller's ray with a NaN origin
        // is a ray like any other (it fails the root's box test, as in DevScene::intersect) and is counted.
        if (!(k < n && (slotList == 0 || rays[6 * k] == rays[6 * k]))) return false;
        i = k;
        return true;
    }
    RD_DEV void findListed(long long k) { i = k; }
    RD_DEV Ray ray(float &tmax) const { return batchRay<ANY>(rays, i, tmax); }
    RD_DEV void store(const DScene &, const RaySlab &, int hitPrim, v2 hitBary, float tmax, bool found) const {
        if (ANY) occluded[i] = found ? 1 : 0;
        else hits[i] = hitRecord(hitPrim, hitBary, tmax);
    }
};

// DEFER (ReSTIR's ray lists): literal-class rays — one wave needs ~1 ms for one of them on the teapots scene, which is then the
// duration of the whole launch — have been listed by the kernel that wrote the rays (at most kWalkDeferCap of them, else none is
// set aside) and are traced by k_trace_wg_list, one 1 024-thread workgroup each, on a second stream beside this launch.
constexpr int kWalkDeferCap = 256;

// The lane-refill walker over `chunks` chunks of 64 items.  !PAIRS: a lane walks the threaded array of its ray's ordering (`nodes`,
// `node`; a finished walk stands at `end`).  PAIRS: it walks the sibling pairs (DScene::pairs; traverse.h, pairStep) with the pair
// it enters next in `cur` and its stack in `sp`: the wave's rows of LDS, `stk`, and behind them its strip of the overflow buffer,
// `ovf`.  deferAll (DEFER): literal-class items have been set aside for a workgroup-per-item launch; they are neither walked nor
// counted here.  Idle lanes are refilled once REFILL_MIN of them wait, records written once FINISH_MIN 64ths of the busy lanes wait.
// `work` is the caller's object, by reference: a copy of it as a by-value parameter changes the whole kernel's code.
template <bool COUNT, bool ANY, bool DEFER, bool PAIRS, int REFILL_MIN, int FINISH_MIN, class Work>
RD_DEV void walkLanes(const DScene &s, PersistCounters *pc, long long chunks, bool deferAll, int2 *stk, int2 *ovf, Work &work) {
    const int lane = int(threadIdx.x) & 63;
    const int end = s.bvhSize;
    WalkStats ws{0, 0};
    unsigned nRays = 0, nHits = 0;
    long long curChunk = (long long)blockIdx.x;
    int slotNext = 0;
    const int gridWavesN = int(gridDim.x);
    bool exhausted = curChunk >= chunks;

    constexpr int W_IDLE = 0, W_TRACE = 1, W_DONE = 2;
    int state = W_IDLE;
    RaySlab rs;
    rs.o = rs.d = rs.inv = mk3(0.f);
    rs.cls = 0;
    const NodeRec *nodes = s.nodes[0];  // !PAIRS
    int node = end;
    int ord = 0, cur = kPairNone;  // PAIRS
    PairStack sp{0, 0};
    int pending = -1;
    float tmax = 0.f;
    int hitPrim = -1;
    v2 hitBary = mk2(0.f, 0.f);
    bool found = false;

    for (;;) {
        // ---------------- new items for idle lanes ----------------
        const unsigned long long idleM = __ballot(state == W_IDLE);
        const int nIdle = __popcll(idleM);
        if (!exhausted && nIdle >= REFILL_MIN) {
            const int myRank = __popcll(idleM & laneMaskLt());
            int taken = 0;
            while (taken < nIdle && !exhausted) {
                if (slotNext == 64) {
                    int b = 0;
                    if (lane == 0) b = atomicAdd(&pc->blockHead, 1);
                    curChunk = (long long)__shfl(b, 0, 64) + gridWavesN;
                    slotNext = 0;
                    if (curChunk >= chunks) {
                        exhausted = true;
                        break;
                    }
                }
                const int avail = 64 - slotNext;
                const int give = (nIdle - taken) < avail ? (nIdle - taken) : avail;
                if (state == W_IDLE && myRank >= taken && myRank < taken + give) {
                    if (work.find(curChunk, slotNext + (myRank - taken))) {
                        const Ray ray = work.ray(tmax);  // by value: filled through a reference it costs registers or time
                        rs = makeRaySlab(ray);
                        hitPrim = -1;
                        hitBary = mk2(0.f, 0.f);
                        found = false;
                        if (!(DEFER && deferAll && raySetAside(rs.cls) && end != 0)) {  // else: the workgroup-per-item launch has it
                            nRays++;
                            state = W_TRACE;
                            pending = -1;
                            if (PAIRS) {
                                ord = getMTBVHId(-ray.d);
                                sp = PairStack{0, 0};
                                if (rs.cls == 0 || end == 0) pairStart<COUNT>(s, rs, tmax, cur, pending, ws);  // the root's box
                                else cur = kPairFresh;  // a literal-class ray: traced whole below
                            } else {
                                nodes = s.nodes[getMTBVHId(-ray.d)];
                                node = 0;
                            }
                        }
                    }
                }
                slotNext += give;
                taken += give;
            }
        }
        if (__ballot(state != W_IDLE) == 0ull) {
            if (exhausted) break;
            continue;
        }
        // ---------------- literal-class rays: traced whole by the whole wave, over the threaded array of their ordering ----------------
        unsigned long long lit = __ballot(PAIRS ? (state == W_TRACE && cur == kPairFresh)
                                                : (state == W_TRACE && rs.cls != 0 && node == 0 && pending < 0 && end != 0));
        while (lit) {
            const int L = __ffsll((long long)lit) - 1;
            lit &= lit - 1ull;
            const NodeRec *un = PAIRS ? s.nodes[0] + (size_t)readlaneI(ord, L) * (size_t)(end + 1) : readlanePtr(nodes, L);
            CoopTrace ct = coopTraceWhole<ANY>(s, un, readlaneRay(rs, L), readlaneF(tmax, L));
            if (lane == L) {
                hitPrim = ct.hitPrim;
                hitBary = ct.bary;
                tmax = ct.tmax;
                found = ct.found;
                node = end;
                cur = kPairNone;
                if (COUNT) {
                    ws.nodes += ct.nodes;
                    ws.tris += ct.tris;
                }
            }
        }
        // ---------------- box steps: until a quarter of the lanes that entered the loop have stopped walking ----------------
        if (PAIRS) {
            bool busy = state == W_TRACE && pending < 0 && (cur >= 0 || sp.sp > 0);
            const int nStart = __popcll(__ballot(busy));
            if (nStart > 0) {
                const int minWalk = (nStart * (RD_LEAF_DEN - RD_LEAF_NUM) + RD_LEAF_DEN - 1) / RD_LEAF_DEN;
                do {
                    pairPopOne<COUNT>(stk, lane, ovf, tmax, busy, cur, sp, pending, ws);
                    if (busy && cur >= 0) {
                        pairStep<COUNT>(s.pairs, stk, lane, ovf, rs, tmax, ord, cur, sp, pending, ws);
                        busy = pending < 0 && (cur >= 0 || sp.sp > 0);
                    }
                } while (__popcll(__ballot(busy)) >= (minWalk > 1 ? minWalk : 1));
            }
        } else {
            bool walking = state == W_TRACE && pending < 0 && node != end;
            const int nStart = __popcll(__ballot(walking));
            if (nStart == 1) {  // a lone walker: the whole wave tests 64 boxes ahead for it
                const int L = __ffsll((long long)__ballot(walking)) - 1;
                CoopResult cr = coopWalk(readlanePtr(nodes, L), readlaneI(node, L), end, readlaneRay(rs, L), readlaneF(tmax, L), RD_COOP_WINDOWS);
                if (lane == L) {
                    node = cr.node;
                    pending = cr.pending;
                    if (COUNT) ws.nodes += cr.visited;
                }
            } else if (nStart > 0) {
                const int minWalk = (nStart * (RD_LEAF_DEN - RD_LEAF_NUM) + RD_LEAF_DEN - 1) / RD_LEAF_DEN;
                do {
                    if (walking) {
                        float4 lo = nodes[node].lo_prim;
                        float4 hi = nodes[node].hi_next;
                        float boundDist;
                        if (COUNT) ws.nodes++;
                        bool boundHit = aabbFast(lo, hi, rs, boundDist);
                        if (boundHit && boundDist < tmax) {
                            pending = __float_as_int(lo.w);
                            node++;
                        } else {
                            node = __float_as_int(hi.w);
                        }
                        walking = pending < 0 && node != end;
                    }
                } while (__popcll(__ballot(walking)) >= (minWalk > 1 ? minWalk : 1));
            }
        }
        // ---------------- leaf tests ----------------
        if (state == W_TRACE && pending >= 0) {
            TriVerts tv = loadTri(s.tris, pending);
            float dist;
            v2 bary;
            if (COUNT) ws.tris++;
            bool hit = intersectTriangle(rs, tv.a, tv.b, tv.c, bary, dist);
            if (hit && dist < tmax) {
                if (ANY) {  // the first accepted hit ends the walk
                    found = true;
                    node = end;
                    cur = kPairNone;
                    sp = PairStack{0, 0};
                } else {
                    hitPrim = pending;
                    tmax = dist;
                    hitBary = bary;
                }
            }
            pending = -1;
        }
        if (state == W_TRACE && pending < 0 && (PAIRS ? (cur == kPairNone && sp.sp == 0) : (node == end))) state = W_DONE;
        // ---------------- records of finished items ----------------
        const unsigned long long doneM = __ballot(state == W_DONE);
        const int nBusy = __popcll(__ballot(state != W_IDLE));
        if (doneM != 0ull && __popcll(doneM) * 64 >= nBusy * FINISH_MIN) {
            if (state == W_DONE) {
                if (!ANY && hitPrim != -1) nHits++;
                work.store(s, rs, hitPrim, hitBary, tmax, found);
                state = W_IDLE;
            }
        }
    }
    if (COUNT) flushCounters(s.counters, ANY ? 0u : nRays, ANY ? nRays : 0u, nHits, ws);
}

template <bool COUNT, bool ANY, bool DEFER = false>
__global__ __launch_bounds__(64) void k_walk_persistent(DScene s, const float *__restrict__ rays, long long n, int4 *__restrict__ hits,
                                                        int *__restrict__ occluded, PersistCounters *pc,
                                                        const int *__restrict__ deferCount = nullptr, int slotList = 0) {
    const bool deferAll = DEFER && *deferCount <= kWalkDeferCap;  // written by the kernel that produced the list, earlier in the stream
    BatchWork<ANY> work{rays, n, hits, occluded, slotList, 0};
    walkLanes<COUNT, ANY, DEFER, false, RD_WALK_REFILL_MIN, RD_WALK_FINISH_MIN>(s, pc, (n + 63) / 64, deferAll, nullptr, nullptr, work);
}

template <bool COUNT, bool ANY, bool DEFER = false>
__global__ __launch_bounds__(64, COUNT ? 1 : 7) void k_walk_pair(DScene s, const float *__restrict__ rays, long long n, int4 *__restrict__ hits,
                                                  int *__restrict__ occluded, PersistCounters *pc, int2 *__restrict__ overflow,
                                                  int overflowDepth, const int *__restrict__ deferCount = nullptr, int slotList = 0) {
    __shared__ int2 stk[kPairLds * 64];
    int2 *const ovf = overflow + (size_t)blockIdx.x * (size_t)overflowDepth * 64;
    const bool deferAll = DEFER && *deferCount <= kWalkDeferCap;
    BatchWork<ANY> work{rays, n, hits, occluded, slotList, 0};
    walkLanes<COUNT, ANY, DEFER, true, RD_WALK_REFILL_MIN, RD_WALK_FINISH_MIN>(s, pc, (n + 63) / 64, deferAll, stk, ovf, work);
}

// ---- closest hits of a COHERENT chunk — consecutive items start side by side, e.g. the primary rays of an 8x8 pixel block in slot
// order — by one wave, walked as a PACKET (traverse.h, packetWalk): one uniform node load per visit for the whole wave
// instead of one L1 request per lane.  Same records, same counters as the lane-refill walkers; on rays that do not travel together
// it is merely slow (a wave then visits the union of 64 unrelated walks), so the caller says when a list is coherent.
// Literal-class rays: set aside for the workgroup-per-item launch when they were listed (deferAll), else traced whole by the wave,
// in place, one after the other.  (deferAll is the lane's own: k_wf_trace_primary, kernels_wave.h, passes "this slot is listed".)
template <bool COUNT, bool DEFER, class Work>
RD_DEV void walkPacket(const DScene &s, long long chunk, bool deferAll, int budget, Work &work) {
    const int lane = int(threadIdx.x) & 63;
    const int end = s.bvhSize;
    WalkStats ws{0, 0};
    unsigned nRays = 0, nHits = 0;
    Ray ray{mk3(0.f), mk3(0.f, 0.f, 1.f)};
    float tmax = 3.402823466e+38f;
    const bool have = work.find(chunk, lane);
    if (have) ray = work.ray(tmax);
    const RaySlab rs = makeRaySlab(ray);
    const int ord = getMTBVHId(-ray.d);
    int hitPrim = -1;
    v2 hitBary = mk2(0.f, 0.f);
    const bool traced = have && !(DEFER && deferAll && raySetAside(rs.cls) && end != 0);
    if (traced) nRays++;
    unsigned long long lit = __ballot(traced && rs.cls != 0 && end != 0);
    while (lit) {
        const int L = __ffsll((long long)lit) - 1;
        lit &= lit - 1ull;
        const NodeRec *nodes = s.nodes[0] + (size_t)readlaneI(ord, L) * (size_t)(end + 1);
        CoopTrace ct = coopTraceWhole<false>(s, nodes, readlaneRay(rs, L), readlaneF(tmax, L));
        if (lane == L) {
            hitPrim = ct.hitPrim;
            hitBary = ct.bary;
            tmax = ct.tmax;
            if (COUNT) {
                ws.nodes += ct.nodes;
                ws.tris += ct.tris;
            }
        }
    }
    packetWalkAll<COUNT>(s, traced && rs.cls == 0 && end != 0, ord, rs, tmax, hitPrim, hitBary, ws, budget);
    if (traced) {
        if (hitPrim != -1) nHits++;
        work.store(s, rs, hitPrim, hitBary, tmax, false);
    }
    if (COUNT) flushCounters(s.counters, nRays, 0u, nHits, ws);
}

template <bool COUNT, bool DEFER>
__global__ __launch_bounds__(256) void k_walk_packet(DScene s, const float *__restrict__ rays, long long n, int4 *__restrict__ hits,
                                                     const int *__restrict__ deferCount, int slotList, int budget) {
    const bool deferAll = DEFER && *deferCount <= kWalkDeferCap;
    BatchWork<false> work{rays, n, hits, nullptr, slotList, 0};
    walkPacket<COUNT, DEFER>(s, (long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6), deferAll, budget, work);
}

// One WORKGROUP per item (wg_trace.h): how the G-buffer and ReSTIR trace the literal-class rays they set aside, and, over a whole
// ray batch (RDH_PT_WG_PER_RAY on the ray-batch entries), how the tests put every kind of ray through wgTraceWhole (closest and
// any-hit) and compare records and counters with the oracle.  Far slower than the walkers for ordinary rays: 16 waves per ray.
template <bool COUNT, bool ANY, class Work, class Entry>
RD_DEV void wgTraceItem(const DScene &s, Entry entry, WgTraceShared &sh, Work work) {
    float tmax;
    work.findListed(entry);
    const Ray ray = work.ray(tmax);
    const RaySlab rs = makeRaySlab(ray);
    CoopTrace ct = wgTraceWhole<ANY>(s, s.nodes[getMTBVHId(-ray.d)], rs, tmax, sh);
    if (threadIdx.x == 0) {
        work.store(s, rs, ct.hitPrim, ct.bary, ct.tmax, ct.found);
        if (COUNT) {
            atomicAdd(ANY ? &s.counters->anyRays : &s.counters->closestRays, 1ull);
            atomicAdd(&s.counters->nodeVisits, (unsigned long long)ct.nodes);
            atomicAdd(&s.counters->triTests, (unsigned long long)ct.tris);
            if (!ANY && ct.hitPrim != -1) atomicAdd(&s.counters->closestHits, 1ull);
        }
    }
}

template <bool COUNT, bool ANY>
__global__ __launch_bounds__(kWgTraceThreads) void k_trace_wg(DScene s, const float *__restrict__ rays, long long n, int4 *__restrict__ hits,
                                                              int *__restrict__ occluded) {
    __shared__ WgTraceShared sh;
    const BatchWork<ANY> work{rays, n, hits, occluded, 0, 0};
    for (long long i = (long long)blockIdx.x; i < n; i += (long long)gridDim.x) wgTraceItem<COUNT, ANY>(s, i, sh, work);
}

// k_trace_wg over an index list (the literal-class rays a producer kernel set aside): list[0 .. *count) are indices into `rays`.
template <bool COUNT, bool ANY>
__global__ __launch_bounds__(kWgTraceThreads) void k_trace_wg_list(DScene s, const float *__restrict__ rays, const int *__restrict__ list,
                                                                   const int *__restrict__ count, int4 *__restrict__ hits,
                                                                   int *__restrict__ occluded) {
    __shared__ WgTraceShared sh;
    const int n = *count;
    if (n > kWalkDeferCap) return;  // the walker traces them all in place
    const BatchWork<ANY> work{rays, 0, hits, occluded, 0, 0};
    for (int k = int(blockIdx.x); k < n; k += int(gridDim.x)) wgTraceItem<COUNT, ANY>(s, (long long)list[k], sh, work);
}
}  // namespace rd
