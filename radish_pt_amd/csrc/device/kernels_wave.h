// radish_pt_amd/csrc/device/kernels_wave.h — the wavefront path tracer: raygen → [trace → shade]* → finish.
//
// The reference has no counterpart (it is a megakernel); the contract is that every pixel receives
// exactly the value singleKernelPT (/root/reference/src/pathtrace.cu:149-291) would give it.  That holds because
//   * the RNG stream depends only on (looper, pixel index, draw count) and its 8-byte state rides with the path;
//   * each path owns its accumulators (no cross-path atomics), and launches are stream-ordered so that the
//     additions to `direct`/`indirect` happen in the megakernel's order (NEE of bounce d, then the emitter hit
//     of bounce d);
//   * all arithmetic is the same device functions the megakernel calls: the bounce body is pathStep (path_step.h), built from the
//     four expressions k_path_trace_mega calls in place, and every shadow ray is shadowRay's (traverse.h).
//
// Launch structure per frame (maxDepth = D):  memset(counters) · raygen · for k = 0..D { trace(k) · shade(k) } · finish
// (optionally as three sub-frames on three streams, see k_wf_raygen; the material sort happens inside shade, see k_wf_shade)
//   trace(k)  = closest-hit for the rays of bounce k, then any-hit for the shadow rays emitted by shade(k-1): one queue of work
//               items, the (long) extension rays handed out first so that the stage ends on the (short) shadow rays.  trace(0) has
//               primary rays only, an 8x8 block per 64 items: k_wf_trace_primary walks them as packets in place of k_wf_trace
//   shade(k)  = surface fetch for hit k, emitter/miss termination, then bounce body k+1 (NEE sample → shadow
//               queue, BSDF sample → next ray queue) with wave64 ballot compaction
// trace and shade are persistent kernels: a fixed grid of waves pulls 64-item packets from device-side queue
// heads (one returning atomic per packet), so no queue length ever travels to the host.
#pragma once
#include "kernels_pt.h"
#include "wg_trace.h"
#include "ray_cull.h"
#include "kernels_walk.h"

namespace rd {

constexpr int kWfLitCap = 8192;   // per stage; rays beyond it stay in the ordinary queues
constexpr int kWfLitShadow = 0x40000000;
constexpr int kMaxWaveDepth = 32;  // 4 + 7*depth Sobol dimensions <= 200 → depth <= 28

// Every counter sits on its own 128-byte line: same-address returning atomics serialise at ~12 ns each, and counters that share
// a line share that queue — the four class counters of k_wf_classify, side by side in one line, made it the slowest kernel of
// the sorted pipeline (0.87 ms per launch on the teapots frame).
struct alignas(128) WaveCounter {
    int v;
    int pad[31];
};
#ifndef RD_WF_TICKET_SHARDS
#define RD_WF_TICKET_SHARDS 8  // workgroup-ticket counters per stage (workgroupTicket); 1: one chip-wide counter (measurements)
#endif
constexpr int kTicketShards = RD_WF_TICKET_SHARDS;
// The two queues a shade stage appends to, and the head its waves pull packets from, are kept as S shards with a counter each
// (WfShardMap below): packet j of shade(k) appends to shard j % S and is pulled from head j % S, so a burst of same-address
// returning atomics is an S-th as long.  1: one counter and one region per queue, the layout until then (measurements).
// Teapots 1080p, 8 bounces, sorted, one pipeline, S = 1 / 2 / 8: 6.56 / 6.36 / 6.35 ms a frame, eight shards with one head 6.52: the
// gain is the heads' (profiles/wf_queue_shards/).
#ifndef RD_WF_QUEUE_SHARDS
#define RD_WF_QUEUE_SHARDS 8
#endif
constexpr int kQueueShards = RD_WF_QUEUE_SHARDS;
static_assert(kQueueShards >= 1 && kQueueShards <= 16, "RD_WF_QUEUE_SHARDS: 1 .. 16");
#ifndef RD_WF_HEAD_SHARDS  // heads the pulls are spread over, at most the queues' shards; 1: sharded appends, one head (measurements)
#define RD_WF_HEAD_SHARDS RD_WF_QUEUE_SHARDS
#endif
constexpr int kHeadShards = RD_WF_HEAD_SHARDS;
static_assert(kHeadShards >= 1 && kHeadShards <= kQueueShards, "RD_WF_HEAD_SHARDS: 1 .. RD_WF_QUEUE_SHARDS");
struct WaveCounters {
    WaveCounter rayCount[kMaxWaveDepth + 2][kQueueShards];     // rays of bounce k per shard (raygen: shard 0 / shade(k-1))
    WaveCounter shadowCount[kMaxWaveDepth + 2][kQueueShards];  // shadow rays emitted by shade(k), per shard
    WaveCounter litCount[kMaxWaveDepth + 2];     // literal-class rays (both kinds) that shade(k-1) set aside for trace(k)
    WaveCounter litShadowCount[kMaxWaveDepth + 2];  // shadow rays that shade(k) put on that list instead of shadowq (rdh_debug_wf_counts)
    WaveCounter traceHead[kMaxWaveDepth + 2];
    WaveCounter shadeHead[kMaxWaveDepth + 2][kQueueShards];  // pulls made from head x of shade(k) (wavePull)
    WaveCounter traceTicket[kMaxWaveDepth + 2][kTicketShards];  // workgroupTicket of trace(k) / shade(k)
    WaveCounter shadeTicket[kMaxWaveDepth + 2][kTicketShards];
    int queueStride[kMaxWaveDepth + 2];  // R of the queues trace(k) / shade(k) read: shard s starts at s * R (stage 0: 0, the identity)
};

// A sharded queue as its consumers see it.  The producer, shade(k - 1), shades its n records in packets of `packet` records (uniform
// over the stage); packet j = base / packet belongs to shard j % S and appends at s * R + (what shard s holds so far), with
// R = ceil(ceil(n / packet) / S) * packet.  A shard receives entries from its own packets only, at most one of a kind per record,
// so it never outgrows R, and S * R <= n + S * packet: the queues are S * kSortPacket entries longer than the slots (radish_hip.hip).
// A stage's item space stays dense: item i of a kind lives at s * R + (i - prefix[s]) with prefix[s] <= i < prefix[s + 1], the
// prefixes being the running sums of the shards' counts.  The counts and the stride are loaded once per kernel with uniform loads
// and the map is two scalars per shard (first[j], the first item of shard j, and shift[j] = j * R - first[j], kept as its steps)
// that a lane resolves its item with at hand-out, in S - 1 compares.  Stage 0's queue is shard 0 alone at offset 0 (k_wf_raygen,
// k_ad_raygen): the identity whatever the stride, which WfSlotWork::find and k_wf_trace_primary read as such.
RD_DEV int wfQueueStride(int n, int packet) {
    const int packets = (n + packet - 1) / packet;
    return ((packets + kQueueShards - 1) / kQueueShards) * packet;
}
struct WfShardMap {
    int first[kQueueShards], step[kQueueShards];  // step[j] = shift[j] - shift[j - 1]: what crossing into shard j adds to the address
    int total;
    // `counts`: the S counters of one queue; `itemBase`: where the queue's items start in the stage's item space
    RD_DEV void load(const WaveCounter *counts, int stride, int itemBase) {
        int at = 0, shift = 0;
#pragma unroll
        for (int j = 0; j < kQueueShards; j++) {
            first[j] = itemBase + at;
            step[j] = j * stride - first[j] - shift;
            shift += step[j];
            at += __builtin_amdgcn_readfirstlane(counts[j].v);
        }
        total = at;
    }
    // The queue address of item `i` (of the stage's item space, within this queue's range).  first[] does not decrease, so the
    // shards at or below the item's own are exactly those with first[j] <= i.  (A sum of steps, not a choice among S shifts: the
    // compiler makes a table in scratch of the latter.)
    RD_DEV int at(int i) const {
        int a = i + step[0];
#pragma unroll
        for (int j = 1; j < kQueueShards; j++) a += i >= first[j] ? step[j] : 0;
        return a;
    }
};

// Slots.  A path's HOME slot is its position in bounce 0's identity queue (k_wf_raygen); its two accumulators stay there for the whole
// frame, and k_wf_finish maps it to the pixel.  Everything else that rides with the path is rewritten by every bounce (pathStep's
// setters), so shade(k) writes it to a FRESH slot: the record's position q in stage k's processing order (k_wf_shade), unique and below
// rayCount[k].  Stage k + 1 then works in a slot space of rayCount[k] entries that are dense but for the paths that died in bounce
// k, instead of survivors scattered over the whole frame's slots: its loads and stores touch the lines of the live paths only.  The
// riding state is two sets: stage k (trace(k), shade(k)) reads set k & 1, shade(k) writes set (k + 1) & 1, k_wf_raygen writes set 0,
// so nothing is written to the set a stage reads.  `hit` is single: trace(k) writes it and shade(k) reads it in the same slot space.
// Home rides in thr.w and, beside the kind, in nee.w (wfNeeTag): where it is needed it has been loaded anyway.
struct WaveWorkspace {
    float4 *ro[2];       // ray origin.xyz (offset applied), w = pdf of the BSDF sample that made this ray
    float4 *rd[2];       // ray direction.xyz, w = 1 if that sample was specular (deltaSample)
    float4 *thr[2];      // throughput.xyz, w = the bits of the home slot
    float4 *prevPos[2];  // position the ray left from (curPos, pathtrace.cu:227) = origin of the pending shadow ray
    float4 *accD;        // direct.xyz, at the HOME slot
    float4 *accI;        // indirect.xyz, at the home slot
    float4 *nee[2];      // pending NEE contribution.xyz, w = the bits of wfNeeTag(home, kind)
    float4 *sht[2];      // shadow-ray target.xyz
    uint2 *rng[2];       // {scramble, ptr}
    int4 *hit;           // {primId, bary.x, bary.y, shading class of the hit's material}
    int *rayq[2];
    int *shadowq;
    int *litq[2];     // path slots of rays that look literal-class (bit 30: a shadow ray); trace(k) starts them first, one per wave
    int litCap;       // entries a stage may hold: min(kWfLitCap, 64 * waves of the trace grid)
    int *treeOvf;     // k_wf_trace<.., true>: its lanes' stacks beyond their LDS rings, [logical wave][treeOvfDepth][64] int2 (traverse.h, pairPush)
    int treeOvfDepth;
#ifdef RD_WF_STAMPS  // diagnostic build only: k_wf_trace's per-wave wall-clock stamps, [stage][logical wave][kWfStampKinds]; null: none
    unsigned long long *stamps;
    int stampWaves;   // logical waves of the trace grid
    int stampStages;  // stages of the pass; behind their stamps lies one word per stage: the shared head has run dry (RD_WF_STAMP_HELD)
#endif
    WaveCounters *ctr;
};

// nee.w: the home slot above two bits of kind, 0 → the contribution goes to direct, 1 → to indirect, 2 → nothing to add (slots stay
// below 2^30: kWfLitShadow).  It travels as a float's bits through loads and stores only.
constexpr unsigned kWfNeeNone = 2u;
RD_DEV float wfNeeTag(int home, unsigned kind) { return __uint_as_float(((unsigned)home << 2) | kind); }
// the addition sampleDirectLight's caller makes (pathtrace.cu:201-207) once the shadow ray of a pending NEE sample `n` ended unoccluded
RD_DEV void wfAddNee(const WaveWorkspace &w, float4 n) {
    const unsigned tag = __float_as_uint(n.w), kind = tag & 3u;
    if (kind == kWfNeeNone) return;
    float4 *acc = (kind == 0u ? w.accD : w.accI) + (tag >> 2);
    const float4 a = *acc;
    *acc = make_float4(a.x + n.x, a.y + n.y, a.z + n.z, 0.f);
}

// The ray trace(k) walks for path slot p of set `set` = k & 1, and how far: the shadow ray of the slot's pending NEE sample (prevPos -> sht), or its
// extension ray as shade(k-1) / raygen stored it.  k_wf_trace builds every ray here, so the workgroup's first list and the lane
// that meets the same entry classify one and the same ray.
RD_DEV Ray wfSlotRay(const WaveWorkspace &w, int set, int p, bool shadow, float &limit) {
    if (shadow) {
        const float4 x = w.prevPos[set][p], y = w.sht[set][p];
        return shadowRay(mk3(x.x, x.y, x.z), mk3(y.x, y.y, y.z), limit);
    }
    const float4 o = w.ro[set][p], d = w.rd[set][p];
    limit = 3.402823466e+38f;
    return Ray{mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z)};
}

// A record of stage k as pathStep sees it (path_step.h): every getter is a load from slot p of the set the stage reads, every setter a
// store to the record's fresh slot q of the other set; the accumulators are at the path's home slot.  Home is p itself at k = 0 and
// arrives with throughput() later, which pathStep asks for before every addIndirect, setNee and setRay of k > 0.
struct WaveSlotPath {
    const WaveWorkspace &w;
    const int rs, p;   // read: set, slot
    const int wr, q;   // write: set, slot
    int home;
    const bool delta;  // rd[rs][p].w, which the caller has loaded with the ray's direction
    bool nullNee = false;  // setNee's sample adds nothing whatever its shadow ray finds: no kind, or a contribution of (+-0, +-0, +-0)
    RD_DEV v3 throughput() {
        const float4 t = w.thr[rs][p];
        home = __float_as_int(t.w);
        return mk3(t.x, t.y, t.z);
    }
    RD_DEV float samplePdf() const { return w.ro[rs][p].w; }
    RD_DEV bool sampleDelta() const { return delta; }
    RD_DEV v3 prevPos() const { const float4 c = w.prevPos[rs][p]; return mk3(c.x, c.y, c.z); }
    RD_DEV void setDirect(v3 v) { w.accD[home] = make_float4(v.x, v.y, v.z, 0.f); }
    RD_DEV void addIndirect(v3 v) { const float4 a = w.accI[home]; w.accI[home] = make_float4(a.x + v.x, a.y + v.y, a.z + v.z, 0.f); }
    RD_DEV Sampler rng(const DScene &s) const { const uint2 r = w.rng[rs][p]; return Sampler{s.sobol, r.x, (int)r.y}; }
    RD_DEV void setNee(v3 c, float nw) {
        w.nee[wr][q] = make_float4(c.x, c.y, c.z, wfNeeTag(home, nw < 0.f ? kWfNeeNone : (nw == 0.f ? 0u : 1u)));
        nullNee = nw < 0.f || (c.x == 0.f && c.y == 0.f && c.z == 0.f);  // (float comparisons: either zero, never a NaN)
    }
    RD_DEV void setPrevPos(v3 x) { w.prevPos[wr][q] = make_float4(x.x, x.y, x.z, 0.f); }
    RD_DEV void setRay(const Ray &ray, float pdf, bool deltaSample, v3 throughput, const Sampler &rng) {
        w.ro[wr][q] = make_float4(ray.o.x, ray.o.y, ray.o.z, pdf);
        w.rd[wr][q] = make_float4(ray.d.x, ray.d.y, ray.d.z, deltaSample ? 1.f : 0.f);
        w.thr[wr][q] = make_float4(throughput.x, throughput.y, throughput.z, __int_as_float(home));
        w.rng[wr][q] = make_uint2(rng.scramble, (unsigned)rng.ptr);
    }
};


// Append `item` for every lane with pred==true: one atomic per wave, order inside the wave preserved.
RD_DEV void waveAppend(bool pred, int item, int *queue, int *count) {
    unsigned long long mask = __ballot(pred);
    if (mask == 0ull) return;
    int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(count, __popcll(mask));
    base = __shfl(base, leader, 64);
    if (pred) queue[base + __popcll(mask & laneMaskLt())] = item;
}

// k_wf_shade's appends.  Its packets are multiples of kShadePacket records; it appends what a wave has shaded to the two queues once
// per RD_WF_APPEND_CHUNKS 64-record chunks and at the end of every packet, with ONE returning atomic per queue.  Until then a
// record's entries wait as three bits in the wave's own sSorted row, in the place of the chunk it has just shaded (the slot is the
// record's position, so it needs no storage), and nothing is carried beyond the packet: 16 = kSortChunks means once per packet.
// Same-address returning atomics queue chip-wide per counter, and a wave cannot store its entries before it has the base: teapots
// 1080p, 8 bounces, sorted, one pipeline, an append per 4 / 8 / 16 chunks: 6.81 / 6.70 / 6.70 ms a frame; stages 0-2 of this
// kernel (packets of 512) 145 169 165 -> 127 148 141 us, the stages with packets of 256 unchanged (profiles/shade_appends/).
// (Before that: an append per 64 records was most of the kernel's time.)
constexpr int kShadeChunks = 4;  // k_wf_shade: 64-record chunks per smallest packet
constexpr int kShadePacket = 64 * kShadeChunks;
#ifndef RD_WF_APPEND_CHUNKS
#define RD_WF_APPEND_CHUNKS 16  // 4 / 8: measurements
#endif
static_assert(RD_WF_APPEND_CHUNKS == 4 || RD_WF_APPEND_CHUNKS == 8 || RD_WF_APPEND_CHUNKS == 16, "RD_WF_APPEND_CHUNKS: 4, 8 or 16");
constexpr int kAppendSpan = 64 * RD_WF_APPEND_CHUNKS;  // records between two appends of a wave, at most

// Work distribution for the persistent kernels.  Same-address returning atomics serialise chip-wide at ~12 ns each
// (MI355X_MICROARCH.md "dequeue"/"fanin"), so (a) the FIRST share of the work is fixed by the logical index and costs no atomic,
// and the shared head only hands out what lies beyond the fixed shares, and (b) a pull reserves many items at once.
// k_wf_shade: wave g's first packet is items [g*packet, (g+1)*packet), and a pull (wavePull) reserves one packet of 256..1 024
// records for the wave, behind gridWaves*packet.  k_wf_trace: packets of kPacket = 128 items; only the waves of workgroups
// WITHOUT list duty own a first packet, and a pull (tracePull) reserves the next one behind those (see the kernel's header).
// Heads and tickets are zeroed once per frame by the counters memset.
//
// The logical wave comes from the workgroup's ticket, taken in the order the workgroups become resident, not from blockIdx:
// a launch is not alone on the chip (the sub-frame pipelines each launch the whole resident grid, and two of them may share a
// hardware queue or run side by side), so the dispatcher may hold some workgroups back until another launch's tail frees
// their slots.  With blockIdx those late workgroups would start their fixed share — first packets, literal-class list entries —
// late; with tickets whatever starts late takes what nobody has taken yet.  Cost: one returning atomic per WORKGROUP, spread
// over kTicketShards = 8 counters (workgroup b uses counter b % 8, the XCD the dispatcher dealt it to), not one per wave.
constexpr int kPacket = 128;  // k_wf_trace: items a wave reserves for itself, fixed first packet and pull alike
RD_DEV int gridWaves() { return int(gridDim.x * (blockDim.x >> 6)); }
// The workgroup's logical index in [0, gridDim.x), a permutation of blockIdx.x: shard x holds exactly the workgroups
// b = x + S t < gridDim.x (S = kTicketShards), and its t-th ticket becomes x + S t.  Every thread of the workgroup must call it (barrier).
RD_DEV int workgroupTicket(WaveCounter *tickets) {
    __shared__ int ticket;
    if (threadIdx.x == 0) {
        const unsigned x = blockIdx.x % (unsigned)kTicketShards;
        ticket = int(x + (unsigned)kTicketShards * (unsigned)atomicAdd(&tickets[x].v, 1));
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(ticket);
}
// (wave-uniform, so kept in a scalar register: the VGPR budget of k_wf_trace has no room for it)
RD_DEV int logicalWave(int wg) { return __builtin_amdgcn_readfirstlane(int(wg * int(blockDim.x >> 6) + int(threadIdx.x >> 6))); }
// k_wf_shade's pull: the next packet behind the waves' fixed first packets, for logical wave g of a stage of n records.  Nothing
// lies behind them if n <= gridWaves * packet: the wave leaves without an atomic (the result is beyond n).  Otherwise wave g pulls
// from head x = g % Se only, Se = min(S, gridWaves) (S = kHeadShards), and the t-th pull of that head is packet
// gridWaves + Se * t + x: every head has a wave, so every packet is taken, and a wave whose head has passed n leaves (no stealing:
// the heads hand out interleaved packets, so they run dry within a packet of each other).
RD_DEV int wavePull(WaveCounter *heads, int g, int packet, int n) {
    const int waves = gridWaves();
    if (n <= waves * packet) return n;
    const int se = kHeadShards < waves ? kHeadShards : waves, x = g % se;
    int t = 0;
    if ((threadIdx.x & 63u) == 0u) t = atomicAdd(&heads[x].v, 1);
    t = __builtin_amdgcn_readfirstlane(t);
    // (a pull beyond the last packet is the wave's last: t stays below packets / Se + the waves of the head, far from overflow)
    return (waves + se * t + x) * packet;
}
// k_wf_trace's pull: the next packet behind `headBase`, the end of the stage's fixed first packets (which depends on how many
// workgroups have list duty, so the caller says where it is).  Called with the whole wave active; the result is wave-uniform.
RD_DEV int tracePull(int *head, int headBase) {
    int base = 0;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(head, kPacket);
    return __builtin_amdgcn_readlane(base, 0) + headBase;
}
// (Round 3 measured GUIDED self-scheduling — after the static packet a pull reserves an even share of half the items still
// unreserved, 32..128 for k_wf_trace, 64..packet for k_wf_shade, since a stage hands every wave only two or three fixed packets —
// and rejected it: teapots 9.07 -> 9.08 ms sorted / 8.90 -> 8.95 unsorted with three sub-frames, one pipeline 11.2 -> 11.8; the
// extra returning atomics cost what the finer tail saves, and with three pipelines a stage's tail is filled by the others anyway.
// profiles/r03_f_experiment_guided_scheduling.txt)

// ---- raygen ---------------------------------------------------------------------------------------------------
// Sub-frames: the wavefront pipeline can run as H independent pipelines over interleaved block sets (block b belongs to
// sub-frame b % H), each with its own workspace and stream, so that one sub-frame's stage tails are filled by the other's
// stage bodies.  `part` / `parts` = h / H; path slots are local to the sub-frame.
RD_DEV unsigned subFrameBlocks(const PixelMap &pm, int part, int parts) { return (unsigned)(pm.numBlocks - part + parts - 1) / (unsigned)parts; }
// Samples: a launch carries `samples` = B samples of every pixel (rdh_path_trace_samples; rdh_path_trace passes 1), so a stage holds
// B times the rays and ends on ONE tail.  Slot order is sample-major: 64-slot group g of the sub-frame is its 8x8 block g % nLocal in
// sample g / nLocal, so every sample's slots lie as the one-sample frame's do (block-major, a block's B samples in B neighbouring
// waves, measured 3-5 % slower per sample on Cornell 400x400 and 0.4 % faster on teapots 1080p: DESIGN 5f).  Sample b draws Sobol
// row (looper + b) % 10000, the wrap of State::looper.  trace and shade see path slots only; k_wf_finish folds a pixel's B slots
// in sample order.
constexpr int kSobolRows = 10000;  // State::looper wraps here (pathtrace.cu:380-381)
// The body is written once for the pinhole kernel and the lens one (k_wf_raygen_lens below; LENS as in kernels_pt.h).
template <bool LENS>
RD_DEV void wfRaygen(const DScene &s, const DCamera &cam, const PixelMap &pm, const WaveWorkspace &w, int looper, int samples, int part,
                     int parts, const DLens &lens) {
    unsigned wg;
    const unsigned nLocal = subFrameBlocks(pm, part, parts);
    const unsigned nGroups = nLocal * (unsigned)samples;
    bool wgValid = xcdSwizzle(blockIdx.x, (nGroups + 3u) >> 2, wg);
    unsigned lane = threadIdx.x & 63u;
    unsigned group = wgValid ? wg * 4u + (threadIdx.x >> 6) : 0xffffffffu / 64u;
    const bool inRange = wgValid && group < nGroups;
    const unsigned b = group / nLocal, blockLocal = group - b * nLocal;
    Pix px = mapPixel(pm, inRange ? blockLocal * (unsigned)parts + (unsigned)part : 0xffffffffu / 64u, lane);
    bool valid = px.valid && inRange;
    int p = int(group * 64u + lane);  // the path's home slot = work index; its slot in stage 0 as well
    bool listed = false;
    if (valid) {
        Sampler rng = makeSeededRandomEngine(int(((unsigned)looper + b) % (unsigned)kSobolRows), px.index, 0, s.sobol);
        Ray ray = cameraSample<LENS>(cam, px.x, px.y, sample4D(rng), lens);
        w.ro[0][p] = make_float4(ray.o.x, ray.o.y, ray.o.z, 0.f);
        w.rd[0][p] = make_float4(ray.d.x, ray.d.y, ray.d.z, 0.f);
        w.accD[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.accI[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.rng[0][p] = make_uint2(rng.scramble, (unsigned)rng.ptr);
        // Primary rays that LOOK literal-class (the hint k_wf_shade uses for the rays it emits) go on stage 0's first list, so that a
        // workgroup of trace(0) traces them before anything else instead of one wave meeting them late (stage 0 was where the last
        // launches above 1 ms were: profiles/r03_w_teapots_trace_stage_time_histogram.txt).  A handful per frame: one atomic each.
        if (fabs_(ray.d.x) < 1.1e-6f || fabs_(ray.d.y) < 1.1e-6f || fabs_(ray.d.z) < 1.1e-6f) {
            const int at = atomicAdd(&w.ctr->litCount[0].v, 1);
            if (at < w.litCap) {
                w.litq[0][at] = p;
                listed = true;
            }
        }
    }
    // Bounce 0's queue is the identity over this launch's slots (-1 marks pixels outside the frame; -2 - slot: on the first list, as
    // k_wf_shade marks such rays): no compaction.
    if (inRange) w.rayq[0][p] = valid ? (listed ? -2 - p : p) : -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) w.ctr->rayCount[0][0].v = int(nGroups) * 64;
}
__global__ __launch_bounds__(256) void k_wf_raygen(DScene s, DCamera cam, PixelMap pm, WaveWorkspace w, int looper, int samples, int part,
                                                   int parts) {
    wfRaygen<false>(s, cam, pm, w, looper, samples, part, parts, DLens{});
}
__global__ __launch_bounds__(256) void k_wf_raygen_lens(DScene s, DCamera cam, PixelMap pm, WaveWorkspace w, int looper, int samples,
                                                        int part, int parts, DLens lens) {
    wfRaygen<true>(s, cam, pm, w, looper, samples, part, parts, lens);
}

// ---- trace(k): closest hits of bounce k + shadow rays of bounce k (from shade(k-1)) ---------------------------
// Persistent waves with LANE REFILL: a wave reserves kPacket = 128 consecutive work items per atomic and hands them to lanes
// one by one as their previous ray finishes, so a wave never idles behind its longest ray (rays of one packet differ
// several-fold in visit count after the first bounce).  Shadow (any-hit) and extension (closest-hit) rays run through
// one walker; a lane's kind only decides how it terminates.
//
// Hand-out ("A workgroup with list duty takes no fixed share").  G = gridDim.x, L = min(nLit, G): the workgroups with
// tickets below L trace a list entry together first (list duty), and their waves own NO first packet: they go to the shared head
// once the list is done, and leave if it is dry by then.  The waves of ticket t >= L own the packets 4 (t - L) .. 4 (t - L) + 3,
// and the head hands out what lies behind 4 (G - L) packets.  Before (RD_WF_DUTY_SHARE=1: measurements) every wave owned a first
// packet, duty or not, so a workgroup with a slow list ray started its 512 fixed items, the stage's lowest-numbered and longest
// rays, when the others were finishing theirs.  Which lane traces an item changes no image and no counter.
#ifndef RD_WF_DUTY_SHARE
#define RD_WF_DUTY_SHARE 0
#endif
#ifndef RD_REFILL_MIN
#define RD_REFILL_MIN 16  // refill once at least this many lanes are idle
#endif
#ifndef RD_WF_FINISH_MIN  // retire finished rays once they are this many 64ths of the wave's busy lanes (0: every iteration).  With
#define RD_WF_FINISH_MIN 16  // three sub-frames, teapots / Cornell: 0 -> 9.31 / 4.02 ms, 8 -> 9.20 / 3.99, 16 -> 9.05 / 3.93, 24 -> 9.08 / 3.98
#endif
// The order of a stage's work items: [0, nRay) are the extension rays of bounce k (rayq), [nRay, nRay + nShadow) the shadow rays that
// shade(k-1) emitted (shadowq), and both the static first packets and the shared head hand items out in increasing order.  A shadow
// ray ends at its first accepted triangle within its segment; an extension ray walks to its closest hit, several times as far.  With
// the shadow rays first (the order until DESIGN 5b, "Extension rays first") every stage ended on its longest rays with nothing left to
// refill the lanes they leave idle.  Nothing reads an order: a shadow ray adds to accD / accI of its path's home slot, an extension ray
// writes hit of its own slot.  1: the old order (measurements).  Teapots 1080p, 8 bounces, sorted, one pipeline, 1 / 0: 8.41 / 7.94 ms per frame,
// stages 1-8 of this kernel 6.31 / 5.80 ms; config 5's scene at 4K 33.04 / 32.59 ms (profiles/wf_order/)
#ifndef RD_WF_SHADOW_FIRST
#define RD_WF_SHADOW_FIRST 0
#endif
// RD_WF_STAMPS (diagnostic build only, like RD_PERSIST_STAMPS): lane 0 of every wave stores wall_clock64() (100 MHz) into its own
// slot of WaveWorkspace::stamps when it enters the kernel, when it first finds the stage's queue exhausted, when it leaves, and when
// it has left the list loop — plain stores, no shared counter.  The entry stamp is the reference the others are read against (the
// earliest one of a stage is the launch's start: scripts/wf_stage_tails.py).  The fifth word is no time: 1 + the reserved items the
// wave had not started at its first refill after the shared head had
// passed the stage's last item; 0: it never came to a refill after that.  (The wave that finds the head dry says so in a word of
// the stage's own behind the stamps, and a refill loads that word: polling the head itself, the line every pull's atomic goes
// to, made the stamped frame 2.7 times as long.)  The sixth is 1 + the
// stage's list entries (nLit), so that the reader knows which workgroups had list duty: those with tickets below it.  The default
// build holds none of it.
constexpr int kWfStampKinds = 6;  // entry, queue dry, exit, list loop left, 1 + items held when the head was dry, 1 + nLit
#ifdef RD_WF_STAMPS
#define RD_WF_STAMP(kind) do { if (stampAt && (threadIdx.x & 63u) == 0u) stampAt[kind] = wall_clock64(); } while (0)
#define RD_WF_STAMP_DRY() do { if (exhausted && !stampedDry) { stampedDry = true; RD_WF_STAMP(1); if (stampAt && (threadIdx.x & 63u) == 0u) *headDry = 1ull; } } while (0)
#define RD_WF_STAMP_HELD(held) do { if (stampAt && !stampedHeld && *headDry != 0ull) { \
        stampedHeld = true; const int h_ = (held); if ((threadIdx.x & 63u) == 0u) stampAt[4] = 1ull + (unsigned long long)h_; } } while (0)
#else
#define RD_WF_STAMP(kind) ((void)0)
#define RD_WF_STAMP_DRY() ((void)0)
#define RD_WF_STAMP_HELD(held) ((void)0)
#endif
#ifndef RD_WF_COOP_LONE  // a lone walking lane is walked by the whole wave (coopWalk): 0.5-1 % on either scene
#define RD_WF_COOP_LONE 1
#endif

// PAIRS: the per-lane walks go over the sibling pairs (DScene::pairs: ONE 64-byte record per inner node for all six orderings, both
// children fetched and tested per round trip, the far one re-checked when the walk reaches it; traverse.h, pairStep) instead of the
// six threaded arrays — same triangle tests in the same order, same counters.  Chosen by the host for big scenes (radish_hip.hip,
// usePairs): a sixth of the node footprint and half the dependent round trips (profiles/r03_h_*).
#ifndef RD_WF_TRACE_WAVES  // waves per SIMD the threaded variant is held to: its occupancy step (72 VGPRs).  Unbounded, the entry
#define RD_WF_TRACE_WAVES 7  // barrier of workgroupTicket makes the allocator take 73 (6 waves); held to 7 it takes 69, no scratch
#endif
#ifndef RD_WF_PAIR_WAVES
#define RD_WF_PAIR_WAVES 1  // waves per SIMD the pair variant is held to (1: whatever its registers allow)
#endif
// ... and AT MOST (8: no bound): its registers are padded to that step, and the host holds its resident grid to as many workgroups
// per CU (radish_hip.hip, wavefrontPathTrace: the runtime's occupancy query goes by the registers used, not the padded number).
// The pair walk is slower with seven waves per SIMD than with six, and how many registers it needs moves between 71 and 75 with
// unrelated edits of this kernel, across the step at 72: teapots 1080p, 8 bounces, one pipeline, the same hand-out at
// 75 registers / six waves 7.52-7.56 ms a frame, at 71 / seven waves 8.51-8.54 (profiles/wf_handout/variants.txt)
#ifndef RD_WF_PAIR_MAX_WAVES
#define RD_WF_PAIR_MAX_WAVES 6
#endif
template <bool COUNT, bool PAIRS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PAIRS && !COUNT ? RD_WF_PAIR_WAVES : (!COUNT ? RD_WF_TRACE_WAVES : 1),
                                                                      PAIRS && !COUNT ? RD_WF_PAIR_MAX_WAVES : 8))) void k_wf_trace(DScene s, WaveWorkspace w, int k) {
    WaveCounters *c = w.ctr;
    const int wg = workgroupTicket(c->traceTicket[k]);  // stands for blockIdx.x below (see wavePull)
#ifdef RD_WF_STAMPS
    unsigned long long *const stampAt = w.stamps ? w.stamps + ((size_t)k * (size_t)w.stampWaves + (size_t)logicalWave(wg)) * kWfStampKinds : nullptr;
    volatile unsigned long long *const headDry = w.stamps ? w.stamps + (size_t)w.stampStages * (size_t)w.stampWaves * kWfStampKinds + k : nullptr;
    bool stampedDry = false, stampedHeld = false;
    RD_WF_STAMP(0);
#endif
    // the two queues' shards in the stage's item space (WfShardMap: uniform loads, scalar registers)
    const int stride = __builtin_amdgcn_readfirstlane(c->queueStride[k]);
    WfShardMap rayMap, shadowMap;
#if RD_WF_SHADOW_FIRST
    shadowMap.load(c->shadowCount[k > 0 ? k - 1 : 0], stride, 0);
    if (k == 0) shadowMap.total = 0;
    rayMap.load(c->rayCount[k], stride, shadowMap.total);
#else
    rayMap.load(c->rayCount[k], stride, 0);
    shadowMap.load(c->shadowCount[k > 0 ? k - 1 : 0], stride, rayMap.total);
    if (k == 0) shadowMap.total = 0;
#endif
    const int nShadow = shadowMap.total, nRay = rayMap.total;
    const int total = nShadow + nRay;
    const int *rayq = w.rayq[k & 1];
    const int set = k & 1;  // the state shade(k-1) / raygen wrote (WaveWorkspace)
    WalkStats ws{0, 0};
    unsigned nClosest = 0, nAny = 0, nHits = 0;
    const int end = s.bvhSize;
    const int END = end;  // `node` of a finished walk (!PAIRS)

    // Fixed first packets and the start of the shared head (wave-uniform arithmetic; see the kernel's header).  A wave whose packet
    // starts beyond the stage's items, or a duty workgroup's when the fixed packets cover the stage, has nothing to trace and never pulls.
    const int nLit = c->litCount[k].v < w.litCap ? c->litCount[k].v : w.litCap;
    const int dutyGroups = RD_WF_DUTY_SHARE ? 0 : (nLit < int(gridDim.x) ? nLit : int(gridDim.x));  // L
    const bool duty = wg < dutyGroups;
    const int headBase = (int(gridDim.x) - dutyGroups) * int(blockDim.x >> 6) * kPacket;
    // the wave's own reservation of work items; the first one is its fixed packet
    int resNext = duty ? headBase : (logicalWave(wg) - dutyGroups * int(blockDim.x >> 6)) * kPacket, resEnd = duty ? resNext : resNext + kPacket;
    bool exhausted = resNext >= total;
    if (resEnd > total) resEnd = total;
    RD_WF_STAMP_DRY();

    // per-lane walker state
    bool alive = false;
    bool isShadow = false;
    int p = -1;
    RaySlab rs;
    rs.o = rs.d = rs.inv = mk3(0.f);
    rs.cls = 0;
    const NodeRec *nodes = s.nodes[0];  // !PAIRS: the ray's threaded array
    int ord = 0, cur = kPairNone;  // PAIRS: the ray's ordering, the pair it enters next, its stack (pairStep)
    PairStack sp{0, 0};
    int node = END, pending = -1;
    float tmax = 0.f;
    int hitPrim = -1;
    v2 hitBary = mk2(0.f, 0.f);
    bool occluded = false;

    // Rays that shade(k-1) found to look literal-class (they wander through the tree for thousands of box steps; one wave needs 90 us
    // (median) to 1.5 ms for one of them on the teapots scene) start FIRST: picked up with a late packet one of them is what the stage
    // ends on (measured ceiling: 0.5-0.95 ms of the teapots frame).  Round 3: the workgroup traces them TOGETHER — its four waves are
    // at the same point only here, before each goes its own way with lane refill — 256 records per round trip with the parallel
    // resolve of wg_trace.h instead of 64 with a scalar one (coopTraceWhole): entry `it` of the list belongs to the workgroup whose
    // ticket is it % grid, so the workgroups that become resident first take the list.
    // The list is a HINT (shade classifies by the direction it emits, this kernel by the ray it builds): an entry whose ray turns out
    // ordinary is left to a lane of the workgroup (first round below), as before.
    // (PAIRS: the four waves' stack rows take over the workgroup trace's LDS once the list is done)
    constexpr int kStackEntries = PAIRS ? 4 * kPairLds * 64 : 1;
    __shared__ union WfTraceLds {
        WgTraceSharedT<256> wg;
        int2 stack[kStackEntries];
    } lds;
    WgTraceSharedT<256> &wgsh = lds.wg;
    int2 *const stk = lds.stack + (PAIRS ? int(threadIdx.x >> 6) * kPairLds * 64 : 0);
    int2 *const ovf = PAIRS ? reinterpret_cast<int2 *>(w.treeOvf) + (size_t)logicalWave(wg) * (size_t)w.treeOvfDepth * 64 : nullptr;
    for (int it = wg; it < nLit; it += int(gridDim.x)) {  // uniform over the workgroup
        const int e = w.litq[k & 1][it];
        const bool sh = (e & kWfLitShadow) != 0;
        const int pp = e & (kWfLitShadow - 1);
        float lim;
        const Ray ray = wfSlotRay(w, set, pp, sh, lim);
        const RaySlab urs = makeRaySlab(ray);
        if (urs.cls == 0 || end == 0) continue;  // the hint did not hold: a lane takes this entry below
        const NodeRec *un = s.nodes[getMTBVHId(-ray.d)];
        const CoopTrace ct = sh ? wgTraceWhole<true, 256>(s, un, urs, lim, wgsh) : wgTraceWhole<false, 256>(s, un, urs, lim, wgsh);
        if (threadIdx.x == 0) {  // the record of the finished ray (as in the retire step of the loop below)
            if (sh) {
                nAny++;
                if (!ct.found) wfAddNee(w, w.nee[set][pp]);
            } else {
                nClosest++;
                const bool hit = ct.hitPrim != -1;
                if (hit) nHits++;
                w.hit[pp] = make_int4(ct.hitPrim, __float_as_int(hit ? ct.bary.x : 0.f), __float_as_int(hit ? ct.bary.y : 0.f),
                                      hit ? int(s.primClass[ct.hitPrim]) : 0);
            }
            if (COUNT) {
                ws.nodes += ct.nodes;
                ws.tris += ct.tris;
            }
        }
    }
    RD_WF_STAMP(3);
#ifdef RD_WF_STAMPS
    if (stampAt && (threadIdx.x & 63u) == 0u) stampAt[5] = 1ull + (unsigned long long)nLit;
#endif
    if (PAIRS) __syncthreads();  // every wave is done with the workgroup trace's LDS
    bool firstRound = true;
    bool fromList = false;  // this lane's item of the first round came from the list: skip it if the workgroup has traced it above
    for (;;) {
        // ---- hand new items to idle lanes ----
        bool doStart = false;  // this lane takes an item in this round: kind and path slot go straight into isShadow / p
        fromList = false;
        if (firstRound) {
            firstRound = false;
            // the workgroup's j-th entry (j = 4 * lane + wave of the workgroup: at most 256 per workgroup) — see above
            const int it = wg + (int(threadIdx.x & 63u) * 4 + int(threadIdx.x >> 6)) * int(gridDim.x);
            if (it < nLit) {
                const int e = w.litq[k & 1][it];
                doStart = true;
                fromList = true;
                isShadow = (e & kWfLitShadow) != 0;
                p = e & (kWfLitShadow - 1);
            }
        }
        unsigned long long idle = __ballot(!alive && !doStart && p < 0);
        int nIdle = __popcll(idle);
        if (!exhausted && nIdle >= RD_REFILL_MIN) {
            RD_WF_STAMP_HELD(resEnd - resNext);
            int myRank = __popcll(idle & laneMaskLt());
            int taken = 0;  // items handed out so far in this refill (wave-uniform)
            while (taken < nIdle && !exhausted) {
                if (resNext == resEnd) {
                    resNext = tracePull(&c->traceHead[k].v, headBase);
                    resEnd = resNext + kPacket;
                    if (resNext >= total) {
                        exhausted = true;
                        break;
                    }
                    if (resEnd > total) resEnd = total;
                }
                int avail = resEnd - resNext;
                int give = (nIdle - taken) < avail ? (nIdle - taken) : avail;
                if (!alive && !doStart && p < 0 && myRank >= taken && myRank < taken + give) {
                    const int item = resNext + (myRank - taken);
                    doStart = true;
#if RD_WF_SHADOW_FIRST
                    isShadow = item < nShadow;
#else
                    isShadow = item >= nRay;
#endif
                    p = isShadow ? w.shadowq[shadowMap.at(item)] : rayq[rayMap.at(item)];  // (each map knows where its items start)
                }
                resNext += give;
                taken += give;
            }
        }
        RD_WF_STAMP_DRY();
        if (doStart) {
            if (p >= 0) {  // else: an off-frame slot of bounce 0, nothing to trace
                const Ray ray = wfSlotRay(w, set, p, isShadow, tmax);
                if (isShadow) nAny++;
                else nClosest++;
                rs = makeRaySlab(ray);
                pending = -1;
                if (PAIRS) {
                    ord = getMTBVHId(-ray.d);
                    sp = PairStack{0, 0};
                    if (rs.cls == 0 || end == 0) pairStart<COUNT>(s, rs, tmax, cur, pending, ws);  // the root's box
                    else cur = kPairFresh;  // a literal-class ray: traced whole below
                    alive = true;  // also when the root's box is missed: the lane goes through the loop once and is retired below
                } else {
                    nodes = s.nodes[getMTBVHId(-ray.d)];
                    node = 0;
                    alive = node != END;
                }
                hitPrim = -1;
                occluded = false;
                if (fromList && rs.cls != 0 && end != 0) {  // traced (and counted, and retired) by the workgroup above
                    if (isShadow) nAny--;
                    else nClosest--;
                    alive = false;
                    p = -1;
                }
            }
        }
        unsigned long long am = __ballot(alive);
        if (am == 0ull) {
            if (exhausted) break;
            continue;
        }

        // ---- literal-class rays: traced whole by the whole wave (traverse.h, coopTraceWhole) ----
        {
            unsigned long long lit = __ballot(PAIRS ? (alive && cur == kPairFresh) : (alive && rs.cls != 0 && node == 0 && pending < 0));
            while (lit) {
                const int L = __ffsll((long long)lit) - 1;
                lit &= lit - 1ull;
                const bool shadowL = readlaneI(isShadow ? 1 : 0, L) != 0;
                const NodeRec *un = PAIRS ? s.nodes[0] + (size_t)readlaneI(ord, L) * (size_t)(end + 1) : readlanePtr(nodes, L);
                const RaySlab ur = readlaneRay(rs, L);
                const float lim = readlaneF(tmax, L);
                CoopTrace ct = shadowL ? coopTraceWhole<true>(s, un, ur, lim) : coopTraceWhole<false>(s, un, ur, lim);
                if (int(threadIdx.x & 63u) == L) {
                    hitPrim = ct.hitPrim;
                    hitBary = ct.bary;
                    tmax = ct.tmax;
                    occluded = ct.found;
                    node = END;
                    cur = kPairNone;
                    alive = false;
                    if (COUNT) {
                        ws.nodes += ct.nodes;
                        ws.tris += ct.tris;
                    }
                }
            }
        }
        // ---- box steps until a quarter of the lanes that entered the loop have stopped walking (parked on a leaf or finished):
        // one ballot + popcount per step, as in k_walk_persistent; every walker here is of class 0 (the others were traced whole).
        // (Until the end of round 2 this loop took two ballots per step, tested "enough lanes alive" as well and went through the
        // class dispatch of boxTest: the teapots frame 10.0 -> 9.3 ms, the Cornell frame 4.6 -> 4.0 ms with three sub-frames.) ----
        if (PAIRS) {
            bool busy = alive && pending < 0;  // cur >= 0 or entries on the stack
            const int nStart = __popcll(__ballot(busy));
            if (nStart > 0) {
                const int minWalk = (nStart * (RD_LEAF_DEN - RD_LEAF_NUM) + RD_LEAF_DEN - 1) / RD_LEAF_DEN;
                const int lane = int(threadIdx.x & 63u);
                do {
                    pairPopOne<COUNT>(stk, lane, ovf, tmax, busy, cur, sp, pending, ws);
                    if (busy && cur >= 0) {
                        pairStep<COUNT>(s.pairs, stk, lane, ovf, rs, tmax, ord, cur, sp, pending, ws);
                        busy = pending < 0 && (cur >= 0 || sp.sp > 0);
                    }
                } while (__popcll(__ballot(busy)) >= (minWalk > 1 ? minWalk : 1));
                alive = alive && (pending >= 0 || cur >= 0 || sp.sp > 0);
            }
        } else
        {
            bool walking = alive && pending < 0;
            const int nStart = __popcll(__ballot(walking));
#if RD_WF_COOP_LONE
            if (nStart == 1) {  // a lone walker (the end of a stage): the whole wave tests 64 boxes ahead for it
                const int L = __ffsll((long long)__ballot(walking)) - 1;
                CoopResult cr = coopWalk(readlanePtr(nodes, L), readlaneI(node, L), end, readlaneRay(rs, L), readlaneF(tmax, L), RD_COOP_WINDOWS);
                if (int(threadIdx.x & 63u) == L) {
                    node = cr.node;
                    pending = cr.pending;
                    if (COUNT) ws.nodes += cr.visited;
                    alive = (node != end) || pending >= 0;
                }
            } else
#endif
            if (nStart > 0) {
                const int minWalk = (nStart * (RD_LEAF_DEN - RD_LEAF_NUM) + RD_LEAF_DEN - 1) / RD_LEAF_DEN;
                do {
                    if (walking) {
                        if (COUNT) ws.nodes++;
                        float4 lo = nodes[node].lo_prim;
                        float4 hi = nodes[node].hi_next;
                        float boundDist;
                        bool boundHit = aabbFast(lo, hi, rs, boundDist);
                        if (boundHit && boundDist < tmax) {
                            pending = __float_as_int(lo.w);
                            node++;
                        } else {
                            node = __float_as_int(hi.w);
                        }
                        walking = pending < 0 && node != END;
                        alive = (node != END) || pending >= 0;
                    }
                } while (__popcll(__ballot(walking)) >= (minWalk > 1 ? minWalk : 1));
            }
        }
        // ---- triangle tests of the parked lanes ----
        if (alive && pending >= 0) {
            TriVerts t = loadTri(s.tris, pending);
            float dist;
            v2 bary;
            if (COUNT) ws.tris++;
            bool hit = intersectTriangle(rs, t.a, t.b, t.c, bary, dist);
            if (hit && dist < tmax) {
                if (isShadow) {
                    occluded = true;
                    node = END;
                    cur = kPairNone;
                    sp = PairStack{0, 0};
                } else {
                    hitPrim = pending;
                    tmax = dist;
                    hitBary = bary;
                }
            }
            pending = -1;
            alive = PAIRS ? (cur >= 0 || sp.sp > 0) : (node != END);
        }
        // ---- retire finished lanes: together, once done lanes * 64 >= (walking + done) lanes * RD_WF_FINISH_MIN (the records are
        // dependent read-modify-writes; a lane that has finished keeps its path slot in p until then and is not refilled) ----
        const unsigned long long doneM = __ballot(!alive && p >= 0);
        if (doneM != 0ull && __popcll(doneM) * 64 >= (__popcll(doneM) + __popcll(__ballot(alive))) * RD_WF_FINISH_MIN)
        if (!alive && p >= 0) {
            if (isShadow) {
                if (!occluded) wfAddNee(w, w.nee[set][p]);
            } else {
                bool hit = hitPrim != -1;
                if (hit) nHits++;
                // .w: the shading class of the hit (shade(k)'s material sort bins by it); the distance is not needed again
                w.hit[p] = make_int4(hitPrim, __float_as_int(hit ? hitBary.x : 0.f), __float_as_int(hit ? hitBary.y : 0.f),
                                     hit ? int(s.primClass[hitPrim]) : 0);
            }
            p = -1;
        }
    }
    RD_WF_STAMP(2);
    if (COUNT) flushCounters(s.counters, nClosest, nAny, nHits, ws);
}

// ---- trace(0) as PACKETS ---------------------------------------------------------------------------------------------------------
// Stage 0 is the one trace stage whose rays travel together: its queue is the identity, so the 64 items of 64-slot group g are the
// primary rays of one 8x8 block (k_wf_raygen; k_ad_raygen: one block's pixels, a pixel's samples side by side).  k_wf_trace walks
// them like any stage's, a record fetch per lane and visit, at the walkers' request-rate ceiling; the packet walk
// (traverse.h, packetWalk; kernels_walk.h, walkPacket) makes the same visits with one scalar record load per visit for the wave.
// So this kernel is launched INSTEAD of k_wf_trace<..>(k = 0) (radish_hip.hip, wavefrontStages; RDH_PT_NO_PACKETS keeps that one):
// one wave per group, four groups per workgroup, no ticket, no head, no pull — the host knows rayCount[0] = 64 nGroups.  A kernel
// of its own: k_wf_trace's pair variant sits on its register step.
//
// A slot of stage 0 as walkPacket's work: the item is the queue entry, the record is the hit record k_wf_trace's retire step writes.
struct WfSlotWork {
    const WaveWorkspace &w;
    int p;  // the path slot taken last

    RD_DEV bool find(long long chunk, int slot) {
        const int e = w.rayq[0][chunk * 64 + slot];
        p = e <= -2 ? -2 - e : e;  // -2 - slot: on the first list as well (k_wf_raygen)
        return e != -1;            // -1: a pixel outside the frame
    }
    RD_DEV Ray ray(float &tmax) const { return wfSlotRay(w, 0, p, false, tmax); }
    RD_DEV void store(const DScene &s, const RaySlab &, int hitPrim, v2 hitBary, float, bool) const {
        const bool hit = hitPrim != -1;
        w.hit[p] = make_int4(hitPrim, __float_as_int(hit ? hitBary.x : 0.f), __float_as_int(hit ? hitBary.y : 0.f),
                             hit ? int(s.primClass[hitPrim]) : 0);
    }
};
// The first list, in the same launch: workgroup b < min(nLit, G) traces the entries b, b + G, ... together (wgTraceWhole) before its
// waves take their groups, so the handful of literal-class primary rays (several hundred microseconds each for a workgroup) start
// with the launch and the other workgroups' packets run beside them, as k_wf_trace hides its list behind its ordinary rays.
// Who traces a listed ray is decided by the ray both sides build (wfSlotRay, makeRaySlab): the list if raySetAside(class) — the
// classes that wander, 1..4 — else the lane that owns the slot, in its packet (class 0: the hint did not hold) or whole (class 5).
// An entry beyond the list's capacity stayed in the queue as a plain slot, and its own wave traces it whole, in place.
#ifndef RD_WF_PRIMARY_WAVES
#define RD_WF_PRIMARY_WAVES 1  // waves per SIMD the kernel is held to (1: whatever its registers allow)
#endif
template <bool COUNT>
__global__ __launch_bounds__(256, COUNT ? 1 : RD_WF_PRIMARY_WAVES) void k_wf_trace_primary(DScene s, WaveWorkspace w, int nGroups, int budget) {
    __shared__ WgTraceSharedT<256> wgsh;
    const int nLit = w.ctr->litCount[0].v < w.litCap ? w.ctr->litCount[0].v : w.litCap;
    WalkStats ws{0, 0};
    unsigned nClosest = 0, nHits = 0;
    for (int it = int(blockIdx.x); it < nLit; it += int(gridDim.x)) {  // uniform over the workgroup
        const int pp = w.litq[0][it];  // (stage 0 lists extension rays only)
        float lim;
        const Ray ray = wfSlotRay(w, 0, pp, false, lim);
        const RaySlab urs = makeRaySlab(ray);
        if (!raySetAside(urs.cls) || s.bvhSize == 0) continue;  // walkPacket's condition: the slot's own lane has this one
        const CoopTrace ct = wgTraceWhole<false, 256>(s, s.nodes[getMTBVHId(-ray.d)], urs, lim, wgsh);
        if (threadIdx.x == 0) {  // the record of the finished ray (as in k_wf_trace)
            nClosest++;
            const bool hit = ct.hitPrim != -1;
            if (hit) nHits++;
            w.hit[pp] = make_int4(ct.hitPrim, __float_as_int(hit ? ct.bary.x : 0.f), __float_as_int(hit ? ct.bary.y : 0.f),
                                  hit ? int(s.primClass[ct.hitPrim]) : 0);
            if (COUNT) {
                ws.nodes += ct.nodes;
                ws.tris += ct.tris;
            }
        }
    }
    if (COUNT && threadIdx.x < 64u) flushCounters(s.counters, nClosest, 0u, nHits, ws);  // (wave 0: lane 0 holds the list's counts)
    const int group = int(blockIdx.x) * 4 + int(threadIdx.x >> 6);
    if (group >= nGroups) return;
    const bool listed = w.rayq[0][(size_t)group * 64 + (threadIdx.x & 63u)] <= -2;  // this lane's ray is the list's if it is set aside
    WfSlotWork work{w, -1};
    walkPacket<COUNT, true>(s, group, listed, budget, work);
}

// ---- shade(k): hit k → terminate or run bounce body k+1 ----------------------------------------------------------
// sorted != 0 (material sort, BASELINE config 3): the wave bins the 1 024 records of its packet by BSDF class BEFORE it
// shades them — class of every record (trace(k) left it in the hit record: one gather), a counting
// sort by ballots into a 4-KB LDS table of the wave, then the 16 chunks are shaded in class order: at most three of the
// sixteen chunks straddle a class boundary, the others run one branch of the material switch.  Round 1 had a separate pass over
// the hit records for this (k_wf_classify: four global class queues, 0.2 ms per bounce on the teapots frame — the sorted
// pipeline was 1.8 ms SLOWER than the unsorted one); the binning now costs no launch, no global queue and no extra read of the
// hit records.  Classes: 0 = terminal (miss / emitter / other), 1 = Lambertian, 2 = metallic workflow, 3 = dielectric.
constexpr int kSortChunks = 16;                  // chunks of 64 records per sorted packet
constexpr int kSortPacket = 64 * kSortChunks;    // records a wave bins at a time
#ifndef RD_WF_SHADE_WAVES
#define RD_WF_SHADE_WAVES 1  // waves per SIMD k_wf_shade is held to (1: whatever its 131 VGPRs allow = 3)
#endif
// ... and AT MOST, as RD_WF_PAIR_MAX_WAVES holds k_wf_trace's pair variant: the kernel needs 127 to 131 registers, across the step
// at 128, and which side it lands on moves with unrelated edits (the sharded pull took it to 127).  Four waves per SIMD gained
// nothing on the tree they were measured on (the entry on the appends; not measured again with the shards) and make
// every stage's grid, packets and append bursts a third larger: three keep the stage what tests/test_kernel_resources.py pins.  The host
// holds the resident grid to as many workgroups per CU (radish_hip.hip, wavefrontPrepare).  8: no bound.
#ifndef RD_WF_SHADE_MAX_WAVES
#define RD_WF_SHADE_MAX_WAVES 3
#endif
// Rays that are not queued ("Rays whose outcome cannot reach the image"; walkAll != 0 — RDH_PT_WALK_ALL, and every
// counting launch — queues them all, the reference's order of work):
//   * RD_WF_CULL_LAST: the extension ray shade(maxDepth - 1) emits is walked by trace(maxDepth) only to learn whether it ends on an
//     emitter — pathStep at k == maxDepth adds an emitter's radiance, or the environment's on a miss, and returns at the depth bound
//     otherwise.  Without an environment map a ray that misses the padded box over the emissive triangles (emitBox, made by
//     k_emitter_bounds earlier in this pass; ray_cull.h) adds nothing: it goes on neither rayq nor the first list, and shade(maxDepth)
//     never sees its record.  The path's shadow ray of the same bounce is queued as ever.
//   * RD_WF_SKIP_NULL_NEE: pathStep has a shadow ray traced for every NEE sample, also for one that can add nothing (no kind, or a
//     contribution of zeros: the light below the horizon).  wfAddNee returns at once for the first, and adds zeros for the second
//     to an accumulator that k_wf_raygen set to +0 and that only ever receives sums, so it is never -0 and a + (+-0) == a bit for
//     bit.  Such a ray goes on neither shadowq nor the first list, and its target is not stored.
#ifndef RD_WF_CULL_LAST
#define RD_WF_CULL_LAST 1  // 0: queue every extension ray (measurements)
#endif
#ifndef RD_WF_SKIP_NULL_NEE
#define RD_WF_SKIP_NULL_NEE 1  // 0: queue every shadow ray (measurements)
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RD_WF_SHADE_WAVES, RD_WF_SHADE_MAX_WAVES)))
void k_wf_shade(DScene s, WaveWorkspace w, int k, int maxDepth, int sorted, const float4 *__restrict__ emitBox, int walkAll) {
    __shared__ int sSorted[4][kSortPacket];  // per wave of the workgroup: the packet's path slots in class order
    WaveCounters *c = w.ctr;
    // the last bounce's extension rays are tested against the emitter box (uniform loads, this stage only)
    const bool cullLast = RD_WF_CULL_LAST && !walkAll && k + 1 == maxDepth && !hasEnvMap(s);
    const bool skipNull = RD_WF_SKIP_NULL_NEE && !walkAll;
    float4 boxLo = make_float4(0.f, 0.f, 0.f, 0.f), boxHi = boxLo;
    if (cullLast) {
        boxLo = emitBox[0];
        boxHi = emitBox[1];
    }
    const int wg = workgroupTicket(c->shadeTicket[k]);  // stands for blockIdx.x (see wavePull)
    const int lane = int(threadIdx.x & 63u);
    int *mySorted = sSorted[threadIdx.x >> 6];
    {
        WfShardMap hitMap;  // this stage's records: the rays trace(k) walked, in item order
        hitMap.load(c->rayCount[k], __builtin_amdgcn_readfirstlane(c->queueStride[k]), 0);
        const int n = hitMap.total;
        const int *hitq = w.rayq[k & 1];
        int pendShadows = 0, pendRays = 0;  // entries waiting in the wave's sSorted row for the next append (wave-uniform)
        // unsorted: packets of kShadePacket = 256 records.  sorted: 256 .. kSortPacket = 1 024 records (multiples of 256), as large
        // as still leaves every wave about two packets — with one big packet per wave there is no dynamic balancing left and a
        // short queue (the Cornell frame after bounce 1) would keep nine waves in ten idle while the others shade 16 chunks each
        int packet = kShadePacket;
        if (sorted) {
            const int perWave = n / (2 * gridWaves());
            packet = ((perWave + kShadePacket - 1) / kShadePacket) * kShadePacket;
            packet = packet < kShadePacket ? kShadePacket : (packet > kSortPacket ? kSortPacket : packet);
        }
        // what this stage appends lies in shards of R entries (WfShardMap); trace(k + 1) and shade(k + 1) read R from the counters
        const int outStride = wfQueueStride(n, packet);
        if (wg == 0 && threadIdx.x == 0) c->queueStride[k + 1] = outStride;
        int packetEnd = 0;  // sorted: records of the current packet that exist (<= kSortPacket)
        for (int base = logicalWave(wg) * packet, sub = 0, fresh = 1;;) {
            if (sub == packet) {
                base = wavePull(c->shadeHead[k], logicalWave(wg), packet, n);
                sub = 0;
                fresh = 1;
            }
            if (base + sub >= n) break;
            if (sorted && fresh) {  // bin this packet: counting sort of up to 1 024 records by class
                fresh = 0;
                packetEnd = (n - base) < packet ? (n - base) : packet;
                int pp[kSortChunks], cls[kSortChunks];
#pragma unroll
                for (int j = 0; j < kSortChunks; j++) {
                    const int i = base + j * 64 + lane;
                    pp[j] = (j * 64 + lane < packetEnd) ? hitq[hitMap.at(i)] : -1;
                    if (pp[j] <= -2) pp[j] = -2 - pp[j];  // a ray trace(k) started first (literal-class list): same path slot
                }
#pragma unroll
                for (int j = 0; j < kSortChunks; j++) {
                    // class of the hit, as trace(k) recorded it; off-frame slots of bounce 0 (p = -1) sort with the terminal
                    // class and are skipped below
                    cls[j] = (pp[j] >= 0) ? w.hit[pp[j]].w : 0;
                }
                int at = 0;  // running position in class order (wave-uniform)
#pragma unroll
                for (int qq = 0; qq < 4; qq++) {
#pragma unroll
                    for (int j = 0; j < kSortChunks; j++) {
                        const bool in = (j * 64 + lane < packetEnd) && cls[j] == qq;
                        const unsigned long long m = __ballot(in);
                        if (in) mySorted[at + __popcll(m & laneMaskLt())] = pp[j];
                        at += __popcll(m);
                    }
                }
                __builtin_amdgcn_wave_barrier();  // one wave writes and then reads its own table: LDS executes a wave's ops in order
            }
            int item = base + sub + lane;
            const int subNow = sub;
            sub += 64;
            bool active = sorted ? (subNow + lane < packetEnd) : (item < n);
            bool emitShadow = false, emitRay = false, litShadow = false, litRay = false, rayFirst = false;
            int p = -1;
            // the record's slot in stage k + 1 if its path goes on: its position in this stage's processing order (the queue index, or
            // the place in class order inside the packet), unique and below n (WaveWorkspace)
            const int q = base + subNow + lane;
            if (active) {
                p = sorted ? mySorted[subNow + lane] : hitq[hitMap.at(item)];
                if (p <= -2) p = -2 - p;  // (see the binning above)
                active = p >= 0;
            }
            if (active) {
                const int4 h = w.hit[p];
                const float4 rdw = w.rd[k & 1][p];
                WaveSlotPath st{w, k & 1, p, (k + 1) & 1, q, p, rdw.w != 0.f};
                const PathStepResult r = pathStep(s, k, maxDepth, h.x, mk2(__int_as_float(h.y), __int_as_float(h.z)), mk3(rdw.x, rdw.y, rdw.z), st);
                // the rays go to trace(k+1)'s queues below.  The two hints (trace classifies the ray it builds): some component of the
                // direction below 1.1e-6 of its length
                if (r.shadow && !(skipNull && st.nullNee)) {
                    w.sht[(k + 1) & 1][q] = make_float4(r.shadowTo.x, r.shadowTo.y, r.shadowTo.z, 0.f);
                    emitShadow = true;
                    const v3 dl = r.shadowTo - r.shadowFrom;
                    const float l2 = dot(dl, dl) * 1.21e-12f;
                    litShadow = dl.x * dl.x < l2 || dl.y * dl.y < l2 || dl.z * dl.z < l2;
                }
                if (r.extension && !(cullLast && !mayReachEmitters(boxLo, boxHi, r.ray.o, r.ray.d))) {
                    emitRay = true;
                    litRay = fabs_(r.ray.d.x) < 1.1e-6f || fabs_(r.ray.d.y) < 1.1e-6f || fabs_(r.ray.d.z) < 1.1e-6f;
                }
            }
            if (__ballot(litShadow || litRay) != 0ull) {  // rare: a few hundred rays per stage
                int *lq = w.litq[(k + 1) & 1];
                int *lc = &c->litCount[k + 1].v;
                for (int kind = 0; kind < 2; kind++) {
                    const bool pred = kind == 0 ? litShadow : litRay;
                    const unsigned long long m = __ballot(pred);
                    if (m == 0ull) continue;
                    int at = 0;
                    if (lane == 0) at = atomicAdd(lc, __popcll(m));
                    at = __shfl(at, 0, 64) + __popcll(m & laneMaskLt());
                    if (kind == 0) {  // (rdh_debug_wf_counts: shadowCount does not hold the listed ones)
                        const int listed = __popcll(__ballot(pred && at < w.litCap));
                        if (lane == 0 && listed > 0) atomicAdd(&c->litShadowCount[k].v, listed);
                    }
                    if (pred && at < w.litCap) {  // beyond the list's capacity the ray stays in its ordinary queue
                        lq[at] = kind == 0 ? (q | kWfLitShadow) : q;
                        if (kind == 0) emitShadow = false;  // nobody else reads the shadow queue
                        else rayFirst = true;  // the ray queue is also shade(k+1)'s list of hits: the entry stays, marked as traced
                    }
                }
            }
            // (the lane has read its entry of this chunk from the row above: the place is free until the next packet is binned)
            mySorted[subNow + lane] = (emitShadow ? 1 : 0) | (emitRay ? 2 : 0) | (rayFirst ? 4 : 0);
            pendShadows += __popcll(__ballot(emitShadow));
            pendRays += __popcll(__ballot(emitRay));
            if ((sub & (kAppendSpan - 1)) == 0 || sub == packet || base + sub >= n) {
                int atS = 0, atR = 0;  // both atomics are in flight together
                const int shard = (base / packet) % kQueueShards;  // the packet's shard: its counters, its region of either queue
                if (lane == 0) {
                    if (pendShadows > 0) atS = atomicAdd(&c->shadowCount[k][shard].v, pendShadows);
                    if (pendRays > 0) atR = atomicAdd(&c->rayCount[k + 1][shard].v, pendRays);
                }
                atS = __builtin_amdgcn_readfirstlane(atS) + shard * outStride;
                atR = __builtin_amdgcn_readfirstlane(atR) + shard * outStride;
                int *nextq = w.rayq[(k + 1) & 1];
                for (int o = subNow & ~(kAppendSpan - 1); o < sub; o += 64) {  // the chunks shaded since the last append
                    const int f = mySorted[o + lane], qq = base + o + lane;
                    const unsigned long long mS = __ballot((f & 1) != 0), mR = __ballot((f & 2) != 0);
                    if (f & 1) w.shadowq[atS + __popcll(mS & laneMaskLt())] = qq;
                    if (f & 2) nextq[atR + __popcll(mR & laneMaskLt())] = (f & 4) ? -2 - qq : qq;
                    atS += __popcll(mS);
                    atR += __popcll(mR);
                }
                pendShadows = pendRays = 0;
            }
        }
    }
}

// ---- finish: NaN scrub, HDRToLDR, running mean (pathtrace.cu:279-290) ------------------------------------------
// One thread per pixel.  The pixel's `samples` slots (k_wf_raygen's order) are folded into its two running
// means in sample order, each with storeRunningMean's expression at its own iter, so the image equals `samples` single launches.
RD_DEV v3 foldRunningMean(v3 mean, float4 acc, int iter) {
    return (mean * float(iter) + finishSample(mk3(acc.x, acc.y, acc.z))) / float(iter + 1);
}
__global__ __launch_bounds__(256) void k_wf_finish(PixelMap pm, WaveWorkspace w, int iter, int samples, float *__restrict__ directIllum,
                                                   float *__restrict__ indirectIllum, int part, int parts) {
    unsigned wg;
    const unsigned nLocal = subFrameBlocks(pm, part, parts);
    bool wgValid = xcdSwizzle(blockIdx.x, (nLocal + 3u) >> 2, wg);
    unsigned lane = threadIdx.x & 63u;
    unsigned blockLocal = wgValid ? wg * 4u + (threadIdx.x >> 6) : 0xffffffffu / 64u;
    const bool inRange = wgValid && blockLocal < nLocal;
    Pix px = mapPixel(pm, inRange ? blockLocal * (unsigned)parts + (unsigned)part : 0xffffffffu / 64u, lane);
    if (!(px.valid && inRange)) return;
    v3 direct = load3(directIllum, px.out), indirect = load3(indirectIllum, px.out);
    for (int b = 0; b < samples; b++) {
        const int p = int(((unsigned)b * nLocal + blockLocal) * 64u + lane);
        direct = foldRunningMean(direct, w.accD[p], iter + b);
        indirect = foldRunningMean(indirect, w.accI[p], iter + b);
    }
    store3(directIllum, px.out, direct);
    store3(indirectIllum, px.out, indirect);
}

}  // namespace rd
