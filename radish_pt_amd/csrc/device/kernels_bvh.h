// radish_pt_amd/csrc/device/kernels_bvh.h — the binned-SAH builder on the device, bit-identical to rdh_build_bvh
// (csrc/host/scene_build.cpp), and the upload-time derivatives of its tree (threaded NodeRec arrays, sibling pairs, root box,
// treeDepth) written directly, so that rdh_scene_update_geometry never takes the tree through the host.
//
// Structure: one persistent launch, k_bvh_build.  Each workgroup (four waves) takes a node job {slot, primitive
// range, the six ordering positions, pair number, pending far children} from a queue, splits the node exactly as the host does
// and pushes the inner children it does not go on with itself; a leaf child is finished in place.  The level loop never leaves
// the device, so a chain (n coincident triangles, n - 1 levels) costs n - 1 node steps of one workgroup, not n host round trips.
//
// What makes it bit-identical:
//  - min/max folds.  The host folds f3min / f3max (`b < a ? b : a`) in index order from an empty box.  Every fold here is the
//    same operation on values normalised as the host's first step would leave them (`x < FLT_MAX ? x : FLT_MAX`: NaN and +inf
//    never replace the empty box), combined in a tree that keeps index order (the earlier operand is always the left one).  On
//    such values `comb` is associative, so the ordered tree gives the host's bits, signs of zero included.
//  - bucketOf, the non-accumulating left/right unions, the glm::mix cost and the first strict minimum: the host's code, with
//    IEEE division (the library builds with -ffp-contract=off -fno-fast-math).
//  - the partition: left primitives forward in order, right ones backward from the end; ranks from wave ballots, wave offsets
//    from the per-wave bucket counts.
//  - the orderings: ordering k's choice of first child needs only the children's box centres along k / 2, which do not depend
//    on the sign of a zero, so the parent takes them from value-exact child bounds it folds during its partition pass.
#pragma once
#include "layouts.h"

namespace rd {

constexpr int kBvhBuckets = 16;
constexpr int kBvhThreads = 256;  // one builder workgroup: four waves
constexpr int kBvhWaves = kBvhThreads / 64;

struct BvhPrim {  // primitive reference: its bound (the three vertices' min / max) and id
    float4 lo_id;  // lo.xyz, primId (int bits)
    float4 hi;     // hi.xyz, 0
};

struct BvhJob {  // one inner node to split; `slot` < 0 = not yet published
    int slot, first, last, buf;
    int pos[6];   // its index in each of the six threaded orderings
    int q;        // its pair number: inner nodes before it in ordering 0
    int pend[6];  // far children pending when a walk in ordering k reaches it
    int pad[7];
};
static_assert(sizeof(BvhJob) == 96, "BvhJob");

// The builder's workspace (device pointers; sized for numPrims).
struct BvhWork {
    const float *verts;     // float[3N][3]
    BvhPrim *prims[2];      // N each: the ranges of a node live in prims[job.buf]; its partition writes prims[buf ^ 1]
    BvhJob *queue;          // max(N - 1, 1)
    int *ctl;               // [0] claimed jobs, [1] pushed jobs, [2] finished inner nodes, [3] treeDepth, [4] error flag
    int *info;              // per depth-first slot: leaf -> primitive id, inner -> -(slots of its subtree)
    int *bits;              // inner slots: bit k set when ordering k visits the RIGHT child first
    int *qnum;              // inner slots: pair number
    float *boxes;           // float[2N - 1][6] (output)
    int *nodes[6];          // int[2N - 1][3] each (output)
    int numPrims;
};

RD_DEV float bvhLo(float x) { return x < 3.402823466e+38f ? x : 3.402823466e+38f; }     // f3min(empty, x)
RD_DEV float bvhHi(float x) { return -3.402823466e+38f < x ? x : -3.402823466e+38f; }   // f3max(empty, x)
RD_DEV float combLo(float a, float b) { return b < a ? b : a; }  // a earlier than b
RD_DEV float combHi(float a, float b) { return a < b ? b : a; }

// Ordered wave reduction: after it every lane holds the fold of the 64 lanes' values in lane order.
template <int N>
RD_DEV void waveFoldOrdered(float (&v)[N], int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool later = (lane & d) != 0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const float o = __shfl_xor(v[j], d, 64);
            const float a = later ? o : v[j], b = later ? v[j] : o;
            v[j] = (j % 6) < 3 ? combLo(a, b) : combHi(a, b);
        }
    }
}

RD_DEV int bvhBucketOf(float c, float lo, float hi) {  // scene_build.cpp bucketOf
    float f = (c - lo) / (hi - lo) * kBvhBuckets;
    if (f != f) return 0;
    if (f >= 2147483648.f) return 0;
    if (f <= -2147483648.f) return 0;
    int b = (int)f;
    return b < 0 ? 0 : (b > kBvhBuckets - 1 ? kBvhBuckets - 1 : b);
}

RD_DEV float bvhCenter(float lo, float hi) { return (lo + hi) * .5f; }
RD_DEV float bvhSurfaceArea(const float *b) {  // {lo.xyz, hi.xyz}
    const float sx = b[3] - b[0], sy = b[4] - b[1], sz = b[5] - b[2];
    return 2.f * (sx * sy + sy * sz + sz * sx);
}

// Primitive references from the soup, and the root (a one-triangle scene: the root is a leaf, written here).
__global__ __launch_bounds__(256) void k_bvh_init(BvhWork w) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = w.numPrims;
    if (i == 0) {
        w.ctl[0] = w.ctl[1] = w.ctl[2] = w.ctl[3] = w.ctl[4] = 0;
        if (N > 1) {
            BvhJob j{};
            j.slot = 0;
            j.first = 0;
            j.last = N - 1;
            w.queue[0] = j;
            w.ctl[1] = 1;
        }
    }
    if (i >= N) return;
    const float *v = w.verts + 9 * (size_t)i;
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {  // f3min(f3min(v0, v1), v2), f3max likewise
        float m = v[3 + a] < v[a] ? v[3 + a] : v[a];
        lo[a] = v[6 + a] < m ? v[6 + a] : m;
        float M = v[a] < v[3 + a] ? v[3 + a] : v[a];
        hi[a] = M < v[6 + a] ? v[6 + a] : M;
    }
    w.prims[0][i].lo_id = make_float4(lo[0], lo[1], lo[2], __int_as_float(i));
    w.prims[0][i].hi = make_float4(hi[0], hi[1], hi[2], 0.f);
    if (N == 1) {
        for (int a = 0; a < 3; a++) {
            w.boxes[a] = bvhLo(lo[a]);
            w.boxes[3 + a] = bvhHi(hi[a]);
        }
        w.info[0] = 0;
        for (int k = 0; k < 6; k++) {
            w.nodes[k][0] = 0;
            w.nodes[k][1] = 0;
            w.nodes[k][2] = 1;
        }
    }
}

// Mark every queue entry unpublished (slot = -1) before a build.
__global__ __launch_bounds__(256) void k_bvh_clear_queue(BvhJob *q, int n, int skipFirst) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x) + skipFirst;
    if (i < n) q[i].slot = -1;
}

__global__ __launch_bounds__(kBvhThreads) void k_bvh_build(BvhWork w) {
    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int N = w.numPrims, S = 2 * N - 1, innerTotal = N - 1;
    __shared__ BvhJob job;
    __shared__ int sExit, sHaveLocal;
    __shared__ float wRes[kBvhWaves][12];
    __shared__ float wBucket[kBvhWaves][kBvhBuckets][6];
    __shared__ int wCount[kBvhWaves][kBvhBuckets];
    __shared__ int sAxis, sSplit, sMid, sLeftOff[kBvhWaves], sRightOff[kBvhWaves];
    __shared__ float sLo, sHi;
    __shared__ float bucketBound[kBvhBuckets][6];  // thread 0's split search works in LDS, not in scratch
    __shared__ int bucketCount[kBvhBuckets], prefix[kBvhBuckets];
    if (tid == 0) sHaveLocal = 0;
    __syncthreads();
    for (;;) {
        if (tid == 0) {
            sExit = 0;
            if (!sHaveLocal) {
                const int idx = atomicAdd(&w.ctl[0], 1);
                if (idx >= innerTotal) {
                    sExit = 1;
                } else {
                    for (;;) {
                        const int s = __hip_atomic_load(&w.queue[idx].slot, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                        if (s >= 0) break;
                        if (__hip_atomic_load(&w.ctl[2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= innerTotal ||
                            __hip_atomic_load(&w.ctl[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                            sExit = 1;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(4);
                    }
                    if (!sExit) {
                        const int *src = reinterpret_cast<const int *>(&w.queue[idx]);
                        int *dstj = reinterpret_cast<int *>(&job);
                        for (int k = 0; k < 24; k++) dstj[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            sHaveLocal = 0;
        }
        __syncthreads();
        if (sExit) break;
        // the node's range was written by other workgroups (queue) or by this one's other waves (local step): drop stale L1 lines
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int first = job.first, last = job.last, count = last - first + 1;
        const BvhPrim *src = w.prims[job.buf];
        BvhPrim *dst = w.prims[job.buf ^ 1];
        const int chunk = (count + kBvhWaves - 1) / kBvhWaves;
        const int wBeg = first + wave * chunk;
        const int wEnd = min(wBeg + chunk, last + 1);

        // pass 1: node bound and centroid bound, in index order
        {
            float acc[12];
#pragma unroll
            for (int j = 0; j < 12; j++) acc[j] = (j % 6) < 3 ? 3.402823466e+38f : -3.402823466e+38f;
            for (int base = wBeg; base < wEnd; base += 64) {
                const int e = base + lane;
                float v[12];
                if (e < wEnd) {
                    const float4 L = src[e].lo_id, H = src[e].hi;
                    v[0] = bvhLo(L.x); v[1] = bvhLo(L.y); v[2] = bvhLo(L.z);
                    v[3] = bvhHi(H.x); v[4] = bvhHi(H.y); v[5] = bvhHi(H.z);
                    const float cx = bvhCenter(L.x, H.x), cy = bvhCenter(L.y, H.y), cz = bvhCenter(L.z, H.z);
                    v[6] = bvhLo(cx); v[7] = bvhLo(cy); v[8] = bvhLo(cz);
                    v[9] = bvhHi(cx); v[10] = bvhHi(cy); v[11] = bvhHi(cz);
                } else {
#pragma unroll
                    for (int j = 0; j < 12; j++) v[j] = (j % 6) < 3 ? 3.402823466e+38f : -3.402823466e+38f;
                }
                waveFoldOrdered(v, lane);
#pragma unroll
                for (int j = 0; j < 12; j++) acc[j] = (j % 6) < 3 ? combLo(acc[j], v[j]) : combHi(acc[j], v[j]);
            }
            if (lane == 0)
                for (int j = 0; j < 12; j++) wRes[wave][j] = acc[j];
        }
        __syncthreads();
        if (tid == 0) {
            float b[12];
            for (int j = 0; j < 12; j++) b[j] = (j % 6) < 3 ? 3.402823466e+38f : -3.402823466e+38f;
            for (int q = 0; q < kBvhWaves; q++)
                for (int j = 0; j < 12; j++) b[j] = (j % 6) < 3 ? combLo(b[j], wRes[q][j]) : combHi(b[j], wRes[q][j]);
            float *ob = w.boxes + 6 * (size_t)job.slot;
            for (int j = 0; j < 6; j++) ob[j] = b[j];
            const float sx = b[9] - b[6], sy = b[10] - b[7], sz = b[11] - b[8];  // Box::longestAxis of the centroid bound
            int axis;
            if (sx < sy) axis = sy > sz ? 1 : 2;
            else axis = sx > sz ? 0 : 2;
            sAxis = axis;
            sLo = b[6 + axis];
            sHi = b[9 + axis];
        }
        __syncthreads();
        const int axis = sAxis;
        const float clo = sLo, chi = sHi;

        // pass 2: bucket bounds and counts per wave, in index order
        if (lane < kBvhBuckets) {
            wCount[wave][lane] = 0;
            for (int j = 0; j < 6; j++) wBucket[wave][lane][j] = j < 3 ? 3.402823466e+38f : -3.402823466e+38f;
        }
        __builtin_amdgcn_wave_barrier();
        for (int base = wBeg; base < wEnd; base += 64) {
            const int e = base + lane;
            const bool valid = e < wEnd;
            float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int bk = -1;
            if (valid) {
                const float4 L = src[e].lo_id, H = src[e].hi;
                v[0] = bvhLo(L.x); v[1] = bvhLo(L.y); v[2] = bvhLo(L.z);
                v[3] = bvhHi(H.x); v[4] = bvhHi(H.y); v[5] = bvhHi(H.z);
                const float c = axis == 0 ? bvhCenter(L.x, H.x) : (axis == 1 ? bvhCenter(L.y, H.y) : bvhCenter(L.z, H.z));
                bk = bvhBucketOf(c, clo, chi);
            }
            for (int j = 0; j < kBvhBuckets; j++) {
                const unsigned long long m = __ballot(bk == j);
                if (m == 0) continue;
                float u[6];
#pragma unroll
                for (int t = 0; t < 6; t++) u[t] = bk == j ? v[t] : (t < 3 ? 3.402823466e+38f : -3.402823466e+38f);
                waveFoldOrdered(u, lane);
                if (lane == 0) {
                    wCount[wave][j] += __popcll(m);
                    for (int t = 0; t < 6; t++)
                        wBucket[wave][j][t] = t < 3 ? combLo(wBucket[wave][j][t], u[t]) : combHi(wBucket[wave][j][t], u[t]);
                }
            }
        }
        __syncthreads();
        if (tid == 0) {  // scene_build.cpp:118-152, as is
            for (int j = 0; j < kBvhBuckets; j++) {
                for (int t = 0; t < 6; t++) bucketBound[j][t] = t < 3 ? 3.402823466e+38f : -3.402823466e+38f;
                bucketCount[j] = 0;
                for (int q = 0; q < kBvhWaves; q++) {
                    for (int t = 0; t < 6; t++)
                        bucketBound[j][t] = t < 3 ? combLo(bucketBound[j][t], wBucket[q][j][t]) : combHi(bucketBound[j][t], wBucket[q][j][t]);
                    bucketCount[j] += wCount[q][j];
                }
            }
            // left[i] = bucket[i-1] (left[0] = bucket[0]), right[j] = bucket[j+1] (right[15] = bucket[15]): growing an empty box by
            // one bucket bound gives that bound's bits (its values are already normalised)
            prefix[0] = bucketCount[0];
            for (int i = 1; i < kBvhBuckets; i++) prefix[i] = prefix[i - 1] + bucketCount[i];
            float best = 3.402823466e+38f;
            int split = 0;
            for (int i = 0; i < kBvhBuckets - 1; i++) {
                const float a = float(prefix[i]) / count;
                const float *lb = bucketBound[i == 0 ? 0 : i - 1];
                const float *rb = bucketBound[i + 1 == kBvhBuckets - 1 ? kBvhBuckets - 1 : i + 2];
                const float cost = bvhSurfaceArea(lb) * (1.f - a) + bvhSurfaceArea(rb) * a;
                if (cost < best) {
                    best = cost;
                    split = i;
                }
            }
            sSplit = split;
            int lOff = first, rOff = last;
            for (int q = 0; q < kBvhWaves; q++) {
                int nl = 0, nAll = 0;
                for (int j = 0; j < kBvhBuckets; j++) {
                    nAll += wCount[q][j];
                    if (j <= split) nl += wCount[q][j];
                }
                sLeftOff[q] = lOff;
                sRightOff[q] = rOff;
                lOff += nl;
                rOff -= nAll - nl;
            }
            sMid = min(max(lOff - 1, first), last - 1);
        }
        __syncthreads();
        const int split = sSplit, mid = sMid;

        // pass 3: partition into dst, and value-exact bounds of the two children (for the orderings' choices)
        {
            int lo = sLeftOff[wave], ro = sRightOff[wave];
            float acc[12];
#pragma unroll
            for (int j = 0; j < 12; j++) acc[j] = (j % 6) < 3 ? 3.402823466e+38f : -3.402823466e+38f;
            for (int base = wBeg; base < wEnd; base += 64) {
                const int e = base + lane;
                const bool valid = e < wEnd;
                BvhPrim p{};
                bool goes = false;
                if (valid) {
                    p = src[e];
                    const float c = axis == 0 ? bvhCenter(p.lo_id.x, p.hi.x) : (axis == 1 ? bvhCenter(p.lo_id.y, p.hi.y) : bvhCenter(p.lo_id.z, p.hi.z));
                    goes = bvhBucketOf(c, clo, chi) <= split;
                }
                const unsigned long long mL = __ballot(valid && goes), mR = __ballot(valid && !goes);
                const unsigned long long below = (1ull << lane) - 1ull;
                const int dest = goes ? lo + __popcll(mL & below) : ro - __popcll(mR & below);
                lo += __popcll(mL);
                ro -= __popcll(mR);
                if (valid) {
                    if (dest >= first && dest <= last) dst[dest] = p;
                    else atomicOr(&w.ctl[4], 1);
                }
                const bool left = valid && dest <= mid, right = valid && dest > mid;
                float v[12];
                const float pv[6] = {bvhLo(p.lo_id.x), bvhLo(p.lo_id.y), bvhLo(p.lo_id.z), bvhHi(p.hi.x), bvhHi(p.hi.y), bvhHi(p.hi.z)};
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    v[t] = left ? pv[t] : (t < 3 ? 3.402823466e+38f : -3.402823466e+38f);
                    v[6 + t] = right ? pv[t] : (t < 3 ? 3.402823466e+38f : -3.402823466e+38f);
                }
                waveFoldOrdered(v, lane);
#pragma unroll
                for (int j = 0; j < 12; j++) acc[j] = (j % 6) < 3 ? combLo(acc[j], v[j]) : combHi(acc[j], v[j]);
            }
            if (lane == 0)
                for (int j = 0; j < 12; j++) wRes[wave][j] = acc[j];
        }
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the leaf children below are read back from dst
            float b[12];
            for (int j = 0; j < 12; j++) b[j] = (j % 6) < 3 ? 3.402823466e+38f : -3.402823466e+38f;
            for (int q = 0; q < kBvhWaves; q++)
                for (int j = 0; j < 12; j++) b[j] = (j % 6) < 3 ? combLo(b[j], wRes[q][j]) : combHi(b[j], wRes[q][j]);
            const int slot = job.slot, slots = 2 * count - 1;
            const int nA = mid - first + 1, nB = last - mid;
            const int slotA = slot + 1, slotB = slot + 1 + (2 * nA - 1);
            int bits = 0, pendMax = 0;
            BvhJob cj[2];  // [0] left child (slot A), [1] right child (slot B)
            cj[0].slot = slotA; cj[0].first = first; cj[0].last = mid;
            cj[1].slot = slotB; cj[1].first = mid + 1; cj[1].last = last;
            for (int k = 0; k < 6; k++) {
                const int dim = k / 2;
                const bool lesser = (k & 1) != 0;
                const bool rightFirst = (bvhCenter(b[dim], b[3 + dim]) < bvhCenter(b[6 + dim], b[9 + dim])) != lesser;
                if (rightFirst) bits |= 1 << k;
                const int f = rightFirst ? 1 : 0;
                const int sizeF = rightFirst ? 2 * nB - 1 : 2 * nA - 1;
                cj[f].pos[k] = job.pos[k] + 1;
                cj[f ^ 1].pos[k] = job.pos[k] + 1 + sizeF;
                cj[f].pend[k] = job.pend[k] + 1;
                cj[f ^ 1].pend[k] = job.pend[k];
                pendMax = max(pendMax, job.pend[k] + 1);
                const int p = job.pos[k];
                if (p >= 0 && p < S) {
                    w.nodes[k][3 * p + 0] = -1;
                    w.nodes[k][3 * p + 1] = slot;
                    w.nodes[k][3 * p + 2] = p + slots;
                } else {
                    atomicOr(&w.ctl[4], 2);
                }
            }
            {  // pair numbers: ordering 0's first child follows its parent, the second follows the first one's inner nodes
                const int f0 = bits & 1;
                const int nF0 = f0 ? nB : nA;
                cj[f0].q = job.q + 1;
                cj[f0 ^ 1].q = job.q + nF0;
            }
            w.info[slot] = -slots;
            w.bits[slot] = bits;
            w.qnum[slot] = job.q;
            atomicMax(&w.ctl[3], pendMax);
            int localNext = -1;
            for (int c = 0; c < 2; c++) {
                cj[c].buf = job.buf ^ 1;
                const int cs = cj[c].slot;
                if (cs >= S) { atomicOr(&w.ctl[4], 4); continue; }
                if (cj[c].first == cj[c].last) {  // leaf: finish it here
                    const BvhPrim p = dst[cj[c].first];
                    const int prim = __float_as_int(p.lo_id.w);
                    float *ob = w.boxes + 6 * (size_t)cs;
                    ob[0] = bvhLo(p.lo_id.x); ob[1] = bvhLo(p.lo_id.y); ob[2] = bvhLo(p.lo_id.z);
                    ob[3] = bvhHi(p.hi.x); ob[4] = bvhHi(p.hi.y); ob[5] = bvhHi(p.hi.z);
                    w.info[cs] = prim;
                    for (int k = 0; k < 6; k++) {
                        const int q = cj[c].pos[k];
                        if (q < 0 || q >= S) { atomicOr(&w.ctl[4], 2); continue; }
                        w.nodes[k][3 * q + 0] = prim;
                        w.nodes[k][3 * q + 1] = cs;
                        w.nodes[k][3 * q + 2] = q + 1;
                    }
                } else if (localNext < 0) {
                    localNext = c;  // this workgroup goes on with it
                } else {
                    const int idx = atomicAdd(&w.ctl[1], 1);
                    if (idx >= innerTotal) { atomicOr(&w.ctl[4], 8); continue; }
                    BvhJob *qj = &w.queue[idx];
                    const int *srcj = reinterpret_cast<const int *>(&cj[c]);
                    int *dq = reinterpret_cast<int *>(qj);
                    for (int k = 1; k < 24; k++) dq[k] = srcj[k];
                    __threadfence();
                    __hip_atomic_store(&qj->slot, cs, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (localNext >= 0) {
                job = cj[localNext];
                sHaveLocal = 1;
            }
            __threadfence();
            __hip_atomic_fetch_add(&w.ctl[2], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
}

// The six threaded orderings as NodeRecs in ONE allocation, (S + 1) records each with the pad record at S — what
// rdh_scene_upload makes of the same arrays.
__global__ __launch_bounds__(256) void k_bvh_noderecs(const float *__restrict__ boxes, BvhWork w, NodeRec *__restrict__ out, int S) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 6ll * (S + 1)) return;
    const int k = int(t / (S + 1)), i = int(t % (S + 1));
    NodeRec r;
    if (i == S) {
        r.lo_prim = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        r.hi_next = make_float4(0.f, 0.f, 0.f, __int_as_float(S));
    } else {
        const int *n = w.nodes[k] + 3 * (size_t)i;
        const int box = min(max(n[1], 0), S - 1);
        const float *b = boxes + 6 * (size_t)box;
        r.lo_prim = make_float4(b[0], b[1], b[2], __int_as_float(n[0]));
        r.hi_next = make_float4(b[3], b[4], b[5], __int_as_float(n[2]));
    }
    out[t] = r;
}

// Sibling pairs (layouts.h, PairRec) with buildSharedTree's numbering: the children of the inner node with pair number q are
// canonical records 2q + 1 (ordering 0's first child) and 2q + 2; bit k of the parent = ordering k visits the second one first.
// Also the header {treeDepth, error, -, -, rootLo, rootHi} for the host.  One thread per depth-first slot.
__global__ __launch_bounds__(256) void k_bvh_pairs(BvhWork w, PairRec *__restrict__ pairs, int4 *__restrict__ header) {
    const int s = int(blockIdx.x * blockDim.x + threadIdx.x);
    const int S = 2 * w.numPrims - 1;
    if (s >= S) return;
    const int inf = w.info[s];
    const int canonBits = inf < 0 ? (w.bits[s] ^ ((w.bits[s] & 1) ? 63 : 0)) : 0;
    if (s == 0) {
        const float *b = w.boxes;
        header[0] = make_int4(w.ctl[3], w.ctl[4], 0, 0);
        header[1] = make_int4(__float_as_int(b[0]), __float_as_int(b[1]), __float_as_int(b[2]), inf >= 0 ? inf : ~0);
        header[2] = make_int4(__float_as_int(b[3]), __float_as_int(b[4]), __float_as_int(b[5]), canonBits);
        if (pairs) pairs[(S - 1) / 2] = PairRec{};  // pad record
    }
    if (inf >= 0 || !pairs) return;
    const int a = s + 1;
    const int ia = w.info[min(a, S - 1)];
    const int bslot = a + (ia >= 0 ? 1 : -ia);
    if (a >= S || bslot >= S) return;
    const int c0 = (w.bits[s] & 1) ? bslot : a, c1 = (w.bits[s] & 1) ? a : bslot;
    const int q = w.qnum[s];
    if (q < 0 || q >= (S - 1) / 2) return;
    auto childW = [&](int c) { const int i = w.info[c]; return i >= 0 ? i : ~w.qnum[c]; };
    const float *b0 = w.boxes + 6 * (size_t)c0, *b1 = w.boxes + 6 * (size_t)c1;
    PairRec r;
    r.lo0_w0 = make_float4(b0[0], b0[1], b0[2], __int_as_float(childW(c0)));
    r.hi0_bits = make_float4(b0[3], b0[4], b0[5], __int_as_float(canonBits));
    r.lo1_w1 = make_float4(b1[0], b1[1], b1[2], __int_as_float(childW(c1)));
    r.hi1_pad = make_float4(b1[3], b1[4], b1[5], 0.f);
    pairs[q] = r;
}

// New positions for the same triangles: TriRec (material id kept), AttrRec (texcoords kept; only when normals are given) and the
// emissive triangles' LightRecs (radiance kept).  With `prevTris` (rdh_scene_track_motion) the record that is about to be
// overwritten is kept there first: the positions the last G-buffer render saw, for the motion plane.
__global__ __launch_bounds__(256) void k_geom_update(const float *__restrict__ verts, const float *__restrict__ normals, TriRec *tris,
                                                     AttrRec *attrs, int N, LightRec *lights, const int *__restrict__ lightPrims, int numLights,
                                                     TriRec *__restrict__ prevTris) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < N) {
        const float *v = verts + 9 * (size_t)i;
        float mid;
        if (prevTris) {
            const TriRec old = tris[i];
            prevTris[i] = old;
            mid = old.c.y;
        } else {
            mid = tris[i].c.y;
        }
        tris[i].a = make_float4(v[0], v[1], v[2], v[3]);
        tris[i].b = make_float4(v[4], v[5], v[6], v[7]);
        tris[i].c = make_float4(v[8], mid, 0.f, 0.f);
        if (normals) {
            const float *n = normals + 9 * (size_t)i;
            const float4 c = attrs[i].c;
            attrs[i].a = make_float4(n[0], n[1], n[2], n[3]);
            attrs[i].b = make_float4(n[4], n[5], n[6], n[7]);
            attrs[i].c = make_float4(n[8], c.y, c.z, c.w);
        }
    }
    if (i < numLights) {
        const int p = lightPrims[i];
        if (p < 0 || p >= N) return;
        const float *v = verts + 9 * (size_t)p;
        const float4 c = lights[i].c;
        lights[i].a = make_float4(v[0], v[1], v[2], v[3]);
        lights[i].b = make_float4(v[4], v[5], v[6], v[7]);
        lights[i].c = make_float4(v[8], c.y, c.z, c.w);
    }
}

}  // namespace rd
