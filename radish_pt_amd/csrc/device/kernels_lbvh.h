// radish_pt_amd/csrc/device/kernels_lbvh.h — the linear BVH builder (RDH_BVH_LBVH): Morton codes of the primitive
// centres, an LSD radix sort, Karras' radix tree over the sorted codes, then boxes and orderings bottom-up and each node's place
// in the six threaded orderings.  It fills the same BvhWork outputs as k_bvh_build (boxes, nodes[6], info, bits, qnum, ctl[3],
// ctl[4]), so k_bvh_noderecs, k_bvh_pairs and everything behind them run unchanged.
//
// The tree is fully determined by the vertices (tests/lbvh_model.py restates it):
//  1. primitive box: the refit contract's leaf box (bvhLo / bvhHi over v0, v1, v2 from the empty box); centre (lo + hi) * 0.5f.
//  2. centroid bounds: combLo / combHi folds of the centres from the empty box (values only are used: any fold order will do).
//  3. cell per axis: e = cHi - cLo, t = e > 0 ? (c - cLo) / e : 0, s = t * 1024, q = s > 0 ? (s < 1023 ? (int)s : 1023) : 0.
//  4. 30-bit Morton code, x at bit 3i + 2, y at 3i + 1, z at 3i.
//  5. stable sort by code (equal codes keep ascending primitive id).
//  6. Karras' radix tree; delta(i, j) = clz(code_i ^ code_j), or 32 + clz(i ^ j) for equal codes.  Depth <= 59.
//  7. slots: depth-first pre-order, lower sorted range first: slot = 2 * first + (ancestors at which the path turns left).
//  8. boxes: the refit contract, combLo / combHi(box a, box b) with a ordering 0's first child.
//  9. orderings: the host's rule (ordering k visits the child of the larger centre along k / 2 first, unless k is odd).
//
// Kernels, in launch order:
//  k_lbvh_leaves (fixed grid) + k_lbvh_bounds (one workgroup): leaf boxes, centroid bounds by a reduction of fixed shape.
//  k_lbvh_codes: codes and the identity permutation.
//  4 x {k_lbvh_hist, k_lbvh_scan, k_lbvh_scatter}: LSD radix sort, 8-bit digits.  Per-tile digit counts (digit-major), one
//    exclusive scan over all of them, then a stable scatter that ranks within the tile with wave64 ballots.  No workgroup waits
//    on another: each pass is three launches.
//  k_lbvh_karras: one lane per inner node: its range, split, children, and the children's parent links.
//  k_lbvh_up: one lane per leaf climbs with per-node arrival counters, as k_refit does; the second arrival computes the node's
//    ordering bits and box.  The hand-off is k_refit's: ordering 0's box stored write-through (sc1), drained before
//    the relaxed agent-scope counter add, and read with sc1 loads.  No lane waits on another.
//  k_lbvh_place: one lane per node climbs to the root (<= 59 steps) and sums its slot, its position in each ordering, its pair
//    number and the far children pending in each ordering; then writes the builder's outputs.
#pragma once
#include "kernels_bvh.h"

namespace rd {

constexpr int kLbvhBlocks = 256;                 // fixed grid of the centroid-bound reduction
constexpr int kLbvhTile = 4096;                  // keys per radix-sort tile: 256 threads x 16
constexpr int kLbvhScanThreads = 1024;
constexpr int kLbvhMaxDepth = 64;                // climb bound (the contract's depth is <= 59)

struct LbvhWork {
    const float *verts;
    float4 *leafBox;     // 2 per primitive: lo.xyz, hi.xyz
    float *bounds;       // kLbvhBlocks partials of 6 floats, then the final {cLo.xyz, cHi.xyz}
    unsigned *keys[2];   // N each (ping-pong)
    int *vals[2];        // N each: primitive ids
    int *hist;           // 256 x numTiles, digit-major
    int4 *rec;           // per node: {parent, first, last, bits}; inner node i -> i, leaf at sorted position j -> N - 1 + j
    int2 *child;         // per inner node: {left, right} node ids
    float *nodeBox;      // per node: lo.xyz, -, hi.xyz, -
    int *counters;       // per inner node: arrivals (memset to 0)
    int numPrims, numTiles;
};

RD_DEV unsigned lbvhSpread(unsigned q) {  // 10 bits -> every third bit
    q = (q | (q << 16)) & 0x030000FFu;
    q = (q | (q << 8)) & 0x0300F00Fu;
    q = (q | (q << 4)) & 0x030C30C3u;
    q = (q | (q << 2)) & 0x09249249u;
    return q;
}

RD_DEV void lbvhLeafBox(const float *v, float (&lo)[3], float (&hi)[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        lo[c] = combLo(combLo(bvhLo(v[c]), v[3 + c]), v[6 + c]);
        hi[c] = combHi(combHi(bvhHi(v[c]), v[3 + c]), v[6 + c]);
    }
}

// Leaf boxes, and per-workgroup bounds of the centres (strided loop, fixed LDS tree).
__global__ __launch_bounds__(256) void k_lbvh_leaves(LbvhWork L) {
    __shared__ float s[6][256];
    const int N = L.numPrims;
    float acc[6] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
    for (int p = int(blockIdx.x * blockDim.x + threadIdx.x); p < N; p += kLbvhBlocks * 256) {
        float lo[3], hi[3];
        lbvhLeafBox(L.verts + 9 * (size_t)p, lo, hi);
        L.leafBox[2 * (size_t)p] = make_float4(lo[0], lo[1], lo[2], 0.f);
        L.leafBox[2 * (size_t)p + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float ctr = bvhCenter(lo[c], hi[c]);
            acc[c] = combLo(acc[c], ctr);
            acc[3 + c] = combHi(acc[3 + c], ctr);
        }
    }
#pragma unroll
    for (int j = 0; j < 6; j++) s[j][threadIdx.x] = acc[j];
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < (unsigned)d) {
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const float o = s[j][threadIdx.x + d];
                s[j][threadIdx.x] = j < 3 ? combLo(s[j][threadIdx.x], o) : combHi(s[j][threadIdx.x], o);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) L.bounds[6 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void k_lbvh_bounds(LbvhWork L) {
    __shared__ float s[6][256];
#pragma unroll
    for (int j = 0; j < 6; j++) s[j][threadIdx.x] = L.bounds[6 * threadIdx.x + j];  // kLbvhBlocks == 256
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < (unsigned)d) {
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const float o = s[j][threadIdx.x + d];
                s[j][threadIdx.x] = j < 3 ? combLo(s[j][threadIdx.x], o) : combHi(s[j][threadIdx.x], o);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) L.bounds[6 * kLbvhBlocks + threadIdx.x] = s[threadIdx.x][0];
}
static_assert(kLbvhBlocks == 256, "k_lbvh_bounds reduces one partial per thread");

__global__ __launch_bounds__(256) void k_lbvh_codes(LbvhWork L) {
    const int p = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= L.numPrims) return;
    const float *b = L.bounds + 6 * kLbvhBlocks;
    const float4 lo = L.leafBox[2 * (size_t)p], hi = L.leafBox[2 * (size_t)p + 1];
    const float c[3] = {bvhCenter(lo.x, hi.x), bvhCenter(lo.y, hi.y), bvhCenter(lo.z, hi.z)};
    unsigned code = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float e = b[3 + a] - b[a];
        const float t = e > 0.f ? (c[a] - b[a]) / e : 0.f;
        const float s = t * 1024.f;
        const int q = s > 0.f ? (s < 1023.f ? (int)s : 1023) : 0;
        code |= lbvhSpread((unsigned)q) << (2 - a);
    }
    L.keys[0][p] = code;
    L.vals[0][p] = p;
}

// ---- radix sort: 8-bit digits, tiles of kLbvhTile keys ----

// Digit counts of one tile: hist[digit * numTiles + tile].
__global__ __launch_bounds__(256) void k_lbvh_hist(const unsigned *__restrict__ keys, int N, int shift, int *hist, int numTiles) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = int(blockIdx.x) * kLbvhTile;
    const int end = min(base + kLbvhTile, N);
    for (int e = base + int(threadIdx.x); e < end; e += 256) atomicAdd(&h[(keys[e] >> shift) & 255u], 1);
    __syncthreads();
    hist[(size_t)threadIdx.x * numTiles + blockIdx.x] = h[threadIdx.x];
}

// Exclusive scan of hist[0 .. M) in place, one workgroup: each thread scans a contiguous run.
__global__ __launch_bounds__(kLbvhScanThreads) void k_lbvh_scan(int *hist, int M) {
    __shared__ int s[kLbvhScanThreads];
    const int t = int(threadIdx.x);
    const int per = (M + kLbvhScanThreads - 1) / kLbvhScanThreads;
    const int beg = min(t * per, M), end = min(beg + per, M);
    int sum = 0;
    for (int i = beg; i < end; i++) sum += hist[i];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kLbvhScanThreads; d <<= 1) {  // inclusive Hillis-Steele scan of the run totals
        const int x = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    int run = s[t] - sum;
    for (int i = beg; i < end; i++) {
        const int v = hist[i];
        hist[i] = run;
        run += v;
    }
}

// Stable scatter of one tile, 256 keys at a time in index order: a lane's rank among the wave's lanes of its digit comes from
// eight ballots; the waves before it and the tile's earlier chunks give the rest.
__global__ __launch_bounds__(256) void k_lbvh_scatter(const unsigned *__restrict__ keysIn, const int *__restrict__ valsIn,
                                                      unsigned *__restrict__ keysOut, int *__restrict__ valsOut, int N, int shift,
                                                      const int *__restrict__ hist, int numTiles) {
    __shared__ int run[256];
    __shared__ int wcnt[4][256];
    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    run[tid] = hist[(size_t)tid * numTiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; w++) wcnt[w][tid] = 0;
    __syncthreads();
    const int base = int(blockIdx.x) * kLbvhTile;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int chunk = base; chunk < base + kLbvhTile && chunk < N; chunk += 256) {
        const int e = chunk + tid;
        const bool valid = e < N;
        const unsigned key = valid ? keysIn[e] : 0u;
        const int val = valid ? valsIn[e] : 0;
        const int digit = int((key >> shift) & 255u);
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool set = (digit >> b) & 1;
            const unsigned long long bb = __ballot(set);
            m &= set ? bb : ~bb;
        }
        const int rank = __popcll(m & below);
        if (valid && rank == 0) wcnt[wave][digit] = __popcll(m);
        __syncthreads();
        if (valid) {
            int off = run[digit] + rank;
            for (int w = 0; w < wave; w++) off += wcnt[w][digit];
            keysOut[off] = key;
            valsOut[off] = val;
        }
        __syncthreads();
        run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
#pragma unroll
        for (int w = 0; w < 4; w++) wcnt[w][tid] = 0;
        __syncthreads();
    }
}

// ---- hierarchy ----

RD_DEV int lbvhDelta(const unsigned *__restrict__ k, int N, int i, long long j) {
    if (j < 0 || j >= N) return -1;
    const unsigned x = k[i] ^ k[j];
    return x ? __clz((int)x) : 32 + __clz(i ^ (int)j);
}

// One lane per inner node i (Karras 2012): its range [first, last], split g (children [first, g], [g + 1, last]), children ids
// and their parent links.  A one-primitive scene: the root is leaf 0 (lane 0 writes it).  ctl[4] |= 16 on an impossible index.
__global__ __launch_bounds__(256) void k_lbvh_karras(LbvhWork L, int *ctl) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = L.numPrims;
    const unsigned *k = L.keys[0];
    if (N == 1) {
        if (i == 0) L.rec[0] = make_int4(-1, 0, 0, 0);
        return;
    }
    if (i >= N - 1) return;
    const int d = lbvhDelta(k, N, i, i + 1) - lbvhDelta(k, N, i, i - 1) > 0 ? 1 : -1;
    const int dmin = lbvhDelta(k, N, i, i - d);
    long long lmax = 2;
    while (lmax <= 2ll * N && lbvhDelta(k, N, i, i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (lbvhDelta(k, N, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = lbvhDelta(k, N, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (lbvhDelta(k, N, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const long long g = i + s * d + min(d, 0);
    const int first = int(min((long long)i, j)), last = int(max((long long)i, j));
    if (first < 0 || last >= N || g < first || g >= last) {
        atomicOr(&ctl[4], 16);
        return;
    }
    const int left = first == g ? N - 1 + int(g) : int(g);
    const int right = last == g + 1 ? N - 1 + int(g) + 1 : int(g) + 1;
    if (i == 0) L.rec[0].x = -1;
    L.rec[i].y = first;
    L.rec[i].z = last;
    L.child[i] = make_int2(left, right);
    if (left >= N - 1) L.rec[left] = make_int4(i, int(g), int(g), 0);
    else L.rec[left].x = i;
    if (right >= N - 1) L.rec[right] = make_int4(i, int(g) + 1, int(g) + 1, 0);
    else L.rec[right].x = i;
}

// Ordering 0's box of node n (the hand-off's payload): written through (sc1).
RD_DEV void lbvhPublish(float *nodeBox, int n, const float (&lo)[3], const float (&hi)[3]) {
    int *d = reinterpret_cast<int *>(nodeBox + 8 * (size_t)n);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        __hip_atomic_store(d + c, __float_as_int(lo[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d + 4 + c, __float_as_int(hi[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Bottom-up: one lane per leaf (sorted position j).  The second lane to arrive at a node reads both children's boxes, sets the
// node's ordering bits (bit k: ordering k visits the right child first) and its box.  counters: N - 1 ints, memset to 0.
__global__ __launch_bounds__(256) void k_lbvh_up(LbvhWork L, int *ctl) {
    const int j = int(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = L.numPrims, S = 2 * N - 1;
    if (j >= N) return;
    int n = N - 1 + j;
    float lo[3], hi[3];
    {
        const int p = L.vals[0][j];
        if (p < 0 || p >= N) {
            atomicOr(&ctl[4], 32);
            return;
        }
        const float4 a = L.leafBox[2 * (size_t)p], b = L.leafBox[2 * (size_t)p + 1];
        lo[0] = a.x; lo[1] = a.y; lo[2] = a.z;
        hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
    }
    lbvhPublish(L.nodeBox, n, lo, hi);
    int parent = L.rec[n].x;
    for (int steps = 0; parent >= 0; steps++) {
        if (parent >= N - 1 || steps >= kLbvhMaxDepth) {
            atomicOr(&ctl[4], 32);
            return;
        }
        // publish (k_refit's form): the sc1 stores of the box drained, then the counter; the lane that draws 1 reads both
        // children's boxes with sc1 loads
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add(&L.counters[parent], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old != 1) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the counter
        n = parent;
        const int2 ch = L.child[n];
        if (ch.x < 0 || ch.x >= S || ch.y < 0 || ch.y >= S) {
            atomicOr(&ctl[4], 32);
            return;
        }
        const int *A = reinterpret_cast<const int *>(L.nodeBox + 8 * (size_t)ch.x);
        const int *B = reinterpret_cast<const int *>(L.nodeBox + 8 * (size_t)ch.y);
        float al[3], ah[3], bl[3], bh[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {  // the children's boxes: sc1 loads past this CU's L1
            al[c] = __int_as_float(__hip_atomic_load(A + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            bl[c] = __int_as_float(__hip_atomic_load(B + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            ah[c] = __int_as_float(__hip_atomic_load(A + 4 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            bh[c] = __int_as_float(__hip_atomic_load(B + 4 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        int bits = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int dim = k / 2;
            if ((bvhCenter(al[dim], ah[dim]) < bvhCenter(bl[dim], bh[dim])) != ((k & 1) != 0)) bits |= 1 << k;
        }
        const bool rightFirst = bits & 1;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = rightFirst ? combLo(bl[c], al[c]) : combLo(al[c], bl[c]);
            hi[c] = rightFirst ? combHi(bh[c], ah[c]) : combHi(ah[c], bh[c]);
        }
        L.rec[n].w = bits;  // read by k_lbvh_place, a later launch
        lbvhPublish(L.nodeBox, n, lo, hi);
        parent = L.rec[n].x;
    }
}

// One lane per node: climb to the root, summing the node's slot (2 * first + left turns), its position in each ordering, its
// pair number (inner nodes before it in ordering 0) and the far children pending in each ordering; then write the builder's
// outputs at those places and fold the most pending children into ctl[3] (treeDepth).
__global__ __launch_bounds__(256) void k_lbvh_place(LbvhWork L, BvhWork w) {
    const int n = int(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = L.numPrims, S = 2 * N - 1;
    int deepest = 0;
    if (n < S) {
        const int4 r = L.rec[n];
        const bool leaf = n >= N - 1;
        const int size = 2 * (r.z - r.y + 1) - 1;
        int pos[6] = {0, 0, 0, 0, 0, 0}, pend[6] = {0, 0, 0, 0, 0, 0};
        int turnsLeft = 0, q = 0, f = r.y, l = r.z, p = r.x;
        bool ok = true;
        for (int steps = 0; p >= 0; steps++) {
            if (p >= N - 1 || steps >= kLbvhMaxDepth) {
                ok = false;
                break;
            }
            const int4 R = L.rec[p];
            const bool isLeft = f == R.y;
            const int sib = (R.z - R.y + 1) - (l - f + 1);  // leaves of the sibling
            turnsLeft += isLeft;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const bool first = isLeft != (((R.w >> k) & 1) != 0);
                pos[k] += first ? 1 : 2 * sib;
                pend[k] += first;
            }
            q += (isLeft != ((R.w & 1) != 0)) ? 1 : sib;
            f = R.y;
            l = R.z;
            p = R.x;
        }
        const int slot = 2 * r.y + turnsLeft;
        if (!ok || slot < 0 || slot >= S) {
            atomicOr(&w.ctl[4], 64);
        } else {
            const int prim = leaf ? L.vals[0][n - (N - 1)] : -1;
            const float *b = L.nodeBox + 8 * (size_t)n;
            float *ob = w.boxes + 6 * (size_t)slot;
            ob[0] = b[0]; ob[1] = b[1]; ob[2] = b[2];
            ob[3] = b[4]; ob[4] = b[5]; ob[5] = b[6];
            w.info[slot] = leaf ? prim : -size;
            w.bits[slot] = leaf ? 0 : r.w;
            w.qnum[slot] = q;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                if (pos[k] < 0 || pos[k] + size > S) {
                    atomicOr(&w.ctl[4], 64);
                    continue;
                }
                int *o = w.nodes[k] + 3 * (size_t)pos[k];
                o[0] = prim;
                o[1] = slot;
                o[2] = pos[k] + size;
                deepest = max(deepest, pend[k]);
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) deepest = max(deepest, __shfl_xor(deepest, d, 64));
    if ((threadIdx.x & 63) == 0 && deepest > 0) atomicMax(&w.ctl[3], deepest);
}

}  // namespace rd
