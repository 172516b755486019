// radish_pt_amd/csrc/device/kernels_refit.h — refit of the uploaded tree in place (rdh_scene_refit_geometry): new boxes for the
// same topology, bottom-up in one launch, and the SAH cost figure of rdh_scene_tree_cost.
//
// Node numbering: a node is named by its position i in ordering 0.  An inner node's children are a = i + 1 (ordering
// 0's first child, the pair's child 0) and b = nextNodeIfMiss(a) (child 1).  The box contract:
//  - leaf holding primitive p: bvhLo / bvhHi folded over v[3p], v[3p+1], v[3p+2] in that order from the empty box;
//  - inner node: combLo / combHi (kernels_bvh.h) of box a and box b, a always the earlier operand.
// The orderings are NOT re-sorted by the new box centres: a refit tree is walked in the orderings of its last build.
//
// The refit plan, derived on the device from the uploaded NodeRec arrays once per topology (after an upload or
// rdh_scene_update_geometry, by the first refit), is one RefitPlanRec per node.  Deriving it also checks that the six arrays are
// six pre-orders of one binary tree whose leaves hold distinct primitives (error bits in err[0]; the host refuses the refit).
//  1. k_refit_links: ordering 0's structure (parent, child b), leaf positions of every primitive in every ordering.
//  2. k_refit_count / k_refit_scan / k_refit_number: pair numbers (inner nodes before i in ordering 0) by a three-kernel scan; each
//     inner node hands (pair << 1) | side to its children.
//  3. k_refit_plan_climb: positions in orderings 1..5.  In a pre-order the last record of a subtree is a leaf, so a node's
//     position in ordering k is (the largest position of its leaves in ordering k) - size + 1, size = next0(i) - i being the
//     same in every ordering of one tree; the largest positions climb bottom-up like the boxes do.
//  4. k_refit_check: every record of orderings 1..5 at those positions is that node (leaf: same primitive, next = pos + 1;
//     inner: next = pos + size, children right behind it in one of the two orders), and the pair records' w fields are the
//     numbering's.  With the root at position 0 this makes each ordering a bijection onto the same tree.
//
// Climbs (memory ordering).  One lane starts at every leaf; a node's arrival counter (memset to zero on the stream in the same
// call) lets the SECOND arriving child's lane go on to the parent, which reads both children's results and writes its own.
// Those results were written by lanes that may sit on another CU or XCD (L1s are per CU, L2s per XCD).  The counter is one word
// with one coherence order, so the second arrival's add comes after the first one's; what must hold is that the first lane's
// result is visible to the second lane once its add is.
//  - k_refit: ordering 0's box of the node (the only bytes another lane of the launch reads) is stored write-through (sc1,
//    relaxed agent-scope atomic stores) and drained (s_waitcnt vmcnt(0)) before the relaxed agent-scope counter add; the lane
//    that draws 1 reads the children's boxes with sc1 loads (relaxed agent-scope atomic loads), past its CU's L1.  No fence:
//    an agent-scope release (buffer_wbl2) would write back every dirty line of the XCD's L2, the other orderings' scattered
//    box stores included, at every step of every wave: 12.3 ms against 0.78 ms for this form at 1 M triangles.
//  - k_refit_plan_climb (once per topology): plain stores, an agent-scope release fence drained before the add, and an
//    agent-scope acquire fence before the loads.
// No lane ever waits, so a chain of any depth finishes in the one launch.
#pragma once
#include "kernels_bvh.h"

namespace rd {

struct __attribute__((aligned(16))) RefitPlanRec {
    int parent;   // ordering-0 position of the parent, -1 at the root
    int pairRef;  // (pair number of the parent << 1) | side (0: the parent's child a, 1: child b); -1 at the root
    int pos[5];   // positions in orderings 1..5
    int w;        // leaf: primitive id; inner: ~b (ordering-0 position of child b)
};
static_assert(sizeof(RefitPlanRec) == 32, "RefitPlanRec");

// Error bits of the plan derivation (err[0]).
constexpr int kRefitErrStructure = 1;   // ordering 0 is not a pre-order of a full binary tree
constexpr int kRefitErrPrims = 2;       // a primitive sits in two leaves of one ordering, or in none of ordering k
constexpr int kRefitErrOrdering = 4;    // ordering k is not the same tree
constexpr int kRefitErrPairs = 8;       // the pair records are not this tree's

RD_DEV int refitPrim(const NodeRec *n, int i) { return __float_as_int(n[i].lo_prim.w); }
RD_DEV int refitNext(const NodeRec *n, int i) { return __float_as_int(n[i].hi_next.w); }

RD_DEV void releaseAgent() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
RD_DEV void acquireAgent() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// 1. ordering 0's structure; leaf positions of every primitive in each ordering (primPos[k][prim], memset to -1).
//    plan is memset to -1 bytes first, parentCount to 0.  One thread per (ordering k, position j).
__global__ __launch_bounds__(256) void k_refit_links(const NodeRec *__restrict__ nodes, int S, int N, RefitPlanRec *plan,
                                                     int *parentCount, int *primPos, int *err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 6ll * S) return;
    const int k = int(t / S), j = int(t % S);
    const NodeRec *nk = nodes + (size_t)k * (S + 1);
    const int prim = refitPrim(nk, j), next = refitNext(nk, j);
    if (prim >= 0) {
        if (prim >= N || next != j + 1) { atomicOr(err, k ? kRefitErrOrdering : kRefitErrStructure); return; }
        if (atomicCAS(&primPos[(size_t)k * N + prim], -1, j) != -1) atomicOr(err, kRefitErrPrims);
        if (k == 0) plan[j].w = prim;
        return;
    }
    if (k != 0) return;
    if (j == 0 && next != S) { atomicOr(err, kRefitErrStructure); return; }
    const int a = j + 1;
    if (a >= S) { atomicOr(err, kRefitErrStructure); return; }
    const int b = refitNext(nk, a);
    if (b <= a || b >= S || refitNext(nk, b) != next) { atomicOr(err, kRefitErrStructure); return; }
    plan[j].w = ~b;
    plan[a].parent = j;
    plan[b].parent = j;
    atomicAdd(&parentCount[a], 1);
    atomicAdd(&parentCount[b], 1);
}

// 2. pair numbers: inner nodes before i in ordering 0.  k_refit_count: per 256-node block; k_refit_scan (one workgroup): the
//    blocks' exclusive prefix; k_refit_number: within the block, and the hand-down of (pair << 1) | side to the children.
__global__ __launch_bounds__(256) void k_refit_count(const NodeRec *__restrict__ nodes0, int S, int *blockSums) {
    __shared__ int wsum[4];
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    const bool inner = i < S && refitPrim(nodes0, i) < 0;
    const int c = __popcll(__ballot(inner));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blockSums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// The exclusive prefix of n block totals, in place, by one 256-lane workgroup that walks them a tile at a time (any n); every lane
// returns the grand total.  Shared with the emitter compaction (kernels_materials.h).
RD_DEV int scanBlockTotals(int *blockSums, int nBlocks) {
    __shared__ int s[256];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nBlocks; base += 256) {
        const int i = base + int(threadIdx.x);
        const int v = i < nBlocks ? blockSums[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {  // inclusive Hillis-Steele scan
            const int x = threadIdx.x >= (unsigned)d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += x;
            __syncthreads();
        }
        if (i < nBlocks) blockSums[i] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += s[255];
        __syncthreads();
    }
    return carry;
}

__global__ __launch_bounds__(256) void k_refit_scan(int *blockSums, int nBlocks) { scanBlockTotals(blockSums, nBlocks); }

__global__ __launch_bounds__(256) void k_refit_number(const NodeRec *__restrict__ nodes0, int S, const int *__restrict__ blockOff,
                                                      RefitPlanRec *plan) {
    __shared__ int wsum[4];
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    const int lane = int(threadIdx.x & 63), wave = int(threadIdx.x >> 6);
    const bool inner = i < S && refitPrim(nodes0, i) < 0;
    const unsigned long long m = __ballot(inner);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    if (!inner) return;
    int q = blockOff[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) q += wsum[w];
    const int bw = plan[i].w;  // ~b (k_refit_links); >= 0 when ordering 0 is malformed
    plan[i + 1 < S ? i + 1 : i].pairRef = q << 1;
    if (bw < 0 && ~bw < S) plan[~bw].pairRef = (q << 1) | 1;
}

// The climb skeleton: returns false when this lane stops (first arrival), true when it goes on with `parent` (and has acquired).
RD_DEV bool refitArrive(int *counters, int pairRef) {
    releaseAgent();
    const int old = __hip_atomic_fetch_add(&counters[pairRef >> 1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old != 1) return false;  // 0: the sibling is still on its way; > 1 only on a malformed plan (flagged elsewhere)
    acquireAgent();
    return true;
}

// 3. positions in orderings 1..5 (counters memset to 0, S entries).
__global__ __launch_bounds__(256) void k_refit_plan_climb(const NodeRec *__restrict__ nodes0, int S, int N, RefitPlanRec *plan,
                                                          const int *__restrict__ primPos, int *counters, int *err) {
    int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= S) return;
    const int prim = plan[i].w;
    if (prim < 0 || prim >= N) return;  // inner nodes are reached by a climb (a malformed w is flagged by the check)
    for (int k = 1; k < 6; k++) {
        const int p = primPos[(size_t)k * N + prim];
        if (p < 0) atomicOr(err, kRefitErrPrims);
        plan[i].pos[k - 1] = p;
    }
    for (int steps = 0; steps < S; steps++) {  // the bound only guards a malformed plan
        const int par = plan[i].parent, ref = plan[i].pairRef;
        if (par < 0 || ref < 0 || (ref >> 1) >= S) return;
        if (!refitArrive(counters, ref)) return;
        const int a = par + 1, bw = plan[par].w;
        if (bw >= 0 || ~bw >= S) return;
        const int b = ~bw;
        const int sa = refitNext(nodes0, a) - a, sb = refitNext(nodes0, b) - b, sp = refitNext(nodes0, par) - par;
        for (int k = 0; k < 5; k++) {
            const int la = __hip_atomic_load(&plan[a].pos[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + sa - 1;
            const int lb = __hip_atomic_load(&plan[b].pos[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + sb - 1;
            plan[par].pos[k] = max(la, lb) - sp + 1;
        }
        i = par;
    }
}

// 4. the other orderings and the pair records against the plan.  One thread per node.
__global__ __launch_bounds__(256) void k_refit_check(const NodeRec *__restrict__ nodes, int S, const RefitPlanRec *__restrict__ plan,
                                                     const int *__restrict__ parentCount, const PairRec *__restrict__ pairs, int *err) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= S) return;
    const RefitPlanRec r = plan[i];
    if (i > 0 && (parentCount[i] != 1 || r.pairRef < 0)) { atomicOr(err, kRefitErrStructure); return; }
    const NodeRec *n0 = nodes;
    const int size = refitNext(n0, i) - i;
    const bool leaf = r.w >= 0;
    const int a = i + 1, b = ~r.w;
    if (!leaf && (b <= a || b >= S)) { atomicOr(err, kRefitErrStructure); return; }
    for (int k = 1; k < 6; k++) {
        const NodeRec *nk = nodes + (size_t)k * (S + 1);
        const int P = r.pos[k - 1];
        if (P < 0 || P + size > S || (i == 0 && P != 0)) { atomicOr(err, kRefitErrOrdering); return; }
        const int prim = refitPrim(nk, P), next = refitNext(nk, P);
        if (leaf) {
            if (prim != r.w || next != P + 1) atomicOr(err, kRefitErrOrdering);
            continue;
        }
        const int pa = plan[a].pos[k - 1], pb = plan[b].pos[k - 1];
        const int za = refitNext(n0, a) - a, zb = refitNext(n0, b) - b;
        const bool aFirst = pa == P + 1 && pb == P + 1 + za, bFirst = pb == P + 1 && pa == P + 1 + zb;
        if (prim != -1 || next != P + size || !(aFirst || bFirst)) atomicOr(err, kRefitErrOrdering);
    }
    if (pairs && !leaf) {
        const int q = plan[a].pairRef >> 1;
        auto childW = [&](int c) { const int w = plan[c].w; return w >= 0 ? w : ~(plan[c + 1].pairRef >> 1); };
        if (__float_as_int(pairs[q].lo0_w0.w) != childW(a) || __float_as_int(pairs[q].lo1_w1.w) != childW(b)) atomicOr(err, kRefitErrPairs);
    }
}

// The refit.  One thread per ordering-0 position; leaves start, inner nodes are reached by climbs.  Writes the box fields of the
// node's record in each of the six orderings, its half of its parent's pair record (when the scene has pairs) and, at the root,
// rootBox = {lo.xyz, -, hi.xyz, -}.  counters: max(N - 1, 1) ints, memset to 0 on the stream before the launch.
RD_DEV void refitWrite(NodeRec *nodes, int S, PairRec *pairs, float4 *rootBox, int i, const RefitPlanRec &r, const float (&lo)[3],
                       const float (&hi)[3]) {
    auto put = [&](float *d) {  // the box fields of one NodeRec (lo_prim.xyz, hi_next.xyz), not its .w fields
        d[0] = lo[0]; d[1] = lo[1]; d[2] = lo[2];
        d[4] = hi[0]; d[5] = hi[1]; d[6] = hi[2];
    };
    {  // ordering 0's record is what the parent's lane reads: written through (sc1), the hand-off's payload
        int *d = reinterpret_cast<int *>(nodes + i);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            __hip_atomic_store(d + c, __float_as_int(lo[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d + 4 + c, __float_as_int(hi[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#pragma unroll
    for (int k = 1; k < 6; k++) put(reinterpret_cast<float *>(nodes + (size_t)k * (S + 1) + r.pos[k - 1]));
    if (r.pairRef >= 0) {
        if (pairs) {
            float *d = reinterpret_cast<float *>(pairs + (r.pairRef >> 1)) + 8 * (r.pairRef & 1);
            put(d);
        }
    } else {
        rootBox[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
        rootBox[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

__global__ __launch_bounds__(256) void k_refit(const float *__restrict__ verts, const RefitPlanRec *__restrict__ plan, NodeRec *nodes,
                                               PairRec *pairs, int *counters, float4 *rootBox, int S) {
    int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= S) return;
    RefitPlanRec r = plan[i];
    if (r.w < 0) return;
    float lo[3], hi[3];
    {
        const float *v = verts + 9 * (size_t)r.w;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = combLo(combLo(bvhLo(v[c]), v[3 + c]), v[6 + c]);
            hi[c] = combHi(combHi(bvhHi(v[c]), v[3 + c]), v[6 + c]);
        }
    }
    refitWrite(nodes, S, pairs, rootBox, i, r, lo, hi);
    while (r.parent >= 0) {
        // publish (R1 form): the sc1 stores of ordering 0's box drained, then the counter; the lane that draws 1 reads both
        // children's boxes with sc1 loads, so neither a release nor an acquire fence is needed.  The other orderings' and the
        // pair records' stores are read by no lane of this launch.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add(&counters[r.pairRef >> 1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old != 1) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the counter
        i = r.parent;
        r = plan[i];
        int *A = reinterpret_cast<int *>(nodes + i + 1), *B = reinterpret_cast<int *>(nodes + ~r.w);
#pragma unroll
        for (int c = 0; c < 3; c++) {  // the children's boxes: sc1 loads past this CU's L1
            const float al = __int_as_float(__hip_atomic_load(A + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const float bl = __int_as_float(__hip_atomic_load(B + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const float ah = __int_as_float(__hip_atomic_load(A + 4 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const float bh = __int_as_float(__hip_atomic_load(B + 4 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            lo[c] = combLo(al, bl);
            hi[c] = combHi(ah, bh);
        }
        refitWrite(nodes, S, pairs, rootBox, i, r, lo, hi);
    }
}

// SAH cost of the tree in ordering 0: sum over every node of surfaceArea(box) / surfaceArea(root box), in double, by a reduction
// of fixed shape (grid = kCostBlocks, strided loop, fixed LDS tree; then one workgroup over the partial sums in index order).
constexpr int kCostBlocks = 256;

RD_DEV double refitArea(float4 l, float4 h) {
    const double sx = (double)h.x - (double)l.x, sy = (double)h.y - (double)l.y, sz = (double)h.z - (double)l.z;
    return 2.0 * (sx * sy + sy * sz + sz * sx);
}

__global__ __launch_bounds__(256) void k_tree_cost_partial(const NodeRec *__restrict__ nodes0, int S, double *partial) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int i = int(blockIdx.x * blockDim.x + threadIdx.x); i < S; i += kCostBlocks * 256) acc += refitArea(nodes0[i].lo_prim, nodes0[i].hi_next);
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < (unsigned)d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

// A root box of zero surface area (every triangle on one line or at one point) leaves every term 0 / 0: each node then counts 1,
// as the root always does, and the cost is the node count S.
__global__ __launch_bounds__(256) void k_tree_cost_final(const NodeRec *__restrict__ nodes0, const double *__restrict__ partial, int S,
                                                         double *out) {
    __shared__ double s[256];
    s[threadIdx.x] = partial[threadIdx.x];  // kCostBlocks == 256
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < (unsigned)d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double root = refitArea(nodes0[0].lo_prim, nodes0[0].hi_next);
        out[0] = root > 0.0 ? s[0] / root : (double)S;
    }
}
static_assert(kCostBlocks == 256, "k_tree_cost_final reduces one partial per thread");

}  // namespace rd
