// radish_pt_amd/csrc/device/kernels_geometry.h — the uploaded scene's triangle set replaced on the device (rdh_scene_set_geometry;
// DESIGN 11i).
//
// rdh_scene_upload checks and lays out the caller's arrays on the host.  Here the same two steps are two streaming launches over
// DEVICE arrays of any triangle count:
//
//   k_geom_check   before anything of the scene is touched: how many triangles carry each material (the host's matPrims, from which
//                  the light count follows without the device), a flag for a material id outside [0, numMaterials), and a flag
//                  for a coordinate that fails the upload's fabs(x) < 1e30f.  Reads 36 B of vertices and 4 B of id per triangle.
//                  Integer sums do not depend on the order of their terms, so the counts repeat exactly whatever the atomics' order.
//   k_geom_pack    one lane per triangle: TriRec (vertices + id), AttrRec (normals + texcoords) and primClass with the upload's
//                  packing (rdh_scene_upload), k_geom_update's read pattern.
//
// Everything behind them (builders, k_bvh_noderecs, k_bvh_pairs, the emitter passes, the alias kernels) runs unchanged.
#pragma once
#include "kernels_materials.h"

namespace rd {

constexpr int kGeomCheckBins = 1024;   // materials whose counts a workgroup keeps in LDS
constexpr int kGeomCheckThreads = 256;
constexpr float kTexcoordLimit = 2097152.f;  // 2^21; rdh_scene_upload applies the same test on the host

// out[0 .. numMaterials): triangles per material (added to: the caller clears them); out[numMaterials]: 1 when an id is out of range
// (such a triangle is counted nowhere); out[numMaterials + 1]: bit 0 when a vertex coordinate is not finite or not below 1e30 in
// magnitude, bit 1 when a texture coordinate is not finite or not below 2^21 (kTexcoordLimit: int(uv * 1024) in proceduralTexture
// must stay a defined conversion).
// Grid-stride over the triangles, so a workgroup's bins serve many of them.  LDS: up to kGeomCheckBins materials the counts are
// collected with integer LDS atomics and leave with one global atomic per non-empty bin and workgroup; beyond that every triangle
// adds to its global counter.  The flags are OR-ed, one atomic per wave that saw one.
template <bool LDS>
__global__ __launch_bounds__(kGeomCheckThreads) void k_geom_check(const float *__restrict__ verts, const float *__restrict__ texcoords,
                                                                 const int *__restrict__ materialIds, int numPrims, int numMaterials,
                                                                 int *__restrict__ out) {
    __shared__ int bins[LDS ? kGeomCheckBins : 1];
    if (LDS) {
        for (int m = (int)threadIdx.x; m < numMaterials; m += kGeomCheckThreads) bins[m] = 0;
        __syncthreads();
    }
    bool badId = false, badCoord = false, badTex = false;
    const long long stride = (long long)gridDim.x * kGeomCheckThreads;
    for (long long p = (long long)blockIdx.x * kGeomCheckThreads + threadIdx.x; p < numPrims; p += stride) {
        const int id = materialIds[p];
        if (id < 0 || id >= numMaterials) badId = true;
        else if (LDS) atomicAdd(&bins[id], 1);
        else atomicAdd(&out[id], 1);
        const float *v = verts + 9 * (size_t)p;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 9; k++) ok = ok && (__builtin_fabsf(v[k]) < 1e30f);  // false for NaN, as the upload's test
        badCoord = badCoord || !ok;
        const float *t = texcoords + 6 * (size_t)p;
        ok = true;
#pragma unroll
        for (int k = 0; k < 6; k++) ok = ok && (__builtin_fabsf(t[k]) < kTexcoordLimit);
        badTex = badTex || !ok;
    }
    const bool anyId = __ballot(badId) != 0ull, anyCoord = __ballot(badCoord) != 0ull;  // (every lane of the wave is here)
    const bool anyTex = __ballot(badTex) != 0ull;
    if ((threadIdx.x & 63) == 0) {
        if (anyId) atomicOr(&out[numMaterials], 1);
        if (anyCoord) atomicOr(&out[numMaterials + 1], 1);
        if (anyTex) atomicOr(&out[numMaterials + 1], 2);
    }
    if (LDS) {
        __syncthreads();
        for (int m = (int)threadIdx.x; m < numMaterials; m += kGeomCheckThreads) {
            const int n = bins[m];
            if (n) atomicAdd(&out[m], n);
        }
    }
}

// The records of triangle i as rdh_scene_upload lays them out.  Every id is in range (k_geom_check has passed).
__global__ __launch_bounds__(256) void k_geom_pack(const float *__restrict__ verts, const float *__restrict__ normals,
                                                   const float *__restrict__ texcoords, const int *__restrict__ materialIds,
                                                   const MatRec *__restrict__ mats, int N, TriRec *__restrict__ tris,
                                                   AttrRec *__restrict__ attrs, unsigned char *__restrict__ primClass) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N) return;
    const float *v = verts + 9 * (size_t)i, *n = normals + 9 * (size_t)i, *t = texcoords + 6 * (size_t)i;
    const int mid = materialIds[i];
    TriRec r;
    r.a = make_float4(v[0], v[1], v[2], v[3]);
    r.b = make_float4(v[4], v[5], v[6], v[7]);
    r.c = make_float4(v[8], __int_as_float(mid), 0.f, 0.f);
    tris[i] = r;
    AttrRec a;
    a.a = make_float4(n[0], n[1], n[2], n[3]);
    a.b = make_float4(n[4], n[5], n[6], n[7]);
    a.c = make_float4(n[8], t[0], t[1], t[2]);
    a.d = make_float4(t[3], t[4], t[5], 0.f);
    attrs[i] = a;
    primClass[i] = shadingClass(__float_as_int(mats[mid].a.x));
}

}  // namespace rd
