// radish_pt_amd/csrc/device/kernels_materials.h — materials edited on the device and the light list that follows from them
// (rdh_scene_set_materials, rdh_build_light_list_device).
//
// rdh_build_light_list (host/scene_build.cpp) walks the triangles in order and appends every one whose material is a Light: the
// list is an ORDERED compaction of the triangle array.  Here it is three launches, ordered by the stream and by nothing else:
//
//   k_emit_count_*    one lane per triangle: the emissive flag, counted per wave (ballot) and per 256-triangle block (LDS)
//   k_emit_scan       one workgroup: the exclusive prefix of the block totals (scanBlockTotals, any number of blocks) and the total
//   k_emit_scatter_*  flag again, rank in the block = waves before (LDS) + lanes before (ballot, mbcnt); slot = block offset + rank
//
// No workgroup waits for another inside a kernel and no atomic decides a slot, so the list repeats exactly and is the host's.
// The passes are written once over a loader that says whether triangle p emits and what its slot receives:
//   SceneEmitters  the uploaded scene's records (TriRec.c.y = material id, MatRec.a = {type, colour}) -> dLightPrims and LightRec,
//                  the upload's packing; the first pass also rewrites primClass, the key of the wavefront material sort
//   RefEmitters    the reference layouts (vertices, materialIds, 44-byte materials) -> lightPrimIds, lightUnitRadiance, lightPower
// k_mat_write puts the listed MatRecs in place before any of this.
#pragma once
#include "kernels_lights.h"
#include "kernels_refit.h"

namespace rd {

constexpr int kMaterialLight = 4;  // Material::Type::Light (src/material.h:129)

// The shading class rdh_scene_upload derives from a Material::Type: Lambertian, MetallicWorkflow, Dielectric; anything else ends a path.
RD_DEV unsigned char shadingClass(int type) { return type == 0 ? 1 : (type == 1 ? 2 : (type == 2 ? 3 : 0)); }

struct SceneEmitters {
    const TriRec *tris;
    const MatRec *mats;
    unsigned char *primClass;
    int *lightPrims;
    LightRec *lights;
    int capacity;  // emitters the two arrays hold: the host's count, which the device's equals (a slot beyond it is not written)

    template <bool FIRST>
    RD_DEV bool emits(int p) const {
        const int type = __builtin_bit_cast(int, mats[__builtin_bit_cast(int, tris[p].c.y)].a.x);
        if (FIRST) primClass[p] = shadingClass(type);
        return type == kMaterialLight;
    }
    RD_DEV void put(int slot, int p) const {
        if (slot >= capacity) return;
        const float4 A = tris[p].a, B = tris[p].b, C = tris[p].c;
        const float4 m = mats[__builtin_bit_cast(int, C.y)].a;
        lightPrims[slot] = p;
        lights[slot].a = A;
        lights[slot].b = B;
        lights[slot].c = make_float4(C.x, m.y, m.z, m.w);
    }
};

struct RefMaterial {  // Material (src/material.h:276-286), as rdh_scene_desc::materials holds it
    int type;
    float r, g, b;
    float metallic, roughness, ior;
    int map[4];
};
static_assert(sizeof(RefMaterial) == 44, "Material layout");

struct RefEmitters {
    const float *vertices;
    const int *materialIds;
    const RefMaterial *materials;
    int numMaterials;
    int *lightPrimIds;
    float *lightUnitRadiance;
    float *lightPower;
    int *err;  // set (never cleared here) when a material id is out of range; such a triangle does not emit

    template <bool FIRST>
    RD_DEV bool emits(int p) const {
        const int id = materialIds[p];
        if (id < 0 || id >= numMaterials) {
            if (FIRST) *err = 1;  // every lane that gets here stores the same value
            return false;
        }
        return materials[id].type == kMaterialLight;
    }
    RD_DEV void put(int slot, int p) const {
        const RefMaterial m = materials[materialIds[p]];
        const float *v = vertices + 9 * (size_t)p;
        lightPrimIds[slot] = p;
        lightUnitRadiance[3 * (size_t)slot + 0] = m.r;
        lightUnitRadiance[3 * (size_t)slot + 1] = m.g;
        lightUnitRadiance[3 * (size_t)slot + 2] = m.b;
        lightPower[slot] = emitterPower(mk3(v[0], v[1], v[2]), mk3(v[3], v[4], v[5]), mk3(v[6], v[7], v[8]), m.r, m.g, m.b);
    }
};

template <typename L>
RD_DEV void emitCount(const L &ld, int n, int *blockTotals) {
    __shared__ int wsum[4];
    const int p = int(blockIdx.x * blockDim.x + threadIdx.x);
    const bool e = p < n && ld.template emits<true>(p);
    const int c = __popcll(__ballot(e));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blockTotals[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

template <typename L>
RD_DEV void emitScatter(const L &ld, int n, const int *blockOff) {
    __shared__ int wsum[4];
    const int p = int(blockIdx.x * blockDim.x + threadIdx.x);
    const int wave = int(threadIdx.x >> 6);
    const bool e = p < n && ld.template emits<false>(p);
    const unsigned long long m = __ballot(e);
    if ((threadIdx.x & 63) == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    if (!e) return;
    int slot = blockOff[blockIdx.x] + laneBelow(m);
    for (int w = 0; w < wave; w++) slot += wsum[w];
    ld.put(slot, p);
}

__global__ __launch_bounds__(256) void k_emit_count_scene(SceneEmitters ld, int n, int *blockTotals) { emitCount(ld, n, blockTotals); }
__global__ __launch_bounds__(256) void k_emit_count_ref(RefEmitters ld, int n, int *blockTotals) { emitCount(ld, n, blockTotals); }
__global__ __launch_bounds__(256) void k_emit_scatter_scene(SceneEmitters ld, int n, const int *blockOff) { emitScatter(ld, n, blockOff); }
__global__ __launch_bounds__(256) void k_emit_scatter_ref(RefEmitters ld, int n, const int *blockOff) { emitScatter(ld, n, blockOff); }

// Block totals -> exclusive offsets in place; *count = the number of emitters, or -1 when *err is set (err may be null).
__global__ __launch_bounds__(256) void k_emit_scan(int *blockTotals, int nBlocks, const int *err, int *count) {
    const int total = scanBlockTotals(blockTotals, nBlocks);
    if (threadIdx.x == 0) *count = err && *err ? -1 : total;
}

// mats[ids[j]] = recs[j]: the ids are distinct (checked on the host), so no two lanes write one record.
__global__ __launch_bounds__(256) void k_mat_write(const MatRec *__restrict__ recs, const int *__restrict__ ids, int count,
                                                   MatRec *__restrict__ mats) {
    const int j = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < count) mats[ids[j]] = recs[j];
}

}  // namespace rd
