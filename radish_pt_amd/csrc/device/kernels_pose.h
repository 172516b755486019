// radish_pt_amd/csrc/device/kernels_pose.h — per-object rigid / affine transforms on the device (rdh_scene_set_objects,
// rdh_scene_pose_objects).
//
// The host loader (csrc/host/scene_load.cpp, loadModel) multiplies an Object block's X = T * R * S into its mesh's vertices and the
// transposed inverse into its normals.  k_pose_objects does the same from the rest pose the context keeps, operand for operand and
// in the loader's order, so that a scene posed here holds the floats a scene file with the same Translate / Rotate / Scale loads to.
// Its output is the flat world-space pair (vertices, normals) that the update and refit entries have always taken; k_geom_update
// turns it into records as for any other caller.
#pragma once
#include <hip/hip_runtime.h>

#include "layouts.h"

namespace rd {

constexpr int kPoseThreads = 256;  // one lane per vertex

struct PoseVec {  // 12 bytes at stride 12: one dwordx3 per lane, 768 contiguous bytes per wave
    float x, y, z;
};
static_assert(sizeof(PoseVec) == 12, "PoseVec layout");

struct PoseRange {  // == rdh_object_range
    int firstPrim, numPrims, restFirstPrim;
};

struct PoseArgs {
    const PoseRange *objects;  // the table of rdh_scene_set_objects
    const PoseVec *restVertices, *restNormals;
    PoseVec *worldVertices, *worldNormals;
    // staged by each rdh_scene_pose_objects, one allocation: prefix[count + 1] (workgroups of the listed objects before entry j),
    // ids[count], xforms[count][32] (X column-major, then inverse(X))
    const int *prefix;
    const int *ids;
    const float *xforms;
    int count;
};

// Workgroups one object of numPrims triangles takes.
__host__ __device__ inline int poseGroups(int numPrims) { return (3 * numPrims + kPoseThreads - 1) / kPoseThreads; }

// The world arrays as the scene's records hold them: TriRec / AttrRec keep the uploaded floats verbatim (k_geom_update), so the
// seed needs no host array.  One lane per triangle.
__global__ __launch_bounds__(256) void k_pose_seed(const TriRec *__restrict__ tris, const AttrRec *__restrict__ attrs, int N,
                                                   float *__restrict__ worldVertices, float *__restrict__ worldNormals) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N) return;
    const float4 a = tris[i].a, b = tris[i].b;
    const float c = tris[i].c.x;
    float *v = worldVertices + 9 * (size_t)i;
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w, v[8] = c;
    const float4 na = attrs[i].a, nb = attrs[i].b;
    const float nc = attrs[i].c.x;
    float *n = worldNormals + 9 * (size_t)i;
    n[0] = na.x, n[1] = na.y, n[2] = na.z, n[3] = na.w, n[4] = nb.x, n[5] = nb.y, n[6] = nb.z, n[7] = nb.w, n[8] = nc;
}

// Every workgroup serves exactly one listed object and finds it from blockIdx.x alone: the entry j with prefix[j] <= blockIdx.x <
// prefix[j + 1].  Everything up to the lane's own vertex index is therefore uniform over the wave, and the search, the object's
// range and the 21 matrix floats used (X: 12, inverse: 9) are scalar loads into SGPRs; the only per-lane memory traffic is one
// 12-byte load and one 12-byte store per array.  Objects without triangles take no workgroup (equal prefix entries): the search
// keeps the LAST entry that starts at or before the workgroup.  No LDS, no atomics, nothing handed between workgroups.
__global__ __launch_bounds__(kPoseThreads) void k_pose_objects(const PoseArgs a) {
    const int wg = (int)blockIdx.x;
    int lo = 0, hi = a.count;  // prefix[lo] <= wg < prefix[hi]; prefix[0] == 0 and prefix[count] == gridDim.x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.prefix[mid] <= wg) lo = mid;
        else hi = mid;
    }
    const PoseRange o = a.objects[a.ids[lo]];
    const int v = (wg - a.prefix[lo]) * kPoseThreads + (int)threadIdx.x;
    if (v >= 3 * o.numPrims) return;
    const float *X = a.xforms + 32 * (size_t)lo, *Xi = X + 16;  // [col][row] at 4 * col + row
    const size_t src = 3 * (size_t)o.restFirstPrim + (size_t)v, dst = 3 * (size_t)o.firstPrim + (size_t)v;
    const PoseVec p = a.restVertices[src], n = a.restNormals[src];
    // loadModel: w[r] = X.m[0][r] * p.x + X.m[1][r] * p.y + X.m[2][r] * p.z + X.m[3][r] * 1.0f
    //            nn[r] = Xi.m[r][0] * n.x + Xi.m[r][1] * n.y + Xi.m[r][2] * n.z
    float w[3], nn[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        w[r] = X[r] * p.x + X[4 + r] * p.y + X[8 + r] * p.z + X[12 + r] * 1.0f;
        nn[r] = Xi[4 * r] * n.x + Xi[4 * r + 1] * n.y + Xi[4 * r + 2] * n.z;
    }
    const float inv = 1.f / sqrtf((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
    a.worldVertices[dst] = PoseVec{w[0], w[1], w[2]};
    a.worldNormals[dst] = PoseVec{nn[0] * inv, nn[1] * inv, nn[2] * inv};
}

}  // namespace rd
