// radish_pt_amd/csrc/device/ray_cull.h — which of the wavefront path's rays need no walk (k_wf_shade; DESIGN 5b, "Rays whose
// outcome cannot reach the image").
//
// The extension ray of the last bounce (trace(maxDepth)) can add something to its path in two ways only (path_step.h): it hits a
// triangle whose material is Light, or it misses and the scene has an environment map.  Without an environment map a ray that
// cannot reach ANY emissive triangle therefore changes no pixel, and one box over those triangles answers that for most rays:
// k_emitter_bounds makes the box, mayReachEmitters tests a ray against it.  The test only ever errs towards "may reach".
#pragma once
#include "traverse.h"

namespace rd {

// The box as it lies in device memory (SceneState::emitBox): {lo.xyz, lo.w = 1 if the scene has an emissive triangle, else 0},
// {hi.xyz, 0}, both ALREADY padded (k_emitter_bounds).
constexpr float kEmitPad = 0.0009765625f;  // 2^-10 of the largest extent of the scene's root box (or of the emitters', if larger)

// false: no walk of this ray can report a hit on an emissive triangle.  A walk tests a triangle only after the box of its leaf — the
// exact bounds of its three vertices, inside the emitters' box — has passed AABB::intersect, so the question is which rays that
// box test can let through; intersectTriangle alone says little for a ray that grazes the triangle's plane (at 1e-5 rad its
// barycentrics are off by 1e-2 of an edge).  For a ray of class 0 (makeRaySlab) AABB::intersect is the slab test below up to the
// rounding of its products, which the padding exceeds by three orders of magnitude.  The other classes are kept untested: a
// direction with a component below 1.1e-6 of its length (the literal-looking hint of k_wf_shade; AABB::intersect drops that axis
// below 1e-6), and one within 1.5e-6 of an axis (above 1 - 1e-6 AABB::intersect treats the ray as parallel to the axis, whatever
// its slope).  Kept as well: an origin inside the padded box, and any NaN (every comparison below is written so that a NaN keeps
// the ray).  The far distance gets a relative margin of 2^-19 on top of the padding, which covers the rounding of the six products
// for origins far outside the scene as well.
RD_DEV bool mayReachEmitters(float4 lo, float4 hi, v3 o, v3 d) {
    if (lo.w == 0.f) return false;  // no emissive triangle at all
    const float len2 = dot(d, d), l2 = len2 * 1.21e-12f;
    if (!(d.x * d.x >= l2 && d.y * d.y >= l2 && d.z * d.z >= l2)) return true;
    if (!(__builtin_fmaxf(__builtin_fmaxf(d.x * d.x, d.y * d.y), d.z * d.z) <= len2 * 0.999997f)) return true;
    if (o.x >= lo.x && o.x <= hi.x && o.y >= lo.y && o.y <= hi.y && o.z >= lo.z && o.z <= hi.z) return true;
    const float ix = 1.f / d.x, iy = 1.f / d.y, iz = 1.f / d.z;
    const float ax = (lo.x - o.x) * ix, bx = (hi.x - o.x) * ix;
    const float ay = (lo.y - o.y) * iy, by = (hi.y - o.y) * iy;
    const float az = (lo.z - o.z) * iz, bz = (hi.z - o.z) * iz;
    const float tNear = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax, bx), __builtin_fminf(ay, by)), __builtin_fminf(az, bz));
    const float tFar = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax, bx), __builtin_fmaxf(ay, by)), __builtin_fmaxf(az, bz));
    const bool miss = tFar < 0.f || tNear > tFar * 1.0000019073486328125f;  // 1 + 2^-19
    return !miss;
}

// One workgroup: the box over the current vertices of the light list's triangles (every triangle whose material is Light:
// rdh_build_light_list), padded.  `root`: the first record of a threaded array = the scene's root box (null: no tree).
__global__ __launch_bounds__(256) void k_emitter_bounds(const TriRec *__restrict__ tris, const int *__restrict__ lightPrims, int numLights,
                                                        const NodeRec *__restrict__ root, float4 *__restrict__ box) {
    const float inf = __builtin_inff();
    v3 lo = mk3(inf), hi = mk3(-inf);
    for (int i = int(threadIdx.x); i < numLights; i += 256) {
        const TriVerts t = loadTri(tris, lightPrims[i]);
        lo.x = __builtin_fminf(lo.x, __builtin_fminf(t.a.x, __builtin_fminf(t.b.x, t.c.x)));
        lo.y = __builtin_fminf(lo.y, __builtin_fminf(t.a.y, __builtin_fminf(t.b.y, t.c.y)));
        lo.z = __builtin_fminf(lo.z, __builtin_fminf(t.a.z, __builtin_fminf(t.b.z, t.c.z)));
        hi.x = __builtin_fmaxf(hi.x, __builtin_fmaxf(t.a.x, __builtin_fmaxf(t.b.x, t.c.x)));
        hi.y = __builtin_fmaxf(hi.y, __builtin_fmaxf(t.a.y, __builtin_fmaxf(t.b.y, t.c.y)));
        hi.z = __builtin_fmaxf(hi.z, __builtin_fmaxf(t.a.z, __builtin_fmaxf(t.b.z, t.c.z)));
    }
    for (int m = 32; m >= 1; m >>= 1) {
        lo.x = __builtin_fminf(lo.x, __shfl_xor(lo.x, m, 64));
        lo.y = __builtin_fminf(lo.y, __shfl_xor(lo.y, m, 64));
        lo.z = __builtin_fminf(lo.z, __shfl_xor(lo.z, m, 64));
        hi.x = __builtin_fmaxf(hi.x, __shfl_xor(hi.x, m, 64));
        hi.y = __builtin_fmaxf(hi.y, __shfl_xor(hi.y, m, 64));
        hi.z = __builtin_fmaxf(hi.z, __shfl_xor(hi.z, m, 64));
    }
    __shared__ float sLo[4][3], sHi[4][3];
    if ((threadIdx.x & 63u) == 0u) {
        const int wv = int(threadIdx.x >> 6);
        sLo[wv][0] = lo.x, sLo[wv][1] = lo.y, sLo[wv][2] = lo.z;
        sHi[wv][0] = hi.x, sHi[wv][1] = hi.y, sHi[wv][2] = hi.z;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int wv = 1; wv < 4; wv++) {
        lo.x = __builtin_fminf(lo.x, sLo[wv][0]), lo.y = __builtin_fminf(lo.y, sLo[wv][1]), lo.z = __builtin_fminf(lo.z, sLo[wv][2]);
        hi.x = __builtin_fmaxf(hi.x, sHi[wv][0]), hi.y = __builtin_fmaxf(hi.y, sHi[wv][1]), hi.z = __builtin_fmaxf(hi.z, sHi[wv][2]);
    }
    if (numLights <= 0) {  // empty: every ray misses it (mayReachEmitters)
        box[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        box[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    float ext = __builtin_fmaxf(__builtin_fmaxf(hi.x - lo.x, hi.y - lo.y), hi.z - lo.z);
    if (root) {
        const float4 rl = root->lo_prim, rh = root->hi_next;
        ext = __builtin_fmaxf(ext, __builtin_fmaxf(__builtin_fmaxf(rh.x - rl.x, rh.y - rl.y), rh.z - rl.z));
    }
    const float pad = ext * kEmitPad;
    box[0] = make_float4(lo.x - pad, lo.y - pad, lo.z - pad, 1.f);
    box[1] = make_float4(hi.x + pad, hi.y + pad, hi.z + pad, 0.f);
}

}  // namespace rd
