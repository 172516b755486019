/* include/radish_hip.h — C ABI of libradish_hip.so, the MI355X (gfx950) implementation of Radish's per-pixel
 * path-tracing inner loop.
 *
 * The reference has no FFI layer: its render API is a set of C++ free functions that read process globals
 * (SURVEY.md §8b).  Each entry point below names the reference function whose body it replaces; the
 * source-compatible C++ shim with the reference's exact signatures is radish_pt_amd/csrc/radish_shim.hpp, and
 * INTEGRATION.md shows the binding a Radish maintainer would add.
 *
 * Conventions: every function returns 0 on success or a negative RDH_ERR_* / positive hipError_t code, and
 * rdh_last_error() gives the message (the reference prints and exit()s: src/cudaUtil.h:16-34 — the shim
 * reproduces that).  All `d_*` pointers are DEVICE pointers owned by the caller; scene arrays passed to
 * rdh_scene_upload are HOST pointers in the reference's DevScene layout.  A context is bound to one device and
 * one stream and is not thread-safe; calls are asynchronous on that stream unless stated otherwise.
 */
#ifndef RADISH_HIP_H
#define RADISH_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDH_OK 0
#define RDH_ERR_ARGS (-1)        /* null / inconsistent arguments                         */
#define RDH_ERR_NO_SCENE (-2)    /* call needs rdh_scene_upload + rdh_set_camera first    */
#define RDH_ERR_UNSUPPORTED (-3) /* a combination that is not built (e.g. a diagnostic entry in a non-diagnostic build) */
#define RDH_ERR_NO_DEVICE (-4)   /* no usable HIP device — there is NO CPU fallback       */
#define RDH_ERR_STATE (-5)       /* e.g. rdh_restir_direct before rdh_restir_init         */
#define RDH_ERR_COMM (-6)        /* RCCL missing or an nccl* call failed (rdh_last_error has ncclGetErrorString's text) */

typedef struct rdh_ctx rdh_ctx;

/* One texture: DevTextureObj (src/image.h:89-91) with a HOST pointer; texels are glm::vec3, row-major (Image::data()). */
typedef struct rdh_texture { int32_t width, height; const float *data; } rdh_texture;

/* Host arrays in the reference's DevScene layout (src/scene.h:494-517).
 * Replaces the argument of DevScene::create(const Scene&) (src/scene.cpp:461-551). */
typedef struct rdh_scene_desc {
    const float *vertices;       /* glm::vec3[3*numPrims], world-space triangle soup (src/scene.cpp:198-222) */
    const float *normals;        /* glm::vec3[3*numPrims]                                                     */
    const float *texcoords;      /* glm::vec2[3*numPrims]                                                     */
    const float *boundingBoxes;  /* AABB[bvhSize] = {pMin, pMax} (src/bvh.h:157-158)                           */
    const int32_t *bvhNodes[6];  /* MTBVHNode[bvhSize] = {primitiveId, boundingBoxId, nextNodeIfMiss} (:167-169) */
    int32_t bvhSize;             /* 2*numPrims-1                                                               */
    int32_t numPrims;
    const int32_t *materialIds;  /* int[numPrims]                                                              */
    const void *materials;       /* Material[numMaterials], 44 B each (src/material.h:276-286)                 */
    int32_t numMaterials;
    int32_t numLights;
    const int32_t *lightPrimIds;      /* int[numLights]                                                        */
    const float *lightUnitRadiance;   /* glm::vec3[numLights]                                                  */
    float sumLightPowerInv;           /* 1 / lightSampler.sum (src/scene.cpp:527)                              */
    int32_t lightSamplerLength;       /* DevDiscreteSampler1D::length (== numLights without an env map)        */
    const void *lightSampler;         /* BinomialDistrib<float>[length] = {float prob; int failId}             */
    const uint32_t *sampleSequence;   /* uint32[10000][200] Sobol table (src/scene.cpp:543-548)                */
    /* Textures and environment map (src/scene.cpp:463-486, 529-532).  Material map ids index `textures`
     * (-1 = NullTextureId, -2 = ProceduralTexId for baseColorMapId only). */
    int32_t numTextures;
    const struct rdh_texture *textures;
    int32_t envMapTexId;              /* Scene::envMapTexId: -1 = no environment map                           */
    int32_t envMapSamplerLength;      /* envMapSampler.length = width*height of the env map, 0 = none;
                                         with an env map the LAST lightSampler entry is the env map (scene.cpp:163) */
    const void *envMapSampler;        /* BinomialDistrib<float>[envMapSamplerLength]                           */
} rdh_scene_desc;

/* Byte-for-byte the reference's GBuffer (src/gBuffer.h:42-57, 272 B) with DENOISER_ENCODE_NORMAL=false,
 * DENOISER_ENCODE_POSITION=true: device pointers owned by the caller (GBuffer::create, src/denoiser.cu:329-359). */
typedef struct rdh_gbuffer {
    float *albedo;     /* glm::vec3[w*h]                                         */
    float *normal[2];  /* glm::vec3[w*h] x2 (double-buffered by frameIdx)        */
    int32_t *motion;   /* int[w*h]                                               */
    float *depth[2];   /* float[w*h] x2                                          */
    int32_t *primId[2];/* int[w*h] x2 — holds the MATERIAL id, -2 light, -1 miss */
    int32_t frameIdx;
    uint8_t lastCam[196];
    int32_t width, height;
} rdh_gbuffer;

typedef struct rdh_hit { int32_t primId; float u, v, t; } rdh_hit;

/* Exact work counters of the launches since the last reset (device atomics, one add per wave). */
typedef struct rdh_counters {
    uint64_t closestRays; /* DevScene::intersect calls       */
    uint64_t anyRays;     /* DevScene::testOcclusion calls   */
    uint64_t nodeVisits;  /* AABB tests                      */
    uint64_t triTests;    /* triangle tests                  */
    uint64_t closestHits;
} rdh_counters;

/* rdh_path_trace flags */
#define RDH_PT_MEGAKERNEL 0u   /* one lane per pixel, whole path in one launch (the reference's structure)  */
#define RDH_PT_WAVEFRONT 1u    /* raygen / extend / shade / connect queues with wave64 ballot compaction    */
#define RDH_PT_SORT_MATERIAL 2u/* wavefront only: each wave bins the 1 024 hit records of its packet by BSDF type before shading them */
#define RDH_PT_COUNT 4u        /* maintain rdh_counters (adds atomics; leave off when timing)               */
#define RDH_PT_PERSISTENT 16u  /* one persistent launch: per-lane state machine with lane refill (kernels_persist.h) */
#define RDH_PT_ONE_LANE_PER_PIXEL 64u /* rdh_gbuffer_render: the one-lane-per-pixel kernel (k_gbuffer) instead of the persistent
                                         lane-refill one (k_gbuffer_persistent)                                              */
#define RDH_PT_MEGA_GBUFFER RDH_PT_ONE_LANE_PER_PIXEL
#define RDH_PT_WG_PER_RAY 256u /* rdh_trace_closest / rdh_trace_occluded: one 1 024-thread workgroup per ray (the routine the
                                  G-buffer uses for literal-class rays); for tests            */
#define RDH_PT_NO_DEFER 128u   /* rdh_gbuffer_render: trace literal-class rays where they are generated (one wave each)
                                  instead of setting them aside for the workgroup-per-ray launch (k_gbuffer_literal)   */
#define RDH_PT_PARTITION_GBUFFER 512u /* rdh_gbuffer_render on a tile partition: render the records of THIS rank's tiles only
                                  (complete the planes with rdh_gbuffer_exchange*); default: every rank renders the whole frame */
#define RDH_PT_WF_SUBFRAMES 2048u /* wavefront only: the frame as sub-frames (8x8 blocks dealt round robin), one pipeline each on its own
                                  stream (frames of >= 2 048 blocks).  One pipeline by default: the streams of a context may share one
                                  hardware queue, and then more pipelines only run in series (RADISH_WF_PARTS=2..3: experiments) */
#define RDH_PT_RESTIR_FUSED 1024u /* rdh_restir_direct: round 1's pass 1, one lane per pixel with both walks inside the kernel
                                  (k_restir_pass1), instead of raygen / walk / RIS / walk / resolve (default; same results) */
#define RDH_PT_WF_SMALL_LISTS 4096u /* for tests.  Wavefront: the per-stage lists of literal-class rays hold 4 entries, so that the
                                  overflow path (such rays stay in the ordinary queues) runs.  rdh_gbuffer_render / rdh_restir_direct /
                                  stage 0 of the wavefront path: a wave walks its block as a packet for 4 visits only (256 normally), so
                                  that every block goes through the hand-over to per-lane walks (traverse.h, packetWalk) */
#define RDH_PT_PAIRS 32768u    /* per-lane walks over SIBLING PAIRS (one 64-byte record per inner node, shared by the six orderings: a lane
                                  that enters a node fetches both children and tests both boxes in one round trip; the far child is
                                  re-checked when the walk reaches it) instead of the six threaded arrays; same records, same counters.
                                  Default: on, whenever the six uploaded arrays are orderings of ONE binary tree at most 2 048 levels
                                  deep (every tree Radish's builder makes is one tree; n coincident triangles make a chain of n - 1
                                  levels).  Otherwise the threaded arrays are walked: silently by the frame entries, while
                                  rdh_trace_closest / rdh_trace_occluded (with RDH_PT_PERSISTENT) return RDH_ERR_UNSUPPORTED when
                                  the flag asks for pairs that do not exist */
#define RDH_PT_NO_PAIRS 16384u /* never walk the sibling pairs */
#define RDH_PT_NO_PACKETS 8192u /* rdh_gbuffer_render, rdh_restir_direct, and stage 0 of the wavefront path tracer (rdh_path_trace*
                                  with RDH_PT_WAVEFRONT): primary rays lane by lane (the lane-refill walkers; wavefront: k_wf_trace at
                                  k = 0) instead of as PACKETS — one 8x8 pixel block per wave, walked through the threaded order
                                  together with one uniform node load per visit (traverse.h, packetWalk; wavefront:
                                  k_wf_trace_primary); same records, same counters */
#define RDH_PT_AUTO 65536u     /* rdh_path_trace / rdh_path_trace_gathered*: the library picks the structure by what this launch holds —
                                  the wavefront pipeline with material sort and three sub-frames for a big tree (>= 100 000 nodes) and a
                                  big share of the frame (>= 12 000 8x8 blocks: a 1080p frame, or half of one), else the persistent kernel
                                  (measured: DESIGN 5d, 8).  Same pixels either way; other structure bits are ignored with it */
#define RDH_PT_WALK_ALL 131072u /* wavefront only: queue and walk every ray the path emits, in the reference's order of work.  By default a
                                  frame skips the last bounce's extension rays that miss the box over the emissive triangles (scenes without
                                  an environment map) and the shadow rays of light samples that contribute zero: same pixels, bit for bit.
                                  RDH_PT_COUNT implies it, so the counters stay the reference's */
#define RDH_PT_NO_SCHEDULE 32u /* persistent only: ignore the longest-paths-first block order of the previous launch   */
#define RDH_PT_PROFILE 8u      /* bracket each launch of the traversal kernel (k_pt_persistent, k_wf_trace, or the megakernel)
                                  with hipEvents on the context's stream; read with rdh_profile_read.  With
                                  RDH_PT_WF_SUBFRAMES the pipelines' launches overlap by design: ONE pair brackets the whole
                                  frame (before the fork to after the join) and rdh_profile_read counts frames            */

/* ReSTIR reuse mask = ReservoirReuse (src/common.h:41-48) */
#define RDH_REUSE_TEMPORAL 1
#define RDH_REUSE_SPATIAL 2

typedef struct rdh_restir_params {
    int32_t reuseMask;    /* Settings::reservoirReuse                                              */
    int32_t risCount;     /* RESERVOIR_SIZE = 32 (src/restir.h:9)                                   */
    int32_t numSpatial;   /* 5 in the reference (src/restir.cu:87); BASELINE config 4 also asks for 4 */
    int32_t temporalClamp;/* 20 (src/restir.cu:168)                                                 */
    int32_t faithfulRIS;  /* 1 = Reservoir::update's truthiness test (src/restir.h:21), 0 = corrected */
} rdh_restir_params;

/* ---- lifetime ---------------------------------------------------------------------------------------- */
int rdh_create(rdh_ctx **out, int device);
void rdh_destroy(rdh_ctx *ctx);
const char *rdh_last_error(const rdh_ctx *ctx);
/* Launch on an existing hipStream_t (e.g. torch's current stream).  NULL selects HIP's default (null) stream; a
 * context on which this is never called uses a private non-blocking stream. */
int rdh_set_stream(rdh_ctx *ctx, void *hipStream);
int rdh_synchronize(rdh_ctx *ctx);

/* ---- scene / camera -------------------------------------------------------------------------------- */
/* Replaces DevScene::create (src/scene.cpp:461-551): uploads and re-lays-out the scene (32-byte threaded nodes,
 * 48-byte triangle records, packed light records).  Blocking. */
int rdh_scene_upload(rdh_ctx *ctx, const rdh_scene_desc *desc);
/* ---- moving geometry (no reference counterpart: the reference rebuilds and re-uploads the whole scene) ------------------------
 * rdh_build_bvh_device: the device twin of rdh_build_bvh (include/radish_host.h) — d_vertices float[3*numPrims][3] -> d_boxes
 * float[2*numPrims-1][6] and d_nodes[k] int32[2*numPrims-1][3] = {primitiveId, boundingBoxId, nextNodeIfMiss}, bit for bit what the
 * host builder writes.  Device pointers; asynchronous on the context's stream; needs no scene.
 * rdh_scene_update_geometry: new positions for the SAME triangles of the uploaded scene (same count, materials, texcoords, light
 * list): d_vertices float[3*numPrims][3] (device), d_normals likewise or NULL (keep the uploaded normals), lights NULL (keep the
 * light table and sumLightPowerInv) or the moved lights' table.  Rewrites the triangle records, builds the tree on the device (the
 * tree rdh_build_bvh makes of these vertices), its six threaded arrays, sibling pairs and root box, the emissive triangles' records
 * and their per-light constants.  Asynchronous on the context's stream (the next render call waits for the build before it
 * launches); restarts the persistent block order; ReSTIR reservoirs are kept.  Coordinates must be finite and below 1e30, as for
 * rdh_scene_upload (not checked here: that would need the vertices on the host).  This is a precondition of the result, not a
 * courtesy: the walkers test class-0 rays with a fast box test whose equality with the literal AABB::intersect rests on every
 * t being finite, i.e. on |coord| < 1e30 (device/traverse.h: aabbFast).  The same holds for the _ex form, for
 * rdh_scene_refit_geometry and for the world positions rdh_scene_pose_objects produces (X * rest pose): vertices outside the
 * bound give undefined hits.  Texture coordinates must be finite and below 2^21 in magnitude (the procedural texture's cell
 * index is int(uv * 1024), undefined beyond): the two entries that take them, rdh_scene_upload and rdh_scene_set_geometry,
 * refuse others with RDH_ERR_ARGS. */
typedef struct rdh_light_update {
    const void *lightSampler;   /* HOST BinomialDistrib<float>[lightSamplerLength], as in rdh_scene_desc              */
    int32_t lightSamplerLength; /* must equal the scene's current (rdh_scene_set_materials changes it)               */
    float sumLightPowerInv;
} rdh_light_update;
int rdh_build_bvh_device(rdh_ctx *ctx, const float *d_vertices, int32_t numPrims, float *d_boxes, int32_t *const d_nodes[6]);
int rdh_scene_update_geometry(rdh_ctx *ctx, const float *d_vertices, const float *d_normals, const rdh_light_update *lights);
/* Builders for the _ex entries.  RDH_BVH_SAH: the binned-SAH builder above (the _ex entries then behave exactly as the plain ones).
 * RDH_BVH_LBVH: a linear BVH, a tree fully determined by the vertices but not the host builder's: primitives sorted by
 * the 30-bit Morton code of their box centre (stable, so equal codes keep primitive order), Karras' radix tree over the sorted
 * codes, depth-first slots with the lower sorted range first, boxes by the refit contract (so a refit with unchanged vertices
 * leaves it as built) and the host's rule for the six orderings.  Built in milliseconds where the SAH builder takes hundreds at
 * 1 M triangles; its depth is at most 59 levels, so it always has sibling pairs.
 * rdh_build_bvh_device_ex / rdh_scene_update_geometry_ex: rdh_build_bvh_device / rdh_scene_update_geometry with the builder named;
 * the same arguments, checks, outputs and asynchrony.  An unknown builder returns RDH_ERR_ARGS before anything is enqueued. */
#define RDH_BVH_SAH 0
#define RDH_BVH_LBVH 1
int rdh_build_bvh_device_ex(rdh_ctx *ctx, const float *d_vertices, int32_t numPrims, int builder, float *d_boxes,
                            int32_t *const d_nodes[6]);
int rdh_scene_update_geometry_ex(rdh_ctx *ctx, const float *d_vertices, const float *d_normals, const rdh_light_update *lights,
                                 int builder);
/* rdh_scene_refit_geometry: the same arguments, checks and light handling as rdh_scene_update_geometry, but the tree KEEPS its
 * topology: leaf primitives, the emission order and miss links of the six orderings, pair numbering, pair w fields and
 * ordering bits, and treeDepth all stay; only the boxes are recomputed, bottom-up: a leaf's box is bvhLo / bvhHi folded over its
 * three vertices in order from the empty box, an inner node's box is combLo / combHi of its two children, ordering 0's first child
 * always the earlier operand.  It writes the box fields of every record of the six NodeRec arrays, the child boxes of every pair
 * record and the root box.  The orderings are NOT re-sorted by the new box centres: a refit tree is walked in the orderings of its
 * last build.  The first refit after an upload or an update derives the refit plan from the uploaded arrays on the device and
 * blocks for it; it returns RDH_ERR_STATE (the scene unchanged and usable) unless the six arrays are six orderings of one tree
 * with one primitive per leaf.  Otherwise asynchronous on the context's stream, like rdh_scene_update_geometry.
 * rdh_scene_tree_cost: the SAH cost of the tree as it stands, sum over every node of surfaceArea(box) / surfaceArea(root box), in
 * double by a reduction of fixed order (it repeats exactly), and the same topology's cost before the first refit since the last
 * upload / update (both equal the current cost before any refit).  A root box of zero surface area (all geometry on one line or
 * point) makes every node count 1: the cost is then bvhSize.  Their ratio says when to rebuild.  Blocking. */
int rdh_scene_refit_geometry(rdh_ctx *ctx, const float *d_vertices, const float *d_normals, const rdh_light_update *lights);
int rdh_scene_tree_cost(rdh_ctx *ctx, double *sahNow, double *sahAtBuild);
/* rdh_scene_track_motion: make the G-buffer's motion plane follow geometry that moved.  The reference projects the
 * CURRENT hit position into the last camera, which names the wrong pixel of last frame's planes once a triangle has moved.  While
 * tracking is on, the context keeps the triangle records as its most recent rdh_gbuffer_render saw them (48 B per triangle: 48 MB
 * for config 5's 1-M-triangle scene), and a render after an update projects the hit point's PREVIOUS position (the same
 * barycentrics on the previous vertices) instead.  enable != 0 allocates the buffer and marks "previous == current"; 0 frees it;
 * the same value twice is a no-op.  Needs an uploaded scene (RDH_ERR_NO_SCENE); rdh_scene_upload and rdh_scene_free switch it
 * off.  "Previous" is what was in force at this context's last rdh_gbuffer_render: the first rdh_scene_update_geometry[_ex] /
 * rdh_scene_refit_geometry after a render saves the records it overwrites (in the same kernel), later ones before the next
 * render save nothing, and an update that is refused saves nothing.  A render with no update since the last one reads nothing and
 * writes the reference's plane.  Off (the default): no buffer, the same kernels' output bit for bit.  Misses keep motion = 0; the
 * plane stays an integer pixel index (-1: out of last frame).  Everything is enqueued on the context's stream; no host wait except
 * when switching off. */
int rdh_scene_track_motion(rdh_ctx *ctx, int enable);
/* Test access to the tree the kernels walk: which = 0 the six NodeRec arrays (6 x (bvhSize + 1) x 32 B, pad records included),
 * 1 the sibling pairs ((bvhSize - 1) / 2 + 1 records of 64 B; 0 bytes when the scene has none), 2 {int32 treeDepth, hasPairs, 0, 0;
 * float rootLo[4]; float rootHi[4]} (48 B).  Returns the byte size (hostOut NULL: only that) or a negative RDH_ERR_*.  Blocking. */
long long rdh_debug_read_tree(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);
/* ---- the light sampler of moving emissive geometry ------------------------------------------------------------------
 * The update and refit entries rewrite the emissive triangles' records; the alias table over their powers and sumLightPowerInv
 * either come with the call (rdh_light_update, built on the host) or are rebuilt here from the records the scene holds.
 * rdh_build_alias_table_device: the device twin of rdh_build_alias_table (include/radish_host.h) — d_values float[n] -> d_table
 * {float prob; int32 failId}[n] and *d_sum (the strictly sequential binary32 sum of the values), bit for bit what the host function
 * writes, NaN payloads aside (a sum of zero gives {NaN, i} entries as on the host).  Device pointers; asynchronous on the context's
 * stream; needs no scene; its scratch grows with n (growing it waits for the stream).  n == 0: RDH_OK, nothing written; n < 0 or a
 * null pointer with n > 0: RDH_ERR_ARGS.
 * rdh_scene_rebuild_lights: the light powers rdh_build_light_list computes, from the scene's CURRENT emissive-triangle records (as
 * the upload or the last update / refit left them; with an environment map the last entry is envPower, the environment's total
 * power as passed to rdh_build_alias_table when the scene was made) -> the scene's alias table, sumLightPowerInv = 1.f / sum and
 * the per-light constants again.  A scene whose lights were rebuilt so renders bit for bit like a fresh upload of the moved scene.
 * Asynchronous on the context's stream: sumLightPowerInv reaches the host the way an update's tree header does, and the next render
 * call waits for it before it launches.  Call it after an update or refit that was given lights = NULL, or at any other time; a
 * later update that brings a rdh_light_update replaces what a rebuild still in flight computes.  Scratch is allocated by the first
 * rebuild of a scene, sized by the lightSamplerLength the scene's arrays hold.  ReSTIR reservoirs are kept.  No scene, or (on a scene with an environment map)
 * an envPower that is negative or not finite: RDH_ERR_ARGS, the scene unchanged and nothing enqueued.  Without an environment map
 * envPower is ignored; lightSamplerLength == 0: RDH_OK, nothing done.
 * rdh_debug_read_lights: test access to the light sampler the kernels read: which = 0 the alias table (lightSamplerLength x 8 B),
 * 1 {float sum, sumLightPowerInv; int32 lightSamplerLength, numLights} (16 B; sum is 1.f / sumLightPowerInv, the reciprocal of the
 * frame kernels' argument as it stands: an upload brings only that value), 2 the per-light constants (numLights x 64 B: the
 * emissive triangle's record, its normal and power * sumLightPowerInv), 4 the current lightPrimIds (numLights x 4 B; 3 is not a selector and stays RDH_ERR_ARGS).  Returns the
 * byte size (hostOut NULL: only that) or a negative RDH_ERR_*.  Blocking; folds a rebuild still in flight in first, like
 * rdh_debug_read_tree.  After an rdh_scene_set_materials that derived the list again it also compares the device's own emitter
 * count with the host's (RDH_ERR_STATE when they differ). */
int rdh_build_alias_table_device(rdh_ctx *ctx, const float *d_values, int32_t n, void *d_table, float *d_sum);
int rdh_scene_rebuild_lights(rdh_ctx *ctx, float envPower);
long long rdh_debug_read_lights(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);
/* ---- objects posed on the device -------------------------------------------------------------------------------------
 * A scene file describes objects: a mesh with Translate / Rotate / Scale (include/radish_host.h: rdh_scene_parse_objects gives the
 * table and the meshes before their transforms, rdh_object_transform the matrices).  These entries keep that table with the scene
 * and produce the world-space arrays the update entries take on the device, with the host loader's roundings: a scene posed here
 * holds, bit for bit, the vertices and normals that a scene file with the same Translate / Rotate / Scale loads to.
 * rdh_scene_set_objects: objects[i] = triangles [firstPrim, firstPrim + numPrims) of the uploaded scene, whose rest pose is
 * triangles [restFirstPrim, restFirstPrim + numPrims) of restVertices / restNormals (HOST vec3[3*numRestPrims], object space; copied
 * once).  Object ranges must lie in the scene and be pairwise disjoint; they need not cover it (triangles of no object never move).
 * Rest ranges must lie in the rest arrays and may be shared.  numObjects == 0 clears the table.  Allocates the context-owned world
 * arrays (vec3[3*numPrims] vertices and normals: 72 B per triangle) and seeds them from the scene's records, which hold the uploaded
 * floats.  Blocking.  rdh_scene_upload and rdh_scene_free drop the table, the rest pose and the world arrays.
 * rdh_scene_pose_objects: objectIds int32[count] (HOST, each at most once), xforms32 float[count][32] (HOST: X column-major, then
 * inverse(X), as rdh_object_transform writes them).  On the context's stream: rewrites the listed objects' ranges of the world
 * arrays from the rest pose — w = X * (p, 1), n' = normalize(transpose(mat3(inverse(X))) * n), the loader's operations in the
 * loader's order — then does with the world arrays what rdh_scene_refit_geometry (tree = RDH_POSE_REFIT),
 * rdh_scene_update_geometry (RDH_POSE_SAH) or rdh_scene_update_geometry_ex with RDH_BVH_LBVH (RDH_POSE_LBVH) does with a caller's,
 * lights = NULL; with RDH_POSE_REBUILD_LIGHTS in flags, rdh_scene_rebuild_lights(ctx, envPower) follows.  Motion tracking, the tree
 * header and the persistent block order behave as for those entries.  No host wait in the steady state: ids and transforms go
 * through pinned memory (O(count)), and the call waits only for the staging copy of two poses ago (a first refit still derives
 * its plan and blocks, as always).  Checked before anything is enqueued, the scene unchanged: no table RDH_ERR_STATE; an id out of
 * range or listed twice, an unknown tree or flag, null pointers with count > 0, an envPower rdh_scene_rebuild_lights would refuse:
 * RDH_ERR_ARGS.  count == 0: RDH_OK, nothing enqueued.  Objects not listed keep what the world arrays hold.  When the tree step
 * refuses (a refit's RDH_ERR_STATE) the records are unchanged and the world arrays are seeded from them again before the next
 * pose; the same happens after the caller's own rdh_scene_update_geometry[_ex] / rdh_scene_refit_geometry, so a pose after those
 * moves the listed objects and leaves the caller's vertices everywhere else.  The posed world positions must satisfy the upload's
 * |coord| < 1e30 (see rdh_scene_update_geometry); the pose does not check it.
 * rdh_debug_read_world: test access to the world arrays (HOST float[9*numPrims] each).  Blocking. */
typedef struct rdh_object_range { int32_t firstPrim, numPrims, restFirstPrim; } rdh_object_range;
#define RDH_POSE_REFIT 0
#define RDH_POSE_SAH 1
#define RDH_POSE_LBVH 2
#define RDH_POSE_REBUILD_LIGHTS 1u
int rdh_scene_set_objects(rdh_ctx *ctx, const rdh_object_range *objects, int32_t numObjects, const float *restVertices,
                          const float *restNormals, int32_t numRestPrims);
int rdh_scene_pose_objects(rdh_ctx *ctx, const int32_t *objectIds, const float *xforms32, int32_t count, int tree, uint32_t flags,
                           float envPower);
int rdh_debug_read_world(rdh_ctx *ctx, float *verticesOut, float *normalsOut);
/* ---- materials edited on the device ------------------------------------------------------------------------------------
 * A scene whose materials were edited here is, bit for bit, the scene a fresh rdh_scene_upload of the edited description gives
 * (the alias table's NaN payloads aside, as for rdh_build_alias_table_device).
 * rdh_scene_set_materials: materialIds int32[count] (HOST, each at most once), materials Material[count] (HOST, 44 B each, as in
 * rdh_scene_desc): the listed materials of the uploaded scene are replaced.  Triangles keep their material ids.  On the context's
 * stream: the listed material records and every triangle's shading class (the wavefront material sort's key) are rewritten; when
 * the set of Light materials changes, or a Light's colour does, the emissive-triangle list is derived again on the device (in
 * ascending triangle order, radiance = the material's colour: what rdh_build_light_list and the upload's packing write), and
 * what rdh_scene_rebuild_lights(ctx, envPower) does follows: powers, alias table, per-light constants, sumLightPowerInv.  The
 * light count is known on the host at once (the context keeps the materials and how many triangles carry each), so
 * lightSamplerLength = numLights (+ 1 with an environment map) changes with the call, and a rdh_light_update, an update, a refit,
 * a pose, a rebuild or a debug read that follows sees the current list and length.  A list longer than the scene's arrays hold
 * reallocates them, which waits for the stream; a shorter one frees nothing.  An edit that leaves no light on a scene without an
 * environment map sets lightSamplerLength = 0 and sumLightPowerInv = 0.  No host wait in the steady state: ids and materials go
 * through pinned memory (O(count)), and the call waits only for the staging copy of two edits ago.  The tree, the pairs, the refit
 * plan, the object table and world arrays, motion tracking and the persistent block order are kept, and so are ReSTIR reservoirs:
 * a caller who switches emitters should call rdh_restir_init, as after every other scene edit that changes the lights.  Checked
 * before anything is enqueued, the scene unchanged: no scene RDH_ERR_NO_SCENE; an id out of range or listed twice, null pointers
 * with count > 0, a map id rdh_scene_upload would refuse (it must name one of the uploaded textures, -1, or -2 for a base
 * colour), an envPower rdh_scene_rebuild_lights would refuse: RDH_ERR_ARGS.  count == 0: RDH_OK, nothing enqueued.
 * Giving triangles other material ids, or another triangle set: rdh_scene_set_geometry, below (textures: rdh_scene_set_texture).
 * rdh_build_light_list_device: the device twin of rdh_build_light_list (include/radish_host.h) — d_vertices float[3*numPrims][3],
 * d_materialIds int32[numPrims], d_materials Material[numMaterials] -> d_lightPrimIds int32[], d_lightUnitRadiance float[][3],
 * d_lightPower float[] (each with room for numPrims entries; the first *d_count are written) and *d_count, bit for bit what the
 * host function writes.  A material id out of range makes *d_count -1 (the host function's RDH_HOST_ERR_ARGS) and leaves the
 * arrays unspecified; numPrims == 0: *d_count = 0.  Device pointers; asynchronous on the context's stream; needs no scene; its
 * scratch grows with numPrims (growing it waits for the stream).  Negative sizes or a null pointer: RDH_ERR_ARGS. */
int rdh_scene_set_materials(rdh_ctx *ctx, const int32_t *materialIds, const void *materials, int32_t count, float envPower);
int rdh_build_light_list_device(rdh_ctx *ctx, const float *d_vertices, const int32_t *d_materialIds, int32_t numPrims,
                                const void *d_materials, int32_t numMaterials, int32_t *d_lightPrimIds, float *d_lightUnitRadiance,
                                float *d_lightPower, int32_t *d_count);
/* ---- textures and the environment map edited on the device -------------------------------------------------------------
 * A scene whose textures were edited here is, bit for bit, the scene a fresh rdh_scene_upload of the edited description gives (the
 * alias tables' NaN payloads aside, as for rdh_build_alias_table_device).
 * rdh_scene_set_texture: d_texels float[height][width][3] (DEVICE, row-major: the layout of rdh_texture::data) replaces the texels
 * of texture texId of the uploaded scene in place; width and height must be the uploaded texture's (another size, another texture
 * count or another environment map still take rdh_scene_upload).  Asynchronous on the context's stream, which orders the copy
 * after the caller's writes to d_texels on that stream; no host wait.  A texture that is not the environment map: the copy and
 * nothing else.  The environment map: the same call also derives, on the device, what rdh_build_envmap_pdf + rdh_build_alias_table
 * (include/radish_host.h) and the upload derive from its texels — the pixel weights luminance * sin((0.5 + i) / height * PI), the
 * pixel alias table over them, and their sum, the environment's power; then what rdh_scene_rebuild_lights does follows with that
 * sum, read from device memory, as the light sampler's last entry: powers, alias table, per-light constants, sumLightPowerInv (which
 * reaches the host as after a rebuild).  The row factors sin(...) are the host's (glibc's sinf, not the device's): the first
 * environment edit of a scene computes them in the call and sends them through pinned memory, and allocates the workspace (20 B per
 * pixel: 4 for the weights, 16 for the construction's two lists); later edits allocate and send nothing.  The construction is rdh_build_alias_
 * table_device's: two single-wave kernels whose time grows linearly with width x height (measured: DESIGN 11h).  The tree, the
 * pairs, the refit plan, the object table and world arrays, motion tracking, the persistent block order and the material copies
 * are kept, and so are ReSTIR reservoirs: a caller who changes the environment should call rdh_restir_init, as after every other
 * scene edit that changes the lights.  Checked before anything is enqueued, the scene unchanged: no scene RDH_ERR_NO_SCENE; texId
 * outside [0, numTextures), a null pointer, a width or height that differs: RDH_ERR_ARGS.
 * rdh_scene_env_power: *out = the power of the environment entry as the scene holds it: after an environment edit that edit's sum
 * (the call waits for it); on a scene never edited the same kernels' sum over the uploaded texels, which has the bits of the sum
 * rdh_build_alias_table returned when the scene was made.  This is the envPower to hand to a later rdh_scene_rebuild_lights,
 * rdh_scene_set_materials or rdh_scene_pose_objects: a value kept from before an environment edit is stale.  Blocking.  No scene:
 * RDH_ERR_NO_SCENE; a scene without an environment map: RDH_ERR_STATE; a null pointer: RDH_ERR_ARGS.
 * rdh_debug_read_textures: test access: which = 0 every texture's texels as the kernels read them (texData, in upload order), 1 the
 * environment map's alias table (envMapSamplerLength x 8 B), 2 {float envPower (rdh_scene_env_power's; 0 without an environment
 * map); int32 envMapTexId, envMapSamplerLength, numTextures} (16 B).  Returns the byte size (hostOut NULL: only that) or a negative
 * RDH_ERR_*.  Blocking. */
int rdh_scene_set_texture(rdh_ctx *ctx, int32_t texId, const float *d_texels, int32_t width, int32_t height);
int rdh_scene_env_power(rdh_ctx *ctx, float *out);
long long rdh_debug_read_textures(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);
/* ---- the lens: depth of field ------------------------------------------------------------------------------------------------
 * The reference's Camera::sample leaves the aperture point at 0 (a pinhole, whatever lensRadius is); rdh_set_lens says how the
 * primary ray's third and fourth draw, which every path draws and the pinhole discards, pick a point pAperture on the unit aperture.
 * pLens = pAperture * lensRadius; the ray leaves position + right * pLens.x + up * pLens.y towards the pixel's point on the focal
 * plane, (ruv * (aspect, 1) * tanFovY, 1) * focalDist, as Camera::sample is written.  The draw cursor behind the primary ray is 4
 * in every mode.
 *   RDH_LENS_OFF   pAperture = 0: the reference's frames, bit for bit (the default, and the state after every rdh_scene_upload /
 *                  rdh_scene_free).
 *   RDH_LENS_DISK  pAperture = concentricSampleDisk(r.z, r.w), a round aperture.
 *   RDH_LENS_MASK  texture maskTexId of the uploaded scene (w x h texels, n = w * h) is the aperture over [-1, 1]^2: texel k is
 *                  chosen with probability luminance(texel k) / sum by an alias table over the n luminances in texel order
 *                  (k0 = min(int(float(n) * r.z), n - 1); k = r.w < prob[k0] ? k0 : failId[k0]), and the point inside it from
 *                  what the lookup leaves of the draws: jx = float(n) * r.z - float(k0), jy = r.w / prob or (r.w - prob) /
 *                  (1 - prob), each clamped to [0, 1); u = (col + jx) / w, v = (row + jy) / h, pAperture = (1 - 2u, 1 - 2v): the
 *                  flip the screen coordinate gets, so the mask lies on the aperture as it would on the screen.
 * While the mode is not OFF and the camera's lensRadius > 0, rdh_path_trace, _samples, _adaptive, _direct, _gathered(_all) and
 * rdh_dump_rays trace lens rays in every structure (a pixel's ray depends on its own index and Sobol row only, so tile partitions
 * agree with whole frames); with lensRadius <= 0 they launch the pinhole kernels.  The G-buffer and the denoisers stay the
 * pinhole's (renderGBuffer hard-codes pLens = 0), and rdh_restir_direct* return RDH_ERR_UNSUPPORTED with nothing enqueued.
 * rdh_set_lens: DISK and MASK need an uploaded scene (RDH_ERR_NO_SCENE).  MASK derives the luminances and the table on the device,
 * into storage that lives and dies with the scene (28 B per texel), with rdh_build_alias_table_device's kernels: a one-off cost that
 * grows linearly with n, and one host wait for the luminances' sum.  An unknown mode, a maskTexId outside
 * [0, numTextures), or a mask whose luminances sum to 0 or to something not finite: RDH_ERR_ARGS, and the previous mode and table
 * stay in force (a bad mode or id enqueues nothing; a bad sum is known once the weight kernels have run).  rdh_scene_set_texture on
 * the mask's texture while MASK is set derives the table again in the same call, from the new texels, and refuses a mask without an
 * aperture (RDH_ERR_ARGS, the scene unchanged); this costs that call the same host wait.
 * rdh_debug_primary_rays: test access: d_rays6 float[H][W][6] (DEVICE) <- {origin, direction} of every pixel's primary ray at Sobol
 * row `looper`, from the draw and the cameraSample call the tracers make (this rank's pixels on a tile partition).  Asynchronous.
 * rdh_debug_read_lens: test access: which = 0 {int32 mode, maskTexId (-1 unless MASK), w, h} (16 B), 1 the mask's alias table
 * (w x h x 8 B; nothing unless MASK).  Returns the byte size (hostOut NULL: only that) or a negative RDH_ERR_*.  Blocking. */
#define RDH_LENS_OFF 0
#define RDH_LENS_DISK 1
#define RDH_LENS_MASK 2
int rdh_set_lens(rdh_ctx *ctx, int mode, int32_t maskTexId);
int rdh_debug_primary_rays(rdh_ctx *ctx, int looper, float *d_rays6);
long long rdh_debug_read_lens(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);
/* ---- the triangle set replaced on the device -----------------------------------------------------------------------------
 * rdh_scene_set_geometry: the uploaded scene's triangles are replaced by numPrims triangles from DEVICE arrays, all four required
 * (the count may differ from the current one): d_vertices and d_normals float[3*numPrims][3], d_texcoords float[3*numPrims][2],
 * d_materialIds int32[numPrims].  builder: RDH_BVH_SAH or RDH_BVH_LBVH; envPower as for rdh_scene_rebuild_lights.  Materials,
 * textures, the environment map, the Sobol table and the camera stay.  With RDH_BVH_SAH the scene is then, bit for bit, what a
 * fresh rdh_scene_upload of the same description gives (these arrays, the scene's current materials and textures, rdh_build_bvh's
 * tree, rdh_build_light_list + rdh_build_alias_table; the alias table's NaN payloads aside): TriRec, AttrRec, shading classes, the
 * six node arrays at the new stride with their pad records, the pairs (none past 2 048 levels), treeDepth and root box, the
 * emissive-triangle list, LightRec, LightPre, alias table, lightSamplerLength and sumLightPowerInv.  With RDH_BVH_LBVH it is what
 * that upload followed by rdh_scene_update_geometry_ex(..., RDH_BVH_LBVH) on the same vertices holds.
 * One call: (1) one kernel over the caller's arrays counts the triangles of every material and flags a material id outside
 * [0, numMaterials), a coordinate that fails the upload's fabs(x) < 1e30f and a texture coordinate that fails its
 * fabs(t) < 2^21; the call waits for these 4 * (numMaterials + 2) bytes
 * through pinned memory, its only host wait apart from growth, and a raised flag returns RDH_ERR_ARGS with the scene unchanged.
 * (2) A count above what the scene's arrays hold (triangles, emitters, sampler entries: each tracked on its own) allocates the new
 * arrays first and releases the old ones then, so a failed allocation leaves the scene as it was; growth waits for the stream and
 * the side streams; a smaller count frees nothing.  (3) The records are packed, (4) the tree is built by `builder` as
 * rdh_scene_update_geometry builds it, and (5) the emissive-triangle list and what rdh_scene_rebuild_lights(ctx, envPower) does
 * follow, always: numLights is the host's sum of the new counts over the Light materials, so lightSamplerLength = numLights (+ 1
 * with an environment map) changes with the call; no light and no environment map: length 0, sumLightPowerInv 0.
 * Dropped, as an upload drops them: the refit plan, the persistent block order, the object table with its rest pose and world
 * arrays (a pose returns RDH_ERR_STATE until rdh_scene_set_objects is called again).  Kept: motion tracking if it was on — the
 * buffer follows the count and is marked "previous == current", because triangle p of the old set has no counterpart, so the next
 * G-buffer render writes the reference's plane — and ReSTIR reservoirs: call rdh_restir_init, as after every other edit that
 * changes the lights.  Refused before anything is enqueued: no scene RDH_ERR_NO_SCENE; a null pointer, numPrims <= 0 or above
 * 1 << 29, six node arrays of 4 GiB or more, an unknown builder, an envPower rdh_scene_rebuild_lights would refuse: RDH_ERR_ARGS.
 * rdh_debug_read_geometry: test access: which = 0 the TriRec bytes (numPrims x 48), 1 the AttrRec bytes (numPrims x 64), 2 the
 * shading classes (numPrims bytes), 3 the context's per-material triangle counts (numMaterials x int32).  Returns the byte size
 * (hostOut NULL: only that) or a negative RDH_ERR_*.  Blocking. */
int rdh_scene_set_geometry(rdh_ctx *ctx, const float *d_vertices, const float *d_normals, const float *d_texcoords,
                           const int32_t *d_materialIds, int32_t numPrims, int builder, float envPower);
long long rdh_debug_read_geometry(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);
/* Replaces DevScene::destroy (src/scene.cpp:553-574). */
int rdh_scene_free(rdh_ctx *ctx);
/* The `Camera cam` kernel argument of every reference kernel (State::scene->camera, src/pathtrace.cu:356). */
int rdh_set_camera(rdh_ctx *ctx, const void *camera196);

/* ---- multi-GPU tile partition (no reference counterpart) --------------------------------- */
/* The frame is cut into tileSize x tileSize pixel tiles, tile t belongs to rank t % world.  With world > 1 the
 * image arguments of the render calls are PACKED per-rank buffers: float[tilesPerRank][tileSize*tileSize][3],
 * tilesPerRank = rdh_tiles_per_rank(); gather them over RCCL and call rdh_untile.  world == 1 renders straight
 * into frame layout (y*W+x), which is the reference's. */
int rdh_set_partition(rdh_ctx *ctx, int rank, int world, int tileSize);
int rdh_tiles_per_rank(const rdh_ctx *ctx);
/* d_gathered: float[world][tilesPerRank][tileSize^2][3] (all-gather output) -> d_frame: float[H*W][3]. */
int rdh_untile(rdh_ctx *ctx, const float *d_gathered, float *d_frame);

/* ---- the hot path ---------------------------------------------------------------------------------- */
/* Replaces pathTrace(glm::vec3*, glm::vec3*, int) (src/pathtrace.cu:351-385) minus the State::looper increment
 * (the caller / shim owns the globals).  looper = State::looper, maxDepth = Settings::traceDepth. */
int rdh_path_trace(rdh_ctx *ctx, float *d_directIllum, float *d_indirectIllum, int iter, int looper, int maxDepth,
                   uint32_t flags);
/* numSamples samples per pixel in one call (the reference's `accumulate` loop, src/main.cpp, in the library).  Afterwards the images
 * and, with RDH_PT_COUNT, the work counters are bit for bit those of
 *     for s in 0..numSamples-1: rdh_path_trace(ctx, d, i, iter + s, (looper + s) % 10000, maxDepth, flags)
 * (the wrap is State::looper's, src/pathtrace.cu:380-381); numSamples == 1 is rdh_path_trace.  Arguments are checked as there;
 * numSamples < 1 or samplesPerPass < 0: RDH_ERR_ARGS, nothing enqueued.
 * With RDH_PT_WAVEFRONT, samplesPerPass samples share one pipeline pass: raygen - (trace - shade) x (maxDepth + 1) - finish over
 * samplesPerPass x the frame's path slots, so that every stage carries that many times the rays and ends on ONE tail instead of
 * one per sample.  Passes run in order on the context's stream over one workspace; the last takes the remainder.  A value above
 * numSamples is clamped to it.  One pass holds fewer than 2^30 path slots (64 per 8x8 block of this rank's tiles, per sample) and
 * at most 4 GiB of them at 164 B each (the workspace keeps its size afterwards; the sub-frame workspaces hold as much again): an
 * explicit samplesPerPass beyond either is RDH_ERR_ARGS, nothing allocated.  0: the library picks (16, measured; within
 * both limits).  The other structures (RDH_PT_PERSISTENT, RDH_PT_MEGAKERNEL) run one launch per sample, back to back, and ignore
 * samplesPerPass.  RDH_PT_AUTO picks the structure as rdh_path_trace does, not by the sample count.  The tile partition is
 * honoured as in rdh_path_trace (packed tiles).  The last-kernel time covers all passes (wavefront) or the last launch (others). */
int rdh_path_trace_samples(rdh_ctx *ctx, float *d_directIllum, float *d_indirectIllum, int iter, int looper, int numSamples,
                           int samplesPerPass, int maxDepth, uint32_t flags);
/* ---- adaptive sampling: per-pixel sample counts in one wavefront pass ---- */
#define RDH_ADAPTIVE_MAX_REQUEST 16 /* samples of one pixel in one pass: the most DESIGN 5f measured in one pass */
/* Trace a request plane.  All planes are in frame layout (y*W+x): d_sampleCount[p] is how many samples pixel p's running means hold
 * (it plays `iter`, per pixel), d_request[p] how many more to take now, 0..RDH_ADAPTIVE_MAX_REQUEST.  d_moments may be null; else it
 * is float[H*W][2], the running means of L and L*L, L = luminance(finishSample(direct) + finishSample(indirect)) of each sample,
 * folded with the running mean's expression (m * float(n) + x) / float(n + 1).
 * Contract.  After the call, for every pixel with r = request[p] > 0 and c = count[p]: the two images at p are bit for bit those of
 *     for j in 0..r-1: rdh_path_trace(ctx, d, i, iter = c + j, looper = (looper + c + j) % 10000, maxDepth, flags)
 * count[p] = c + r, and the moments are folded alike: every pixel walks its own Sobol rows however unevenly the frame is sampled.
 * A pixel with request[p] == 0 is not read beyond its request and not written in any plane.  With every request r and every count
 * c the call is rdh_path_trace_samples(.., iter = c, (looper + c) % 10000, numSamples = r, ..), work counters included; with
 * RDH_PT_COUNT the counters are those of the requested (pixel, sample) pairs and nothing else.  *samplesTraced (may be null)
 * receives the plane's sum T.
 * The requested pairs become a dense slot list (pixel-major inside 8x8-block order), made by an ordered count / scan / scatter on
 * the device, and the wavefront stages run over it: the cost of a call follows T, not the frame.  T is known only after the scan:
 * the entry reads it, together with the device's error flag, in one blocking copy — ONE host synchronisation per call — and sizes
 * the workspace and the grids by it.  T == 0: nothing more is launched, nothing written, RDH_OK.  A request outside
 * 0..RDH_ADAPTIVE_MAX_REQUEST, or a requested pixel's count negative or overflowing int32 with its request: RDH_ERR_ARGS, nothing
 * traced, no plane written.  T beyond what one pass holds (fewer than 2^30 slots, 4 GiB of them: rdh_path_trace_samples):
 * RDH_ERR_ARGS with T and the limit in rdh_last_error, nothing allocated; the caller lowers its step.
 * Always one pipeline: RDH_PT_WF_SUBFRAMES is accepted and ignored, because the slot list is dense already.  RDH_PT_SORT_MATERIAL,
 * RDH_PT_COUNT, RDH_PT_PAIRS / RDH_PT_NO_PAIRS, RDH_PT_WALK_ALL, RDH_PT_WF_SMALL_LISTS and RDH_PT_PROFILE mean what they mean in
 * rdh_path_trace.  Refused before anything is enqueued: without RDH_PT_WAVEFRONT, or with RDH_PT_PERSISTENT or RDH_PT_AUTO,
 * RDH_ERR_UNSUPPORTED; a tile partition with world > 1 RDH_ERR_UNSUPPORTED; null images, counts or requests, a maxDepth or looper
 * rdh_path_trace refuses: RDH_ERR_ARGS; RDH_ERR_NO_SCENE as there. */
int rdh_path_trace_adaptive(rdh_ctx *ctx, float *d_directIllum, float *d_indirectIllum, int32_t *d_sampleCount,
                            const int32_t *d_request, float *d_moments, int looper, int maxDepth, uint32_t flags,
                            int64_t *samplesTraced);
/* Decide the requests on the device from the counts and moments above.  All float32, in this order: with n = count[p], m1 and m2
 * the pixel's moments, a pixel WANTS samples if n < minSamples, or if err2 > tol * tol with var = m2 - m1 * m1,
 * err2 = var / float(n), tol = threshold * (m1 + 0.01f) (false for NaN).  An 8x8 block (the renderer's own blocks) is ACTIVE if any
 * of its pixels wants; every pixel of an active block with n < maxSamples gets request = min(step, maxSamples - n), every other
 * pixel 0.  `out` (may be null) receives the sums over the frame through one blocking read; with null the call is asynchronous.
 * step outside 1..RDH_ADAPTIVE_MAX_REQUEST, minSamples < 0, maxSamples < minSamples, a threshold that is negative or not finite,
 * null planes: RDH_ERR_ARGS.  Needs the camera (its resolution) and no scene; a tile partition with world > 1: RDH_ERR_UNSUPPORTED. */
typedef struct rdh_adaptive_stats { int64_t samplesRequested; int32_t activeBlocks; int32_t wantingPixels; } rdh_adaptive_stats;
int rdh_adaptive_plan(rdh_ctx *ctx, const int32_t *d_sampleCount, const float *d_moments, int32_t *d_request,
                      int minSamples, int maxSamples, int step, float threshold, rdh_adaptive_stats *out);
/* Replaces pathTraceDirect(glm::vec3*, int) (src/pathtrace.cu:387-407). */
int rdh_path_trace_direct(rdh_ctx *ctx, float *d_directIllum, int iter, int looper, uint32_t flags);
/* Replaces GBuffer::render(DevScene*, const Camera&) (src/gBuffer.cu:83-103). */
int rdh_gbuffer_render(rdh_ctx *ctx, const rdh_gbuffer *gb, uint32_t flags);
/* Replaces ReSTIRInit / ReSTIRFree (src/restir.cu:235-251): three DirectReservoir[w*h] buffers, zeroed. */
int rdh_restir_init(rdh_ctx *ctx);
int rdh_restir_free(rdh_ctx *ctx);
/* Replaces ReSTIRDirect(glm::vec3*, int, const GBuffer&) (src/restir.cu:205-233) incl. the reservoir swap and
 * the first-frame flag; two launches instead of one so that spatial reuse is race-free. */
int rdh_restir_direct(rdh_ctx *ctx, float *d_directIllum, int iter, int looper, const rdh_gbuffer *gb,
                      const rdh_restir_params *params, uint32_t flags);
/* Tile partition (world > 1): rdh_gbuffer_render always renders the WHOLE frame on every rank (temporal and spatial
 * reuse read the G-buffer at arbitrary / neighbouring pixels); rdh_restir_direct shades this rank's tiles into a
 * PACKED image buffer (as rdh_path_trace does), computing pass 1 on an 8-pixel apron as well so that pass 2 is local.
 * Temporal reuse needs last frame's reservoirs of the whole frame: after each rdh_restir_direct call
 * rdh_restir_exchange_pack(d_packed: float[tilesPerRank][tile^2][9]) → all-gather → rdh_restir_exchange_unpack(d_gathered:
 * float[world][tilesPerRank][tile^2][9]).  Results are bit-identical to the single-GPU frame. */
int rdh_restir_exchange_pack(rdh_ctx *ctx, float *d_packed);
int rdh_restir_exchange_unpack(rdh_ctx *ctx, const float *d_gathered);
/* G-buffer on a tile partition without replicated work: rdh_gbuffer_render(..., RDH_PT_PARTITION_GBUFFER) writes the records of
 * this rank's tiles (one primary ray per OWN pixel instead of per frame pixel); rdh_gbuffer_exchange_pack gathers them into
 * d_packed: float[tilesPerRank][tile^2][9] = {albedo.xyz, normal.xyz, motion, depth, primId} (ints as their bits) → all-gather →
 * rdh_gbuffer_exchange_unpack(d_gathered: float[world][tilesPerRank][tile^2][9]) scatters every rank's records into the
 * current planes (gb->frameIdx) of this rank's G-buffer: 36 B per pixel of the frame received per rank and frame. */
int rdh_gbuffer_exchange_pack(rdh_ctx *ctx, const rdh_gbuffer *gb, float *d_packed);
int rdh_gbuffer_exchange_unpack(rdh_ctx *ctx, const rdh_gbuffer *gb, const float *d_gathered);

/* ---- collectives from C++: RCCL over xGMI (no reference counterpart: the reference is single-device,
 *      /root/reference/src/preview.cpp:109 cudaGLSetGLDevice(0); frame loop /root/reference/src/main.cpp:163-202) ------------
 * One process (or host thread) per GPU.  Rank 0 calls rdh_comm_unique_id and hands the 128 bytes (== ncclUniqueId) to the other
 * ranks by any channel; every rank then calls rdh_comm_init on its context, which creates the communicator (ncclCommInitRank)
 * and sets the tile partition to (rank, world, current tile size).  RCCL is bound at run time (dlopen of the copy the process
 * already holds, else librccl.so.1; RADISH_RCCL_LIB overrides) so the library itself links only the HIP runtime.
 * Every collective below is enqueued on the context's stream and returns without synchronising.
 *   rdh_allgather_tiles          d_packed float[tilesPerRank][tile^2][3] → ONE ncclAllGather → k_untile → d_frame float[H*W][3]
 *   rdh_path_trace_gathered      pathTrace for N GPUs with the reference's signature semantics: whole-frame images in and out on
 *                                every rank (the running mean reads the caller's frame); renders this rank's tiles, then two
 *                                all-gathers (direct, indirect).  Works with world == 1 (RCCL accepts a single rank).
 *   rdh_restir_exchange          this rank's pre-spatial reservoirs of the frame just rendered → all-gather → every rank's
 *                                `last` reservoir buffer holds the whole frame (next frame's temporal reuse): 36 B/px
 *   rdh_restir_direct_gathered   ReSTIRDirect for N GPUs: whole-frame image in and out, includes rdh_restir_exchange
 *   rdh_gbuffer_exchange         pack → all-gather → unpack of the G-buffer records (see above)
 * ONE process driving n GPUs (the reference's host model: one process, one frame loop, /root/reference/src/main.cpp:71-116,
 * :163-202; SURVEY §8e "single process ... one host thread + stream per device"):
 *   rdh_comm_init_all            ctxs[i] (created on n DIFFERENT devices) becomes rank i of n: the n ncclCommInitRank calls are
 *                                made inside one ncclGroupStart/End, so one host thread can create them (rdh_comm_init blocks
 *                                until every rank has called it and therefore needs a thread or process per rank)
 *   rdh_path_trace_gathered_all  rdh_path_trace_gathered for all n contexts from one thread: n renders enqueued on n streams,
 *                                then per image ONE RCCL group with the n all-gathers, then n un-tile kernels.
 *                                d_directFrames[i] / d_indirectFrames[i]: whole-frame images on ctxs[i]'s device.
 *   rdh_gbuffer_exchange_all / rdh_restir_direct_gathered_all   the same for the ReSTIR frame: gbs[i] is context i's G-buffer
 *                                (planes on its device); one RCCL group per collective.
 * ReSTIR's exchanges OVERLAP rendering (default; rdh_comm_set_overlap(ctx, 0) puts everything back on the render stream): every
 * collective of rdh_gbuffer_exchange / rdh_restir_direct_gathered / rdh_restir_exchange is issued on a communication stream of
 * the context, in one order.  The G-buffer gather runs beside pass 1's ray generation, walks and RIS — rdh_restir_direct waits
 * for it where it first reads the planes (resolve step) — and the reservoir gather runs beside the NEXT frame's G-buffer pass and
 * pass 1.  The gathered IMAGE is complete in render-stream order when rdh_restir_direct_gathered returns.  Anything else that
 * reads G-buffer planes after rdh_gbuffer_exchange (the denoisers and rdh_copy_image_to_pbo do it themselves) calls
 * rdh_comm_join first: the render stream then waits for the exchanges in flight.  rdh_synchronize waits for both streams.        */
int rdh_comm_unique_id(void *id128);
int rdh_comm_init(rdh_ctx *ctx, const void *id128, int rank, int world);
int rdh_comm_init_all(rdh_ctx **ctxs, int n);
int rdh_comm_destroy(rdh_ctx *ctx);
int rdh_allgather_tiles(rdh_ctx *ctx, const float *d_packed, float *d_frame);
int rdh_path_trace_gathered(rdh_ctx *ctx, float *d_directFrame, float *d_indirectFrame, int iter, int looper, int maxDepth,
                            uint32_t flags);
int rdh_path_trace_gathered_all(rdh_ctx **ctxs, int n, float *const *d_directFrames, float *const *d_indirectFrames, int iter,
                                int looper, int maxDepth, uint32_t flags);
int rdh_restir_exchange(rdh_ctx *ctx);
int rdh_restir_direct_gathered(rdh_ctx *ctx, float *d_directFrame, int iter, int looper, const rdh_gbuffer *gb,
                               const rdh_restir_params *params, uint32_t flags);
int rdh_gbuffer_exchange(rdh_ctx *ctx, const rdh_gbuffer *gb);
int rdh_gbuffer_exchange_all(rdh_ctx **ctxs, int n, const rdh_gbuffer *gbs);
int rdh_restir_direct_gathered_all(rdh_ctx **ctxs, int n, float *const *d_directFrames, int iter, int looper, const rdh_gbuffer *gbs,
                                   const rdh_restir_params *params, uint32_t flags);
int rdh_comm_set_overlap(rdh_ctx *ctx, int enable);
int rdh_comm_join(rdh_ctx *ctx);

/* Display path (the step after the hot path): replaces copyImageToPBO's four overloads → sendImageToPBO
 * (/root/reference/src/pathtrace.cu:32-147; declared src/pathtrace.h:25-29).  d_pbo: uchar4[width*height] (alpha 0).
 * kind 0: d_image is vec3[w*h], colour = image * scale, tone mapping 0 None / 1 Filmic / 2 ACES (src/common.h:23-25),
 *         then gamma 1/2.2 (src/mathUtil.h:110-126);
 * kind 1: vec2[w*h] shown as (r, g, 0); kind 2: float[w*h] shown as grey; kind 3: int[w*h] pixel indices shown as
 *         normalised (x, y) (the motion-vector view).  toneMapping and scale are read for kind 0 only.
 * Asynchronous on the context's stream, like the reference's launch. */
int rdh_copy_image_to_pbo(rdh_ctx *ctx, void *d_pbo, const void *d_image, int width, int height, int kind, int toneMapping,
                          float scale);

/* Denoisers (/root/reference/src/denoiser.cu, declared src/denoiser.h).  One entry per reference kernel;
 * the filter classes (LeveledEAWFilter, SpatioTemporalFilter: buffers + the level schedule, denoiser.cu:411-558) are
 * composed from them by the C++ shim / the Python mirror.  All images are vec3[w*h] device buffers, variances float[w*h];
 * gb is the G-buffer rdh_gbuffer_render filled (current planes = gb->frameIdx, last = the other).  Asynchronous on the
 * context's stream.
 *   rdh_denoise_eaw                   waveletFilter, EAW (:17-84)  — EAWaveletFilter::filter (:388-397)
 *   rdh_denoise_svgf                  waveletFilter with variance (:92-173) — EAWaveletFilter::filter (:399-409)
 *   rdh_denoise_modulate              modulate (:175-185) — modulateAlbedo (:363-371)
 *   rdh_denoise_add                   add (:187-206) — addImage (:373-386); d_out may be d_in1
 *   rdh_denoise_temporal_accumulate   temporalAccumulate (:208-262)
 *   rdh_denoise_estimate_variance     estimateVariance (:264-299)
 *   rdh_denoise_filter_variance       filterVariance (:301-328)                                                      */
int rdh_denoise_eaw(rdh_ctx *ctx, float *d_colorOut, const float *d_colorIn, const rdh_gbuffer *gb, const void *camera196,
                    float sigLumin, float sigNormal, float sigDepth, int level);
int rdh_denoise_svgf(rdh_ctx *ctx, float *d_colorOut, const float *d_colorIn, float *d_varianceOut, const float *d_varianceIn,
                     const float *d_filteredVar, const rdh_gbuffer *gb, const void *camera196, float sigLumin, float sigNormal,
                     float sigDepth, int level);
int rdh_denoise_modulate(rdh_ctx *ctx, float *d_image, const rdh_gbuffer *gb);
int rdh_denoise_add(rdh_ctx *ctx, float *d_out, const float *d_in1, const float *d_in2, int width, int height);
int rdh_denoise_temporal_accumulate(rdh_ctx *ctx, float *d_colorAccumOut, const float *d_colorAccumIn, float *d_momentAccumOut,
                                    const float *d_momentAccumIn, const float *d_colorIn, const rdh_gbuffer *gb, int first);
int rdh_denoise_estimate_variance(rdh_ctx *ctx, float *d_variance, const float *d_moment, int width, int height);
int rdh_denoise_filter_variance(rdh_ctx *ctx, float *d_varianceOut, const float *d_varianceIn, int width, int height);

/* Test access to the reservoir buffers (36-byte DirectReservoir[w*h]): which = 0 current out, 1 last, 2 temp. */
int rdh_restir_read(rdh_ctx *ctx, int which, void *hostOut);
/* Test / analysis access to what the last split pass 1 (rdh_restir_direct without RDH_PT_RESTIR_FUSED) left between its launches,
 * per slot of its launch domain: which = 0 primary rays (6 floats), 1 shadow segments (6 floats, NaN first = none),
 * 2 the set-aside lists {int count[4]; int primarySlots[256]; int shadowSlots[256]}.  Returns the byte size (hostOut NULL: only
 * that), or a negative RDH_ERR_*. */
long long rdh_restir_read_scratch(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);

/* ---- traversal entry points (tests / roofline bench) ------------------------------------------------ */
/* d_rays: {origin.xyz, direction.xyz}[n].  DevScene::intersect (src/scene.h:262-301) per ray.
   flags: RDH_PT_COUNT; RDH_PT_PERSISTENT selects the walk-only lane-refill kernel (device/kernels_walk.h: a lane whose ray
   has ended takes the next ray of the batch; 1.6x the one-lane-per-ray kernel's rate, same records and counters) — for both
   entries. */
int rdh_trace_closest(rdh_ctx *ctx, const float *d_rays, int64_t n, rdh_hit *d_hits, uint32_t flags);
/* d_segments: {x.xyz, y.xyz}[n] -> d_occluded[n] in {0,1}.  DevScene::testOcclusion (src/scene.h:303-334). */
int rdh_trace_occluded(rdh_ctx *ctx, const float *d_segments, int64_t n, int32_t *d_occluded, uint32_t flags);

/* The ray lists of one frame, for the traversal-only measurements (bench.py roofline.traversal_only, cpu_baseline): runs the
 * frame `looper` of pathTrace (iter 0, one-lane-per-pixel kernel, scratch images) and appends every DevScene::intersect ray
 * {origin, direction} to d_closest (float[capClosest][6]) and every DevScene::testOcclusion segment {x, y} to d_any
 * (float[capAny][6]) — the input layouts of rdh_trace_closest / rdh_trace_occluded.  *nClosest / *nAny are the numbers of rays
 * the frame traces (rays beyond a capacity are counted, not stored; pass capacities 0 to size the lists).  Blocking. */
int rdh_dump_rays(rdh_ctx *ctx, int looper, int maxDepth, float *d_closest, int64_t capClosest, float *d_any, int64_t capAny,
                  int64_t *nClosest, int64_t *nAny);
/* Contexts that render CONCURRENTLY on one GPU (several frames in flight, each on its own stream): the persistent kernels size
 * their grid to fill the chip; `share` divides it so that `share` contexts together fill it once.  Default 1. */
int rdh_set_occupancy_share(rdh_ctx *ctx, int share);

int rdh_counters_reset(rdh_ctx *ctx);
int rdh_counters_read(rdh_ctx *ctx, rdh_counters *out); /* blocking */

/* Sum of the hipEvent-measured durations of the traversal-kernel launches made with RDH_PT_PROFILE since the last
 * rdh_profile_reset, and how many launches that was (at most 8192 are recorded).  Both calls block. */
int rdh_profile_reset(rdh_ctx *ctx);
int rdh_profile_read(rdh_ctx *ctx, double *totalMs, int64_t *launches);

/* Diagnostic builds only (-DRD_PERSIST_STAMPS): wall-clock stamps (100 MHz ticks) of the last persistent launch —
 * [0][w] wave w started, [1][w] it found the pixel supply dry, [2][w] it ended, [3][w] ticks it spent tracing literal-class rays
 * whole, [4][w] how many of those it had.  RDH_ERR_UNSUPPORTED otherwise. */
int rdh_debug_persist_stamps(rdh_ctx *ctx, uint64_t *out5x4096);
/* Diagnostic builds only (-DRD_PERSIST_PHASES): of the last persistent launch, summed over its waves — [0..5] s_memtime
 * ticks (100 MHz) spent in raygen / whole-wave rays / box loop / leaf tests / retire / shading, [6] total; [8] box
 * wave-steps, [9] box lane-steps, [10] leaf calls, [11] leaf lanes, [12] shade calls, [13] shade lanes, [14] raygen calls,
 * [15] raygen lanes.  RDH_ERR_UNSUPPORTED otherwise. */
int rdh_debug_persist_phases(rdh_ctx *ctx, uint64_t *out16);
/* Test access to the persistent path tracer's block scheduler (k_persist_schedule and the launch sequence rdh_path_trace keeps
 * around it with RDH_PT_PERSISTENT).
 * rdh_debug_persist_schedule: the schedule kernel alone, one launch on the context's stream over the CALLER's device arrays:
 * d_cost and d_ema (n words each, read and written: the costs are folded into the running means and zeroed) and d_order (n words,
 * written: the blocks in descending quarter-octave bucket of their new mean).  Nothing beyond word n - 1 of any array is touched.
 * Asynchronous; needs no scene and no camera.  A null pointer or n < 1: RDH_ERR_ARGS.
 * rdh_debug_persist_read: the sequence's state.  Blocking: waits for the context's stream and its side stream.  Returns the block
 * count B the arrays are sized for (0 before the first persistent launch) or a negative RDH_ERR_*.  state4 (may be NULL):
 * {persistent launches since the last restart, 1 while the sequence is valid (0: the next launch restarts it), B, the block count of
 * a pending rdh_debug_persist_set_order or 0}.  When capacity >= B > 0, each array that is not NULL is filled: orders = both
 * blockOrder buffers, 2 * B words (buffer 0, then buffer 1; a buffer no schedule has written yet holds whatever the allocation
 * held), costs = both blockCost buffers alike, ema = the B running means.  Launch n of a sequence writes costs to buffer n & 1;
 * its schedule writes order buffer n & 1, which launch n + 2 reads.
 * rdh_debug_persist_set_order: the NEXT persistent launch of this context, and only that one, visits its blocks in the order of
 * the HOST array `order`, whatever its place in the sequence and with or without RDH_PT_NO_SCHEDULE.  Costs, running means, the
 * schedule kernel and the launch count go on as they would have.  `order` must be a permutation of 0 .. n - 1 and n the block
 * count of the current camera and partition; otherwise RDH_ERR_ARGS and nothing changes (RDH_ERR_NO_SCENE without a camera).
 * Whatever restarts the sequence (a new scene or tree, another resolution, partition, stream or occupancy share) drops a pending
 * order.  Blocking (waits for the context's stream). */
int rdh_debug_persist_schedule(rdh_ctx *ctx, uint32_t *d_cost, uint32_t *d_ema, int32_t *d_order, int32_t n);
int rdh_debug_persist_read(rdh_ctx *ctx, int32_t *state4, int32_t *orders, uint32_t *costs, uint32_t *ema, int32_t capacity);
int rdh_debug_persist_set_order(rdh_ctx *ctx, const int32_t *order, int32_t n);
/* Diagnostic builds only (-DRD_WF_STAMPS): wall-clock stamps (100 MHz ticks) of the trace stages of the last wavefront pass
 * (its first pipeline), out[(stage * waves + logical wave) * 3 + i] — i = 0 the wave entered k_wf_trace, 1 it first found the
 * stage's queue exhausted, 2 it left; 0 where a wave wrote none.  *stages and *waves are always set; the stamps are copied when
 * capacity (in uint64_t) holds stages * waves * 3 of them, so a first call with capacity 0 sizes the second.  Blocking.
 * RDH_ERR_UNSUPPORTED otherwise. */
int rdh_debug_wf_stamps(rdh_ctx *ctx, uint64_t *out, int64_t capacity, int32_t *stages, int32_t *waves);
/* The rays the last wavefront pass of this context queued, summed over its pipelines: rays[k] = entries of trace(k)'s ray queue
 * (k = 0: 64 per 8x8 block of the launch, off-frame pixels included), shadows[k] = shadow rays shade(k) queued for trace(k + 1),
 * those on the first list included; k = 0 .. *stages - 1, *stages = maxDepth + 1 (0: no pass yet).  *stages is always set; the
 * counts are written when capacity (entries of each array) holds them.  With RDH_PT_WALK_ALL or RDH_PT_COUNT that is every ray
 * the reference traces; a default frame queues fewer (RDH_PT_WALK_ALL).  Blocking. */
int rdh_debug_wf_counts(rdh_ctx *ctx, int32_t *rays, int32_t *shadows, int32_t capacity, int32_t *stages);

/* Time of the most recent render call's kernels, measured with hipEvents on the context's stream (blocking);
 * the reference prints this figure from pathTrace (src/pathtrace.cu:364-374). */
int rdh_last_kernel_ms(rdh_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
