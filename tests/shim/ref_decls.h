// tests/shim/ref_decls.h — the reference-shaped declarations radish_pt_amd/csrc/radish_shim.hpp is compiled AND run against.
//
// The shim is the reference-signature side of the drop-in boundary; glm and the reference's headers are not in this image, so
// it cannot be compiled against them here.  This header declares — in its own minimal form, members named and ordered as the
// shim reads them — the few types of the reference the shim touches (src/sceneStructs.h:118-130 Camera, src/gBuffer.h:15-58
// GBuffer, src/scene.h:33-70,520-577 MeshData / Scene, src/sampler.h:76-139 DiscreteSampler1D, src/image.h:9-40 Image,
// src/common.h:50-72 Settings / State, src/denoiser.h:16-82 the filter classes).  Two files include it, then the shim:
//   tests/shim/shim_syntax_check.cpp   -fsyntax-only -Wall -Werror (tests/test_shim_compiles.py)
//   tests/shim/shim_runner.cpp         linked against libradish_hip.so and run on the GPU (tests/test_gpu_shim_runs.py)
// so what is compiled is what is run.  The layout asserts below hold the types the shim reinterprets or memcpy's to the C ABI
// of include/radish_hip.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>  // hipMalloc / hipFree used by the denoiser section; also brings uchar4

#include "radish_hip.h"  // rdh_gbuffer, for the layout asserts

namespace glm {
struct vec2 { float x, y; };
struct vec3 { float x, y, z; };
struct ivec2 { int x, y; };
struct mat3 { vec3 c[3]; };
struct mat4 { float m[16]; };
}  // namespace glm

struct Camera {  // 196 bytes, field order of src/sceneStructs.h:118-130
    glm::ivec2 resolution;
    glm::vec3 position, rotation, view, up, right;
    glm::vec2 fov, pixelLength;
    glm::mat3 rotationMatInv;
    glm::mat4 viewProjection;
    float lensRadius, focalDist, tanFovY;
};
static_assert(sizeof(Camera) == 196, "Camera layout");

struct DevScene;
struct GBuffer {  // src/gBuffer.h:15-58 with DENOISER_ENCODE_NORMAL false, DENOISER_ENCODE_POSITION true
    void create(int width, int height);
    void destroy();
    void render(DevScene *scene, const Camera &cam);
    void update(const Camera &cam);
    glm::vec3 *albedo = nullptr;
    glm::vec3 *normal[2] = {nullptr};
    int *motion = nullptr;
    float *depth[2] = {nullptr};
    int *primId[2] = {nullptr};
    int frameIdx = 0;
    Camera lastCam;
    int width;
    int height;
};
// radish_shim::toC memcpy's a GBuffer into an rdh_gbuffer: every member sits where the C struct has it
static_assert(sizeof(GBuffer) == sizeof(rdh_gbuffer) && sizeof(rdh_gbuffer) == 272, "GBuffer size");
static_assert(offsetof(GBuffer, albedo) == offsetof(rdh_gbuffer, albedo), "GBuffer::albedo");
static_assert(offsetof(GBuffer, normal) == offsetof(rdh_gbuffer, normal) && sizeof(GBuffer::normal) == sizeof(rdh_gbuffer::normal), "GBuffer::normal");
static_assert(offsetof(GBuffer, motion) == offsetof(rdh_gbuffer, motion), "GBuffer::motion");
static_assert(offsetof(GBuffer, depth) == offsetof(rdh_gbuffer, depth) && sizeof(GBuffer::depth) == sizeof(rdh_gbuffer::depth), "GBuffer::depth");
static_assert(offsetof(GBuffer, primId) == offsetof(rdh_gbuffer, primId) && sizeof(GBuffer::primId) == sizeof(rdh_gbuffer::primId), "GBuffer::primId");
static_assert(offsetof(GBuffer, frameIdx) == offsetof(rdh_gbuffer, frameIdx), "GBuffer::frameIdx");
static_assert(offsetof(GBuffer, lastCam) == offsetof(rdh_gbuffer, lastCam) && sizeof(GBuffer::lastCam) == sizeof(rdh_gbuffer::lastCam), "GBuffer::lastCam");
static_assert(offsetof(GBuffer, width) == offsetof(rdh_gbuffer, width), "GBuffer::width");
static_assert(offsetof(GBuffer, height) == offsetof(rdh_gbuffer, height), "GBuffer::height");

struct Material { int type; glm::vec3 baseColor; float metallic, roughness, ior; int maps[4]; };
static_assert(sizeof(Material) == 44, "Material layout");
struct AABB { glm::vec3 pMin, pMax; };
static_assert(sizeof(AABB) == 24, "AABB layout");
struct MTBVHNode { int primitiveId, boundingBoxId, nextNodeIfMiss; };
static_assert(sizeof(MTBVHNode) == 12, "MTBVHNode layout");
template <typename T> struct BinomialDistrib { T prob; int failId; };
static_assert(sizeof(BinomialDistrib<float>) == 8, "BinomialDistrib<float> layout");
template <typename T> struct DiscreteSampler1D {
    std::vector<BinomialDistrib<T>> binomDistribs;
    T sum = static_cast<T>(0);
};
struct Image {
    int width() const { return w; }
    int height() const { return h; }
    glm::vec3 *data() const { return pixels; }
    int w = 0, h = 0;
    glm::vec3 *pixels = nullptr;
};
struct MeshData { std::vector<glm::vec3> vertices, normals; std::vector<glm::vec2> texcoords; };
struct Scene {
    std::vector<Image *> textures;
    std::vector<Material> materials;
    std::vector<int> materialIds;
    int BVHSize = 0;
    std::vector<AABB> boundingBoxes;
    std::vector<std::vector<MTBVHNode>> BVHNodes;
    MeshData meshData;
    std::vector<int> lightPrimIds;
    std::vector<glm::vec3> lightUnitRadiance;
    DiscreteSampler1D<float> lightSampler, envMapSampler;
    int envMapTexId = -1;
    DevScene *devScene = nullptr;
    Camera camera;
};
struct Settings { static int traceDepth; static int reservoirReuse; };
struct State { static bool camChanged; static int looper; static Scene *scene; };

struct EAWaveletFilter {
    EAWaveletFilter() = default;
    EAWaveletFilter(int width, int height, float sigLumin, float sigNormal, float sigDepth)
        : sigLumin(sigLumin), sigNormal(sigNormal), sigDepth(sigDepth), width(width), height(height) {}
    void filter(glm::vec3 *colorOut, glm::vec3 *colorIn, const GBuffer &gBuffer, const Camera &cam, int level);
    void filter(glm::vec3 *colorOut, glm::vec3 *colorIn, float *varianceOut, float *varianceIn, float *filteredVar,
                const GBuffer &gBuffer, const Camera &cam, int level);
    float sigLumin, sigNormal, sigDepth;
    int width = 0, height = 0;
};
struct LeveledEAWFilter {
    void create(int width, int height, int level);
    void destroy();
    void filter(glm::vec3 *&colorOut, glm::vec3 *colorIn, const GBuffer &gBuffer, const Camera &cam);
    EAWaveletFilter waveletFilter;
    int level = 0;
    glm::vec3 *tmpImg = nullptr;
};
struct SpatioTemporalFilter {
    void create(int width, int height, int level);
    void destroy();
    void temporalAccumulate(glm::vec3 *colorIn, const GBuffer &gBuffer);
    void estimateVariance();
    void filterVariance();
    void filter(glm::vec3 *&colorOut, glm::vec3 *colorIn, const GBuffer &gBuffer, const Camera &cam);
    void nextFrame();
    EAWaveletFilter waveletFilter;
    int level = 0;
    glm::vec3 *accumColor[2] = {nullptr};
    glm::vec3 *accumMoment[2] = {nullptr};
    float *variance = nullptr;
    bool firstTime = true;
    glm::vec3 *tmpColor = nullptr;
    float *tmpVar = nullptr;
    float *filteredVar = nullptr;
    int frameIdx = 0;
};
