// tests/shim/shim_runner.cpp — runs radish_pt_amd/csrc/radish_shim.hpp on the GPU (tests/test_gpu_shim_runs.py).
//
// A host-only program: tests/shim/ref_decls.h (the declarations tests/shim/shim_syntax_check.cpp compiles the shim against),
// then the shim itself, linked against libradish_hip.so and the HIP runtime.  Built three times by
// radish_pt_amd/_build.py build_shim_runner: plain, -DRADISH_SHIM_MULTI_GPU, -DRADISH_SHIM_ONE_PROCESS_GPUS.
//
//   shim_runner <dir>
//
// <dir> holds, as raw little-endian arrays: vertices.bin normals.bin texcoords.bin material_ids.bin materials.bin boxes.bin
// nodes0.bin .. nodes5.bin light_ids.bin light_radiance.bin light_sampler.bin light_sum.bin env_sampler.bin
// texture_sizes.bin (int32 {w, h} per texture) texture_<k>.bin env_map_tex_id.bin sobol.bin (uint32 [10000][200])
// cameras.bin (196-byte records), whatever files the plan loads, and plan.txt: one step per line (see runStep).  The runner
// fills a Scene from the files, hands it over with radish_shim::devSceneCreate (then commInit / commInitAll in the two
// multi-GPU forms, for ONE GPU), and executes the plan through the shim's free functions and classes only; the bodies it
// adds are the ones the shim leaves to the reference (GBuffer::create / destroy / update, the Settings / State statics).
// <dir>/log.txt receives the loaded HIP runtime / RCCL objects and, after every step, State::looper; `dump` steps write
// device buffers to <dir>.  The expected values are computed by the test, on the CPU oracle; nothing of that is read here.
#include <link.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "ref_decls.h"

#define RADISH_SHIM_NO_REFERENCE_HEADERS
#define RADISH_SHIM_WITH_DENOISER
#include "radish_shim.hpp"

// ---- what the shim leaves to the reference --------------------------------------------------------------------------------
int Settings::traceDepth = 0;
int Settings::reservoirReuse = 0;
bool State::camChanged = true;
int State::looper = 0;
Scene *State::scene = nullptr;

[[noreturn]] static void die(const std::string &why) {
    std::fprintf(stderr, "shim_runner: %s\n", why.c_str());
    std::exit(2);
}
static void hipOk(hipError_t e, const char *what) {
    if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e));
}
template <typename T>
static T *zeroed(size_t n) {
    void *p = nullptr;
    hipOk(hipMalloc(&p, n * sizeof(T)), "hipMalloc");
    hipOk(hipMemset(p, 0, n * sizeof(T)), "hipMemset");
    return static_cast<T *>(p);
}

void GBuffer::create(int w, int h) {  // plain allocation (src/denoiser.cu:329-344)
    width = w;
    height = h;
    const size_t n = (size_t)w * h;
    albedo = zeroed<glm::vec3>(n);
    motion = zeroed<int>(n);
    for (int k = 0; k < 2; k++) {
        normal[k] = zeroed<glm::vec3>(n);
        depth[k] = zeroed<float>(n);
        primId[k] = zeroed<int>(n);
    }
    frameIdx = 0;
}
void GBuffer::destroy() {
    hipOk(hipFree(albedo), "hipFree");
    hipOk(hipFree(motion), "hipFree");
    for (int k = 0; k < 2; k++) {
        hipOk(hipFree(normal[k]), "hipFree");
        hipOk(hipFree(depth[k]), "hipFree");
        hipOk(hipFree(primId[k]), "hipFree");
    }
    albedo = nullptr;
    motion = nullptr;
    for (int k = 0; k < 2; k++) normal[k] = nullptr, depth[k] = nullptr, primId[k] = nullptr;
}
void GBuffer::update(const Camera &cam) {  // src/gBuffer.cu:78-81
    lastCam = cam;
    frameIdx ^= 1;
}

// ---- input ----------------------------------------------------------------------------------------------------------------
static std::string g_dir;
static std::string inDir(const std::string &name) { return g_dir + "/" + name; }

template <typename T>
static std::vector<T> readAll(const std::string &name) {
    std::ifstream f(inDir(name), std::ios::binary | std::ios::ate);
    if (!f) die("cannot open " + inDir(name));
    const size_t bytes = (size_t)f.tellg();
    if (bytes % sizeof(T)) die(name + ": size is no multiple of the record size");
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    if (bytes) f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)bytes);
    if (!f) die("cannot read " + inDir(name));
    return v;
}

static std::FILE *g_log = nullptr;
static int logObject(struct dl_phdr_info *info, size_t, void *tag) {
    const char *n = info->dlpi_name;
    if (n && (std::strstr(n, "amdhip64") || std::strstr(n, "rccl"))) std::fprintf(g_log, "loaded %s %s\n", static_cast<const char *>(tag), n);
    return 0;
}
static void logLoaded(const char *tag) {
    dl_iterate_phdr(logObject, const_cast<char *>(tag));
    std::fflush(g_log);
}

// ---- device buffers the plan names ----------------------------------------------------------------------------------------
// A name is a POINTER VARIABLE: the filters take their output by reference and swap it with their own buffers (all images of
// one plan have one size), so after a filter step the name holds whatever the shim left in it.
struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
};
static std::map<std::string, Buf> g_bufs;
static Buf &buf(const std::string &name) {
    static Buf null;
    if (name == "null") return null = Buf();
    auto it = g_bufs.find(name);
    if (it == g_bufs.end()) die("plan names an unknown buffer: " + name);
    return it->second;
}
static glm::vec3 *&v3(const std::string &name) { return reinterpret_cast<glm::vec3 *&>(buf(name).p); }

static std::vector<Camera> g_cams;
static GBuffer g_gb;
static LeveledEAWFilter g_eaw;
static SpatioTemporalFilter g_svgf;

static Buf special(const std::string &what) {
    const size_t n = (size_t)g_gb.width * g_gb.height;
    if (what == "gb.albedo") return {g_gb.albedo, n * 12};
    if (what == "gb.motion") return {g_gb.motion, n * 4};
    for (int k = 0; k < 2; k++) {
        const std::string s = std::to_string(k);
        if (what == "gb.normal" + s) return {g_gb.normal[k], n * 12};
        if (what == "gb.depth" + s) return {g_gb.depth[k], n * 4};
        if (what == "gb.primId" + s) return {g_gb.primId[k], n * 4};
    }
    const size_t m = (size_t)g_svgf.waveletFilter.width * g_svgf.waveletFilter.height;
    if (what == "svgf.variance") return {g_svgf.variance, m * 4};
    if (what == "svgf.accumColor") return {g_svgf.accumColor[g_svgf.frameIdx], m * 12};
    return buf(what);
}

// One step of the plan.  Image arguments are buffer names (`null`: a null pointer).
static void runStep(const std::string &op, std::istringstream &a) {
    auto I = [&] { int v = 0; if (!(a >> v)) die(op + ": missing integer argument"); return v; };
    auto F = [&] { float v = 0; if (!(a >> v)) die(op + ": missing float argument"); return v; };
    auto S = [&] { std::string v; if (!(a >> v)) die(op + ": missing name"); return v; };
    if (op == "alloc") {  // alloc NAME BYTES (zeroed)
        const std::string name = S();
        const size_t bytes = (size_t)I();
        g_bufs[name] = Buf{zeroed<unsigned char>(bytes), bytes};
    } else if (op == "load") {  // load NAME FILE
        const std::string name = S();
        std::vector<unsigned char> h = readAll<unsigned char>(S());
        Buf b{zeroed<unsigned char>(h.size()), h.size()};
        hipOk(hipMemcpy(b.p, h.data(), h.size(), hipMemcpyHostToDevice), "hipMemcpy (load)");
        g_bufs[name] = b;
    } else if (op == "camera") {
        const int k = I();
        if (k < 0 || k >= (int)g_cams.size()) die("camera index out of range");
        State::scene->camera = g_cams[(size_t)k];
    } else if (op == "depth") {
        Settings::traceDepth = I();
    } else if (op == "reuse") {
        Settings::reservoirReuse = I();
    } else if (op == "looper") {
        State::looper = I();
    } else if (op == "gbuffer_create") {  // the very first frame's lastCam is uninitialised in the reference: defined as the first camera
        const int w = I(), h = I();
        g_gb.create(w, h);
        g_gb.lastCam = g_cams[0];
    } else if (op == "gbuffer_render") {
        g_gb.render(State::scene->devScene, State::scene->camera);
    } else if (op == "gbuffer_update") {
        g_gb.update(State::scene->camera);
    } else if (op == "gbuffer_destroy") {
        g_gb.destroy();
    } else if (op == "restir_init") {
        ReSTIRInit();
    } else if (op == "restir_direct") {  // restir_direct IMAGE ITER
        glm::vec3 *img = v3(S());
        ReSTIRDirect(img, I(), g_gb);
    } else if (op == "restir_free") {
        ReSTIRFree();
    } else if (op == "path_trace_init") {
        pathTraceInit();
    } else if (op == "path_trace_free") {
        pathTraceFree();
    } else if (op == "path_trace") {  // path_trace DIRECT INDIRECT ITER
        glm::vec3 *d = v3(S()), *i = v3(S());
        pathTrace(d, i, I());
    } else if (op == "path_trace_samples") {  // path_trace_samples DIRECT INDIRECT ITER SAMPLES
        glm::vec3 *d = v3(S()), *i = v3(S());
        const int iter = I();
        pathTraceSamples(d, i, iter, I());
    } else if (op == "path_trace_direct") {  // path_trace_direct DIRECT ITER
        glm::vec3 *d = v3(S());
        pathTraceDirect(d, I());
    } else if (op == "pbo_vec3") {  // pbo_vec3 PBO IMAGE W H TONE SCALE
        uchar4 *pbo = static_cast<uchar4 *>(buf(S()).p);
        glm::vec3 *img = v3(S());
        const int w = I(), h = I(), tone = I();
        copyImageToPBO(pbo, img, w, h, tone, F());
    } else if (op == "pbo_vec3_default_scale") {  // pbo_vec3_default_scale PBO IMAGE W H TONE
        uchar4 *pbo = static_cast<uchar4 *>(buf(S()).p);
        glm::vec3 *img = v3(S());
        const int w = I(), h = I();
        copyImageToPBO(pbo, img, w, h, I());
    } else if (op == "pbo_vec2" || op == "pbo_float" || op == "pbo_int") {  // pbo_<type> PBO IMAGE W H
        uchar4 *pbo = static_cast<uchar4 *>(buf(S()).p);
        void *img = buf(S()).p;
        const int w = I(), h = I();
        if (op == "pbo_vec2") copyImageToPBO(pbo, static_cast<glm::vec2 *>(img), w, h);
        else if (op == "pbo_float") copyImageToPBO(pbo, static_cast<float *>(img), w, h);
        else copyImageToPBO(pbo, static_cast<int *>(img), w, h);
    } else if (op == "eaw_create") {
        const int w = I(), h = I();
        g_eaw.create(w, h, 5);
    } else if (op == "eaw_filter") {  // eaw_filter OUT IN: OUT is taken by reference and swapped
        glm::vec3 *&out = v3(S());
        g_eaw.filter(out, v3(S()), g_gb, State::scene->camera);
    } else if (op == "eaw_destroy") {
        g_eaw.destroy();
    } else if (op == "svgf_create") {
        const int w = I(), h = I();
        g_svgf.create(w, h, 5);
    } else if (op == "svgf_filter") {  // svgf_filter OUT IN
        glm::vec3 *&out = v3(S());
        g_svgf.filter(out, v3(S()), g_gb, State::scene->camera);
    } else if (op == "svgf_next_frame") {
        g_svgf.nextFrame();
    } else if (op == "svgf_destroy") {
        g_svgf.destroy();
    } else if (op == "modulate") {
        modulateAlbedo(v3(S()), g_gb);
    } else if (op == "add2") {  // add2 IMAGE IN W H
        glm::vec3 *img = v3(S()), *in = v3(S());
        const int w = I();
        addImage(img, in, w, I());
    } else if (op == "add3") {  // add3 OUT IN1 IN2 W H
        glm::vec3 *out = v3(S()), *in1 = v3(S()), *in2 = v3(S());
        const int w = I();
        addImage(out, in1, in2, w, I());
    } else if (op == "dump") {  // dump WHAT FILE: the shim's display and denoiser calls are asynchronous, so wait for the device first
        const Buf b = special(S());
        const std::string file = S();
        if (!b.p) die("dump of a null buffer");
        std::vector<unsigned char> h(b.bytes);
        hipOk(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hipOk(hipMemcpy(h.data(), b.p, b.bytes, hipMemcpyDeviceToHost), "hipMemcpy (dump)");
        std::ofstream f(inDir(file), std::ios::binary);
        f.write(reinterpret_cast<const char *>(h.data()), (std::streamsize)h.size());
        if (!f) die("cannot write " + inDir(file));
    } else if (op == "scene_destroy") {
        radish_shim::devSceneDestroy();
    } else {
        die("unknown step: " + op);
    }
}

int main(int argc, char **argv) {
    if (argc != 2) die("usage: shim_runner <dir>");
    g_dir = argv[1];
    g_log = std::fopen(inDir("log.txt").c_str(), "w");
    if (!g_log) die("cannot write " + inDir("log.txt"));
    logLoaded("start");

    // ---- a Scene as Scene::buildDevData leaves it (src/scene.cpp:190-249), from the files ----
    Scene scene;
    scene.meshData.vertices = readAll<glm::vec3>("vertices.bin");
    scene.meshData.normals = readAll<glm::vec3>("normals.bin");
    scene.meshData.texcoords = readAll<glm::vec2>("texcoords.bin");
    scene.materialIds = readAll<int>("material_ids.bin");
    scene.materials = readAll<Material>("materials.bin");
    scene.boundingBoxes = readAll<AABB>("boxes.bin");
    scene.BVHSize = (int)scene.boundingBoxes.size();
    for (int k = 0; k < 6; k++) scene.BVHNodes.push_back(readAll<MTBVHNode>("nodes" + std::to_string(k) + ".bin"));
    scene.lightPrimIds = readAll<int>("light_ids.bin");
    scene.lightUnitRadiance = readAll<glm::vec3>("light_radiance.bin");
    scene.lightSampler.binomDistribs = readAll<BinomialDistrib<float>>("light_sampler.bin");
    scene.lightSampler.sum = readAll<float>("light_sum.bin").at(0);
    scene.envMapSampler.binomDistribs = readAll<BinomialDistrib<float>>("env_sampler.bin");
    scene.envMapTexId = readAll<int>("env_map_tex_id.bin").at(0);
    const std::vector<int> sizes = readAll<int>("texture_sizes.bin");
    std::vector<std::vector<glm::vec3>> texels(sizes.size() / 2);
    std::vector<Image> images(sizes.size() / 2);
    for (size_t k = 0; k < images.size(); k++) {
        texels[k] = readAll<glm::vec3>("texture_" + std::to_string(k) + ".bin");
        if (texels[k].size() != (size_t)sizes[2 * k] * (size_t)sizes[2 * k + 1]) die("texture size does not match its file");
        images[k].w = sizes[2 * k];
        images[k].h = sizes[2 * k + 1];
        images[k].pixels = texels[k].data();
    }
    for (Image &im : images) scene.textures.push_back(&im);
    const std::vector<uint32_t> sobol = readAll<uint32_t>("sobol.bin");
    if (sobol.size() != (size_t)10000 * 200) die("sobol.bin is not uint32[10000][200]");
    g_cams = readAll<Camera>("cameras.bin");
    if (g_cams.empty()) die("cameras.bin is empty");
    scene.camera = g_cams[0];
    State::scene = &scene;

    radish_shim::devSceneCreate(scene, sobol.data());
#if defined(RADISH_SHIM_ONE_PROCESS_GPUS)
    radish_shim::commInitAll(scene, sobol.data(), 1);
    logLoaded("comm");
#elif defined(RADISH_SHIM_MULTI_GPU)
    unsigned char id[128];
    radish_shim::commUniqueId(id);
    radish_shim::commInit(id, 0, 1);
    logLoaded("comm");
#endif
    std::fprintf(g_log, "scene looper %d\n", State::looper);

    std::ifstream plan(inDir("plan.txt"));
    if (!plan) die("cannot open " + inDir("plan.txt"));
    std::string line;
    int step = 0;
    while (std::getline(plan, line)) {
        std::istringstream a(line);
        std::string op;
        if (!(a >> op)) continue;
        runStep(op, a);
        std::fprintf(g_log, "step %d %s looper %d\n", step++, op.c_str(), State::looper);
        std::fflush(g_log);
    }
    std::fclose(g_log);
    return 0;
}
