// tests/shim/shim_syntax_check.cpp — compile check of radish_pt_amd/csrc/radish_shim.hpp (tests/test_shim_compiles.py).
//
// Includes tests/shim/ref_decls.h (the minimal reference-shaped declarations the shim touches, with their layout asserts; the
// same header tests/shim/shim_runner.cpp is built and run with), then the shim with every section switched on, and
// instantiates its templates.  It is compiled with -fsyntax-only -Wall -Werror: a typo, a wrong argument count against
// include/radish_hip.h or a layout static_assert that no longer holds fails the CPU test suite.  Nothing here is linked or
// run; the runner is.
#include "ref_decls.h"

#define RADISH_SHIM_NO_REFERENCE_HEADERS
#define RADISH_SHIM_WITH_DENOISER
#ifdef SHIM_CHECK_MULTI_GPU
#define RADISH_SHIM_MULTI_GPU
#endif
#ifdef SHIM_CHECK_ONE_PROCESS
#define RADISH_SHIM_ONE_PROCESS_GPUS
#endif
#include "radish_shim.hpp"

// use everything once, so that templates are instantiated and overloads resolved
void shim_syntax_check_uses(Scene &scene, GBuffer &gb, glm::vec3 *img, glm::vec3 *img2, uchar4 *pbo, const uint32_t *sobol) {
    radish_shim::devSceneCreate(scene, sobol);
#ifdef SHIM_CHECK_ONE_PROCESS
    radish_shim::commInitAll(scene, sobol, 2);
#else
    unsigned char id[128];
    radish_shim::commUniqueId(id);
    radish_shim::commInit(id, 0, 1);
#endif
    pathTraceInit();
    pathTrace(img, img2, 0);
    pathTraceDirect(img, 0);
    ReSTIRInit();
    gb.render(scene.devScene, scene.camera);
    ReSTIRDirect(img, 0, gb);
    copyImageToPBO(pbo, img, 4, 4, 2);
    copyImageToPBO(pbo, reinterpret_cast<glm::vec2 *>(img), 4, 4);
    copyImageToPBO(pbo, reinterpret_cast<float *>(img), 4, 4);
    copyImageToPBO(pbo, reinterpret_cast<int *>(img), 4, 4);
    LeveledEAWFilter eaw;
    eaw.create(4, 4, 5);
    glm::vec3 *out = img2;
    eaw.filter(out, img, gb, scene.camera);
    eaw.destroy();
    SpatioTemporalFilter svgf;
    svgf.create(4, 4, 5);
    svgf.filter(out, img, gb, scene.camera);
    svgf.nextFrame();
    svgf.destroy();
    modulateAlbedo(img, gb);
    addImage(img, img2, 4, 4);
    addImage(img, img2, img, 4, 4);
    ReSTIRFree();
    pathTraceFree();
    radish_shim::devSceneDestroy();
}
