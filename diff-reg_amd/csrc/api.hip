// api.hip -- version / error reporting of the C ABI.
#include <stdlib.h>
#include "kernels.h"
#include <vector>
#include <stdio.h>
#include <string.h>

namespace dr {
static thread_local char g_hip_err[512] = "";
void set_hip_error(hipError_t e, const char* where) {
    snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s (%d)", where, hipGetErrorString(e), (int)e);
}

static bool g_env_knobs = false;
void enable_env_knobs(bool on) { g_env_knobs = on; }
int env_knob(const char* name, int def) {
    if (!g_env_knobs) return def;
    const char* e = getenv(name);
    return e ? atoi(e) : def;
}

int device_cu_count() {
    static int cache[64];                                          // 0 = not asked yet
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return 256;
    if (!cache[d]) {
        hipDeviceProp_t pr;
        cache[d] = hipGetDeviceProperties(&pr, d) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    }
    return cache[d];
}

bool g_prof_on = false;
struct ProfRec { int kind; double work; hipEvent_t a, b; };
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_pool;
static hipEvent_t get_event() {
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}
void prof_begin(int kind, double work, hipStream_t st) {
    ProfRec r; r.kind = kind; r.work = work; r.a = get_event(); r.b = nullptr;
    (void)hipEventRecord(r.a, st);
    g_prof.push_back(r);
}
void prof_end(int kind, hipStream_t st) {
    for (size_t i = g_prof.size(); i-- > 0;)
        if (g_prof[i].kind == kind && !g_prof[i].b) { g_prof[i].b = get_event(); (void)hipEventRecord(g_prof[i].b, st); return; }
}
}  // namespace dr

namespace dr {
__global__ void noop_kernel(int* p) { if (p && threadIdx.x == 0 && blockIdx.x == 0) *p = 0; }
}

extern "C" {
void dr_prof_enable(int on) { dr::g_prof_on = on != 0; }

/* synchronises the device, then fills calls[k], ms[k], work[k] (k < DR_PROF_KINDS) and clears the log */
int dr_prof_collect(int* calls, double* ms, double* work) {
    using namespace dr;
    DR_HIP_CHECK(hipDeviceSynchronize());
    for (int k = 0; k < PK_COUNT; ++k) { calls[k] = 0; ms[k] = 0; work[k] = 0; }
    for (auto& r : g_prof) {
        if (r.b) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, r.a, r.b);
            calls[r.kind] += 1; ms[r.kind] += t; work[r.kind] += r.work;
            g_pool.push_back(r.b);
        }
        g_pool.push_back(r.a);
    }
    g_prof.clear();
    return DR_OK;
}

/* diagnostics: n launches of a kernel that does nothing, each dependent on the one before (same stream) -- what a dependent launch
 * costs on this platform whatever it does: the floor under the single-pair latency (tools/launch_floor.py) */
int dr_debug_launch_chain(int n, int workgroups, int threads, void* stream) {
    if (n < 0 || workgroups < 1 || threads < 64 || threads > 1024) return DR_EINVAL;
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(dr::noop_kernel, dim3(workgroups), dim3(threads), 0, (hipStream_t)stream, (int*)nullptr);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_version(void) { return DR_ABI_VERSION; /* 0.7.0: the header this library was built from */ }

const char* dr_strerror(int code) {
    switch (code) {
        case DR_OK: return "ok";
        case DR_EINVAL: return "invalid argument";
        case DR_ELAUNCH: return "HIP call failed";
        case DR_ENOSUP: return "shape not supported by this build";
        case DR_EWORKSPACE: return "workspace missing or too small";
        case DR_ETIMEOUT: return "a kernel gave up waiting for a workgroup that was not resident (outputs of that call are unspecified: NaN where the waiting workgroup wrote)";
        default: return "unknown error";
    }
}

const char* dr_last_hip_error(void) { return dr::g_hip_err; }
}
