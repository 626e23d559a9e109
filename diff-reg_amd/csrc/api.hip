// api.hip -- the parts of the C ABI that stand on their own: version / error reporting, profiling, dr_init and the debug setters, and the
// entries of the individual ops (position code, linear / batched GEMM, Procrustes, top-1 read-out) -- thin argument checks in front of
// the launch interface of kernels.h.
#include <stdlib.h>
#include "loop_common.h"
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

using namespace dr;

extern "C" {

int dr_init(void) {
    int rc = attention_configure();
    if (rc == DR_OK) rc = gemm_configure();
    if (rc == DR_OK) rc = pgemm_configure();
    if (rc == DR_OK) rc = vit_f32_configure();
    if (rc == DR_OK) rc = nonrigid_configure();
    if (rc == DR_OK) rc = geo_graph_configure();
    if (rc == DR_OK && !device_status_word()) rc = DR_ELAUNCH;       // resolved here, outside any stream capture (eval2d3d.hip)
    return rc;
}

/* diagnostics for tools/ and tests: force the GEMM tile configuration (-1 auto, 0, 9, 11, 12), run the internal problem form */
void dr_debug_enable_env(int on) { enable_env_knobs(on != 0); }
void dr_debug_gemm_config(int c) { gemm_force_config(c); }

int dr_debug_gemm_f32(const dr_debug_gemm_problem* problems, int n, void* stream) {
    if (!problems || n < 1 || n > 4) return DR_EINVAL;
    GemmBatch g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < n; ++i) {
        const dr_debug_gemm_problem& q = problems[i];
        const int K1 = q.A2 ? q.K1 : q.K;
        if (q.rows < 0 || q.ncols <= 0 || q.K <= 0 || !q.A || !q.W || !q.out || q.nbatch < 0) return DR_EINVAL;
        if (q.lda < K1 || q.ldo < q.ncols || (q.A2 && (K1 <= 0 || K1 >= q.K || q.lda2 < q.K - K1))) return DR_EINVAL;
        if ((q.epilogue & ~(EPI_RELU | EPI_ROTARY)) ||
            ((q.epilogue & EPI_ROTARY) && (!q.cos_t || !q.sin_t || q.rot_C <= 0 || (q.rot_C & 1))))
            return DR_EINVAL;
        GemmProblem& p = g.p[i];
        p.A = q.A; p.A2 = q.A2; p.W = q.W; p.out = q.out; p.cosT = q.cos_t; p.sinT = q.sin_t; p.bias = q.bias; p.addend = q.addend;
        p.rows = q.rows; p.ncols = q.ncols; p.K = q.K; p.K1 = K1; p.lda = q.lda; p.lda2 = q.A2 ? q.lda2 : 0; p.ldo = q.ldo;
        p.epi = q.epilogue; p.rot_C = q.rot_C; p.scale = q.scale;
        p.nbatch = q.nbatch; p.sA = q.stride_a; p.sW = q.stride_w; p.sO = q.stride_o;
    }
    g.n = n;
    return launch_gemm(g, (hipStream_t)stream);
}
void dr_debug_attention_config(int flash_min_workgroups) { attention_force_flash_min(flash_min_workgroups); }
void dr_debug_attention_split(int on) { attention_force_split(on); }
int dr_debug_attention_last_form(void) { return attention_last_form(); }
int dr_debug_procrustes_last_form(void) { return procrustes_last_form(); }
int dr_debug_pgemm_acc_forms(int clear) { return pgemm_acc_forms(clear != 0); }
void dr_debug_fps_force_streaming(int on) { fps_force_streaming(on); }

/* diagnostics for the per-kernel edge tests: one launch of a row / state kernel of the loops; every check stands in front of the launch */
int dr_debug_layernorm_f32(int rows, int C, const float* x, int ldx, const float* gamma, const float* beta, const float* res, int ldres,
                           int postadd, float* out, int ldo, float* rowmax, void* stream) {
    if (rows < 0 || C < 1 || !x || !gamma || !beta || !out || ldx < C || ldo < C || (res && ldres < C)) return DR_EINVAL;
    if (postadd && (!res || rowmax)) return DR_EINVAL;
    if (C > 1024) return DR_ENOSUP;
    if (postadd) return launch_layernorm_postadd(x, ldx, gamma, beta, res, ldres, out, ldo, rows, C, (hipStream_t)stream);
    return launch_layernorm(x, ldx, gamma, beta, res, ldres, out, ldo, rows, C, (hipStream_t)stream, rowmax);
}

int dr_debug_fourier_f32(int D, int P, int rows_per_pair, const float* pts, const float* R, const float* t, int L, float* emb, int ldo,
                         float* warped_ws, void* stream) {
    if ((D != 2 && D != 3) || P < 0 || rows_per_pair < 0 || !pts || !emb || L < 0 || L > 30 || ldo < (2 * L + 1) * D) return DR_EINVAL;
    if (D == 3 && (!warped_ws || (R == nullptr) != (t == nullptr))) return DR_EINVAL;
    if ((long long)P * rows_per_pair * ldo > 0x7fffffffLL) return DR_ENOSUP;       // the kernels index rows * ldo in 32 bits
    if (P == 0 || rows_per_pair == 0) return DR_OK;
    if (D == 3) return launch_fourier3d(pts, P, rows_per_pair, R, t, L, emb, ldo, warped_ws, (hipStream_t)stream);
    return launch_fourier2d(pts, P * rows_per_pair, L, emb, ldo, (hipStream_t)stream);
}

size_t dr_debug_pair_min_scratch_bytes(int P) { return pair_min_scratch_bytes(P); }

int dr_debug_pair_min_f64(int P, int N, int M, const double* x, const uint8_t* src_mask, const uint8_t* tgt_mask, double* out, void* scratch,
                          void* stream) {
    if (P < 0 || N < 1 || M < 1 || !x || !out || (src_mask == nullptr) != (tgt_mask == nullptr)) return DR_EINVAL;
    if ((long long)N * M > 0x7fffffffLL) return DR_ENOSUP;
    return launch_pair_min(x, P, N * M, out, (hipStream_t)stream, M, src_mask, tgt_mask, scratch);
}

int dr_debug_ddim_f64(const dr_debug_ddim_args* a, int P, void* stream) {
    if (!a || P < 0 || a->N < 1 || a->M < 1 || !a->x || !a->x0 || (a->src_mask == nullptr) != (a->tgt_mask == nullptr)) return DR_EINVAL;
    if ((long long)a->N * a->M > 0x7fffffffLL) return DR_ENOSUP;
    DdimArgs d;
    d.x = a->x; d.x0 = a->x0; d.shift = a->shift; d.noise = a->noise; d.src_mask = a->src_mask; d.tgt_mask = a->tgt_mask;
    d.N = a->N; d.M = a->M; d.first_step = a->first_step; d.sra = a->sra; d.srm1 = a->srm1; d.c = a->c; d.sigma = a->sigma; d.sqrt_an = a->sqrt_an;
    return launch_ddim(d, P, (hipStream_t)stream);
}

int dr_debug_state_map(int kind, const void* in, void* out, long long n, void* stream) {
    if (kind < 0 || kind > 2 || n < 0 || (n > 0 && (!in || !out))) return DR_EINVAL;
    if (kind == 0) return launch_f32_to_f64((const float*)in, (double*)out, (size_t)n, (hipStream_t)stream);
    if (kind == 1) return launch_f64_to_f32((const double*)in, (float*)out, (size_t)n, (hipStream_t)stream);
    return launch_sigmoid((const double*)in, (double*)out, (size_t)n, (hipStream_t)stream);
}

int dr_vol_pe_f32(int rows, int rows_per_pair, int C, const float* xyz, const float* R, const float* t, float origin_x,
                  float origin_y, float origin_z, float voxel, const float* freq, float* cos_out, float* sin_out,
                  void* stream) {
    if (rows < 0 || C <= 0 || !xyz || !freq || !cos_out || !sin_out || rows_per_pair < 1) return DR_EINVAL;
    if ((R == nullptr) != (t == nullptr)) return DR_EINVAL;
    return launch_vol_pe(xyz, rows, rows_per_pair, R, t, C, origin_x, origin_y, origin_z, voxel, freq, cos_out, sin_out,
                         (hipStream_t)stream);
}

int dr_linear_f32(int rows, int ncols, int K, const float* x, const float* W, float* out, int epilogue, const float* cos_t,
                  const float* sin_t, int rot_C, float scale, void* stream) {
    if (rows < 0 || ncols <= 0 || K <= 0 || !x || !W || !out) return DR_EINVAL;
    if ((epilogue & EPI_ROTARY) && (!cos_t || !sin_t || rot_C <= 0 || (rot_C & 1))) return DR_EINVAL;
    return gemm1(x, K, W, nullptr, out, ncols, rows, ncols, K, epilogue, scale, nullptr, (hipStream_t)stream, cos_t, sin_t, rot_C);
}

int dr_gemm_nt_batched_f32(int nbatch, int rows, int ncols, int K, const float* A, long long stride_a, const float* W, long long stride_w, float* out,
                           long long stride_o, float scale, void* stream) {
    if (nbatch < 0 || rows < 0 || ncols <= 0 || K <= 0 || (K & 3) || !A || !W || !out) return DR_EINVAL;
    if (nbatch == 0 || rows == 0) return DR_OK;
    return gemm1(A, K, W, nullptr, out, ncols, rows, ncols, K, EPI_NONE, scale, nullptr, (hipStream_t)stream, nullptr, nullptr, 0, nbatch, stride_a,
                 stride_w, stride_o);
}

int dr_linear_ex_f32(int rows, int ncols, int K, const float* x, int lda, const float* W, const float* bias, float* out, int ldo,
                     int epilogue, float scale, void* stream) {
    if (rows < 0 || ncols <= 0 || K <= 0 || !x || !W || !out || lda < K || ldo < ncols || (epilogue & EPI_ROTARY)) return DR_EINVAL;
    return gemm1(x, lda, W, bias, out, ldo, rows, ncols, K, epilogue, scale, nullptr, (hipStream_t)stream);
}

size_t dr_procrustes_workspace_bytes(int P, int N, int M) {
    return (P < 1 || N < 1 || M < 1) ? 0 : procrustes_workspace_bytes(P, N, M);
}

int dr_procrustes_f32(int P, int N, int M, const float* conf, const float* src_pcd, const float* tgt_pcd,
                      const uint8_t* src_mask, const uint8_t* tgt_mask, int use_mask_len, float sample_rate,
                      float max_condition_num, float* R, float* t, float* R_forwd, float* t_forwd, double* condition,
                      int32_t* solution_mask, int32_t* topk_idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || N < 1 || M < 1 || !conf || !src_pcd || !tgt_pcd || !R || !t || !R_forwd || !t_forwd || !condition || !solution_mask)
        return DR_EINVAL;
    if (P == 0) return DR_OK;
    // tiles beyond 256 x 256 select with the whole chip: the caller's scratch (header contract: the caller owns every buffer)
    const size_t wsb = procrustes_workspace_bytes(P, N, M);
    if (wsb && (!workspace || workspace_bytes < wsb)) return DR_EWORKSPACE;
    return launch_procrustes(conf, src_pcd, tgt_pcd, src_mask, tgt_mask, P, N, M, use_mask_len, sample_rate, max_condition_num,
                             R, t, R_forwd, t_forwd, condition, solution_mask, topk_idx, (hipStream_t)stream, wsb ? workspace : nullptr, wsb);
}

size_t dr_top1_union_workspace_bytes(int P, int N, int M, int elem_bytes) {
    return (P < 1 || N < 1 || M < 1 || (elem_bytes != 4 && elem_bytes != 8)) ? 0 : top1_union_workspace_bytes(P, N, M, (size_t)elem_bytes);
}

}  // extern "C"
template <typename T>
static int top1_union_entry(const T* conf, int P, int N, int M, int64_t* matches, int32_t* count, void* ws, size_t ws_bytes, hipStream_t st) {
    if (P < 0 || N < 1 || M < 1 || !conf || !matches || !count) return DR_EINVAL;
    if (P == 0) return DR_OK;
    const size_t wsb = top1_union_workspace_bytes(P, N, M, sizeof(T));
    if (wsb && (!ws || ws_bytes < wsb)) return DR_EWORKSPACE;
    return launch_top1_union<T>(conf, P, N, M, (long long*)matches, count, st, nullptr, nullptr, wsb ? ws : nullptr, wsb);
}
extern "C" {
int dr_top1_union_f64(int P, int N, int M, const double* conf, int64_t* matches, int32_t* count, void* workspace, size_t workspace_bytes,
                      void* stream) {
    return top1_union_entry<double>(conf, P, N, M, matches, count, workspace, workspace_bytes, (hipStream_t)stream);
}
int dr_top1_union_f32(int P, int N, int M, const float* conf, int64_t* matches, int32_t* count, void* workspace, size_t workspace_bytes,
                      void* stream) {
    return top1_union_entry<float>(conf, P, N, M, matches, count, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
