// optim.hip -- the closing leg of a training iteration on the device (twelfth set after ABI 0.7.0):
//   dr_grads_finite_multi_f32   validate_gradient(model)                         3D/lib/utils.py:96-106 (called at lib/trainer.py:195-201)
//                               check_gradients                                  2D-3D vision3d/engine/base_trainer.py:311-325
//   dr_sgd_step_multi_f32       optimizer.step() of torch.optim.SGD              3D/main.py:90-96, lib/trainer.py:197-199
//   dr_adam_step_multi_f32      optimizer.step() of torch.optim.Adam / AdamW     3D/main.py:97-103; vision3d/utils/optimizer.py:134-141,
//                                                                                vision3d/engine/base_trainer.py:253-254
//   dr_optim_finish             the bookkeeping of `if gradient_valid: step()`   lib/trainer.py:196-201
// A parameter set is a HOST array of descriptors {param, grad, state0, state1, numel}; the entries copy it by value into the argument blocks of
// their launches (OPT_CAP tensors each), so nothing of the caller's host memory is read after the call returns, no device table exists and no
// pinned buffer has a lifetime.  Every entry is asynchronous on the given stream, reads nothing back, allocates nothing, and uses no atomic
// but the integer OR of the finite sweep's flags: two runs are bit-equal, and the sequence can be captured on one stream.
//
// Every index below comes from optim_index.h (walked on the host by tools/optim_index_check.cpp): a workgroup finds its (tensor, chunk) by a
// binary search of the launch's chunk prefix sums with uniform loads of its own argument block, and a lane's slot is either one aligned 16-byte
// access or up to four 4-byte ones.  A chunk is OPT_UNROLL rounds: all loads of a chunk are issued before the first is used.
#include "common.h"
#include "optim_index.h"
#include "../../include/diffreg_hip.h"

// The float32 updates restate torch's single-tensor statements operation by operation.  Each torch statement is one elementwise kernel of its
// own, and inside such a kernel `self + alpha * other` is one fused multiply-add; so is it here, written out (fmaf), and nothing else is fused.
#pragma clang fp contract(off)

namespace dr {

static_assert(sizeof(OptTensor) == sizeof(dr_optim_tensor), "dr_optim_tensor is the descriptor of optim_index.h");
static_assert(OPT_OK == DR_OK && OPT_ENOSUP == DR_ENOSUP, "optim_index.h returns the library's status codes");
static_assert(sizeof(OptLaunch) + 128 <= 4096, "a launch's argument block fits the 4 KiB of kernel arguments");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// streaming accesses: the optimizer states are read and written once per step and by nothing else
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4_nt(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4_nt(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }

// the workgroup's tensor and chunk; false behind the launch's last chunk (never: the grid is first[n])
__device__ __forceinline__ bool opt_locate(const OptLaunch& L, int& t, unsigned long long& chunk) {
    const uint32_t b = blockIdx.x;
    if (b >= L.first[L.n]) return false;
    t = opt_find_tensor(L.first, L.n, b);
    chunk = b - L.first[t];
    return true;
}

// ------------------------------------------------------------------------------------------------------------
// the finite sweep: bit 0 NaN, bit 1 +Inf, bit 2 -Inf
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int finite_flags(float x) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7f800000u) != 0x7f800000u) return 0;
    return (b & 0x007fffffu) ? DR_GRAD_NAN : ((b >> 31) ? DR_GRAD_NEG_INF : DR_GRAD_POS_INF);
}

__global__ __launch_bounds__(OPT_BLOCK) void grads_finite_kernel(OptLaunch L, int* __restrict__ word) {
    int t;
    unsigned long long chunk;
    if (!opt_locate(L, t, chunk)) return;
    const float* g = L.t[t].grad;
    const size_t numel = L.t[t].numel;
    const OptTensorMap m = L.m[t];
    const int lane = threadIdx.x;
    int flags = 0;
    OptSlot sl[OPT_UNROLL];
    f32x4 v[OPT_UNROLL];
#pragma unroll
    for (int r = 0; r < OPT_UNROLL; ++r) {
        sl[r] = opt_slot(numel, m, chunk, r, lane);
        v[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (sl[r].whole) v[r] = ld4(opt_at(g, sl[r].e0));
        else
#pragma unroll
            for (int k = 0; k < OPT_VEC; ++k)
                if (k < sl[r].count) v[r][k] = *opt_at(g, sl[r].e0 + k);
    }
#pragma unroll
    for (int r = 0; r < OPT_UNROLL; ++r)
        flags |= finite_flags(v[r][0]) | finite_flags(v[r][1]) | finite_flags(v[r][2]) | finite_flags(v[r][3]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) flags |= __shfl_xor(flags, s);
    if (lane_id() == 0 && flags) atomicOr(word, flags);
}

// ------------------------------------------------------------------------------------------------------------
// the updates.  An update is a functor over one element: apply(p, g, s0, s1) in torch's order of operations.
// ------------------------------------------------------------------------------------------------------------
struct SgdK {
    float lr, wd, momentum, one_minus_damp;
    int nesterov, maximize, zero_grads, has_momentum;
};

struct SgdOp {
    float neg_lr, wd, momentum, omd;
    bool nesterov, maximize, has_mom, first;
    static constexpr int STATES = 1;
    __device__ __forceinline__ bool uses(int s) const { return s == 0 && has_mom; }
    __device__ __forceinline__ void apply(float& p, float g, float& b, float&) const {
        if (maximize) g = -g;
        if (wd != 0.f) g = fmaf(wd, p, g);                         // grad.add(param, alpha=weight_decay)
        if (has_mom) {
            if (first) b = g;                                      // torch.clone(grad)
            else {
                b = b * momentum;                                  // buf.mul_(momentum)
                b = fmaf(omd, g, b);                               //    .add_(grad, alpha=1 - dampening)
            }
            g = nesterov ? fmaf(momentum, b, g) : b;               // grad.add(buf, alpha=momentum) | buf
        }
        p = fmaf(neg_lr, g, p);                                    // param.add_(grad, alpha=-lr)
    }
};

struct AdamK {
    double lr, beta1, beta2, eps, wd;
    int decoupled, maximize, zero_grads;
};

struct AdamOp {
    float wd, decay_mul, w1, one_minus_w1, beta2, omb2, inv_bc2_sqrt, eps, neg_step_size;
    bool decoupled, maximize;
    static constexpr int STATES = 2;
    __device__ __forceinline__ bool uses(int) const { return true; }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v) const {
        if (maximize) g = -g;
        if (wd != 0.f) {
            if (decoupled) p = p * decay_mul;                      // param.mul_(1 - lr * weight_decay)
            else g = fmaf(wd, p, g);                               // grad.add(param, alpha=weight_decay)
        }
        const float d = g - m;                                     // exp_avg.lerp_(grad, 1 - beta1)
        m = w1 < 0.5f ? fmaf(w1, d, m) : fmaf(-d, one_minus_w1, g);
        v = v * beta2;                                             // exp_avg_sq.mul_(beta2)
        v = fmaf(omb2, g * g, v);                                  //    .addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(v) * inv_bc2_sqrt + eps;         // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps): a division by a
                                                                   // host scalar is a multiplication by its float32 reciprocal in torch
        p = fmaf(neg_step_size, m / denom, p);                     // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
};

// beta^n in double by squaring (n >= 1): the bias corrections come from the DEVICE step counter, which the host cannot know
__device__ __forceinline__ double pow_int(double b, int n) {
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

template <typename Op>
__device__ __forceinline__ void update_chunk(const OptLaunch& L, const Op& op, bool gated_off, bool zero_grads) {
    int t;
    unsigned long long chunk;
    if (!opt_locate(L, t, chunk)) return;
    float* P = L.t[t].param;
    float* G = L.t[t].grad;
    float* S0 = L.t[t].state0;
    float* S1 = L.t[t].state1;
    const size_t numel = L.t[t].numel;
    const OptTensorMap m = L.m[t];
    const int lane = threadIdx.x;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    OptSlot sl[OPT_UNROLL];
#pragma unroll
    for (int r = 0; r < OPT_UNROLL; ++r) sl[r] = opt_slot(numel, m, chunk, r, lane);
    if (gated_off) {                       // a non-finite gradient somewhere in the set: nothing is written but the zeroed gradients
        if (!zero_grads) return;
#pragma unroll
        for (int r = 0; r < OPT_UNROLL; ++r) {
            if (sl[r].whole) st4(opt_at(G, sl[r].e0), zero);
            else
#pragma unroll
                for (int k = 0; k < OPT_VEC; ++k)
                    if (k < sl[r].count) *opt_at(G, sl[r].e0 + k) = 0.f;
        }
        return;
    }
    const bool u0 = op.uses(0), u1 = Op::STATES > 1 && op.uses(1);
    f32x4 p[OPT_UNROLL], g[OPT_UNROLL], a[OPT_UNROLL], b[OPT_UNROLL];
#pragma unroll
    for (int r = 0; r < OPT_UNROLL; ++r) {
        p[r] = g[r] = a[r] = b[r] = zero;
        if (sl[r].whole) {
            const size_t e = sl[r].e0;
            g[r] = ld4_nt(opt_at(G, e));
            p[r] = ld4(opt_at(P, e));
            if (u0) a[r] = ld4_nt(opt_at(S0, e));
            if (u1) b[r] = ld4_nt(opt_at(S1, e));
        } else {
#pragma unroll
            for (int k = 0; k < OPT_VEC; ++k) {
                if (k >= sl[r].count) continue;
                const size_t e = sl[r].e0 + k;
                g[r][k] = *opt_at(G, e);
                p[r][k] = *opt_at(P, e);
                if (u0) a[r][k] = *opt_at(S0, e);
                if (u1) b[r][k] = *opt_at(S1, e);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < OPT_UNROLL; ++r) {
#pragma unroll
        for (int k = 0; k < OPT_VEC; ++k) {
            float pk = p[r][k], ak = a[r][k], bk = b[r][k];
            op.apply(pk, g[r][k], ak, bk);
            p[r][k] = pk; a[r][k] = ak; b[r][k] = bk;
        }
        if (sl[r].whole) {
            const size_t e = sl[r].e0;
            st4(opt_at(P, e), p[r]);
            if (u0) st4_nt(opt_at(S0, e), a[r]);
            if (u1) st4_nt(opt_at(S1, e), b[r]);
            if (zero_grads) st4(opt_at(G, e), zero);
        } else {
#pragma unroll
            for (int k = 0; k < OPT_VEC; ++k) {
                if (k >= sl[r].count) continue;
                const size_t e = sl[r].e0 + k;
                *opt_at(P, e) = p[r][k];
                if (u0) *opt_at(S0, e) = a[r][k];
                if (u1) *opt_at(S1, e) = b[r][k];
                if (zero_grads) *opt_at(G, e) = 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(OPT_BLOCK) void sgd_step_kernel(OptLaunch L, SgdK K, const int* __restrict__ word, const int* __restrict__ step) {
    SgdOp op;
    op.neg_lr = -K.lr; op.wd = K.wd; op.momentum = K.momentum; op.omd = K.one_minus_damp;
    op.nesterov = K.nesterov != 0; op.maximize = K.maximize != 0; op.has_mom = K.has_momentum != 0;
    op.first = *step == 0;
    update_chunk(L, op, *word != 0, K.zero_grads != 0);
}

__global__ __launch_bounds__(OPT_BLOCK) void adam_step_kernel(OptLaunch L, AdamK K, const int* __restrict__ word, const int* __restrict__ step) {
    const int n = *step + 1;                                       // step_t += 1
    const double bc1 = 1.0 - pow_int(K.beta1, n), bc2 = 1.0 - pow_int(K.beta2, n);
    AdamOp op;
    op.wd = (float)K.wd;
    op.decay_mul = (float)(1.0 - K.lr * K.wd);
    op.w1 = (float)(1.0 - K.beta1);
    op.one_minus_w1 = 1.f - op.w1;
    op.beta2 = (float)K.beta2;
    op.omb2 = (float)(1.0 - K.beta2);
    op.inv_bc2_sqrt = 1.f / (float)sqrt(bc2);                      // bias_correction2 ** 0.5, rounded to float32, then its reciprocal
    op.eps = (float)K.eps;
    op.neg_step_size = (float)(-(K.lr / bc1));                     // step_size = lr / bias_correction1
    op.decoupled = K.decoupled != 0; op.maximize = K.maximize != 0;
    update_chunk(L, op, *word != 0, K.zero_grads != 0);
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_finish_kernel(int* word, int* step, int* skipped, float* mirror, size_t n_mirror) {
    __shared__ int s_step;
    if (threadIdx.x == 0) {
        int n = *step;
        if (*word == 0) *step = ++n;
        else if (skipped) *skipped = *skipped + 1;
        *word = 0;
        s_step = n;
    }
    __syncthreads();
    const float f = (float)s_step;
    for (size_t i = threadIdx.x; i < n_mirror; i += OPT_BLOCK) *opt_at(mirror, i) = f;
}

static int validate_set(const dr_optim_tensor* ts, size_t count, int needs) {
    if (count > 0 && !ts) return DR_EINVAL;
    for (size_t i = 0; i < count; ++i) {
        const dr_optim_tensor& d = ts[i];
        if (d.numel == 0) continue;
        const void* ptrs[4] = {d.grad, d.param, d.state0, d.state1};
        for (int k = 0; k < 4; ++k)
            if ((needs & (1 << k)) && (!ptrs[k] || !opt_float_aligned(ptrs[k]))) return DR_EINVAL;
    }
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_grads_finite_multi_f32(const dr_optim_tensor* tensors, size_t count, int32_t* status_word, void* stream) {
    if (!status_word || !opt_float_aligned(status_word)) return DR_EINVAL;
    const int rc = validate_set(tensors, count, OPT_NEED_GRAD);
    if (rc != DR_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return opt_for_each_launch(reinterpret_cast<const OptTensor*>(tensors), count, OPT_NEED_GRAD, [&](const OptLaunch& L) {
        hipLaunchKernelGGL(grads_finite_kernel, dim3(L.first[L.n]), dim3(OPT_BLOCK), 0, st, L, status_word);
        DR_LAUNCH_CHECK();
        return DR_OK;
    });
}

int dr_sgd_step_multi_f32(const dr_optim_tensor* tensors, size_t count, const dr_sgd_options* o, const int32_t* status_word,
                          const int32_t* step_counter, void* stream) {
    if (!o || !status_word || !step_counter || !opt_float_aligned(status_word) || !opt_float_aligned(step_counter)) return DR_EINVAL;
    // torch.optim.SGD's own argument checks
    if (!(o->lr >= 0.0) || !(o->momentum >= 0.0) || !(o->weight_decay >= 0.0)) return DR_EINVAL;
    if (o->nesterov && (o->momentum <= 0.0 || o->dampening != 0.0)) return DR_EINVAL;
    const int has_mom = o->momentum != 0.0;
    const int needs = OPT_NEED_GRAD | OPT_NEED_PARAM | (has_mom ? OPT_NEED_S0 : 0);
    const int rc = validate_set(tensors, count, needs);
    if (rc != DR_OK) return rc;
    const SgdK K = {(float)o->lr, (float)o->weight_decay, (float)o->momentum, (float)(1.0 - o->dampening),
                    o->nesterov, o->maximize, o->zero_grads, has_mom};
    hipStream_t st = (hipStream_t)stream;
    return opt_for_each_launch(reinterpret_cast<const OptTensor*>(tensors), count, needs, [&](const OptLaunch& L) {
        hipLaunchKernelGGL(sgd_step_kernel, dim3(L.first[L.n]), dim3(OPT_BLOCK), 0, st, L, K, status_word, step_counter);
        DR_LAUNCH_CHECK();
        return DR_OK;
    });
}

int dr_adam_step_multi_f32(const dr_optim_tensor* tensors, size_t count, const dr_adam_options* o, const int32_t* status_word,
                           const int32_t* step_counter, void* stream) {
    if (!o || !status_word || !step_counter || !opt_float_aligned(status_word) || !opt_float_aligned(step_counter)) return DR_EINVAL;
    // torch.optim.Adam's own argument checks
    if (!(o->lr >= 0.0) || !(o->eps >= 0.0) || !(o->weight_decay >= 0.0)) return DR_EINVAL;
    if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return DR_EINVAL;
    const int needs = OPT_NEED_GRAD | OPT_NEED_PARAM | OPT_NEED_S0 | OPT_NEED_S1;
    const int rc = validate_set(tensors, count, needs);
    if (rc != DR_OK) return rc;
    const AdamK K = {o->lr, o->beta1, o->beta2, o->eps, o->weight_decay, o->decoupled, o->maximize, o->zero_grads};
    hipStream_t st = (hipStream_t)stream;
    return opt_for_each_launch(reinterpret_cast<const OptTensor*>(tensors), count, needs, [&](const OptLaunch& L) {
        hipLaunchKernelGGL(adam_step_kernel, dim3(L.first[L.n]), dim3(OPT_BLOCK), 0, st, L, K, status_word, step_counter);
        DR_LAUNCH_CHECK();
        return DR_OK;
    });
}

int dr_optim_finish(int32_t* status_word, int32_t* step_counter, int32_t* skipped_counter, float* step_mirror, size_t n_mirror, void* stream) {
    if (!status_word || !step_counter || !opt_float_aligned(status_word) || !opt_float_aligned(step_counter) ||
        !opt_float_aligned(skipped_counter) || (n_mirror > 0 && (!step_mirror || !opt_float_aligned(step_mirror))))
        return DR_EINVAL;
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(OPT_BLOCK), 0, (hipStream_t)stream, status_word, step_counter, skipped_counter,
                       step_mirror, n_mirror);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
