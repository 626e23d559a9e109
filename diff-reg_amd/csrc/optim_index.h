// optim_index.h -- every index the optimizer kernels (optim.hip: dr_grads_finite_multi_f32, dr_sgd_step_multi_f32, dr_adam_step_multi_f32)
// compute, stated once for the device and for the host check (tools/optim_index_check.cpp): how a set of tensors is cut into launches of at
// most OPT_CAP tensors, how a workgroup of a launch finds its (tensor, chunk), and how a lane's slot of a chunk splits into the 16-byte aligned
// body and the ragged head and tail.  The kernels form no address any other way.  Outside hipcc the file compiles as plain C++.
//
// A tensor is `numel` float32 values behind pointers that need only 4-byte alignment.  Let s = (address / 4) mod 4 be the pointer's distance in
// floats from the 16-byte boundary below it, and number the floats from that boundary: element e is u = s + e.  The u axis is cut into chunks of
// OPT_CHUNK floats, one workgroup each; a chunk into OPT_UNROLL rounds of OPT_BLOCK lanes; a lane's slot of a round is the four floats
// u0 .. u0 + 3 with u0 a multiple of 4.  A slot that lies wholly inside [s, s + numel) is one 16-byte access, aligned by construction; the slot
// that holds the tensor's first or last element may be partly outside and is accessed float by float; a slot outside is skipped.  When the
// pointers of one tensor (param, grad, states) do NOT share s, no common cut makes all of them aligned: that tensor is walked with s = 0 and
// every slot float by float (OptTensorMap::vec == 0).  torch's allocator hands out 512-byte aligned blocks, so this is the path of views only.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <stddef.h>
#include <stdint.h>

namespace dr {

constexpr int OPT_BLOCK = 256;                                   // lanes per workgroup
constexpr int OPT_VEC = 4;                                       // floats per slot (one 16-byte access)
constexpr int OPT_UNROLL = 4;                                    // rounds per chunk: 4 x 16 B in flight per lane and array
constexpr int OPT_CHUNK = OPT_BLOCK * OPT_VEC * OPT_UNROLL;      // 4096 floats (16 KiB per array) per workgroup
constexpr int OPT_CAP = 64;                                      // tensors per launch: 64 x (40 + 8) B + 65 x 4 B + 4 B = 3336 B of the 4 KiB argument block

// a tensor of the set as it crosses the ABI (dr_optim_tensor of include/diffreg_hip.h has the same layout)
struct OptTensor {
    float* param;
    float* grad;
    float* state0;
    float* state1;
    size_t numel;
};

// how one tensor is walked: s (see above), vec = 1 when whole slots are 16-byte accesses
struct OptTensorMap {
    unsigned s;
    int vec;
};

// the argument block of one launch: n tensors, first[t] = chunks of the tensors before t (first[n] = the grid)
struct OptLaunch {
    OptTensor t[OPT_CAP];
    OptTensorMap m[OPT_CAP];
    uint32_t first[OPT_CAP + 1];
    int n;
};

__host__ __device__ inline unsigned opt_misalign(const void* p) { return (unsigned)(((uintptr_t)p >> 2) & 3u); }
__host__ __device__ inline bool opt_float_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// the walk of a tensor whose listed pointers are all touched (NULL = not touched)
__host__ __device__ inline OptTensorMap opt_tensor_map(const void* a, const void* b, const void* c, const void* d) {
    const void* p[4] = {a, b, c, d};
    OptTensorMap m = {0u, 1};
    bool have = false;
    for (int i = 0; i < 4; ++i) {
        if (!p[i]) continue;
        const unsigned s = opt_misalign(p[i]);
        if (!have) {
            m.s = s;
            have = true;
        } else if (s != m.s) {
            m.s = 0u;
            m.vec = 0;
            return m;
        }
    }
    return m;
}

// chunks a tensor occupies (0 for an empty one)
__host__ __device__ inline unsigned long long opt_chunks(size_t numel, unsigned s) {
    return numel == 0 ? 0ull : ((unsigned long long)numel + s + OPT_CHUNK - 1) / OPT_CHUNK;
}

// workgroup b of a launch -> tensor t with first[t] <= b < first[t + 1] (empty tensors have first[t] == first[t + 1] and are never returned);
// b < first[n] is the caller's.  Every operand is uniform over the workgroup: the loads of `first` are scalar loads.
__host__ __device__ inline int opt_find_tensor(const uint32_t* first, int n, uint32_t b) {
    int lo = 0, hi = n;                      // invariant: first[lo] <= b < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// lane `lane`'s slot of round `round` of chunk `chunk`: elements [e0, e0 + count) of the tensor, count in 0 .. 4.
// whole: count == 4 and every pointer of the tensor + e0 is 16-byte aligned (one vector access); otherwise `count` scalar accesses
struct OptSlot {
    size_t e0;
    int count;
    bool whole;
};
__host__ __device__ inline OptSlot opt_slot(size_t numel, OptTensorMap m, unsigned long long chunk, int round, int lane) {
    const unsigned long long u0 = chunk * OPT_CHUNK + ((unsigned long long)round * OPT_BLOCK + (unsigned)lane) * OPT_VEC;
    const unsigned long long lo_t = m.s, hi_t = (unsigned long long)m.s + numel;
    const unsigned long long lo = u0 > lo_t ? u0 : lo_t, hi = u0 + OPT_VEC < hi_t ? u0 + OPT_VEC : hi_t;
    OptSlot r;
    if (hi <= lo) {
        r.e0 = 0;
        r.count = 0;
        r.whole = false;
        return r;
    }
    r.e0 = (size_t)(lo - lo_t);
    r.count = (int)(hi - lo);
    r.whole = m.vec != 0 && r.count == OPT_VEC;
    return r;
}

// the only address formation of the kernels: element e of a tensor's array
template <typename T>
__host__ __device__ inline T* opt_at(T* base, size_t e) { return base + e; }

// ---- host side: cutting a set into launches --------------------------------------------------------------------------------------------
// Appends tensor `t` (walked as `m`) to launch `L`.  false: the launch is full (OPT_CAP tensors, or its grid would pass 2^31 - 1) and must be
// sent first; a tensor that does not fit an EMPTY launch has more than 2^31 - 1 chunks and is not supported.
inline bool opt_launch_push(OptLaunch& L, const OptTensor& t, OptTensorMap m) {
    if (L.n == 0) L.first[0] = 0;
    if (L.n >= OPT_CAP) return false;
    const unsigned long long g = (unsigned long long)L.first[L.n] + opt_chunks(t.numel, m.s);
    if (g > 0x7fffffffull) return false;
    L.t[L.n] = t;
    L.m[L.n] = m;
    L.first[L.n + 1] = (uint32_t)g;
    ++L.n;
    return true;
}

// which pointers of a descriptor an entry touches (the others are not looked at and travel as NULL)
enum OptNeeds { OPT_NEED_GRAD = 1, OPT_NEED_PARAM = 2, OPT_NEED_S0 = 4, OPT_NEED_S1 = 8 };
constexpr int OPT_OK = 0, OPT_ENOSUP = -3;      // DR_OK, DR_ENOSUP of include/diffreg_hip.h

// Cuts the set into launches and sends each with `launch(L)` (-> OPT_OK or an error, which ends the walk).  Empty tensors are left out.  A tensor
// of more than 2^31 - 1 chunks (beyond any device memory) is OPT_ENOSUP before the first launch.
template <typename F>
inline int opt_for_each_launch(const OptTensor* ts, size_t count, int needs, F launch) {
    for (size_t i = 0; i < count; ++i)
        if (opt_chunks(ts[i].numel, 3u) > 0x7fffffffull) return OPT_ENOSUP;
    OptLaunch L;
    L.n = 0;
    for (size_t i = 0; i < count; ++i) {
        const OptTensor& d = ts[i];
        if (d.numel == 0) continue;
        const OptTensor t = {(needs & OPT_NEED_PARAM) ? d.param : nullptr, (needs & OPT_NEED_GRAD) ? d.grad : nullptr,
                             (needs & OPT_NEED_S0) ? d.state0 : nullptr, (needs & OPT_NEED_S1) ? d.state1 : nullptr, d.numel};
        const OptTensorMap m = opt_tensor_map(t.param, t.grad, t.state0, t.state1);
        if (!opt_launch_push(L, t, m)) {
            const int rc = launch(L);
            if (rc != OPT_OK) return rc;
            L.n = 0;
            if (!opt_launch_push(L, t, m)) return OPT_ENOSUP;
        }
    }
    return L.n > 0 ? launch(L) : OPT_OK;
}

}  // namespace dr
