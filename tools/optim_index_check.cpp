// optim_index_check.cpp -- host check of csrc/optim_index.h, the only place dr_grads_finite_multi_f32, dr_sgd_step_multi_f32 and
// dr_adam_step_multi_f32 compute an index.  Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/optim_index_check.cpp \
//         -o /tmp/optim_index_check && /tmp/optim_index_check
//
// It walks sets as the entries and the kernels do -- opt_for_each_launch cuts the set, every workgroup of a launch's grid finds its (tensor,
// chunk), every lane of every round takes its slot -- over
//   * single tensors of every numel in 0 .. 2 OPT_CHUNK + 5 with every combination of (param, grad, state) starting 0 .. 3 floats behind a
//     16-byte boundary (64 combinations each; the gradient-only walk of the finite sweep on each of the 4 gradient offsets),
//   * sets of 1, OPT_CAP - 1, OPT_CAP, OPT_CAP + 1 and 3 OPT_CAP + 2 tensors of mixed sizes and offsets, empty tensors among them.
// Every array is a real allocation of exactly offset + numel floats on a 16-byte boundary (AddressSanitizer guards its end), every access the
// kernels would make is made, and the walk asserts: every element of every tensor is assigned to exactly one (launch, workgroup, round, lane)
// slot; no slot reaches outside its tensor; every access issued as a vector is 16-byte aligned on EVERY pointer of the tensor; tensors whose
// pointers share their offset are walked in vectors except for at most one ragged slot at either end; the launches hold at most OPT_CAP tensors
// and are as few as that allows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "optim_index.h"

using namespace dr;

static long long g_slots = 0, g_vec = 0, g_launches = 0;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "optim_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

// `off` floats behind a 16-byte boundary, exactly off + n floats long
struct Buf {
    float* raw = nullptr;
    float* p = nullptr;
    Buf(size_t n, unsigned off) {
        void* q = nullptr;
        CHECK(posix_memalign(&q, 16, (n + off) * sizeof(float) + (n + off == 0 ? 16 : 0)) == 0);
        raw = (float*)q;
        std::memset((void*)raw, 0, (n + off) * sizeof(float));
        p = raw + off;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : raw(o.raw), p(o.p) { o.raw = o.p = nullptr; }
    ~Buf() { std::free(raw); }
};

static bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// one entry's walk of a set: every array in `needs` counts the visits of each of its elements in place
static int walk(const std::vector<OptTensor>& set, int needs) {
    int launches = 0;
    size_t nonempty = 0;
    for (const OptTensor& t : set) nonempty += t.numel != 0;
    const int rc = opt_for_each_launch(set.data(), set.size(), needs, [&](const OptLaunch& L) {
        ++launches;
        CHECK(L.n >= 1 && L.n <= OPT_CAP && L.first[0] == 0 && L.first[L.n] >= 1 && L.first[L.n] <= 0x7fffffffu);
        for (uint32_t b = 0; b < L.first[L.n]; ++b) {
            const int t = opt_find_tensor(L.first, L.n, b);
            CHECK(t >= 0 && t < L.n && L.first[t] <= b && b < L.first[t + 1]);
            const unsigned long long chunk = b - L.first[t];
            const OptTensor& T = L.t[t];
            const OptTensorMap m = L.m[t];
            CHECK(chunk < opt_chunks(T.numel, m.s));
            float* arr[4] = {T.param, T.grad, T.state0, T.state1};
            int ragged = 0;
            for (int r = 0; r < OPT_UNROLL; ++r)
                for (int lane = 0; lane < OPT_BLOCK; ++lane) {
                    const OptSlot s = opt_slot(T.numel, m, chunk, r, lane);
                    CHECK(s.count >= 0 && s.count <= OPT_VEC);
                    if (s.count == 0) continue;
                    ++g_slots;
                    CHECK(s.e0 < T.numel && s.e0 + (size_t)s.count <= T.numel);
                    if (s.whole) ++g_vec;
                    else ++ragged;
                    for (int a = 0; a < 4; ++a) {
                        if (!arr[a]) continue;
                        if (s.whole) {
                            CHECK(s.count == OPT_VEC && al16(opt_at(arr[a], s.e0)));
                            float v[4];
                            std::memcpy(v, opt_at(arr[a], s.e0), 16);                   // the 16-byte load
                            for (int k = 0; k < 4; ++k) v[k] += 1.f;
                            std::memcpy(opt_at(arr[a], s.e0), v, 16);                   // the 16-byte store
                        } else {
                            for (int k = 0; k < s.count; ++k) *opt_at(arr[a], s.e0 + k) += 1.f;
                        }
                    }
                }
            // pointers that share their offset: vectors except for the slot of the tensor's first and of its last element
            if (m.vec) CHECK(ragged <= 2);
        }
        return OPT_OK;
    });
    CHECK(rc == OPT_OK);
    CHECK((size_t)launches == (nonempty + OPT_CAP - 1) / OPT_CAP);
    g_launches += launches;
    // exactly one visit per element of every array the entry touches, none of the others
    for (const OptTensor& T : set) {
        float* arr[4] = {T.param, T.grad, T.state0, T.state1};
        const int bit[4] = {OPT_NEED_PARAM, OPT_NEED_GRAD, OPT_NEED_S0, OPT_NEED_S1};
        for (int a = 0; a < 4; ++a) {
            if (!arr[a]) continue;
            const float want = (needs & bit[a]) ? 1.f : 0.f;
            for (size_t e = 0; e < T.numel; ++e) {
                CHECK(arr[a][e] == want);
                arr[a][e] = 0.f;
            }
        }
    }
    return launches;
}

int main() {
    const int SGD = OPT_NEED_GRAD | OPT_NEED_PARAM | OPT_NEED_S0, ADAM = SGD | OPT_NEED_S1, GATE = OPT_NEED_GRAD, PLAIN = OPT_NEED_GRAD | OPT_NEED_PARAM;
    // single tensors: every numel, every (param, grad, state) offset
    for (size_t n = 0; n <= 2 * (size_t)OPT_CHUNK + 5; ++n) {
        std::vector<Buf> P, G, S;
        for (unsigned o = 0; o < 4; ++o) {
            P.emplace_back(n, o);
            G.emplace_back(n, o);
            S.emplace_back(n, o);
        }
        for (unsigned op = 0; op < 4; ++op)
            for (unsigned og = 0; og < 4; ++og)
                for (unsigned os = 0; os < 4; ++os) {
                    const std::vector<OptTensor> set = {{P[op].p, G[og].p, S[os].p, nullptr, n}};
                    walk(set, SGD);
                    if (os == 0) walk(set, PLAIN);                 // momentum == 0: the state is not looked at
                    if (os == 0 && op == 0) walk(set, GATE);       // the finite sweep: the gradient alone, always in vectors
                }
        CHECK(opt_chunks(n, 0) == (n + OPT_CHUNK - 1) / OPT_CHUNK);
    }
    // the maps at the alignment rules
    CHECK(opt_tensor_map((void*)16, (void*)32, nullptr, (void*)48).vec == 1 && opt_tensor_map((void*)20, (void*)36, (void*)4, nullptr).s == 1);
    CHECK(opt_tensor_map((void*)20, (void*)32, nullptr, nullptr).vec == 0 && opt_tensor_map((void*)20, (void*)32, nullptr, nullptr).s == 0);
    CHECK(opt_tensor_map(nullptr, (void*)28, nullptr, nullptr).s == 3 && opt_tensor_map(nullptr, (void*)28, nullptr, nullptr).vec == 1);
    // sets of mixed sizes and offsets
    const size_t sizes[] = {7, 0, 1, 3, 4, 5, OPT_CHUNK - 1, OPT_CHUNK, OPT_CHUNK + 1, 2 * OPT_CHUNK + 3, 0, 130, 4093, 64};
    const int NS = (int)(sizeof(sizes) / sizeof(sizes[0]));
    const int counts[] = {1, OPT_CAP - 1, OPT_CAP, OPT_CAP + 1, 3 * OPT_CAP + 2};
    for (int c : counts)
        for (int shift = 0; shift < 3; ++shift) {
            std::vector<Buf> bufs;
            std::vector<OptTensor> set;
            bufs.reserve((size_t)c * 4);
            for (int i = 0; i < c; ++i) {
                const size_t n = sizes[(i + shift) % NS];
                // shift 0: torch's case, everything on 16 bytes; 1: a common offset per tensor; 2: offsets that differ inside a tensor
                const unsigned o0 = shift == 0 ? 0u : (unsigned)(i % 4), o1 = shift == 2 ? (unsigned)((i / 4 + 1) % 4) : o0;
                bufs.emplace_back(n, o0);
                bufs.emplace_back(n, o1);
                bufs.emplace_back(n, o0);
                bufs.emplace_back(n, shift == 2 ? (unsigned)((i / 2) % 4) : o0);
                const size_t k = bufs.size() - 4;
                set.push_back({bufs[k].p, bufs[k + 1].p, bufs[k + 2].p, bufs[k + 3].p, n});
            }
            walk(set, ADAM);
            walk(set, SGD);
            walk(set, GATE);
        }
    // an empty set and a set of empty tensors launch nothing
    CHECK(walk({}, ADAM) == 0);
    CHECK(walk({{nullptr, nullptr, nullptr, nullptr, 0}, {nullptr, nullptr, nullptr, nullptr, 0}}, ADAM) == 0);
    // a launch closes before its grid passes 2^31 - 1, and a tensor beyond it is refused before any launch (nothing is dereferenced here)
    {
        OptLaunch L;
        L.n = 0;
        const OptTensor big = {nullptr, nullptr, nullptr, nullptr, (size_t)0x7fffffffull * OPT_CHUNK - 3};
        const OptTensorMap m0 = {0u, 1};
        CHECK(opt_launch_push(L, big, m0) && L.first[1] == 0x7fffffffu);
        const OptTensor one = {nullptr, nullptr, nullptr, nullptr, 1};
        CHECK(!opt_launch_push(L, one, m0));
        const OptTensor too_big = {nullptr, nullptr, nullptr, nullptr, (size_t)0x7fffffffull * OPT_CHUNK + 1};
        int sent = 0;
        CHECK(opt_for_each_launch(&too_big, 1, GATE, [&](const OptLaunch&) { ++sent; return OPT_OK; }) == OPT_ENOSUP && sent == 0);
    }
    std::printf("optim_index_check ok: %lld slots walked (%lld as 16-byte vectors) in %lld launches\n", g_slots, g_vec, g_launches);
    return 0;
}
