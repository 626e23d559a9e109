// vit_schedule_check.cpp -- host check of csrc/vit_forward.h, the one schedule both ViT encoders run.  Build and run:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/vit_schedule_check.cpp -o /tmp/vit_schedule_check && /tmp/vit_schedule_check
//
// vit_forward<P> is instantiated with a policy that records every step instead of launching it, for operand sizes 2 (fp16 structs, raw takes) and
// 4 (float32 structs, normed takes), on the smallest geometry that has every step: a 28 x 42 image, p = 14 (6 patches, L = 7), D = 64, one head,
// Dh = 128, two blocks, takes [0, 1].  The recorded list must be exactly the schedule written out below -- kind, M / K / N, mode, column scale,
// operands, in order; every workspace operand starts at the carve region of its name and ends inside it; the regions are disjoint and the carve
// total is what the size query reports.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "vit_forward.h"

using namespace dr;

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            std::fprintf(stderr, "vit_schedule_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

struct Op {
    std::string kind;
    int M, K, N, mode, cs_cols;
    float cs;
    const void *a, *w, *out, *bias, *gamma, *addend;
};
static std::vector<Op> g_ops;
enum { COLSCALE = 10, GELU = 11, SCALE_RESID = 12, ADDEND = 13 };

template <int E>
struct Rec {
    typedef typename std::conditional<E == 2, dr_vit_config_f16, dr_vit_config_f32>::type config;
    typedef typename std::conditional<E == 2, dr_vit_block_f16, dr_vit_block_f32>::type block;
    enum { ELEM = E, COLSCALE = ::COLSCALE, GELU = ::GELU, SCALE_RESID = ::SCALE_RESID, ADDEND = ::ADDEND };
    static int img_f32(const dr_vit_config_f16& c) { return c.img_f32; }
    static int img_f32(const dr_vit_config_f32&) { return 1; }
    static int norm_take(const dr_vit_config_f16&) { return 0; }
    static int norm_take(const dr_vit_config_f32& c) { return c.norm_take; }
    static bool aligned(const config&) { return true; }
    static bool aligned(const block&) { return true; }
    static bool take_aligned(const void*) { return true; }
    static int rec(Op o) { g_ops.push_back(o); return DR_OK; }
    static int patch_rows(int H, int W, int p, const void* img, int f32, void* out, int ldo, void*) { return rec({"patch", H, W, p, f32, ldo, 0.f, img, 0, out, 0, 0, 0}); }
    static int cls_row(int D, const float* cls, const float* pos, float* x, void*) { return rec({"cls", D, 0, 0, 0, 0, 0.f, cls, pos, x, 0, 0, 0}); }
    static int gemm(const void* a, int lda, int M, int K, int N, const void* w, const float* bias, int mode, void* out, int ldo, float cs, int cs_cols,
                    const float* gamma, const float* addend, int ld_addend, void*) {
        CHECK(lda == K && ldo == N && ld_addend == (addend ? N : 0));      // every row buffer of the schedule is dense
        return rec({"gemm", M, K, N, mode, cs_cols, cs, a, w, out, bias, gamma, addend});
    }
    static int layernorm(int L, int D, const float* x, const float* g, const float* b, float eps, void* out, void*) {
        CHECK(eps == 1e-6f);
        return rec({"ln", L, D, 0, 0, 0, 0.f, x, g, out, b, 0, 0});
    }
    static int attention(int L, int heads, int D, const void* qkv, void* ao, void*) { return rec({"attn", L, heads, D, 0, 0, 0.f, qkv, 0, ao, 0, 0, 0}); }
    static int copy_rows(void* dst, const void* src, size_t bytes, void*) { return rec({"copy", (int)bytes, 0, 0, 0, 0, 0.f, src, 0, dst, 0, 0, 0}); }
};

template <int E>
static void check() {
    typedef Rec<E> P;
    const int H = 28, W = 42, p = 14, D = 64, Dh = 128, Np = 6, L = 7, Kp = 608, depth = 2;
    static float pool[4096];                                        // distinct caller pointers, never read
    int next = 0;
    auto fresh = [&]() { return pool + 16 * next++; };
    const VitCarve cv = vit_carve(L, D, Dh, Np, Kp, E);
    CHECK(cv.total == vit_workspace_bytes(H, W, p, D, Dh, E) && Kp == vit_patch_kp(p));
    std::vector<char> ws(cv.total);
    const size_t off[6] = {cv.xn, cv.qkv, cv.ao, cv.hid, cv.patches, cv.total};
    const size_t len[5] = {(size_t)L * D * E, (size_t)L * 3 * D * E, (size_t)L * D * E, (size_t)L * Dh * E, (size_t)Np * Kp * E};
    for (int i = 0; i < 5; ++i) CHECK(off[i] % 256 == 0 && off[i] + len[i] <= off[i + 1]);      // disjoint, in order, inside the total
    char *xn = ws.data() + cv.xn, *qkv = ws.data() + cv.qkv, *ao = ws.data() + cv.ao, *hid = ws.data() + cv.hid, *patches = ws.data() + cv.patches;

    typename P::block blk[depth];
    for (auto& b : blk)
        b = {fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh(), fresh()};
    float *x = fresh(), *take_out[2] = {fresh(), fresh()};
    const int take[2] = {0, 1};
    typename P::config c = {};
    c.H = H; c.W = W; c.p = p; c.D = D; c.heads = 1; c.Dh = Dh; c.depth = depth; c.eps = 1e-6f;
    c.img = fresh(); c.patch_w = fresh(); c.patch_b = fresh(); c.cls = fresh(); c.pos = fresh(); c.blocks = blk; c.norm_g = fresh(); c.norm_b = fresh();
    c.x_prenorm = x; c.x_norm = fresh(); c.n_take = 2; c.take = take; c.take_out = take_out; c.workspace = ws.data(); c.workspace_bytes = cv.total;
    if constexpr (E == 4) c.norm_take = 1;
    const void* x_norm = c.x_norm;

    g_ops.clear();
    CHECK(vit_forward<P>(c, nullptr) == DR_OK);
    std::vector<Op> want = {
        {"patch", H, W, p, E == 4, Kp, 0.f, c.img, 0, patches, 0, 0, 0},
        {"cls", D, 0, 0, 0, 0, 0.f, c.cls, c.pos, x, 0, 0, 0},
        {"gemm", Np, Kp, D, ADDEND, 0, 1.f, patches, c.patch_w, x + D, c.patch_b, 0, c.pos + D},
    };
    for (int i = 0; i < depth; ++i) {
        const auto& b = blk[i];
        want.push_back({"ln", L, D, 0, 0, 0, 0.f, x, b.norm1_g, xn, b.norm1_b, 0, 0});
        want.push_back({"gemm", L, D, 3 * D, COLSCALE, D, 0.125f, xn, b.qkv_w, qkv, b.qkv_b, 0, 0});
        want.push_back({"attn", L, 1, D, 0, 0, 0.f, qkv, 0, ao, 0, 0, 0});
        want.push_back({"gemm", L, D, D, SCALE_RESID, 0, 1.f, ao, b.proj_w, x, b.proj_b, b.ls1, 0});
        want.push_back({"ln", L, D, 0, 0, 0, 0.f, x, b.norm2_g, xn, b.norm2_b, 0, 0});
        want.push_back({"gemm", L, D, Dh, GELU, 0, 1.f, xn, b.fc1_w, hid, b.fc1_b, 0, 0});
        want.push_back({"gemm", L, Dh, D, SCALE_RESID, 0, 1.f, hid, b.fc2_w, x, b.fc2_b, b.ls2, 0});
        if (E == 4) want.push_back({"ln", L, D, 0, 0, 0, 0.f, x, c.norm_g, take_out[i], c.norm_b, 0, 0});
        else want.push_back({"copy", L * D * 4, 0, 0, 0, 0, 0.f, x, 0, take_out[i], 0, 0, 0});
    }
    want.push_back({"ln", L, D, 0, 0, 0, 0.f, x, c.norm_g, x_norm, c.norm_b, 0, 0});
    CHECK(g_ops.size() == want.size());
    for (size_t i = 0; i < want.size(); ++i) {
        const Op &g = g_ops[i], &w = want[i];
        CHECK(g.kind == w.kind && g.M == w.M && g.K == w.K && g.N == w.N && g.mode == w.mode && g.cs_cols == w.cs_cols && g.cs == w.cs);
        CHECK(g.a == w.a && g.w == w.w && g.out == w.out && g.bias == w.bias && g.gamma == w.gamma && g.addend == w.addend);
        // a GEMM's workspace operands end inside their regions: [M, K] read, [M, N] written, E bytes each
        if (g.kind != "gemm") continue;
        for (int r = 0; r < 5; ++r) {
            if (g.a == ws.data() + off[r]) CHECK((size_t)g.M * g.K * E <= len[r]);
            if (g.out == ws.data() + off[r]) CHECK((size_t)g.M * g.N * E <= len[r]);
        }
    }
    // a refusal records nothing: one byte less of workspace
    g_ops.clear();
    c.workspace_bytes = cv.total - 1;
    CHECK(vit_forward<P>(c, nullptr) == DR_EINVAL && g_ops.empty());
}

int main() {
    check<2>();
    check<4>();
    std::printf("vit_schedule_check: ok\n");
    return 0;
}
