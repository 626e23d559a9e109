// vit_check_common.h -- what the host checks of the two ViT encoders share (tools/vit_index_check.cpp, tools/vit_f32_index_check.cpp): the walk of
// the patch gather (csrc/vit_index.h's map, one for both precisions) and of the workspace carve (csrc/vit_forward.h's, with the element size).
// Each program defines CHECK (it names the program in its message) and g_slots before including this.
#pragma once
#include <cstdint>
#include <vector>

#include "vit_forward.h"

// every (patch, k) of an image with elements of type T, on real allocations of exactly the documented sizes (AddressSanitizer guards their ends):
// in-image offsets are a bijection onto the image and follow the definition, pad columns are -1, every row element is written
template <typename T>
static void check_patches(int H, int W, int p) {
    using namespace dr;
    const int Np = (H / p) * (W / p), Kp = vit_patch_kp(p);
    CHECK(Kp % 32 == 0 && Kp >= 3 * p * p && Kp - 3 * p * p < 32);
    std::vector<T> img((size_t)3 * H * W, (T)1), rows((size_t)Np * Kp, (T)7);
    std::vector<unsigned char> seen(img.size(), 0);
    for (int patch = 0; patch < Np; ++patch)
        for (int k = 0; k < Kp; ++k) {
            const long long s = vit_patch_src(H, W, p, patch, k);
            if (k >= 3 * p * p) CHECK(s == -1);
            else {
                CHECK(s >= 0 && s < (long long)img.size() && !seen[s]);
                seen[s] = 1;
                // the definition: Conv2d weight [D, 3, p, p] flattened, patch row-major
                const int c = k / (p * p), dy = (k / p) % p, dx = k % p, py = patch / (W / p), px = patch % (W / p);
                CHECK(s == ((long long)c * H + py * p + dy) * W + px * p + dx);
            }
            rows.data()[(size_t)patch * Kp + k] = s < 0 ? (T)0 : img.data()[s];
            ++g_slots;
        }
    for (unsigned char v : seen) CHECK(v);
}

// the carve's regions are disjoint, aligned and inside the total; the total is what the size query reports
static void check_carve(int H, int W, int p, int D, int Dh, size_t elem) {
    using namespace dr;
    const int Np = (H / p) * (W / p), L = Np + 1, Kp = vit_patch_kp(p);
    const VitCarve c = vit_carve(L, D, Dh, Np, Kp, elem);
    CHECK(c.total == vit_workspace_bytes(H, W, p, D, Dh, elem));
    const size_t off[5] = {c.xn, c.qkv, c.ao, c.hid, c.patches};
    const size_t len[5] = {(size_t)L * D * elem, (size_t)L * 3 * D * elem, (size_t)L * D * elem, (size_t)L * Dh * elem, (size_t)Np * Kp * elem};
    for (int i = 0; i < 5; ++i) {
        CHECK(off[i] % 256 == 0 && off[i] + len[i] <= c.total);
        if (i) CHECK(off[i] >= off[i - 1] + len[i - 1]);
    }
    std::vector<unsigned char> ws(c.total, 0);
    for (int i = 0; i < 5; ++i) ws.data()[off[i]] = ws.data()[off[i] + len[i] - 1] = 1;
}
