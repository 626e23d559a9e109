// vit_forward.h -- the ViT encoder forward both precisions run (dr_vit_forward_f16 of vit.hip, dr_vit_forward_f32 of vit_f32.hip): the geometry
// check, the workspace carve, the validation order and the launch schedule, each stated once.  What differs between the precisions comes in
// through a policy struct P that each .hip file defines next to its kernels ("the policy"):
//   P::config, P::block         the public config and block structs (their field names match; the code below reads b.qkv_w etc. directly)
//   P::ELEM                     bytes of a GEMM operand element: the workspace rows xn, qkv, ao, hid and patches have this type
//   P::COLSCALE, GELU, SCALE_RESID, ADDEND   the rows GEMM's four epilogue modes under that precision's names
//   P::img_f32(c), P::norm_take(c)   the two flags (fp32: the image is always float32; fp16: a take is never normed here)
//   P::aligned(c), P::aligned(block), P::take_aligned(ptr)   the pointer alignments that precision demands, and no others
//   P::patch_rows, cls_row, gemm, layernorm, attention, copy_rows   check and launch one step on `stream`; layernorm writes rows of the
//                               operand type (into xn, a normed take and x_norm alike)
// No HIP type in here: plain C++, the stream is a void*.  tools/vit_schedule_check.cpp instantiates vit_forward with a recording policy on the host.
#pragma once
#include <stddef.h>

#include "../../include/diffreg_hip.h"
#include "carve.h"               // align256
#include "vit_index.h"

namespace dr {

inline bool vit_dims_ok(int H, int W, int p, int D, int Dh) {
    return p >= 1 && p <= 64 && H >= p && W >= p && H % p == 0 && W % p == 0 && D >= 64 && D % 64 == 0 && Dh >= 32 && Dh % 32 == 0 &&
           (long long)H * W < (1ll << 26) && (long long)((H / p) * (W / p) + 1) * (Dh > 3 * D ? Dh : 3 * D) < (1ll << 31);
}

// ---- the workspace: rows of `elem` bytes per element -----------------------------------------------------------------------------------------
struct VitCarve {
    size_t xn, qkv, ao, hid, patches, total;      // byte offsets (256-byte aligned) and the total
};
inline VitCarve vit_carve(int L, int D, int Dh, int Np, int Kp, size_t elem) {
    VitCarve c;
    size_t o = 0;
    c.xn = o; o = align256(o + (size_t)L * D * elem);
    c.qkv = o; o = align256(o + (size_t)L * 3 * D * elem);
    c.ao = o; o = align256(o + (size_t)L * D * elem);
    c.hid = o; o = align256(o + (size_t)L * Dh * elem);
    c.patches = o; o = align256(o + (size_t)Np * Kp * elem);
    c.total = o;
    return c;
}
// both size queries: 0 outside the domain
inline size_t vit_workspace_bytes(int H, int W, int p, int D, int Dh, size_t elem) {
    if (!vit_dims_ok(H, W, p, D, Dh)) return 0;
    const int Np = (H / p) * (W / p);
    return vit_carve(Np + 1, D, Dh, Np, vit_patch_kp(p), elem).total;
}

// ---- the forward -----------------------------------------------------------------------------------------------------------------------------
template <class P>
int vit_forward(const typename P::config& c, void* stream) {
    if (!vit_dims_ok(c.H, c.W, c.p, c.D, c.Dh)) return DR_EINVAL;
    const int D = c.D, Dh = c.Dh, heads = c.heads, img_f32 = P::img_f32(c), norm_take = P::norm_take(c);
    if (heads < 1 || heads * 64 != D || c.depth < 0 || (c.depth && !c.blocks) || !(c.eps >= 0.f) || (img_f32 != 0 && img_f32 != 1) ||
        (norm_take != 0 && norm_take != 1))
        return DR_EINVAL;
    if (!c.img || !c.patch_w || !c.cls || !c.pos || !c.x_prenorm || !c.x_norm || !c.workspace) return DR_EINVAL;
    if (!P::aligned(c)) return DR_EINVAL;
    if (c.n_take < 0 || (c.n_take && (!c.take || !c.take_out))) return DR_EINVAL;
    for (int i = 0; i < c.n_take; ++i)
        if (c.take[i] < 0 || c.take[i] >= c.depth || !c.take_out[i] || !P::take_aligned(c.take_out[i])) return DR_EINVAL;
    for (int i = 0; i < c.depth; ++i) {
        const typename P::block& b = c.blocks[i];
        if (!b.qkv_w || !b.proj_w || !b.fc1_w || !b.fc2_w || !P::aligned(b)) return DR_EINVAL;
    }
    const int Np = (c.H / c.p) * (c.W / c.p), L = Np + 1, Kp = vit_patch_kp(c.p);
    const VitCarve cv = vit_carve(L, D, Dh, Np, Kp, P::ELEM);      // the one carve the size query reports
    if (c.workspace_bytes < cv.total) return DR_EINVAL;
    char* ws = (char*)c.workspace;
    void *xn = ws + cv.xn, *qkv = ws + cv.qkv, *ao = ws + cv.ao, *hid = ws + cv.hid, *patches = ws + cv.patches;
    float* x = c.x_prenorm;                                        // the fp32 residual stream lives in the x_prenorm output

    // patch_embed.py:69-82 and dinov2.py:187-196 (the hub's vision_transformer.py:212-219): tokens = [cls; conv(x)] + pos
    int rc = P::patch_rows(c.H, c.W, c.p, c.img, img_f32, patches, Kp, stream);
    if (rc == DR_OK) rc = P::cls_row(D, c.cls, c.pos, x, stream);
    if (rc == DR_OK) rc = P::gemm(patches, Kp, Np, Kp, D, c.patch_w, c.patch_b, P::ADDEND, x + D, D, 1.f, 0, nullptr, c.pos + D, D, stream);
    if (rc != DR_OK) return rc;
    for (int i = 0; i < c.depth; ++i) {
        const typename P::block& b = c.blocks[i];
        // block.py:83-84, attention.py:49-62: x += ls1(proj(softmax(q d^-0.5 k^T) v)); q takes d^-0.5 = 1 / 8 in the qkv GEMM's epilogue
        rc = P::layernorm(L, D, x, b.norm1_g, b.norm1_b, c.eps, xn, stream);
        if (rc == DR_OK) rc = P::gemm(xn, D, L, D, 3 * D, b.qkv_w, b.qkv_b, P::COLSCALE, qkv, 3 * D, 0.125f, D, nullptr, nullptr, 0, stream);
        if (rc == DR_OK) rc = P::attention(L, heads, D, qkv, ao, stream);
        if (rc == DR_OK) rc = P::gemm(ao, D, L, D, D, b.proj_w, b.proj_b, P::SCALE_RESID, x, D, 1.f, 0, b.ls1, nullptr, 0, stream);
        // block.py:86-87: x += ls2(fc2(gelu(fc1(norm2(x)))))
        if (rc == DR_OK) rc = P::layernorm(L, D, x, b.norm2_g, b.norm2_b, c.eps, xn, stream);
        if (rc == DR_OK) rc = P::gemm(xn, D, L, D, Dh, b.fc1_w, b.fc1_b, P::GELU, hid, Dh, 1.f, 0, nullptr, nullptr, 0, stream);
        if (rc == DR_OK) rc = P::gemm(hid, Dh, L, Dh, D, b.fc2_w, b.fc2_b, P::SCALE_RESID, x, D, 1.f, 0, b.ls2, nullptr, 0, stream);
        // vision_transformer.py:271-281, :309-310: the stream after a taken block, through the final norm when norm_take is set
        for (int k = 0; k < c.n_take && rc == DR_OK; ++k) {
            if (c.take[k] != i) continue;
            rc = norm_take ? P::layernorm(L, D, x, c.norm_g, c.norm_b, c.eps, c.take_out[k], stream)
                           : P::copy_rows(c.take_out[k], x, (size_t)L * D * 4, stream);
        }
        if (rc != DR_OK) return rc;
    }
    return P::layernorm(L, D, x, c.norm_g, c.norm_b, c.eps, c.x_norm, stream);
}

}  // namespace dr
