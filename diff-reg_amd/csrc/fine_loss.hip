// fine_loss.hip -- FineMatchingLoss.forward behind its random_choice (Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1/loss.py:175,
// 186-213) and its backward: the M <= 1024 selected correspondences give an M x M problem on C <= 256 channels.
//   rows = the selected pixels (img_points / img_feats at v * image_w + u), columns = the selected points (pcd_points under `transform`,
//   pcd_pixels, pcd_feats); dist3d / dist2d = float32 norms of differences (pairwise_distance(strict=True)); positives: both under their radius,
//   negatives: either above its radius; fdist = clamp(x^2 - 2 x y + y^2, 0) (squared, normalized=False); the unweighted circle loss
//   (vision3d/loss/circle_loss.py:11-52: an entry outside a mask keeps the logit 0 and counts in the log-sum-exp); get_recall (loss.py:146-155).
// A latency problem, not a bandwidth one: nothing M x M ever reaches memory.  A workgroup owns FL_AN anchors -- rows in grid.y = 0, columns in
// grid.y = 1: the problem is the same with the two sides exchanged -- keeps their feature rows, and the geometry of every partner, in LDS and
// streams the partners' feature rows through a 64 x 64 LDS tile (a lane per partner, the anchor's channel broadcast).  Forward: that kernel
// (online log-sum-exp per anchor, row arg-min) and a one-workgroup kernel for the means, the recall and the anchors' gradient coefficients.
// Backward: the same sweep recomputes each entry, forms d loss / d fdist from the saved row AND column statistics and contracts it against the
// partner tile once more (grad x_i = 2 (x_i sum_j g_ij - sum_j g_ij y_j)); a last kernel adds the compact rows of equal pixel / point indices
// in selection order into the zero-filled dense gradients.  Dot products, logits, log-sum-exps and means in double (M^2 C is 8 M multiply-adds at
// the configuration's size: the float32 rounding of fdist would move a logit by 24 * 2.6 * 2e-7 ~ 1e-5, the bar the gradients are held to);
// every sum in one fixed order, no atomics: two runs are bit-identical.  This departs ON PURPOSE from circle_loss.hip, whose logits are the
// reference's float32 arithmetic: the device's fdist is not the float32 reference's to the last bit, so a clamp decision at fdist = 0 exactly (two
// identical feature rows) can differ from a float32 run; the mask decisions are float32 as the reference's.
#include <limits.h>
#include "train_common.h"

namespace dr {
namespace {

constexpr int FL_AN = 8;          // anchors per workgroup: two per wave
constexpr int FL_PT = 64;         // partners per tile: one per lane
constexpr int FL_CH = 64;         // channels per tile
constexpr int FL_MAXM = 1024;
constexpr int FL_MAXC = 256;

struct FineArgs {
    float pr3, nr3, pr2, nr2, pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale;
    int image_w;
};

struct FineIn {
    const float *img_points, *img_feats, *pcd_points, *pcd_pixels, *pcd_feats, *transform;
    const int64_t *sel_pixels, *sel_idx;
    int HW, N, M, C;
};

// the dense row a selection addresses on `side` (0: pixels, 1: points); -1 outside the tensor (the reference raises there)
__device__ __forceinline__ int sel_row(const FineIn& in, int image_w, int side, int m) {
    if (side == 0) {
        const int64_t v = in.sel_pixels[2 * m], u = in.sel_pixels[2 * m + 1];
        const int64_t r = v * image_w + u;
        return (v >= 0 && u >= 0 && u < image_w && r < in.HW) ? (int)r : -1;
    }
    const int64_t r = in.sel_idx[m];
    return (r >= 0 && r < in.N) ? (int)r : -1;
}

// g[0..2] = the 3-D point (a point of the cloud under `transform`: p R^T + t in float32), g[3..4] = the pixel (v, u)
__device__ __forceinline__ int sel_geometry(const FineIn& in, int image_w, int side, int m, float* g) {
    const int r = sel_row(in, image_w, side, m);
    g[0] = g[1] = g[2] = g[3] = g[4] = 0.f;
    if (r < 0) return r;
    if (side == 0) {
        g[0] = in.img_points[3 * (size_t)r]; g[1] = in.img_points[3 * (size_t)r + 1]; g[2] = in.img_points[3 * (size_t)r + 2];
        g[3] = (float)in.sel_pixels[2 * m]; g[4] = (float)in.sel_pixels[2 * m + 1];
    } else {
        const float x = in.pcd_points[3 * (size_t)r], y = in.pcd_points[3 * (size_t)r + 1], z = in.pcd_points[3 * (size_t)r + 2];
        const float* T = in.transform;
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = fmaf(z, T[4 * i + 2], fmaf(y, T[4 * i + 1], x * T[4 * i])) + T[4 * i + 3];
        g[3] = in.pcd_pixels[2 * (size_t)r]; g[4] = in.pcd_pixels[2 * (size_t)r + 1];
    }
    return r;
}

struct Pair { double A, B, pw, nw, fd; bool pos, neg, pass; };
__device__ __forceinline__ Pair pair_eval(double x2, double y2, double dot, const float* ga, const float* gb, const FineArgs& a) {
    Pair p;
    const double raw = x2 - 2.0 * dot + y2;
    p.pass = raw >= 0.0;                                      // clamp(min = 0) lets the gradient through where its input is >= 0
    p.fd = p.pass ? raw : 0.0;
    const float dx = ga[0] - gb[0], dy = ga[1] - gb[1], dz = ga[2] - gb[2], dv = ga[3] - gb[3], du = ga[4] - gb[4];
    const float d3 = sqrtf(dx * dx + dy * dy + dz * dz), d2 = sqrtf(dv * dv + du * du);
    p.pos = d3 < a.pr3 && d2 < a.pr2;
    p.neg = d3 > a.nr3 || d2 > a.nr2;
    p.pw = fmax(0.0, (p.fd - (p.pos ? 0.0 : 1e5)) - (double)a.pos_optimal);
    p.nw = fmax(0.0, (double)a.neg_optimal - (p.fd + (p.neg ? 0.0 : 1e5)));
    p.A = (double)a.log_scale * (p.fd - (double)a.pos_margin) * p.pw;
    p.B = (double)a.log_scale * ((double)a.neg_margin - p.fd) * p.nw;
    return p;
}

struct FineLds {
    float A[FL_AN][FL_MAXC];       // the anchors' feature rows
    float T[FL_PT][FL_CH + 1];     // one tile of partner rows
    float G[FL_MAXM][5];           // every partner's geometry
    int row[FL_MAXM];              // ... and dense row
    float AG[FL_AN][5];
    int arow[FL_AN];
    double x2[FL_AN];
};

// geometry of all partners and of this workgroup's anchors, the anchors' feature rows and squared norms
__device__ void fine_prologue(const FineIn& in, const FineArgs& a, int mode, int a0, FineLds& s) {
    const int tid = threadIdx.x, M = in.M, C = in.C;
    for (int m = tid; m < M; m += 256) s.row[m] = sel_geometry(in, a.image_w, 1 - mode, m, s.G[m]);
    if (tid < FL_AN) s.arow[tid] = (a0 + tid < M) ? sel_geometry(in, a.image_w, mode, a0 + tid, s.AG[tid]) : -1;
    __syncthreads();
    const float* F = mode == 0 ? in.img_feats : in.pcd_feats;
    for (int e = tid; e < FL_AN * C; e += 256) {
        const int q = e / C, c = e - q * C, r = s.arow[q];
        s.A[q][c] = r >= 0 ? F[(size_t)r * C + c] : 0.f;
    }
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        double v = 0.0;
        for (int c = lane; c < C; c += 64) v += (double)s.A[2 * w + q][c] * (double)s.A[2 * w + q][c];
        v = wave_sum(v);
        if (lane == 0) s.x2[2 * w + q] = v;
    }
    __syncthreads();
}

// partner rows [p0, p0 + 64) x channels [c0, c0 + 64) -> s.T (zeros outside the problem)
__device__ __forceinline__ void fine_load_tile(const FineIn& in, int mode, int p0, int c0, FineLds& s) {
    const float* F = mode == 0 ? in.pcd_feats : in.img_feats;
    for (int e = threadIdx.x; e < FL_PT * FL_CH; e += 256) {
        const int r = e >> 6, c = e & 63, pm = p0 + r;
        const int row = pm < in.M ? s.row[pm] : -1;
        s.T[r][c] = (row >= 0 && c0 + c < in.C) ? F[(size_t)row * in.C + c0 + c] : 0.f;
    }
}

// this lane's partner against the wave's two anchors: dot products and the partner's squared norm, in double
__device__ __forceinline__ void fine_dots(const FineIn& in, int mode, int p0, FineLds& s, double* dot, double& y2) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    dot[0] = dot[1] = 0.0; y2 = 0.0;
    for (int c0 = 0; c0 < in.C; c0 += FL_CH) {
        __syncthreads();
        fine_load_tile(in, mode, p0, c0, s);
        __syncthreads();
        const int cn = min(FL_CH, in.C - c0);
        for (int c = 0; c < cn; ++c) {
            const double y = (double)s.T[lane][c];
            dot[0] = fma((double)s.A[2 * w][c0 + c], y, dot[0]);
            dot[1] = fma((double)s.A[2 * w + 1][c0 + c], y, dot[1]);
            y2 = fma(y, y, y2);
        }
    }
}

// la / lb [2][M]: log-sum-exp of the positive / negative logits of each row (index 0) and column (1); flags [2][M]: bit 0 = an anchor (holds a
// positive and a negative); rows only: bit 1 = holds a positive, bit 2 = the row's arg-min of fdist (first minimum) is a positive
__global__ __launch_bounds__(256) void fine_stats_kernel(FineIn in, FineArgs a, double* __restrict__ la, double* __restrict__ lb,
                                                         int* __restrict__ flags) {
    __shared__ FineLds s;
    const int mode = blockIdx.y, a0 = blockIdx.x * FL_AN, M = in.M;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    fine_prologue(in, a, mode, a0, s);
    double mA[2] = {-INFINITY, -INFINITY}, sA[2] = {0.0, 0.0}, mB[2] = {-INFINITY, -INFINITY}, sB[2] = {0.0, 0.0};
    double minv[2] = {INFINITY, INFINITY};
    int mini[2] = {INT_MAX, INT_MAX}, f[2] = {0, 0};
    for (int p0 = 0; p0 < M; p0 += FL_PT) {
        double dot[2], y2;
        fine_dots(in, mode, p0, s, dot, y2);
        const int b = p0 + lane;
        if (b < M) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const Pair p = pair_eval(s.x2[2 * w + q], y2, dot[q], s.AG[2 * w + q], s.G[b], a);
                if (p.A > mA[q]) { sA[q] = sA[q] * exp(mA[q] - p.A) + 1.0; mA[q] = p.A; } else sA[q] += exp(p.A - mA[q]);
                if (p.B > mB[q]) { sB[q] = sB[q] * exp(mB[q] - p.B) + 1.0; mB[q] = p.B; } else sB[q] += exp(p.B - mB[q]);
                f[q] |= (p.pos ? 1 : 0) | (p.neg ? 2 : 0);
                if (p.fd < minv[q]) { minv[q] = p.fd; mini[q] = b; f[q] = (f[q] & 3) | (p.pos ? 4 : 0); }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int m = a0 + 2 * w + q;                                      // (uniform in the wave)
        const double MA = wave_max(mA[q]), MB = wave_max(mB[q]);
        const double SA = wave_sum(sA[q] > 0.0 ? sA[q] * exp(mA[q] - MA) : 0.0), SB = wave_sum(sB[q] > 0.0 ? sB[q] * exp(mB[q] - MB) : 0.0);
        const int any = wave_max(f[q] & 1) | (wave_max((f[q] >> 1) & 1) << 1);
        const double wmin = wave_min(minv[q]);
        const int widx = wave_min(minv[q] == wmin ? mini[q] : INT_MAX);
        const int hit = wave_max((minv[q] == wmin && mini[q] == widx) ? ((f[q] >> 2) & 1) : 0);
        if (lane == 0 && m < M) {
            la[mode * M + m] = MA + log(SA);
            lb[mode * M + m] = MB + log(SB);
            flags[mode * M + m] = (any == 3 ? 1 : 0) | ((any & 1) ? 2 : 0) | (hit ? 4 : 0);
        }
    }
}

__device__ __forceinline__ double softplus20(double x) { return x > 20.0 ? x : log1p(exp(x)); }   // F.softplus(beta = 1, threshold = 20)
__device__ __forceinline__ double softplus20_grad(double x) { if (x > 20.0) return 1.0; const double z = exp(x); return z / (z + 1.0); }

__device__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// out[0] = (mean over the anchor rows of softplus(la + lb) / ls + the same over the anchor columns) / 2 (an empty set: 0 / 0 = NaN, torch's mean of
// an empty selection); out[1] = the recall; coef [2][M]: 0.5 / |anchors| softplus'(la + lb) of an anchor, 0 elsewhere (and everywhere when a set is
// empty on its side)
__global__ __launch_bounds__(256) void fine_final_kernel(int M, float log_scale, const double* __restrict__ la, const double* __restrict__ lb,
                                                         const int* __restrict__ flags, double* __restrict__ coef, float* __restrict__ out) {
    __shared__ double red[256];
    double mean[2];
    for (int mode = 0; mode < 2; ++mode) {
        double sum = 0.0, n = 0.0;
        for (int i = threadIdx.x; i < M; i += 256)
            if (flags[mode * M + i] & 1) { sum += softplus20(la[mode * M + i] + lb[mode * M + i]) / (double)log_scale; n += 1.0; }
        sum = block_sum(sum, red); n = block_sum(n, red);
        mean[mode] = sum / n;
        for (int i = threadIdx.x; i < M; i += 256)
            coef[mode * M + i] = ((flags[mode * M + i] & 1) && n > 0) ? 0.5 / n * softplus20_grad(la[mode * M + i] + lb[mode * M + i]) : 0.0;
    }
    double hits = 0.0, npos = 0.0;
    for (int i = threadIdx.x; i < M; i += 256) { hits += ((flags[i] & 4) && (flags[i] & 2)) ? 1.0 : 0.0; npos += (flags[i] & 2) ? 1.0 : 0.0; }
    hits = block_sum(hits, red); npos = block_sum(npos, red);
    if (threadIdx.x == 0) {
        out[0] = (float)((mean[0] + mean[1]) / 2.0);
        out[1] = (float)hits / ((float)npos + 1e-12f);
    }
}

// compact gradient rows: Gc [2][M][C], row m of side `mode` = d loss / d (the feature row selection m reads) * *grad_loss
__global__ __launch_bounds__(256) void fine_grad_kernel(FineIn in, FineArgs a, const double* __restrict__ la, const double* __restrict__ lb,
                                                        const double* __restrict__ coef, const float* __restrict__ grad_loss, float* __restrict__ Gc) {
    __shared__ FineLds s;
    __shared__ double sg[FL_AN][FL_PT];
    const int mode = blockIdx.y, a0 = blockIdx.x * FL_AN, M = in.M, C = in.C;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qa = threadIdx.x >> 5, cl = threadIdx.x & 31;               // the contraction's thread: anchor qa, channels c0 + cl and c0 + cl + 32
    const double gl = grad_loss ? (double)*grad_loss : 1.0;
    fine_prologue(in, a, mode, a0, s);
    double acc[FL_MAXC / FL_CH][2] = {}, gsum = 0.0;
    for (int p0 = 0; p0 < M; p0 += FL_PT) {
        double dot[2], y2;
        fine_dots(in, mode, p0, s, dot, y2);
        const int b = p0 + lane;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int m = a0 + 2 * w + q;
            double g = 0.0;
            if (b < M && m < M) {
                const Pair p = pair_eval(s.x2[2 * w + q], y2, dot[q], s.AG[2 * w + q], s.G[b], a);
                const double ca = coef[mode * M + m], cb = coef[(1 - mode) * M + b];
                if (ca != 0.0) g += ca * (exp(p.A - la[mode * M + m]) * p.pw - exp(p.B - lb[mode * M + m]) * p.nw);
                if (cb != 0.0) g += cb * (exp(p.A - la[(1 - mode) * M + b]) * p.pw - exp(p.B - lb[(1 - mode) * M + b]) * p.nw);
                g = p.pass ? g * gl : 0.0;
            }
            sg[2 * w + q][lane] = g;
        }
#pragma unroll
        for (int kc = 0; kc < FL_MAXC / FL_CH; ++kc) {
            if (kc * FL_CH < C) {
                __syncthreads();                                           // (the first: sg complete; the tile still holds the last chunk of fine_dots)
                if (C > FL_CH) {
                    fine_load_tile(in, mode, p0, kc * FL_CH, s);
                    __syncthreads();
                }
                double s0 = 0.0, s1 = 0.0, sq = 0.0;
                for (int j = 0; j < FL_PT; ++j) {
                    const double g = sg[qa][j];
                    s0 = fma(g, (double)s.T[j][cl], s0);
                    s1 = fma(g, (double)s.T[j][cl + 32], s1);
                    sq += g;
                }
                acc[kc][0] += s0; acc[kc][1] += s1;
                if (kc == 0) gsum += sq;
            }
        }
        __syncthreads();                                                   // sg and the tile are rewritten by the next sweep
    }
    const int m = a0 + qa;
    if (m < M) {
#pragma unroll
        for (int kc = 0; kc < FL_MAXC / FL_CH; ++kc)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = kc * FL_CH + cl + 32 * h;
                if (c < C) Gc[((size_t)mode * M + m) * C + c] = (float)(2.0 * ((double)s.A[qa][c] * gsum - acc[kc][h]));
            }
    }
}

// dense[row] = sum of the compact rows whose selection addresses `row`, in selection order (torch's index backward accumulates); a wave per
// selection, the first selection of a row owns it
__global__ __launch_bounds__(256) void fine_scatter_kernel(FineIn in, int image_w, const float* __restrict__ Gc, float* __restrict__ grad_img,
                                                           float* __restrict__ grad_pcd) {
    const int side = blockIdx.y, m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, M = in.M, C = in.C;
    if (m >= M) return;
    const int row = sel_row(in, image_w, side, m);
    if (row < 0) return;
    const int t0 = (m >> 6) << 6;
    for (int k0 = 0; k0 <= t0; k0 += 64) {
        const int m2 = k0 + lane;
        const bool match = m2 < m && sel_row(in, image_w, side, m2) == row;
        if (__ballot(match) != 0ull) return;
    }
    double acc[FL_MAXC / 64] = {};
    for (int k0 = t0; k0 < M; k0 += 64) {
        const int m2 = k0 + lane;
        const bool match = m2 >= m && m2 < M && sel_row(in, image_w, side, m2) == row;
        unsigned long long bits = __ballot(match);
        while (bits) {
            const int j = k0 + __ffsll((long long)bits) - 1;
            bits &= bits - 1;
#pragma unroll
            for (int k = 0; k < FL_MAXC / 64; ++k)
                if (lane + 64 * k < C) acc[k] += (double)Gc[((size_t)side * M + j) * C + lane + 64 * k];
        }
    }
    float* dst = (side == 0 ? grad_img : grad_pcd) + (size_t)row * C;
#pragma unroll
    for (int k = 0; k < FL_MAXC / 64; ++k)
        if (lane + 64 * k < C) dst[lane + 64 * k] = (float)acc[k];
}

struct FineSaved {
    double *la, *lb, *coef;
    int* flags;
    static size_t carve(void* buf, FineSaved& w, int M) {
        Carver c(buf);
        w.la = reinterpret_cast<double*>(c.take<float>(4 * (size_t)M)); w.lb = reinterpret_cast<double*>(c.take<float>(4 * (size_t)M));
        w.coef = reinterpret_cast<double*>(c.take<float>(4 * (size_t)M)); w.flags = reinterpret_cast<int*>(c.take<float>(2 * (size_t)M));
        return c.off + 256;
    }
};

int fine_check(int HW, int N, int M, int C, const float* img_points, const float* img_feats, const float* pcd_points, const float* pcd_pixels,
               const float* pcd_feats, const float* transform, const int64_t* sel_pixels, const int64_t* sel_idx, int image_w,
               const dr_fine_loss_params* p) {
    if (HW < 1 || N < 1 || M < 1 || C < 1 || image_w < 1 || !img_points || !img_feats || !pcd_points || !pcd_pixels || !pcd_feats || !transform ||
        !sel_pixels || !sel_idx || !p || !(p->log_scale > 0.f))
        return DR_EINVAL;
    if (M > FL_MAXM || C > FL_MAXC) return DR_ENOSUP;
    return DR_OK;
}

void fine_fill(FineIn& in, FineArgs& a, int HW, int N, int M, int C, const float* img_points, const float* img_feats, const float* pcd_points,
               const float* pcd_pixels, const float* pcd_feats, const float* transform, const int64_t* sel_pixels, const int64_t* sel_idx, int image_w,
               const dr_fine_loss_params* p) {
    in.img_points = img_points; in.img_feats = img_feats; in.pcd_points = pcd_points; in.pcd_pixels = pcd_pixels; in.pcd_feats = pcd_feats;
    in.transform = transform; in.sel_pixels = sel_pixels; in.sel_idx = sel_idx; in.HW = HW; in.N = N; in.M = M; in.C = C;
    a.pr3 = p->pos_radius_3d; a.nr3 = p->neg_radius_3d; a.pr2 = p->pos_radius_2d; a.nr2 = p->neg_radius_2d;
    a.pos_margin = p->pos_margin; a.neg_margin = p->neg_margin; a.pos_optimal = p->pos_optimal; a.neg_optimal = p->neg_optimal;
    a.log_scale = p->log_scale; a.image_w = image_w;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_fine_loss_saved_bytes(int M) {
    if (M < 1) return 0;
    FineSaved w;
    return FineSaved::carve(nullptr, w, M);
}

size_t dr_fine_loss_backward_workspace_bytes(int M, int C) {
    if (M < 1 || C < 1) return 0;
    return 2 * (size_t)M * C * sizeof(float) + 256;
}

int dr_fine_loss_f32(int HW, int N, int M, int C, const float* img_points, const float* img_feats, const float* pcd_points, const float* pcd_pixels,
                     const float* pcd_feats, const float* transform, const int64_t* img_sel_pixels, const int64_t* pcd_sel_indices, int image_w,
                     const dr_fine_loss_params* params, float* loss_recall, void* saved, size_t saved_bytes, void* stream) {
    int rc = fine_check(HW, N, M, C, img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices, image_w, params);
    if (rc) return rc;
    if (!loss_recall) return DR_EINVAL;
    if (!saved || saved_bytes < dr_fine_loss_saved_bytes(M)) return DR_EWORKSPACE;
    FineIn in; FineArgs a; FineSaved w;
    fine_fill(in, a, HW, N, M, C, img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices, image_w, params);
    FineSaved::carve(saved, w, M);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fine_stats_kernel, dim3((M + FL_AN - 1) / FL_AN, 2), dim3(256), 0, st, in, a, w.la, w.lb, w.flags);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(fine_final_kernel, dim3(1), dim3(256), 0, st, M, a.log_scale, w.la, w.lb, w.flags, w.coef, loss_recall);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_fine_loss_backward_f32(int HW, int N, int M, int C, const float* img_points, const float* img_feats, const float* pcd_points,
                              const float* pcd_pixels, const float* pcd_feats, const float* transform, const int64_t* img_sel_pixels,
                              const int64_t* pcd_sel_indices, int image_w, const dr_fine_loss_params* params, const void* saved, size_t saved_bytes,
                              const float* grad_loss, float* grad_img_feats, float* grad_pcd_feats, void* workspace, size_t workspace_bytes,
                              void* stream) {
    int rc = fine_check(HW, N, M, C, img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices, image_w, params);
    if (rc) return rc;
    if (!grad_img_feats || !grad_pcd_feats) return DR_EINVAL;
    if (!saved || saved_bytes < dr_fine_loss_saved_bytes(M) || !workspace || workspace_bytes < dr_fine_loss_backward_workspace_bytes(M, C))
        return DR_EWORKSPACE;
    FineIn in; FineArgs a; FineSaved w;
    fine_fill(in, a, HW, N, M, C, img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices, image_w, params);
    FineSaved::carve(const_cast<void*>(saved), w, M);
    Carver cv(workspace);
    float* Gc = cv.take<float>(2 * (size_t)M * C);
    hipStream_t st = (hipStream_t)stream;
    DR_HIP_CHECK(hipMemsetAsync(grad_img_feats, 0, (size_t)HW * C * sizeof(float), st));
    DR_HIP_CHECK(hipMemsetAsync(grad_pcd_feats, 0, (size_t)N * C * sizeof(float), st));
    hipLaunchKernelGGL(fine_grad_kernel, dim3((M + FL_AN - 1) / FL_AN, 2), dim3(256), 0, st, in, a, w.la, w.lb, w.coef, grad_loss, Gc);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(fine_scatter_kernel, dim3((M + 3) / 4, 2), dim3(256), 0, st, in, image_w, Gc, grad_img_feats, grad_pcd_feats);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
