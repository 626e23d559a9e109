// partition2d3d.hip -- the block of MATR2D3D.forward between the backbones and the coarse matching (EXP/model.py:395-540; EXP = Diff-Reg-2d3d/
// experiments/2d3dmatr.rgbdv2.stage4.level3.stage1) and the training-only ground-truth search behind it (model.py:565-600):
//   point_to_node_partition   vision3d/ops/point_cloud_partition.py:41-104 (return_count, gather_points)
//   patchify                  EXP/utils.py:28-56
//   node_correspondences      EXP/utils.py:59-175 (get_2d3d_node_correspondences, the whole function)
//   mutual_nn_radius          EXP/utils.py:234-252 (multual_nn_correspondence, knn = 1)
//   radius_pairs              EXP/utils.py:426-446 (get_correspondences / KDTree_corr)
// Index work: every list comes out in the reference's order (torch.nonzero's row-major order, ascending distance inside a node) by a
// count / scan / write compaction or a sort -- no atomics on floats, no order that depends on scheduling.  Distances are sums of squared
// differences in float32.  Nothing of size (nodes x points) or (candidates x Ki x Kc) goes to memory.
#include "loop_common.h"

namespace dr {
namespace {

constexpr int PT_MAX_LIMIT = 128;      // point_limit of dr_point_to_node_partition_f32
constexpr int PT_NODE_CHUNK = 1024;    // nodes staged in LDS at a time (12 KB)
constexpr int NC_MAX_KI = 256, NC_MAX_KC = 128;

__device__ __forceinline__ float sq_dist3(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;
}

// ---- point_to_node_partition ---------------------------------------------------------------------------------------------------------------
// one point per lane, the node set through LDS in chunks: nearest node (equal distances: the lower node index), and the sort key
// (node << 32 | bits of the squared distance): non-negative floats order like their bit patterns
__global__ __launch_bounds__(256) void pt_assign_kernel(int Nf, int Nc, int n_pad, const float* __restrict__ points, const float* __restrict__ nodes,
                                                        long long* __restrict__ point_to_node, unsigned long long* __restrict__ keys,
                                                        unsigned* __restrict__ vals) {
    __shared__ float s_n[PT_NODE_CHUNK * 3];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (i < Nf) { px = points[3 * (size_t)i]; py = points[3 * (size_t)i + 1]; pz = points[3 * (size_t)i + 2]; }
    float best = INFINITY;
    int arg = 0;
    for (int c0 = 0; c0 < Nc; c0 += PT_NODE_CHUNK) {
        const int cn = min(PT_NODE_CHUNK, Nc - c0);
        __syncthreads();
        for (int e = threadIdx.x; e < 3 * cn; e += 256) s_n[e] = nodes[3 * (size_t)c0 + e];
        __syncthreads();
        for (int c = 0; c < cn; ++c) {
            const float d = sq_dist3(px, py, pz, s_n[3 * c], s_n[3 * c + 1], s_n[3 * c + 2]);
            if (d < best) { best = d; arg = c0 + c; }
        }
    }
    if (i < Nf) {
        point_to_node[i] = arg;
        keys[i] = ((unsigned long long)(unsigned)arg << 32) | (unsigned long long)__float_as_uint(best);
        vals[i] = (unsigned)i;
    } else if (i < n_pad) {
        keys[i] = ~0ull;
        vals[i] = (unsigned)i;
    }
}

__device__ __forceinline__ int lower_bound_u64(const unsigned long long* __restrict__ a, int n, unsigned long long v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per node: its segment of the sorted list by two binary searches, then the first K entries (ascending distance, equal distances by
// ascending point index: the order of the (key, value) sort), padded with Nf
__global__ __launch_bounds__(256) void pt_gather_kernel(int Nf, int Nc, int K, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                        long long* __restrict__ node_sizes, uint8_t* __restrict__ node_masks,
                                                        long long* __restrict__ knn_indices, uint8_t* __restrict__ knn_masks, int* __restrict__ max_points) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= Nc) return;
    const int start = lower_bound_u64(keys, Nf, (unsigned long long)(unsigned)c << 32);
    const int end = lower_bound_u64(keys, Nf, (unsigned long long)((unsigned)c + 1u) << 32);
    const int size = end - start;
    for (int j = lane; j < K; j += 64) {
        const bool in = j < size;
        knn_indices[(size_t)c * K + j] = in ? (long long)vals[start + j] : (long long)Nf;
        knn_masks[(size_t)c * K + j] = in ? 1 : 0;
    }
    if (lane == 0) {
        node_sizes[c] = size;
        node_masks[c] = size > 0 ? 1 : 0;
        atomicMax(max_points, size);
    }
}

// ---- patchify --------------------------------------------------------------------------------------------------------------------------------
// one wave per image node: the pixel indices of its (strided) block, every gather, and the two `any` masks
__global__ __launch_bounds__(64) void patchify_kernel(int W_f, int W_c, int bh, int bw, int stride, int kh, int kw, const float* __restrict__ points,
                                                      const float* __restrict__ points_da, const float* __restrict__ pixels, const uint8_t* __restrict__ masks,
                                                      const uint8_t* __restrict__ masks_da, float* __restrict__ o_points, float* __restrict__ o_points_da,
                                                      float* __restrict__ o_pixels, long long* __restrict__ o_indices, uint8_t* __restrict__ o_masks,
                                                      uint8_t* __restrict__ o_masks_da, uint8_t* __restrict__ node_masks, uint8_t* __restrict__ node_masks_da) {
    const int node = blockIdx.x, r = node / W_c, c = node % W_c, lane = threadIdx.x, Ki = kh * kw;
    bool any = false, any_da = false;
    for (int e = lane; e < Ki; e += 64) {
        const int a = e / kw, b = e % kw;
        const size_t src = (size_t)(r * bh + a * stride) * W_f + (size_t)c * bw + (size_t)b * stride;
        const size_t dst = (size_t)node * Ki + e;
        o_indices[dst] = (long long)src;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o_points[3 * dst + k] = points[3 * src + k]; o_points_da[3 * dst + k] = points_da[3 * src + k]; }
        o_pixels[2 * dst] = pixels[2 * src];
        o_pixels[2 * dst + 1] = pixels[2 * src + 1];
        const uint8_t m = masks[src] ? 1 : 0, md = masks_da[src] ? 1 : 0;
        o_masks[dst] = m;
        o_masks_da[dst] = md;
        any |= m != 0;
        any_da |= md != 0;
    }
    const unsigned long long b0 = __ballot(any), b1 = __ballot(any_da);
    if (lane == 0) { node_masks[node] = b0 ? 1 : 0; node_masks_da[node] = b1 ? 1 : 0; }
}

// ---- ordered compaction of the entries (i, j) of a rows x cols predicate ------------------------------------------------------------------
// three launches: one wave per row counts; one workgroup scans the counts; one wave per row writes its entries at their ranks.  The pairs come
// out in row-major order whatever the schedule.  counts[0] = entries written (<= capacity), counts[1] = entries found.
template <typename Pred>
__global__ __launch_bounds__(256) void rc_count_kernel(int rows, int cols, Pred pred, int* __restrict__ row_count) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= rows) return;
    int n = 0;
    for (int j0 = 0; j0 < cols; j0 += 64) {
        const int j = j0 + lane;
        n += __popcll(__ballot(j < cols && pred(i, j)));
    }
    if (lane == 0) row_count[i] = n;
}

// exclusive scan of row_count in place (one workgroup of 1024, 1024 rows a step); counts as above
__global__ __launch_bounds__(1024) void rc_scan_kernel(int rows, int* __restrict__ row_count, long long capacity, int* __restrict__ counts) {
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < rows; i0 += 1024) {
        const int i = i0 + t;
        const int v = i < rows ? row_count[i] : 0;
        int inc = v;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int o = __shfl_up(inc, m);
            if (lane >= m) inc += o;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        int before = s_base;
        for (int q = 0; q < w; ++q) before += s_w[q];
        if (i < rows) row_count[i] = before + inc - v;
        __syncthreads();
        if (t == 0) { int tot = 0; for (int q = 0; q < 16; ++q) tot += s_w[q]; s_base += tot; }
        __syncthreads();
    }
    if (t == 0) { counts[0] = (long long)s_base < capacity ? s_base : (int)capacity; counts[1] = s_base; }
}

template <typename Pred, typename Out>
__global__ __launch_bounds__(256) void rc_write_kernel(int rows, int cols, Pred pred, const int* __restrict__ row_start, long long capacity,
                                                       Out* __restrict__ out_i, Out* __restrict__ out_j) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= rows) return;
    long long at = row_start[i];
    for (int j0 = 0; j0 < cols; j0 += 64) {
        const int j = j0 + lane;
        const bool hit = j < cols && pred(i, j);
        const unsigned long long b = __ballot(hit);
        const long long pos = at + __popcll(b & ((1ull << lane) - 1ull));
        if (hit && pos < capacity) { out_i[pos] = (Out)i; out_j[pos] = (Out)j; }
        at += __popcll(b);
    }
}

template <typename Pred, typename Out>
int compact_pairs(int rows, int cols, Pred pred, int* row_count, long long capacity, Out* out_i, Out* out_j, int* counts, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rc_count_kernel<Pred>), dim3((rows + 3) / 4), dim3(256), 0, st, rows, cols, pred, row_count);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rc_scan_kernel, dim3(1), dim3(1024), 0, st, rows, row_count, capacity, counts);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rc_write_kernel<Pred, Out>), dim3((rows + 3) / 4), dim3(256), 0, st, rows, cols, pred, row_count, capacity, out_i, out_j);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// ---- get_2d3d_node_correspondences -----------------------------------------------------------------------------------------------------------
// blocks [0, M): an image node (both masked means, the enclosing radius about the first); blocks [M, M + N): a point node (its patch moved by
// `transform` into the workspace, masked mean, radius).  Sums in double in index order; masked_mean divides by count + 1e-6 (masked_ops.py:23-41).
__global__ __launch_bounds__(64) void nc_centers_kernel(int M, int Ki, int N, int Kc, const float* __restrict__ img_pts, const float* __restrict__ img_pts_da,
                                                        const uint8_t* __restrict__ img_km, const uint8_t* __restrict__ img_km_da,
                                                        const float* __restrict__ pcd_pts, const uint8_t* __restrict__ pcd_km,
                                                        const float* __restrict__ transform, float* __restrict__ pcd_moved, float* __restrict__ img_centers,
                                                        float* __restrict__ img_centers_da, float* __restrict__ pcd_centers, float* __restrict__ img_rad,
                                                        float* __restrict__ pcd_rad) {
    const int lane = threadIdx.x;
    const bool is_img = (int)blockIdx.x < M;
    const int node = is_img ? blockIdx.x : blockIdx.x - M, K = is_img ? Ki : Kc;
    const uint8_t* km = (is_img ? img_km : pcd_km) + (size_t)node * K;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = transform[k];
    double sx = 0, sy = 0, sz = 0, ax = 0, ay = 0, az = 0;
    int cnt = 0, cnt_da = 0;
    for (int e = lane; e < K; e += 64) {
        const size_t at = (size_t)node * K + e;
        if (is_img) {
            if (km[e]) { sx += img_pts[3 * at]; sy += img_pts[3 * at + 1]; sz += img_pts[3 * at + 2]; ++cnt; }
            if (img_km_da[at]) { ax += img_pts_da[3 * at]; ay += img_pts_da[3 * at + 1]; az += img_pts_da[3 * at + 2]; ++cnt_da; }
        } else {
            const float x = pcd_pts[3 * at], y = pcd_pts[3 * at + 1], z = pcd_pts[3 * at + 2];
            const float qx = x * T[0] + y * T[1] + z * T[2] + T[3], qy = x * T[4] + y * T[5] + z * T[6] + T[7], qz = x * T[8] + y * T[9] + z * T[10] + T[11];
            pcd_moved[3 * at] = qx; pcd_moved[3 * at + 1] = qy; pcd_moved[3 * at + 2] = qz;
            if (km[e]) { sx += qx; sy += qy; sz += qz; ++cnt; }
        }
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    cnt = wave_sum(cnt);
    const float den = (float)cnt + 1e-6f;
    const float cx = (float)sx / den, cy = (float)sy / den, cz = (float)sz / den;
    float* centers = is_img ? img_centers : pcd_centers;
    if (lane == 0) { centers[3 * node] = cx; centers[3 * node + 1] = cy; centers[3 * node + 2] = cz; }
    if (is_img) {
        ax = wave_sum(ax); ay = wave_sum(ay); az = wave_sum(az);
        cnt_da = wave_sum(cnt_da);
        const float dd = (float)cnt_da + 1e-6f;
        if (lane == 0) { img_centers_da[3 * node] = (float)ax / dd; img_centers_da[3 * node + 1] = (float)ay / dd; img_centers_da[3 * node + 2] = (float)az / dd; }
    }
    const float* pts = is_img ? img_pts : pcd_moved;      // (a lane re-reads only the rows it wrote itself)
    float r2 = 0.f;
    for (int e = lane; e < K; e += 64) {
        const size_t at = (size_t)node * K + e;
        if (km[e]) r2 = fmaxf(r2, sq_dist3(pts[3 * at], pts[3 * at + 1], pts[3 * at + 2], cx, cy, cz));
    }
    r2 = wave_max(r2);
    if (lane == 0) (is_img ? img_rad : pcd_rad)[node] = sqrtf(r2);
}

// the enclosing-sphere test of utils.py:113-116
struct NcCandidate {
    const float *img_c, *pcd_c, *img_rad, *pcd_rad;
    const uint8_t *img_masks, *pcd_masks;
    float r3d;
    __device__ bool operator()(int i, int j) const {
        if (!img_masks[i] || !pcd_masks[j]) return false;
        const float d = sqrtf(sq_dist3(img_c[3 * i], img_c[3 * i + 1], img_c[3 * i + 2], pcd_c[3 * j], pcd_c[3 * j + 1], pcd_c[3 * j + 2]));
        return img_rad[i] + pcd_rad[j] + r3d - d > 0.f;
    }
};

// one workgroup per candidate (grid-stride), both patches in LDS: every image point's nearest patch point and every patch point's nearest image
// point (over ALL entries of the other patch, masked ones included, as the reference's k-NN sees them; equal distances: the lower index), the
// 3D radius, the 2D radius and both mask tests, the two ratios (utils.py:129-163)
__global__ __launch_bounds__(256) void nc_overlap_kernel(int Ki, int Kc, const int* __restrict__ counts, const int* __restrict__ cand_i, const int* __restrict__ cand_j,
                                                         const float* __restrict__ img_pts, const float* __restrict__ img_pix, const uint8_t* __restrict__ img_km,
                                                         const float* __restrict__ pcd_moved, const float* __restrict__ pcd_pix, const uint8_t* __restrict__ pcd_km,
                                                         float r2d, float r3d, float* __restrict__ ratio_img, float* __restrict__ ratio_pcd) {
    __shared__ float s_ip[NC_MAX_KI * 3], s_ix[NC_MAX_KI * 2], s_pp[NC_MAX_KC * 3], s_px[NC_MAX_KC * 2];
    __shared__ uint8_t s_im[NC_MAX_KI], s_pm[NC_MAX_KC];
    __shared__ int s_cnt[4];
    const int t = threadIdx.x, n = counts[0];
    for (int b = blockIdx.x; b < n; b += gridDim.x) {
        const size_t i = cand_i[b], j = cand_j[b];
        __syncthreads();
        for (int e = t; e < 3 * Ki; e += 256) s_ip[e] = img_pts[i * 3 * Ki + e];
        for (int e = t; e < 2 * Ki; e += 256) s_ix[e] = img_pix[i * 2 * Ki + e];
        for (int e = t; e < Ki; e += 256) s_im[e] = img_km[i * Ki + e];
        for (int e = t; e < 3 * Kc; e += 256) s_pp[e] = pcd_moved[j * 3 * Kc + e];
        for (int e = t; e < 2 * Kc; e += 256) s_px[e] = pcd_pix[j * 2 * Kc + e];
        for (int e = t; e < Kc; e += 256) s_pm[e] = pcd_km[j * Kc + e];
        if (t < 4) s_cnt[t] = 0;
        __syncthreads();
        int ov_i = 0, tot_i = 0, ov_p = 0, tot_p = 0;
        for (int a = t; a < Ki; a += 256) {
            float best = INFINITY;
            int arg = 0;
            for (int c = 0; c < Kc; ++c) {
                const float d = sq_dist3(s_ip[3 * a], s_ip[3 * a + 1], s_ip[3 * a + 2], s_pp[3 * c], s_pp[3 * c + 1], s_pp[3 * c + 2]);
                if (d < best) { best = d; arg = c; }
            }
            const float dx = s_ix[2 * a] - s_px[2 * arg], dy = s_ix[2 * a + 1] - s_px[2 * arg + 1];
            const bool m = s_im[a] != 0;
            tot_i += m;
            ov_i += m && s_pm[arg] && sqrtf(best) < r3d && sqrtf(dx * dx + dy * dy) < r2d;
        }
        for (int c = t; c < Kc; c += 256) {
            float best = INFINITY;
            int arg = 0;
            for (int a = 0; a < Ki; ++a) {
                const float d = sq_dist3(s_pp[3 * c], s_pp[3 * c + 1], s_pp[3 * c + 2], s_ip[3 * a], s_ip[3 * a + 1], s_ip[3 * a + 2]);
                if (d < best) { best = d; arg = a; }
            }
            const float dx = s_px[2 * c] - s_ix[2 * arg], dy = s_px[2 * c + 1] - s_ix[2 * arg + 1];
            const bool m = s_pm[c] != 0;
            tot_p += m;
            ov_p += m && s_im[arg] && sqrtf(best) < r3d && sqrtf(dx * dx + dy * dy) < r2d;
        }
        ov_i = wave_sum(ov_i); tot_i = wave_sum(tot_i); ov_p = wave_sum(ov_p); tot_p = wave_sum(tot_p);
        if ((t & 63) == 0) { atomicAdd(&s_cnt[0], ov_i); atomicAdd(&s_cnt[1], tot_i); atomicAdd(&s_cnt[2], ov_p); atomicAdd(&s_cnt[3], tot_p); }
        __syncthreads();
        if (t == 0) {                    // integer quotients in float32, as counts.float() / totals.float() (0 / 0 = NaN fails the > 0 filter, as torch's)
            ratio_img[b] = (float)s_cnt[0] / (float)s_cnt[1];
            ratio_pcd[b] = (float)s_cnt[2] / (float)s_cnt[3];
        }
    }
}

// the final filter (both ratios > 0), in candidate order: one workgroup, 1024 candidates a step (the scheme of unique_sorted_kernel, fine2d3d.hip)
__global__ __launch_bounds__(1024) void nc_filter_kernel(const int* __restrict__ counts, const int* __restrict__ cand_i, const int* __restrict__ cand_j,
                                                         const float* __restrict__ ratio_img, const float* __restrict__ ratio_pcd, long long* __restrict__ out_i,
                                                         long long* __restrict__ out_j, float* __restrict__ out_ri, float* __restrict__ out_rp,
                                                         int* __restrict__ out_count) {
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, n = counts[0];
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int b0 = 0; b0 < n; b0 += 1024) {
        const int b = b0 + t;
        const float ri = b < n ? ratio_img[b] : 0.f, rp = b < n ? ratio_pcd[b] : 0.f;
        const bool keep = b < n && ri > 0.f && rp > 0.f;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_w[w] = __popcll(bal);
        __syncthreads();
        int before = s_base;
        for (int q = 0; q < w; ++q) before += s_w[q];
        if (keep) {
            const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));      // pos <= b < capacity of the outputs
            out_i[pos] = cand_i[b]; out_j[pos] = cand_j[b]; out_ri[pos] = ri; out_rp[pos] = rp;
        }
        __syncthreads();
        if (t == 0) { int tot = 0; for (int q = 0; q < 16; ++q) tot += s_w[q]; s_base += tot; }
        __syncthreads();
    }
    if (t == 0) *out_count = s_base;
}

// ---- mutual nearest neighbours within a radius ------------------------------------------------------------------------------------------
// nearest b of every a (one a per lane, b through LDS in chunks; equal distances: the lower index) and its squared distance
__global__ __launch_bounds__(256) void nn1_kernel(int na, int nb, const float* __restrict__ a, const float* __restrict__ b, int* __restrict__ arg_out,
                                                  float* __restrict__ d2_out) {
    __shared__ float s_b[PT_NODE_CHUNK * 3];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (i < na) { px = a[3 * (size_t)i]; py = a[3 * (size_t)i + 1]; pz = a[3 * (size_t)i + 2]; }
    float best = INFINITY;
    int arg = 0;
    for (int c0 = 0; c0 < nb; c0 += PT_NODE_CHUNK) {
        const int cn = min(PT_NODE_CHUNK, nb - c0);
        __syncthreads();
        for (int e = threadIdx.x; e < 3 * cn; e += 256) s_b[e] = b[3 * (size_t)c0 + e];
        __syncthreads();
        for (int c = 0; c < cn; ++c) {
            const float d = sq_dist3(s_b[3 * c], s_b[3 * c + 1], s_b[3 * c + 2], px, py, pz);
            if (d < best) { best = d; arg = c0 + c; }
        }
    }
    if (i < na) { arg_out[i] = arg; d2_out[i] = best; }
}

// sources whose nearest target has them as its nearest source, closer than the radius, in ascending source order (one workgroup)
__global__ __launch_bounds__(1024) void mutual_select_kernel(int ns, const int* __restrict__ s2t, const float* __restrict__ s2t_d2, const int* __restrict__ t2s,
                                                             float radius, long long* __restrict__ out_src, long long* __restrict__ out_tgt, int* __restrict__ count) {
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < ns; i0 += 1024) {
        const int i = i0 + t;
        const int j = i < ns ? s2t[i] : 0;
        const bool keep = i < ns && t2s[j] == i && sqrtf(s2t_d2[i]) < radius;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_w[w] = __popcll(bal);
        __syncthreads();
        int before = s_base;
        for (int q = 0; q < w; ++q) before += s_w[q];
        if (keep) {
            const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
            out_src[pos] = i; out_tgt[pos] = j;
        }
        __syncthreads();
        if (t == 0) { int tot = 0; for (int q = 0; q < 16; ++q) tot += s_w[q]; s_base += tot; }
        __syncthreads();
    }
    if (t == 0) *count = s_base;
}

// ---- radius pairs ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void move_points_kernel(int n, const float* __restrict__ pts, const float* __restrict__ transform, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const float* T = transform;
    out[3 * (size_t)i] = T ? x * T[0] + y * T[1] + z * T[2] + T[3] : x;
    out[3 * (size_t)i + 1] = T ? x * T[4] + y * T[5] + z * T[6] + T[7] : y;
    out[3 * (size_t)i + 2] = T ? x * T[8] + y * T[9] + z * T[10] + T[11] : z;
}

struct RadiusPred {
    const float *src, *tgt;
    float r2;
    __device__ bool operator()(int i, int j) const {
        return sq_dist3(src[3 * i], src[3 * i + 1], src[3 * i + 2], tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]) < r2;
    }
};

}  // namespace
}  // namespace dr

extern "C" {

size_t dr_point_to_node_partition_workspace_bytes(int Nf) {
    return Nf < 1 ? 256 : dr::sort_carve(nullptr, Nf).bytes;
}

int dr_point_to_node_partition_f32(int Nf, int Nc, int point_limit, const float* points, const float* nodes, int64_t* point_to_node, int64_t* node_sizes,
                                   uint8_t* node_masks, int64_t* node_knn_indices, uint8_t* node_knn_masks, int32_t* max_points_per_node, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (Nf < 1 || Nc < 1 || point_limit < 1 || !points || !nodes || !point_to_node || !node_sizes || !node_masks || !node_knn_indices || !node_knn_masks ||
        !max_points_per_node || !workspace)
        return DR_EINVAL;
    if (point_limit > dr::PT_MAX_LIMIT || Nf > (1 << 28)) return DR_ENOSUP;
    if (workspace_bytes < dr_point_to_node_partition_workspace_bytes(Nf)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dr::SortWs w = dr::sort_carve(workspace, Nf);
    DR_HIP_CHECK(hipMemsetAsync(max_points_per_node, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(dr::pt_assign_kernel, dim3((w.n_pad + 255) / 256), dim3(256), 0, st, Nf, Nc, w.n_pad, points, nodes, (long long*)point_to_node, w.keys, w.vals);
    DR_LAUNCH_CHECK();
    const int rc = dr::launch_bitonic_sort(w.keys, w.vals, w.n_pad, st);
    if (rc) return rc;
    hipLaunchKernelGGL(dr::pt_gather_kernel, dim3((Nc + 3) / 4), dim3(256), 0, st, Nf, Nc, point_limit, w.keys, w.vals, (long long*)node_sizes, node_masks,
                       (long long*)node_knn_indices, node_knn_masks, (int*)max_points_per_node);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_patchify_f32(int H_f, int W_f, int H_c, int W_c, int stride, const float* img_points, const float* img_points_da, const float* img_pixels,
                    const uint8_t* img_masks, const uint8_t* img_masks_da, float* knn_points, float* knn_points_da, float* knn_pixels, int64_t* knn_indices,
                    uint8_t* knn_masks, uint8_t* knn_masks_da, uint8_t* node_masks, uint8_t* node_masks_da, void* stream) {
    if (H_f < 1 || W_f < 1 || H_c < 1 || W_c < 1 || stride < 1 || H_f % H_c || W_f % W_c || !img_points || !img_points_da || !img_pixels || !img_masks ||
        !img_masks_da || !knn_points || !knn_points_da || !knn_pixels || !knn_indices || !knn_masks || !knn_masks_da || !node_masks || !node_masks_da)
        return DR_EINVAL;
    if ((long long)H_f * W_f > (1ll << 30)) return DR_ENOSUP;
    const int bh = H_f / H_c, bw = W_f / W_c, kh = (bh + stride - 1) / stride, kw = (bw + stride - 1) / stride;     // [::stride] of a block side
    hipLaunchKernelGGL(dr::patchify_kernel, dim3(H_c * W_c), dim3(64), 0, (hipStream_t)stream, W_f, W_c, bh, bw, stride, kh, kw, img_points, img_points_da,
                       img_pixels, img_masks, img_masks_da, knn_points, knn_points_da, knn_pixels, (long long*)knn_indices, knn_masks, knn_masks_da, node_masks,
                       node_masks_da);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_node_correspondences_2d3d_workspace_bytes(int M, int N, int Kc, long long capacity) {
    return (M < 1 || N < 1 || Kc < 1 || capacity < 1) ? 256 : dr::node_corr_carve(nullptr, M, N, Kc, (size_t)capacity).bytes;
}

int dr_node_correspondences_2d3d_f32(int M, int Ki, int N, int Kc, const uint8_t* img_masks, const float* img_knn_points, const float* img_knn_points_da,
                                     const float* img_knn_pixels, const uint8_t* img_knn_masks, const uint8_t* img_knn_masks_da, const uint8_t* pcd_masks,
                                     const float* pcd_knn_points, const float* pcd_knn_pixels, const uint8_t* pcd_knn_masks, const float* transform,
                                     float pos_radius_2d, float pos_radius_3d, long long capacity, int64_t* img_corr_indices, int64_t* pcd_corr_indices,
                                     float* img_corr_overlaps, float* pcd_corr_overlaps, int32_t* counts, float* pcd_centers, float* img_centers,
                                     float* img_centers_da, void* workspace, size_t workspace_bytes, void* stream) {
    if (M < 1 || N < 1 || Ki < 1 || Kc < 1 || capacity < 1 || !img_masks || !img_knn_points || !img_knn_points_da || !img_knn_pixels || !img_knn_masks ||
        !img_knn_masks_da || !pcd_masks || !pcd_knn_points || !pcd_knn_pixels || !pcd_knn_masks || !transform || !img_corr_indices || !pcd_corr_indices ||
        !img_corr_overlaps || !pcd_corr_overlaps || !counts || !pcd_centers || !img_centers || !img_centers_da || !workspace)
        return DR_EINVAL;
    if (Ki > dr::NC_MAX_KI || Kc > dr::NC_MAX_KC || capacity > (1ll << 30) || (long long)M * N > (1ll << 30)) return DR_ENOSUP;
    if (workspace_bytes < dr_node_correspondences_2d3d_workspace_bytes(M, N, Kc, capacity)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dr::NodeCorrWs w = dr::node_corr_carve(workspace, M, N, Kc, (size_t)capacity);
    hipLaunchKernelGGL(dr::nc_centers_kernel, dim3(M + N), dim3(64), 0, st, M, Ki, N, Kc, img_knn_points, img_knn_points_da, img_knn_masks, img_knn_masks_da,
                       pcd_knn_points, pcd_knn_masks, transform, w.pcd_moved, img_centers, img_centers_da, pcd_centers, w.img_rad, w.pcd_rad);
    DR_LAUNCH_CHECK();
    dr::NcCandidate pred{img_centers, pcd_centers, w.img_rad, w.pcd_rad, img_masks, pcd_masks, pos_radius_3d};
    // counts[1], [2] = candidates kept / found (found > capacity: the list was cut and the caller must not use the result); counts[0] = pairs written
    const int rc = dr::compact_pairs(M, N, pred, w.row_count, capacity, w.cand_i, w.cand_j, (int*)counts + 1, st);
    if (rc) return rc;
    const int grid = (int)(capacity < 16384 ? capacity : 16384);
    hipLaunchKernelGGL(dr::nc_overlap_kernel, dim3(grid), dim3(256), 0, st, Ki, Kc, (const int*)counts + 1, w.cand_i, w.cand_j, img_knn_points, img_knn_pixels,
                       img_knn_masks, w.pcd_moved, pcd_knn_pixels, pcd_knn_masks, pos_radius_2d, pos_radius_3d, w.ratio_img, w.ratio_pcd);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(dr::nc_filter_kernel, dim3(1), dim3(1024), 0, st, (const int*)counts + 1, w.cand_i, w.cand_j, w.ratio_img, w.ratio_pcd,
                       (long long*)img_corr_indices, (long long*)pcd_corr_indices, img_corr_overlaps, pcd_corr_overlaps, (int*)counts);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_mutual_nn_radius_workspace_bytes(int ns, int nt) {
    return (ns < 1 || nt < 1) ? 256 : dr::mutual_nn_carve(nullptr, ns, nt).bytes;
}

int dr_mutual_nn_radius_f32(int ns, int nt, const float* src, const float* tgt, float radius, int64_t* out_src, int64_t* out_tgt, int32_t* count,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (ns < 0 || nt < 0 || !count || !workspace || (ns > 0 && (!src || !out_src || !out_tgt)) || (nt > 0 && !tgt)) return DR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (ns == 0 || nt == 0) { DR_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int32_t), st)); return DR_OK; }
    if (workspace_bytes < dr_mutual_nn_radius_workspace_bytes(ns, nt)) return DR_EWORKSPACE;
    const dr::MutualNnWs w = dr::mutual_nn_carve(workspace, ns, nt);
    hipLaunchKernelGGL(dr::nn1_kernel, dim3((ns + 255) / 256), dim3(256), 0, st, ns, nt, src, tgt, w.s2t, w.s2t_d2);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(dr::nn1_kernel, dim3((nt + 255) / 256), dim3(256), 0, st, nt, ns, tgt, src, w.t2s, w.t2s_d2);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(dr::mutual_select_kernel, dim3(1), dim3(1024), 0, st, ns, w.s2t, w.s2t_d2, w.t2s, radius, (long long*)out_src, (long long*)out_tgt, (int*)count);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_radius_pairs_workspace_bytes(int ns, int nt) {
    return ns < 1 ? 256 : dr::radius_pairs_carve(nullptr, ns).bytes;
}

int dr_radius_pairs_f32(int ns, int nt, const float* src, const float* tgt, const float* transform, float radius, long long capacity, int64_t* out_src,
                        int64_t* out_tgt, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (ns < 0 || nt < 0 || capacity < 0 || !counts || !workspace || (ns > 0 && !src) || (nt > 0 && !tgt) || (capacity > 0 && (!out_src || !out_tgt)))
        return DR_EINVAL;
    if ((long long)ns * nt > (1ll << 30) || capacity > (1ll << 30)) return DR_ENOSUP;
    hipStream_t st = (hipStream_t)stream;
    if (ns == 0 || nt == 0) { DR_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st)); return DR_OK; }
    if (workspace_bytes < dr_radius_pairs_workspace_bytes(ns, nt)) return DR_EWORKSPACE;
    const dr::RadiusPairsWs w = dr::radius_pairs_carve(workspace, ns);
    hipLaunchKernelGGL(dr::move_points_kernel, dim3((ns + 255) / 256), dim3(256), 0, st, ns, src, transform, w.moved);
    DR_LAUNCH_CHECK();
    dr::RadiusPred pred{w.moved, tgt, radius * radius};
    return dr::compact_pairs(ns, nt, pred, w.row_count, capacity, (long long*)out_src, (long long*)out_tgt, (int*)counts, st);
}

}  // extern "C"
