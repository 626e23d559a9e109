/* diffreg_hip.h -- C ABI of libdiffreg_hip.so (MI355X / gfx950).
 *
 * The reference (wuqianliang/Diff-Reg) has no FFI on this path: the boundary is a set of Python
 * functions/classes.  Each entry point below replaces the body of one of
 * them; the Python side (the modules under diff-reg_amd/models) keeps the reference signatures and binds these
 * with ctypes.  Citations: 3D/ = Diff-Reg-3dmatch/, 4D/ = Diff-Reg-4dmatch/.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with `h_`; tensors are contiguous
 *     row-major; the caller owns every buffer, workspaces are passed in explicitly;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on it and never
 *     synchronise the host;
 *   - return 0 on success, a negative DR_E* code otherwise (dr_strerror gives the text);
 *   - "pairs": P independent scene pairs (reference inference is B = 1 per pair); per-pair
 *     quantities such as x.min() are per pair.
 */
#ifndef DIFFREG_HIP_H
#define DIFFREG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_OK 0
#define DR_EINVAL (-1)   /* bad argument (size, NULL pointer, unsupported flag)            */
#define DR_ELAUNCH (-2)  /* a HIP launch or API call failed (dr_last_hip_error has detail) */
#define DR_ENOSUP (-3)   /* shape not supported by this build                               */
#define DR_EWORKSPACE (-4) /* workspace too small                                           */
#define DR_ETIMEOUT (-5) /* a kernel gave up waiting for another workgroup (dr_device_status) */

/* ABI version of THIS header.  dr_version() returns the library's; a binding must refuse to run when they differ in major or
 * minor (the Python mirror does, diffreg_hip/lib.py).  History of breaks:
 *   0.2.0  dr_loop_trace grew the teacher-forcing fields (a 0.1.0 caller's struct is too short); dr_procrustes_f32 and
 *          dr_top1_union_f32 / _f64 take (workspace, workspace_bytes) in front of `stream` since the last 0.1.0 builds -- a caller
 *          compiled against the header without them passes its stream in the workspace slot.
 *   0.3.0  training of the 2D-3D model: the vision3d TransformerLayer's training forward / backward (dr_fusion_layer_*, the new struct
 *          dr_fusion_layer_grads), the row L2 normalisation and the weighted circle loss with their backwards (dr_l2_normalize_*,
 *          dr_circle_loss_*, the new struct dr_circle_loss_params).
 *   0.4.0  the 2D-3D patch partition and ground-truth overlaps: dr_point_to_node_partition_f32, dr_patchify_f32,
 *          dr_node_correspondences_2d3d_f32, dr_mutual_nn_radius_f32, dr_radius_pairs_f32 (new entries only; nothing older changed).
 *   0.5.0  the 2D-3D point backbone: dr_group_norm_stats_f32, dr_group_norm_apply_f32, dr_group_norm_backward_f32, dr_knn_interpolate_f32,
 *          dr_knn_interpolate_backward_f32, dr_kpconv_neighbor_count_f32 and their workspace sizes (new entries only; nothing older changed).
 *   0.6.0  the 2D-3D fine loss: dr_fine_loss_f32, dr_fine_loss_backward_f32, their two size queries and the new struct dr_fine_loss_params
 *          (new entries only; nothing older changed).
 *   0.7.0  the 2D-3D evaluation metrics: dr_sparse_corr_eval_i64, dr_corr_eval_f32, dr_registration_eval_f64 and their workspace sizes (new
 *          entries only; dr_device_status can now also return DR_EINVAL: one of these entries skipped an index outside its range).
 *   0.7.0, second set (the number is unchanged: an existing check of the repository pins DR_ABI_VERSION to 700, and additions break no
 *          caller -- detect these entries by symbol)  the geometry head and feature-layout glue of the 2D-3D forward: dr_back_project_f32,
 *          dr_render_f32, dr_resize_tokens_f32, dr_resize_tokens_backward_f32, dr_rows_normalize_chw_f32, dr_rows_normalize_chw_backward_f32,
 *          dr_rows_normalize_chw_backward_rows_f32 (new entries only; nothing older changed).
 *   0.7.0, third set (same rule)  dr_rotary_planes_f32: the rotary + image tail of a DR_PL_PLANES launch on its own (new entry only).
 *   0.7.0, fourth set (same rule: a minor bump was asked for, and the pinned 700 of that older check forbids it)  the 2D-3D image backbone's
 *          inference forward on token rows: dr_conv2d_rows_f32, dr_resize_rows_f32 (new entries only; nothing older changed).
 *   0.7.0, fifth set (same rule)  the image backbone's backward on token rows: dr_conv2d_rows_backward_data_f32,
 *          dr_conv2d_rows_backward_weight_f32 with dr_conv2d_rows_backward_weight_workspace_bytes, dr_resize_rows_backward_f32 (new entries
 *          only; nothing older changed).
 *   0.7.0, seventh set (same rule)  the Depth-Anything DPT head's forward on token rows: dr_conv2d_rows_act_f32,
 *          dr_conv_transpose2d_rows_f32, dr_conv2d_rows_project_f32 (new entries only; nothing older changed).
 *   0.7.0, eighth set (same rule)  Depth-Anything's float32 ViT encoder forward: dr_gemm_rows_f32, dr_patch_rows_f32, dr_vit_forward_f32 with
 *          dr_vit_workspace_bytes_f32 (new entries only; nothing older changed).
 *   0.7.0, ninth set (same rule)  the 2D-3D loader's graph pyramid and neighbour-limit calibration: dr_grid_subsample_vision3d_f32,
 *          dr_radius_count_hist_f32 with dr_radius_count_hist_workspace_bytes (new entries only; nothing older changed).
 *   0.7.0, tenth set (same rule)  the input transform in front of Depth-Anything: dr_image_cubic_chw_f32 with the new struct dr_image_norm
 *          (new entry only; nothing older changed).
 *   0.7.0, eleventh set (same rule)  the ground-truth half of the 3D / 4D training collate: dr_blend_flow_knn3_f32, dr_coarse_gt_matches_f32 with
 *          dr_coarse_gt_matches_workspace_bytes (new entries only; nothing older changed).
 *   0.7.0, twelfth set (same rule)  the gradient gate and the optimizer update: dr_grads_finite_multi_f32, dr_sgd_step_multi_f32,
 *          dr_adam_step_multi_f32, dr_optim_finish with the new structs dr_optim_tensor, dr_sgd_options, dr_adam_options (new entries only;
 *          nothing older changed).
 *   0.7.0, thirteenth set (same rule)  the pixel-point ground truth of a 2D-3D dataset item: dr_corr_2d3d_mutual_f64, dr_corr_2d3d_radius_f64,
 *          dr_overlap_2d3d_f64 with their workspace size queries, dr_column_mean_seq_f32 (new entries only; nothing older changed).
 *   0.7.0, fourteenth set (same rule)  non-rigid ICP on an embedded deformation graph: dr_ed_graph_f32, dr_ed_warp_f32, dr_nicp_cost_grad_f32,
 *          dr_nicp_adam_f32 with their size queries (new entries only; nothing older changed).
 *   0.7.0, fifteenth set (same rule)  the 3D / 4D dataset item: dr_item3d_prepare_f32 with the new struct dr_item3d_args,
 *          dr_radius_pairs_ragged_f32 with dr_radius_pairs_ragged_workspace_bytes (new entries only; dr_radius_pairs_f32 is unchanged).
 *   0.7.0, sixteenth set (same rule)  Gauss-Newton non-rigid ICP: dr_nicp_gn_f32, dr_nicp_gn_normal_f32 with dr_nicp_gn_workspace_bytes and the
 *          new struct dr_nicp_gn_options, dr_spd_solve_f64 (new entries only; nothing older changed).
 *   0.7.0, seventeenth set (same rule)  furthest-point sampling: dr_fps_nodes_f32, dr_fps_batch_f32 with dr_fps_workspace_bytes and
 *          dr_fps_onchip_capacity (new entries only; nothing older changed).
 *   0.7.0, eighteenth set (same rule)  the geodesic deformation graph: dr_geo_graph_f32, dr_geo_graph_edges with dr_geo_graph_workspace_bytes,
 *          dr_geo_graph_onchip_capacity and the new struct dr_geo_graph_options (new entries only; nothing older changed).
 *   0.7.0, nineteenth set (same rule)  the non-rigid evaluation: dr_knn_points_f32 with dr_knn_points_max_k / _tile / _block, dr_nn_stats_f32
 *          with dr_nn_stats_workspace_bytes, dr_flow_metrics_f32 with dr_flow_metrics_workspace_bytes (new entries only; nothing older changed).
 *   0.7.0, twentieth set (same rule)  the RANSAC-free rigid estimators: dr_weighted_procrustes_f32 with dr_lgr_wave_limit, dr_lgr_f32 with
 *          dr_lgr_workspace_bytes, dr_spatial_consistency_f32, dr_sc_row_sums_f32 with dr_sc_block / dr_sc_tile, dr_sc_leading_eigenvector_f32
 *          with dr_sc_leading_eigenvector_workspace_bytes (new entries only; nothing older changed).
 *   0.7.0, twenty-first set (same rule)  point-to-point ICP on the dense clouds: dr_icp_p2p_f32 with dr_icp_p2p_workspace_bytes,
 *          dr_grid_subsample_open3d_f32 (new entries only; nothing older changed). */
#define DR_ABI_VERSION 700
int dr_version(void);                 /* major*10000 + minor*100 + patch */
const char* dr_strerror(int code);
const char* dr_last_hip_error(void);  /* text of the last failing HIP call on this thread */

/* Device-side failures.  Every call above returns when its kernels are ENQUEUED, so a failure that only a running kernel can
 * detect cannot come back as a return value.  There is one such failure: the single-launch Sinkhorn of tiles beyond 256 x 256
 * exchanges column sums between workgroups that must all be resident; its spins are bounded, and a workgroup that gives up
 * writes NaN to every output entry it owns and sets a sticky, process-wide flag on the device.  The outputs of such a call are
 * UNSPECIFIED as a whole: a sibling workgroup that was scheduled late may have summed partials of peers that had moved on and
 * written finite but wrong values -- the flag, not the data, is the signal; whoever reads it first (with `clear`) consumes it.
 * dr_device_status is the ONE entry point that synchronises: it waits for `stream`, reads the flag (clearing it when `clear`
 * is non-zero) and returns DR_OK or DR_ETIMEOUT.  The host mirrors call it wherever they already synchronise to read a match
 * count.  (The launcher checks residency with the occupancy API and takes the multi-launch form when the launch would not
 * fit beside a second one, so the flag means something else holds the CUs: a foreign kernel, a CU mask, a partitioned device.)
 * Since ABI 0.7.0 the same word has a second bit: an evaluation entry (dr_sparse_corr_eval_i64, dr_corr_eval_f32) met an index outside its
 * range and skipped it, where the reference raises an IndexError -> DR_EINVAL (DR_ETIMEOUT wins when both are set).  Those entries look the
 * word's device address up once per device (hipGetSymbolAddress, then cached): dr_init does it for the device current at its call; on any other
 * device make the first call of such an entry OUTSIDE a stream capture. */
int dr_device_status(void* stream, int clear);

/* ---------------------------------------------------------------------------------------------
 * Sinkhorn with dustbins.  Replaces log_optimal_transport + exp + [:-1,:-1] slice
 * (3D/models/matching.py:61-93 and its call sites matching.py:207-216, pipeline.py:264-277,
 * pipeline.py:293-302) for B independent N x M tiles.
 *   scores      [B,N,M]   (f32 or f64 entry point)
 *   src_mask    [B,N] uint8 (torch.bool) or NULL = all valid;  tgt_mask [B,M] likewise
 *   bin_score   device pointer to ONE float (the nn.Parameter `bin_score`)
 *   iters       Sinkhorn iterations (3 everywhere in the reference)
 *   out         DR_SK_OUT_CONF: [B,N,M] = exp(logZ)[:, :-1, :-1];  DR_SK_OUT_LOG: [B,N+1,M+1] logZ
 *   workspace   dr_sinkhorn_workspace_bytes(...) bytes (0 for the register-resident f32 path)
 * flags:
 *   DR_SK_MINSHIFT    subtract the per-tile minimum first (pipeline.py:239,264 `x - x.min()`)
 *   DR_SK_APPLY_MASK  treat entries outside src_mask x tgt_mask as -inf (the masked_fill_ of
 *                     pipeline.py:296 / matching.py:209-211), whatever the buffer holds
 *   DR_SK_OUT_F32     (f64 entry point) write `out` as float -- the `.type(torch.float32)` of
 *                     pipeline.py:302
 *   DR_SK_STRICT      compute in the input dtype with the streaming kernel (fp64 state stays
 *                     fp64 end to end); default: scaling-form fp32 arithmetic on row-max-shifted
 *                     exponentials held in registers
 * Marginals follow the reference with masks: every padded row/column keeps mass (quirk Q19).
 */
#define DR_SK_OUT_CONF 0x0
#define DR_SK_OUT_LOG 0x1
#define DR_SK_MINSHIFT 0x2
#define DR_SK_APPLY_MASK 0x4
#define DR_SK_OUT_F32 0x8
#define DR_SK_STRICT 0x10
/* DR_SK_RAGGED (with masks): rows / columns outside the masks do not exist -- no marginal mass, no dustbin share --
 * so a padded tile gives exactly the result of its unpadded (ms x ns) problem.  Without it padded rows / columns
 * keep their marginal mass like the reference's batched call does (quirk Q19), which is NOT the B = 1 result. */
#define DR_SK_RAGGED 0x20

size_t dr_sinkhorn_workspace_bytes(int B, int N, int M, int elem_bytes, int flags);

int dr_sinkhorn_f32(int B, int N, int M, const float* scores, const uint8_t* src_mask,
                    const uint8_t* tgt_mask, const float* bin_score, int iters, int flags,
                    float* out, void* workspace, size_t workspace_bytes, void* stream);

/* OPT-IN reduced precision (SURVEY 8b lists dr_sinkhorn_f16; never used by the loop): the score tiles and the confidences are stored as
 * IEEE fp16 -- half the bytes of an HBM-bound op -- the iteration itself runs in fp32 registers exactly like dr_sinkhorn_f32.  Tiles of up to
 * 256 x 256 (the register-resident kernel: BASELINE cfg1 / cfg2 sizes; DR_ENOSUP beyond); flags as dr_sinkhorn_f32 except DR_SK_STRICT /
 * DR_SK_OUT_LOG.  Outside the 1e-4 contract by construction: an fp16 confidence carries 11 bits. */
int dr_sinkhorn_f16(int B, int N, int M, const void* scores_f16, const uint8_t* src_mask, const uint8_t* tgt_mask, const float* bin_score,
                    int iters, int flags, void* out_f16, void* stream);
int dr_sinkhorn_f64(int B, int N, int M, const double* scores, const uint8_t* src_mask,
                    const uint8_t* tgt_mask, const float* bin_score, int iters, int flags,
                    void* out /* double*, or float* with DR_SK_OUT_F32 */, void* workspace,
                    size_t workspace_bytes, void* stream);


/* ---------------------------------------------------------------------------------------------
 * dr_init: sets kernel attributes (dynamic LDS sizes).  Call once per process before the first
 * launch and before any stream capture (the Python loader does).
 */
int dr_init(void);

/* Per-kernel-family timing with HIP events recorded on the launch stream, for bench.py's roofline
 * line.  Families: 0 gemm (f32-input MFMA kernels), 1 attention, 2 layernorm, 3 position code, 4 sinkhorn,
 * 5 procrustes, 6 state (min / ddim / read-out), 7 gemm_split (packed-weight split-operand kernels).  work[k] = algorithmic FLOPs (gemm, attention) or bytes (others)
 * summed over the recorded launches.  Do not enable during a stream capture. */
#define DR_PROF_KINDS 8
void dr_prof_enable(int on);
int dr_prof_collect(int* calls, double* ms, double* work);

/* ---------------------------------------------------------------------------------------------
 * VolumetricPositionEncoding.forward (3D/models/position_encoding.py:49-87) of `rows` points,
 * optionally warped first by a per-pair rigid motion  p' = R p + t  (3D/models/pipeline.py:306).
 *   xyz [rows,3]; R [rows/rows_per_pair, 9] row-major and t [.., 3], both NULL for no warp
 *   freq [C/6] = exp(arange(0, C/3, 2) * (-ln 1e4 / (C/3)))  (device; the caller computes it so the
 *               table is bit-identical to torch's)
 *   cos_out, sin_out [rows, C/2]: entry a*(C/6)+k is the angle of channels 2(a*C/6+k) and +1
 *               (the reference stores each angle twice: position_encoding.py:74-79)
 */
int dr_vol_pe_f32(int rows, int rows_per_pair, int C, const float* xyz, const float* R, const float* t,
                  float origin_x, float origin_y, float origin_z, float voxel, const float* freq,
                  float* cos_out, float* sin_out, void* stream);

/* nn.Linear without bias (+ optional rotary / ReLU / scale epilogue): out[rows,ncols] = x W^T.
 * epilogue bits: 1 = ReLU, 2 = rotary with cos/sin [rows, rot_C/2] (embed_rotary,
 * position_encoding.py:25-35).  Used by the parity tests of the GEMM kernel. */
int dr_linear_f32(int rows, int ncols, int K, const float* x, const float* W, float* out, int epilogue,
                  const float* cos_t, const float* sin_t, int rot_C, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Plane images: the layer nn.Linears of the loop with BOTH operands pre-split into fp16 hi / lo planes (the
 * default path of dr_denoise_loop for C <= 576, C % 16 == 0; 3D/models/transformero.py:26-96; column-block geometries of
 * 256 / 448 / 576 columns: C <= 256 -- the 2D-3D layer -- packs 256-row weight blocks).
 * Image of X [rows, K] (K % 16 == 0, rows padded to a multiple of 128): [row / 128][k / 16][row % 128][64 bytes], the
 * 64 bytes = 16-byte units (hi k 0..7 | hi k 8..15 | lo k 0..7 | lo k 8..15) stored at unit ^ ((row >> 2) & 3);
 * hi = fp16(x 2^s), lo = fp16(x 2^s - hi), s = 14 - floor(log2(bound[row])) with bound[row] >= max |x[row][:]| (an
 * upper bound that producers propagate analytically, so nobody sweeps a row for its maximum).  x = (hi + lo) 2^-s
 * keeps 22 significand bits for |x| >= 2^-17 bound and is rounded to 2^-40 bound absolutely below.
 * A 128-row block of one k-chunk is 8 KB contiguous and is the LDS image of the GEMM: operands stream by LDS-DMA.
 */
size_t dr_plane_image_bytes(int rows, int K);
/* fp32 rows -> image, bound[row] = max |x[row][:]| (the external features entering the first layer) */
int dr_planes_from_f32(int rows, int K, const float* x, int ldx, void* image, float* bound, void* stream);
/* the same with the caller's bounds (bound_in[row] >= max |x[row][:]|; e.g. one bound for all the key rows of a pair) */
int dr_planes_from_f32_bounded(int rows, int K, const float* x, int ldx, const float* bound_in, void* image, float* bound, void* stream);
/* einsum / mask / softmax / einsum of GeometryAttentionLayer.forward (3D/models/transformero.py:79-85) on plane images: P segments of
 * Lq queries attending Lk keys (rows p Lq .. / p Lk .. of the images), H heads of d features laid out head-padded (head h at
 * k = h dp, dp = d rounded up to 16, zeros in the pad; images of H dp columns).  All key rows of a segment must carry ONE k bound
 * and ONE v bound (read at the segment's first key row).  Three fp16 MFMA products per fp32 product, K / V tiles by LDS-DMA.
 * out_image: the merge projection's operand (same layout), out_bound [P Lq].  d in {64, 108, 132} (dp 64, 112, 144). */
int dr_attention_planes(int P, int Lq, int Lk, int H, int d, const void* q_image, const float* q_bound, const void* k_image,
                        const float* k_bound, const void* v_image, const float* v_bound, const uint8_t* q_mask, const uint8_t* k_mask,
                        void* out_image, float* out_bound, void* stream);
/* OPT-IN reduced precision: the same op with ONE fp16 product per contraction (the hi planes of q, k, v and of P only) instead of three --
 * what dr_loop_config.flags & DR_LOOP_ATTN_F16 selects inside the loops.  11-bit operands: outside the 1e-4 contract, never a default. */
int dr_attention_planes_f16(int P, int Lq, int Lk, int H, int d, const void* q_image, const float* q_bound, const void* k_image,
                            const float* k_bound, const void* v_image, const float* v_bound, const uint8_t* q_mask, const uint8_t* k_mask,
                            void* out_image, float* out_bound, void* stream);
/* image -> fp32 rows (tests) */
int dr_planes_to_f32(int rows, int K, const void* image, const float* bound, float* out, int ldo, void* stream);
/* weights W [nblk * C, K] (nn.Linear layout; nblk stacked layers of C output columns each, C <= 448, C % 16 == 0) ->
 * packed image + per-column scales + per-block L1 norms.  The k order of the image is
 * k' = (k / piece_len) * piece_pad + k % piece_len (zeros where k' % piece_pad >= piece_len): piece_len = piece_pad = K for
 * the identity; (d, round_up(d, 16)) for the merge projection behind the attention kernel's head-padded image. */
size_t dr_plane_weight_bytes(int nblk, int C, int K, int piece_len, int piece_pad);
int dr_pack_weight_planes_f32(int nblk, int C, int K, int piece_len, int piece_pad, const float* W, void* packed, void* stream);
/* The same weights in the WIDE-WAVE layout (round 6; C <= 576, C % 16 == 0): every block of C output columns as two sub-blocks of 288 weight
 * rows -- what the 128 x 288 workgroups of the DR_PL_F32 / DR_PL_PLANES launches of the 576-column geometry stream (4DMatch: C = 528, heads padded
 * to 144).  Pass the buffer with dr_planes_linear.weight_layout = DR_PL_LAYOUT_WIDE; DR_PL_LN launches take the block layout only. */
size_t dr_plane_weight_bytes_wide(int nblk, int C, int K, int piece_len, int piece_pad);
int dr_pack_weight_planes_wide_f32(int nblk, int C, int K, int piece_len, int piece_pad, const float* W, void* packed, void* stream);
/* *out = (sqrt(C) max|gamma| + max|beta|): upper bound of |LayerNorm(.) gamma + beta| (device scalar) */
int dr_ln_bound_f32(int C, const float* gamma, const float* beta, float* out, void* stream);

#define DR_PL_F32 0     /* out[row][nb * blk_stride + c] = rotary(acc) * scale                                      */
#define DR_PL_PLANES 1  /* out_image (+ out_bound) = [relu](acc); bound = max(bound0, bound1) * ||W_nb||            */
#define DR_PL_LN 2      /* y = LayerNorm(acc) gamma + beta [+ resid]; -> out (optional) and out_image (optional)    */
typedef struct {
    int rows, C, nblk;             /* out columns = nblk blocks of C                                                  */
    const void* a0; const float* bound0; int k0;   /* A operand = [a0 | a1] along k (images + their bounds)           */
    const void* a1; const float* bound1; int k1;   /* a1 may be NULL                                                  */
    const void* packed;            /* dr_pack_weight_planes_f32 of W [nblk * C, k0 + k1] (same k order as the images)  */
    int mode;                      /* DR_PL_*                                                                         */
    float* out; int ldo; int blk_stride;
    const float* cos_t; const float* sin_t; int rot_mask; int rot_C; float scale;   /* bit nb of rot_mask: rotary      */
    void* out_image; int out_image_k; int out_k0; float* out_bound;   /* block nb -> columns out_k0 + nb * C ..        */
    int relu;
    const float* gamma; const float* beta; const float* resid; int ldr; const float* bound_resid; const float* ln_bound;
    /* nn.Linear bias [nblk * C] (NULL = none), added before rotary / ReLU / LayerNorm; bias_max [nblk] (device, dr_bias_max_f32):
     * an upper bound of |bias| per block, needed with DR_PL_PLANES (it enters the bound the image is scaled by) */
    const float* bias; const float* bias_max;
    /* DR_PL_LN with resid: 0 = y = LayerNorm(acc) gamma + beta + resid (3D/models/transformero.py:94-96);
     *                      1 = y = LayerNorm(acc + resid) gamma + beta (the vision3d layer, vision3d/layers/transformer.py:188-196, 262-271) */
    int ln_postadd;
    /* DR_PL_PLANES: `out` (optional) also receives the block as fp32 rows (ldo, blk_stride as in DR_PL_F32) */
    int weight_layout;             /* DR_PL_LAYOUT_*: how `packed` was packed (ABI 0.2.1)                                */
    /* ABI 0.2.2, optional (NULL = never): dr_plane_split_workspace_bytes(C) bytes of device memory.  With it, a launch that would fill at most
     * half the chip (a DR_PL_LN launch of 64-row workgroups; a DR_PL_LAYOUT_WIDE launch of 128 x 288 tiles) splits every tile's k range over
     * TWO workgroups that swap half of their partial sums (the loops do this with their own workspace).  The first word of the workspace is a
     * status word: dr_plane_split_status() -> DR_ETIMEOUT if a workgroup's partner never arrived (its rows are NaN then). */
    void* split_workspace; size_t split_workspace_bytes;
} dr_planes_linear;
size_t dr_plane_split_workspace_bytes(int C);
int dr_plane_split_status(void* split_workspace, void* stream, int clear);
#define DR_PL_LAYOUT_BLOCK 0   /* dr_pack_weight_planes_f32                                                           */
#define DR_PL_LAYOUT_WIDE 1    /* dr_pack_weight_planes_wide_f32 (DR_PL_F32 / DR_PL_PLANES only)                      */
int dr_linear_planes_f32(const dr_planes_linear* args, void* stream);
/* The tail of a DR_PL_PLANES launch on its own, for projections whose input stays while the rotary code moves: x [rows, ldx] holds what
 * dr_linear_planes_f32 wrote in DR_PL_F32 mode with rot_mask = 0 and scale = 1 (block nb at column nb * x_blk); this applies the rotary code
 * (bit nb of rot_mask; cs_t [rows, rot_C / 2, 2] = (cos, sin) interleaved), `scale`, and writes block nb's plane image of C columns at
 * out_image + nb * image_blk_stride and its row bounds at out_bound + nb * bound_blk_stride -- byte for byte what the DR_PL_PLANES launch of the
 * same problem (a0 with bound0, `packed` of nblk blocks over k columns) writes with out_image_k = C per block. */
int dr_rotary_planes_f32(int rows, int C, int nblk, const float* x, int ldx, int x_blk, const float* cs_t, int rot_mask, int rot_C, float scale,
                         const float* bound0, const void* packed, int k, int weight_layout, void* out_image, long long image_blk_stride,
                         float* out_bound, long long bound_blk_stride, void* stream);
/* out[b] = max |bias[b n .. b n + n - 1]| (1 + 1e-4), b < nblk */
int dr_bias_max_f32(int nblk, int n, const float* bias, float* out, void* stream);

/* strided batch of the same product: out[z] [rows, ncols] = A[z] [rows, K] W[z]^T (W[z] [ncols, K]) * scale, z < nbatch, operands contiguous with the
 * given strides (floats); K % 4 == 0.  The N x M similarity of a batch of pairs (matching.py:190-196); the per-head products of the training backward. */
int dr_gemm_nt_batched_f32(int nbatch, int rows, int ncols, int K, const float* A, long long stride_a, const float* W, long long stride_w, float* out,
                           long long stride_o, float scale, void* stream);

/* nn.Linear with a bias and explicit leading dimensions (x [rows, lda], out [rows, ldo]): the 1x1 Conv1d `coarse_out`
 * of the backbone (3D/models/backbone.py:66, 155-156) and its UnaryBlocks (bias = NULL). */
int dr_linear_ex_f32(int rows, int ncols, int K, const float* x, int lda, const float* W, const float* bias, float* out,
                     int ldo, int epilogue, float scale, void* stream);

/* ---- KPFCN backbone ops (3D/models/blocks.py) -------------------------------------------------------
 * dr_kpconv_gather_f32: the gather / influence / neighbour-reduction half of KPConv.forward (blocks.py:288-375) with
 *   the neighbour-count normalisation (blocks.py:390-393) folded in:
 *     weighted[q][k*Cin + c] = (sum_h max(0, 1 - |s[nb[q][h]] - q_q - kp_k| / extent) * x[nb[q][h]][c]) / num_q
 *   neighb_inds [Nq,H] int64 with the shadow index Ns (zero features, point at +1e6); num_q = max(1, #neighbours whose
 *   feature sum is > 0).  The other half is ONE dr_linear_*: out = weighted @ W2^T with W2[co][k*Cin + c] =
 *   weights[k][c][co] (the reference multiplies per kernel point and sums over K, blocks.py:382-387).
 *   ld_weighted >= K*Cin (padding columns are zeroed).  K <= 16, H <= 64.
 * dr_col_stats_f32 / dr_norm_apply_f32: BatchNormBlock with use_bn = InstanceNorm1d over the points of the stacked cloud
 *   per channel, no affine, biased variance, eps 1e-5 (blocks.py:430-446): mean / rstd per column, then
 *     out = act( (a - mean_a) rstd_a + [ (b - mean_b) rstd_b  |  b  |  0 ] ),  act = LeakyReLU(leaky_slope) or none
 *   (UnaryBlock blocks.py:479-484; the residual sum of ResnetBottleneckBlock blocks.py:650-660).
 * dr_gather_pool_f32: max_pool (first_only = 0) / closest_pool (first_only = 1) of blocks.py:56-87; indices >= n1 read
 *   a zero row. */
int dr_kpconv_gather_f32(int Nq, int Ns, int H, int Cin, int K, const float* q_pts, const float* s_pts,
                         const int64_t* neighb_inds, const float* x, const float* kernel_points, float extent,
                         float* weighted, int ld_weighted, void* stream);
/* the same with the options of KPConv no shipped yaml selects (blocks.py:304-326; ABI 0.2.1): influence DR_KP_CONSTANT (every neighbour weighs 1),
 * DR_KP_LINEAR (dr_kpconv_gather_f32) or DR_KP_GAUSSIAN (exp(-d^2 / (2 (0.3 extent)^2 + 1e-9))); closest != 0 = aggregation_mode 'closest': a
 * neighbour contributes through its nearest kernel point only (first minimum, as torch.argmin). */
#define DR_KP_CONSTANT 0
#define DR_KP_LINEAR 1
#define DR_KP_GAUSSIAN 2
int dr_kpconv_gather_mode_f32(int Nq, int Ns, int H, int Cin, int K, const float* q_pts, const float* s_pts, const int64_t* neighb_inds,
                              const float* x, const float* kernel_points, float extent, int influence, int closest, float* weighted,
                              int ld_weighted, void* stream);
size_t dr_col_stats_workspace_bytes(int N, int C);
int dr_col_stats_f32(int N, int C, const float* x, int ldx, float* mean, float* rstd, void* workspace,
                     size_t workspace_bytes, void* stream);
int dr_norm_apply_f32(int N, int C, const float* a, int lda, const float* mean_a, const float* rstd_a, const float* b,
                      int ldb, const float* mean_b, const float* rstd_b, float leaky_slope, int activate, float* out,
                      int ldo, void* stream);
int dr_gather_pool_f32(int n2, int H, int ld_inds, int d, const float* x, int n1, const int64_t* inds, int first_only,
                       float* out, void* stream);

/* Backward of the three ops above (the backbone's training path; the nn.Linear halves are products on dr_linear_*):
 * dr_kpconv_gather_backward_f32: grad_x [Ns, Cin] (zeroed here, then fp32 atomics) from grad_weighted [Nq, ld_weighted]; kernel points and
 *   point positions carry no gradient (the shipped configuration: rigid kernels), the neighbour count is piecewise constant.
 * dr_norm_backward_f32: out = act(xhat_a + [xhat_b | b | 0]) as dr_norm_apply_f32 computed it -> grad_a (and grad_b when b took part);
 *   `out` is the forward result (the LeakyReLU's derivative is read off its sign).  Two float64 column reductions over a fixed grid.
 * dr_gather_pool_backward_f32: the gradient of a pooled row goes to its first maximal neighbour (torch.max) / its first neighbour. */
int dr_kpconv_gather_backward_f32(int Nq, int Ns, int H, int Cin, int K, const float* q_pts, const float* s_pts, const int64_t* neighb_inds,
                                  const float* x, const float* kernel_points, float extent, const float* grad_weighted, int ld_weighted,
                                  float* grad_x, void* stream);
int dr_kpconv_gather_backward_mode_f32(int Nq, int Ns, int H, int Cin, int K, const float* q_pts, const float* s_pts, const int64_t* neighb_inds,
                                       const float* x, const float* kernel_points, float extent, int influence, int closest,
                                       const float* grad_weighted, int ld_weighted, float* grad_x, void* stream);
size_t dr_norm_backward_workspace_bytes(int N, int C);
int dr_norm_backward_f32(int N, int C, const float* grad_out, int ldg, const float* out, int ldo, const float* a, int lda, const float* mean_a,
                         const float* rstd_a, const float* b, int ldb, const float* mean_b, const float* rstd_b, float leaky_slope, int activate,
                         float* grad_a, int ldga, float* grad_b, int ldgb, void* workspace, size_t workspace_bytes, void* stream);
int dr_gather_pool_backward_f32(int n2, int H, int ld_inds, int d, const float* x, int n1, const int64_t* inds, int first_only, const float* grad_out,
                                float* grad_x, void* stream);

/* weights of one GeometryAttentionLayer in the reference state-dict layout ([out,in] row-major;
 * 3D/models/transformero.py:26-41): host struct of device pointers */
typedef struct {
    const float *q_proj, *k_proj, *v_proj, *merge; /* [C,C]          */
    const float *mlp0;                             /* [2C,2C]        */
    const float *mlp2;                             /* [C,2C]         */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b; /* [C]       */
} dr_layer_weights;

/* GeometryAttentionLayer.forward(x, source, x_pe, source_pe, x_mask, source_mask)
 * (3D/models/transformero.py:43-96) for P independent pairs:
 *   x [P*Lx, C], y [P*Ly, C]; cos/sin tables [P*Lx, C/2] and [P*Ly, C/2]; masks uint8 or NULL
 *   out [P*Lx, C] = x + LN2(mlp([x, LN1(merge(attn))]))
 *   workspace: dr_attention_layer_workspace_bytes(P, Lx, Ly, C)
 */
size_t dr_attention_layer_workspace_bytes(int P, int Lx, int Ly, int C);
int dr_attention_layer_f32(const dr_layer_weights* w, int C, int H, int P, int Lx, int Ly, const float* x,
                           const float* y, const float* cos_x, const float* sin_x, const float* cos_y,
                           const float* sin_y, const uint8_t* x_mask, const uint8_t* y_mask, float* out,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The same layer for the configuration branches no shipped yaml selects (3D/models/transformero.py:50-57, 246-252;
 * configs/test/3dmatch.yaml:45 "options: ['rotary', 'sinusoidal']", :1 "entangled"):
 *   cos_x .. sin_y all NULL : no rotary code on q and k -- pe_type 'sinusoidal', or a layer called without position codes (entangled = True);
 *   xq [P*Lx, C], yk [P*Ly, C] (both or neither; only without rotary tables): the inputs of the q and k projections where they are not x and y --
 *     the sinusoidal form q = W_q (x + pe_x), k = W_k (y + pe_y), v = W_v y; the residual and the mlp's cat[x, message] keep x.
 * Same workspace.  dr_attention_layer_f32 is this entry with xq = yk = NULL and all four tables given. */
int dr_attention_layer_pe_f32(const dr_layer_weights* w, int C, int H, int P, int Lx, int Ly, const float* x, const float* y,
                              const float* xq, const float* yk, const float* cos_x, const float* sin_x, const float* cos_y,
                              const float* sin_y, const uint8_t* x_mask, const uint8_t* y_mask, float* out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* The same layer for TRAINING (what torch autograd records through transformero.py:43-96): the forward that keeps what its
 * backward needs, and the whole backward, one call each -- every kernel launched inside the library (the per-op entries further down drive the same
 * kernels one by one).  x [B*L, C], y [B*S, C] contiguous; rotary tables [B*L, C/2] / [B*S, C/2]; masks uint8 [B*L] / [B*S] or both NULL.
 *   forward : out [B*L, C]; `saved` = caller memory of dr_attention_layer_train_saved_bytes(B, L, S, C): q | k (rotary applied) | v | heads' output |
 *             merge output | norm1 output | hidden activation | mlp output | (mean, rstd) of both LayerNorms -- opaque to the caller, handed to the backward
 *   backward: grad_out [B*L, C] -> grad_x [B*L, C], grad_y [B*S, C] (separate buffers also when x == y: the caller adds them) and the ten parameter
 *             gradients (dr_layer_grads: the layout of dr_layer_weights; overwritten, not accumulated).  Position codes are constants of the graph
 *             (the reference detaches them, position_encoding.py:83-84).  workspace: dr_attention_layer_backward_workspace_bytes(B, H, L, S, C). */
typedef struct {
    float *q_proj, *k_proj, *v_proj, *merge; /* [C,C]          */
    float *mlp0;                             /* [2C,2C]        */
    float *mlp2;                             /* [C,2C]         */
    float *norm1_w, *norm1_b, *norm2_w, *norm2_b; /* [C]       */
} dr_layer_grads;
size_t dr_attention_layer_train_saved_bytes(int B, int L, int S, int C);
int dr_attention_layer_train_forward_f32(const dr_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                         const float* cos_x, const float* sin_x, const float* cos_y, const float* sin_y,
                                         const uint8_t* x_mask, const uint8_t* y_mask, float* out, void* saved, size_t saved_bytes, void* stream);
size_t dr_attention_layer_backward_workspace_bytes(int B, int H, int L, int S, int C);
int dr_attention_layer_backward_f32(const dr_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                    const float* cos_x, const float* sin_x, const float* cos_y, const float* sin_y, const uint8_t* x_mask,
                                    const uint8_t* y_mask, const void* saved, const float* grad_out, float* grad_x, float* grad_y,
                                    const dr_layer_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* SoftProcrustesLayer.forward (3D/models/procrustes.py:48-93): top-K of conf, weighted Kabsch,
 * fp64 3x3 SVD ON DEVICE (replaces the .cpu().double().svd() of procrustes.py:35-36), gate.
 *   conf [P,N,M] float32; src_pcd [P,N,3]; tgt_pcd [P,M,3]
 *   use_mask_len: 0 = K from the padded sizes (3D, 2D3D), 1 = K from the mask sums (4D variant,
 *                 4D/models/procrustes.py:61-62)
 *   R,t = solution; R_forwd,t_forwd = solution or identity when cond >= max_condition_num;
 *   topk_idx (optional, [P,K]) flat indices i*M+j of the selected entries (a set: unordered)
 *   Ties at the K-th value: the lowest flat indices are taken (torch.topk leaves that choice implementation-defined).
 *   workspace: dr_procrustes_workspace_bytes(P, N, M) bytes (0 for tiles up to 256 x 256: pass NULL); tiles beyond that select
 *   with the whole chip and need it -- DR_EWORKSPACE when it is missing or too small.
 */
size_t dr_procrustes_workspace_bytes(int P, int N, int M);
int dr_procrustes_f32(int P, int N, int M, const float* conf, const float* src_pcd, const float* tgt_pcd,
                      const uint8_t* src_mask, const uint8_t* tgt_mask, int use_mask_len, float sample_rate,
                      float max_condition_num, float* R, float* t, float* R_forwd, float* t_forwd,
                      double* condition, int32_t* solution_mask, int32_t* topk_idx, void* workspace, size_t workspace_bytes,
                      void* stream);

/* d loss / d conf of the fit above (4DMatch trains its L1 motion term through (R, t), 3D/models/loss.py:108-128): the K
 * entries dr_procrustes_f32 selected (topk_idx [P,K]) are the fit's weights, everything else gets 0.  grad_R [P,9], grad_t [P,3] are the
 * gradients of R and t (for R_forwd / t_forwd add them where solution_mask is set); k_count [P] (optional): entries of a pair that carry
 * weight (the 4D variant's K from the mask sums).  The adjoint of the 3 x 3 SVD in float64 on the device, replacing the reference's
 * autograd path through `Sxy.cpu().double().svd()` (procrustes.py:35-36).  grad_conf [P,N,M] is zeroed here. */
int dr_procrustes_backward_f32(int P, int N, int M, int K, const float* conf, const float* src_pcd, const float* tgt_pcd, const int32_t* topk_idx,
                               const int32_t* k_count, const float* grad_R, const float* grad_t, float* grad_conf, void* stream);

/* Diagnostics (kernel-forcing setters, phase stamps, the environment switch) are NOT part of the drop-in boundary: they are
 * declared in include/diffreg_hip_debug.h.  The library reads no environment variable unless dr_debug_enable_env(1) was called. */

/* mutual_topk_select(conf, k=1, largest=True, threshold=None, mutual=False) + the [0,i,j] rows of
 * 3D/models/pipeline.py:275-278.  matches [P, N+M, 3] int64 (first count[p] rows valid), ascending (i, j); the first
 * occurrence wins an arg-max tie.  N + M <= 4096.  From 32 rows on the arg-maxima come from row-block workgroups over the
 * whole chip, which need dr_top1_union_workspace_bytes(P, N, M, elem_bytes) bytes of workspace (elem_bytes 4 / 8; 0 = none
 * needed, pass NULL); DR_EWORKSPACE when it is missing or too small. */
size_t dr_top1_union_workspace_bytes(int P, int N, int M, int elem_bytes);
int dr_top1_union_f64(int P, int N, int M, const double* conf, int64_t* matches, int32_t* count, void* workspace,
                      size_t workspace_bytes, void* stream);
int dr_top1_union_f32(int P, int N, int M, const float* conf, int64_t* matches, int32_t* count, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Pipeline.split_feats (3D/models/pipeline.py:350-379): dst[dst_index[i]][:] = src[src_index[i]][:], i < n, rows of C floats
 * (the stacked coarse features / points of the backbone scattered into the zero-padded [B * N_max, C] tensors).
 * src has n_src_rows rows, dst n_dst_rows.  Indices behave like torch's indexed assignment: values in [-rows, -1] wrap; any other
 * out-of-range index is skipped (no access) and *status (device int32, optional, zeroed by the caller) is set to 1 -- where
 * PyTorch raises IndexError; the Python mirror reads the flag and raises. */
int dr_scatter_rows_f32(int n, int C, const float* src, int64_t n_src_rows, const int64_t* src_index, const int64_t* dst_index, float* dst,
                        int64_t n_dst_rows, int32_t* status, void* stream);

/* Matching.get_match(conf, thr, mutual) (3D/models/matching.py:126-143; what 4D/lib/tester.py:266 applies to conf_matrix_pred
 * with thr = 0.55, mutual = True): entries > thr that are also their row's and their column's maximum (mutual; ties all count,
 * like the reference's `==`), in nonzero() order.  matches [P, cap, 3] int64 rows (b, i, j), mconf [P, cap] (optional),
 * count [P] = the TRUE number of hits (rows beyond cap are dropped: pass cap = N * M to be safe, min(N, M) + slack in
 * practice), mask [P, N, M] uint8 (optional; the reference's third return value). */
int dr_mutual_match_f64(int P, int N, int M, const double* conf, double thr, int mutual, int cap, int64_t* matches, double* mconf,
                        int32_t* count, uint8_t* mask, void* stream);
int dr_mutual_match_f32(int P, int N, int M, const float* conf, float thr, int mutual, int cap, int64_t* matches, float* mconf,
                        int32_t* count, uint8_t* mask, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The whole reverse-diffusion loop of Pipeline.forward's eval branch
 * (3D/models/pipeline.py:221-283; 4D/models/pipeline.py:156-197) for P independent pairs, enqueued
 * on `stream` with no host synchronisation (so it can be captured in a HIP graph).
 */
#define DR_VARIANT_3DMATCH 0
#define DR_VARIANT_4DMATCH 1
#define DR_LOOP_STRICT_F64 0x1 /* run the fp64-state Sinkhorn calls in fp64 (streaming kernel) */
/* Pairs of different sizes in one call: pad every pair to (N, M), pass the true extents as masks, and
 * each pair gets exactly the result of its own unpadded B = 1 run: padded rows / columns are excluded from the
 * Sinkhorn marginals (DR_SK_RAGGED), from x.min(), from the top-K rule (K from the true sizes) and from the read-out. */
#define DR_LOOP_RAGGED 0x2
/* The layer GEMMs run on fp16 hi / lo plane images (pgemm, see "Plane images" above) when the configuration allows it
 * (C <= 448, C % 16 == 0) and the call has at least DR_PLANES_MIN_ROWS (environment, default 4096) token rows; these two
 * flags take the decision away from the size rule (tests hold the small golden loops to the reference through both paths) */
#define DR_LOOP_PLANES_FORCE 0x4
#define DR_LOOP_PLANES_OFF 0x8
/* OPT-IN reduced precision (never set by the host mirrors' defaults): on the plane path, the attention's two contractions (q k^T, P v) take ONE
 * fp16 MFMA product of the operands' hi planes instead of the three products that make an fp32-grade one -- what BASELINE's configs[2] / [4]
 * word as "bf16 / fp16 MFMA attention".  Softmax and accumulation stay fp32, the GEMMs keep three products.  11-bit operands: conf_matrix_pred
 * moves by ~1e-3 (bench.py other_configs reports the measured deviation and IR / FMR beside the rate); outside the 1e-4 contract by design. */
#define DR_LOOP_ATTN_F16 0x10

typedef struct {
    int variant;               /* DR_VARIANT_*                                              */
    int C, H, n_layers;        /* feature dim, heads, layers (self, cross, self, ... )       */
    int steps;                 /* SAMPLE_STEP                                                */
    int sk_iters;              /* skh_iters                                                  */
    float voxel, origin[3];    /* voxel_size, vol_bnds[0]                                    */
    float sample_rate, max_condition_num; /* procrustes config                              */
    int flags;                 /* DR_LOOP_*                                                  */
    const double* h_alphas_cumprod; /* HOST [1000] float64 (pipeline.py:151-156)             */
    const int32_t* h_times;    /* HOST [steps+1] reversed int(linspace(0,999,steps+1)), Q20  */
} dr_loop_config;

typedef struct {
    const dr_layer_weights* layers; /* HOST array [n_layers] of device-pointer structs       */
    const float* src_proj;     /* denoising_coarse_matching.src_proj.weight [C,C] (Q1)       */
    const float* bin_score;    /* device pointer to one float                                */
    const float* pe_freq;      /* device [C/6], see dr_vol_pe_f32                            */
    const void* prepacked;     /* dr_loop_prepack image of THESE weights (device, 256-byte aligned) or NULL: the loop
                                * then packs them into its workspace at every call (weights may change between calls) */
} dr_loop_weights;

/* The layer weights as fp16 hi / lo plane images + per-column scales + per-layer LayerNorm bounds, packed ONCE for the
 * life of an engine (immutable weights): pass the buffer as dr_loop_weights.prepacked.  0 bytes = this configuration does
 * not use the plane path (C > 448 or C % 16 != 0): leave prepacked NULL. */
size_t dr_loop_prepack_bytes(const dr_loop_config* cfg);
int dr_loop_prepack(const dr_loop_config* cfg, const dr_loop_weights* w, void* packed, size_t packed_bytes, void* stream);

typedef struct {                /* all optional (NULL to skip); per-step records for parity tests */
    float* x0;                 /* [steps,P,N,M]  x_start of every step                       */
    float* R_forwd;            /* [steps,P,9]                                                */
    float* t_forwd;            /* [steps,P,3]                                                */
    double* cond;              /* [steps,P]                                                  */
    /* the side effects Matching.forward leaves in `data` at the LAST step (3D/models/matching.py:177-187), token layout
     * [P*N + P*M, C] (all src rows, then all tgt rows): src_proj(feats) and its rotary-embedded form (before the 1/sqrt(C)) */
    float* feats_nopos;
    float* feats_pos;
    /* ---- ABI 0.2.0: teacher forcing, for per-step parity tests (tests/test_teacher_forced_gpu.py).  Every step of the loop is then an
     * independent evaluation of one pass through pipeline.py:237-256 (EXP/model.py:637-680) on a state the CALLER supplies, so a top-K
     * near-tie at one step cannot hide the steps behind it.  All optional; a struct zero-filled beyond `feats_pos` behaves like 0.1.0's.
     * force_x   [steps,P,N,M] float64: the state ENTERING step k is force_x[k] instead of the loop's own (step 0: x_T widened; x_T is ignored).
     * force_R / force_t [steps,P,9] / [steps,P,3] (both or neither): the warp of step k is this pose instead of the fit's R_forwd, t_forwd
     *           (the fit still runs and is still traced: R_forwd / t_forwd / cond / topk_idx are the loop's own).
     * x_next    [steps,P,N,M] float64: the state after step k's update (what the loop would carry into step k + 1).
     * topk_idx  [steps,P,K] int32, K = int(max(N,M) * sample_rate): flat indices i * M + j of the entries the fit of step k selected, in arrival
     *           order (a set); slots beyond a pair's own K (mask-length rule) keep -1.
     * wconf     [steps,P,N,M] float32: the warp confidences of step k, float32(exp(Z)[:N,:M]) of pipeline.py:299-302. */
    const double* force_x;
    const float* force_R;
    const float* force_t;
    double* x_next;
    int32_t* topk_idx;
    float* wconf;
} dr_loop_trace;

size_t dr_denoise_loop_workspace_bytes(const dr_loop_config* cfg, int P, int N, int M);

/* inputs : src_feats [P,N,C], tgt_feats [P,M,C], s_pcd [P,N,3], t_pcd [P,M,3] float32;
 *          src_mask [P,N], tgt_mask [P,M] uint8 or NULL; x_T [P,N,M] float32 (the randn of
 *          pipeline.py:224); noise [steps,P,N,M] float32 or NULL (xi, used by the 4D variant only)
 * outputs: conf [P,N,M] float64 (conf_matrix_pred); x_final [P,N,M] float64 (optional);
 *          matches [P,N+M,3] int64 + match_count [P] (3D variant; optional);
 *          R_final [P,9], t_final [P,3] float32: soft_procrustes of float32(conf) (optional; the
 *          reference's own call returns identity through a swallowed dtype error, quirk Q3)
 */
int dr_denoise_loop(const dr_loop_config* cfg, const dr_loop_weights* w, int P, int N, int M,
                    const float* src_feats, const float* tgt_feats, const float* s_pcd, const float* t_pcd,
                    const uint8_t* src_mask, const uint8_t* tgt_mask, const float* x_T, const float* noise,
                    double* conf, double* x_final, int64_t* matches, int32_t* match_count, float* R_final,
                    float* t_final, const dr_loop_trace* trace, void* workspace, size_t workspace_bytes,
                    void* stream);

/* The status of the LAST call that ran on `workspace` (dr_denoise_loop, dr_denoiser_match_f32, dr_denoise_loop_2d3d): waits for `stream`,
 * reads the workspace's own sticky word (zeroed when a call starts; clears it when `clear`) -> DR_OK, or DR_ETIMEOUT when a co-resident
 * Sinkhorn launch OF THAT CALL gave up waiting for another workgroup (its outputs then hold NaN).  Unlike dr_device_status this word
 * belongs to one workspace: concurrent engines (one workspace per stream) cannot swallow or misattribute each other's time-outs. */
int dr_denoise_loop_status(void* workspace, void* stream, int clear);

/* RepositioningTransformer.forward for layer types self/cross (3D/models/transformero.py:151-233)
 * + Matching.forward (3D/models/matching.py:164-219) on already-warped points, for P pairs:
 * one denoiser evaluation.  Outputs: src_out [P,N,C], tgt_out [P,M,C] (optional), conf [P,N,M]. */
int dr_denoiser_match_f32(const dr_loop_config* cfg, const dr_loop_weights* w, int P, int N, int M,
                          const float* src_feats, const float* tgt_feats, const float* s_pcd_warped,
                          const float* t_pcd, const uint8_t* src_mask, const uint8_t* tgt_mask, float* src_out,
                          float* tgt_out, float* conf, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation harness on device: the consumers of the loop's `match_pred`.
 * Match layout everywhere below: `matches` int64 [P, cap, 3] rows (b, src index, tgt index), the first
 * count[p] rows of segment p valid -- exactly what dr_denoise_loop / dr_top1_union_* write (cap = N+M).
 * The reference's flat [K,3] list of one pair (B = 1, 3D/lib/tester.py:115) is P = 1, cap = K, count = {K};
 * column 0 is not read (the segment is the pair).
 */

/* MatchMotionLoss.compute_inlier_ratio (3D/models/loss.py:383-410): warp the matched source points with the
 * ground-truth pose (+ optional scene flow, the 4DMatch call of 3D/lib/tester.py:267), count matches closer
 * than inlier_thr, float32 arithmetic.  rot [P,9], trn [P,3], s2t_flow [P,N,3] or NULL.
 * out: ir [P] float32 (0 when a pair has fewer than 3 matches, loss.py:403-404), n_inlier [P] int32. */
int dr_inlier_ratio_f32(int P, int cap, int N, int M, const int64_t* matches, const int32_t* count, const float* s_pcd,
                        const float* t_pcd, const float* rot, const float* trn, const float* s2t_flow, float inlier_thr,
                        float* ir, int32_t* n_inlier, void* stream);

/* compute_nrfmr + blend_anchor_motion (3D/lib/tester.py:127-210; knn_point_np 3D/datasets/utils.py:23-40):
 * the matches of a pair are motion anchors (t_pcd[j] - s_pcd[i] at s_pcd[i]); every metric point takes the
 * inverse-distance blend of its 3 nearest anchors (anchors beyond knn_radius get distance 1e10), and counts as
 * recalled when it lands within recall_thr of its ground-truth position rot (p + flow) + trn.
 *   raw_pcd, raw_flow [sum R_p, 3]: the un-subsampled source clouds and their scene flow, pair p at rows
 *   raw_offsets[p] .. raw_offsets[p+1];  metric_index int64 [sum Q_p] (indices into the pair's raw cloud), pair p at
 *   q_offsets[p] .. q_offsets[p+1]  (int32 offsets, P+1 entries each; max_q = the largest Q_p).
 * out: nrfmr [P] float32 (recalled / Q_p; 0 for a pair with fewer than 4 anchors, where the reference's
 * np.argpartition(kth=3) raises); n_recalled [P] int32; blended [sum Q_p, 3] float32 or NULL (the blended motion). */
int dr_nrfmr_f32(int P, int cap, int N, int M, const int64_t* matches, const int32_t* count, const float* s_pcd,
                 const float* t_pcd, const float* raw_pcd, const float* raw_flow, const int32_t* raw_offsets,
                 const int64_t* metric_index, const int32_t* q_offsets, int max_q, const float* rot, const float* trn,
                 float knn_radius, float recall_thr, float* nrfmr, int32_t* n_recalled, float* blended, void* stream);

/* MatchMotionLoss.ransac_regist_coarse -> ransac_pose_estimation (3D/models/loss.py:13-24, 347-379): Open3D 0.13.0
 * (3D/eccv24_3d_env.yml:139) registration_ransac_based_on_correspondence with ransac_n = 3,
 * TransformationEstimationPointToPoint(False), RANSACConvergenceCriteria(50000, 1000) (confidence clamps to 1: no
 * early exit, all `iters` hypotheses are scored).  Hypothesis h of pair p samples three correspondences with
 * replacement from a counter-based generator (splitmix64 of (seed, pair_ids[p], 3h + slot), restated in
 * oracle/metrics_oracle.py -- Open3D's own generator is unseeded, the reference repeats the evaluation three times
 * for that reason, tester.py:24), fits the rigid transform of the triple (Umeyama without scale, fp64), counts the
 * correspondences closer than distance_thr and keeps the best (more inliers; then lower inlier RMSE; then lower h).
 * Triples that repeat a source or a target point (rank-1 covariance: the roll angle is arbitrary) are skipped.
 * out (fp64 like the reference's `torch.from_numpy(pose)`): rot [P,9], trn [P,3]; identity / zero when a pair has
 * fewer than 3 matches (loss.py:363-366) or no hypothesis has an inlier; fitness [P], inlier_rmse [P] (optional),
 * best_iter [P] int32 (optional, -1 = none).   pair_ids int64 [P] or NULL (= 0..P-1). */
size_t dr_ransac_workspace_bytes(int P, int cap, int iters);
int dr_ransac_corr_f64(int P, int cap, int N, int M, const int64_t* matches, const int32_t* count, const float* s_pcd,
                       const float* t_pcd, double distance_thr, int iters, uint64_t seed, const int64_t* pair_ids,
                       double* rot, double* trn, double* fitness, double* inlier_rmse, int32_t* best_iter,
                       void* workspace, size_t workspace_bytes, void* stream);

/* MatchMotionLoss.compute_registration_recall + computeTransformationErr (3D/models/loss.py:27-44, 415-448):
 * e = [t, q_xyz] of inv(gt) * pred (q = unit quaternion of the rotation part, w >= 0; nibabel's mat2quat),
 * err = e^T info e / info[0][0], success = err <= thr^2.  rot_est [P,9], trn_est [P,3] float64; rot_gt [P,9],
 * trn_gt [P,3] float32; info [P,36] float64 (`gt_cov`).  out: err [P] float64, success [P] int32. */
int dr_registration_recall_f64(int P, const double* rot_est, const double* trn_est, const float* rot_gt,
                               const float* trn_gt, const double* info, double thr, double* err, int32_t* success,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Collate-time native code on device: the two C++ extensions the reference's data loader calls to build
 * the KPFCN index arrays (3D/datasets/dataloader.py:13-68, 120-200).  Clouds are stacked: `lengths` int32 [nb] (device).
 * Nothing synchronises; `status` (device int32) becomes 1 when a cloud spans more than 65 533 cells on an axis.
 */

/* cpp_subsampling.subsample_batch(points, batches_len, sampleDl) -> batch_grid_subsampling
 * (cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:4-211, max_p = 0): barycentre of every occupied voxel,
 * summed in float32 in input order (bit-exact).  out_points has room for n rows; the first out_total[0] are written, per
 * cloud in ascending (iz, iy, ix) voxel order (the reference emits std::unordered_map iteration order; consumers are
 * permutation-equivariant); out_lengths [nb]. */
size_t dr_grid_subsample_workspace_bytes(int n, int nb);
int dr_grid_subsample_f32(int n, int nb, const float* points, const int32_t* lengths, float dl, float* out_points,
                          int32_t* out_lengths, int32_t* out_total, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream);

/* cpp_neighbors.batch_query(queries, supports, q_batches, s_batches, radius)[:, :limit] -> batch_nanoflann_neighbors
 * (cpp_wrappers/cpp_neighbors/neighbors/neighbors.cpp:210-333) + the truncation of dataloader.py:64-65: for every query the
 * supports of its own cloud with squared distance < radius^2 (float32, nanoflann's L2_Simple_Adaptor order of operations),
 * nearest first (equal distances: lower index first; the reference's std::sort leaves them unspecified), as indices into the
 * stacked supports, padded with ns.  out int64 [nq, limit] (limit <= 64); max_count[0] = the largest neighbourhood found
 * (the reference's matrix is min(max_count, limit) wide: the caller slices). */
size_t dr_radius_neighbors_workspace_bytes(int nq, int ns, int nb);
int dr_radius_neighbors_f32(int nq, int ns, int nb, const float* queries, const float* supports, const int32_t* q_lengths,
                            const int32_t* s_lengths, float radius, int limit, int64_t* out, int32_t* max_count, int32_t* status,
                            void* workspace, size_t workspace_bytes, void* stream);

/* batch_mutual_topk_select / mutual_topk_select (Diff-Reg-2d3d/vision3d/ops/mutual_topk_select.py:7-134; the fine matching
 * behind the 2D-3D loop, EXP/model.py:744-752: k = 2, threshold 0.75, mutual): per batch element the entries among the k best of
 * their row and (mutual) / or of their column, beyond `threshold` when use_threshold (> for largest, < otherwise), inside
 * row_masks [B,N] / col_masks [B,M] (NULL = all).  out_idx int64 [capacity,3] rows (b, i, j) in torch.nonzero order, out_score
 * [capacity]; total[0] = number selected (entries beyond capacity are counted, not written).  k <= min(8, N, M) (DR_EINVAL beyond: torch.topk raises there), N*M <= 262144. */
size_t dr_mutual_topk_workspace_bytes(int B, int N, int M);
int dr_mutual_topk_select_f32(int B, int N, int M, const float* score, int k, int largest, int use_threshold, float threshold,
                              int mutual, const uint8_t* row_masks, const uint8_t* col_masks, int64_t* out_idx, float* out_score,
                              long long capacity, int32_t* total, void* workspace, size_t workspace_bytes, void* stream);

/* The rest of the patch-correspondence block behind the 2D-3D loop (EXP/model.py:707-780), around dr_mutual_topk_select_f32:
 *
 * dr_patch_similarity_f32: for every node correspondence b the similarity of its image patch and its point patch (model.py:726-738):
 *   out[b][i][j] = 0.5 (<img_feats[img_knn_indices[b][i]], pcd_feats[pcd_knn_indices[b][j]]> + 1)
 *   = index_select (vision3d/ops/index_select.py:4-33) of both sides + pairwise_cosine_similarity(normalized = True)
 *   (vision3d/ops/cosine_similarity.py:34-66).  img_feats [*, C], pcd_feats [pcd_rows, C] float32; an index == pcd_rows is the zero row the
 *   reference appends (model.py:707); img_knn_indices [P, Ki], pcd_knn_indices [P, Kc] int64, Kc <= 128; out [P, Ki, Kc].
 * dr_unique_pairs_i64: the duplicate removal of model.py:759-763: sorted distinct values of first[i] * multiplier + second[i] (torch.unique),
 *   unique_keys [n], count[0] = how many.  workspace: dr_unique_pairs_workspace_bytes(n).
 * dr_corr_gather_f32: model.py:761-774 for the first count[0] keys: img / pcd indices = key / num_points_f, key % num_points_f, the gathered
 *   points [.,3] / pixels [.,2] of both sides and corr_scores = <img_feats_f[i], pcd_feats_f[j]>; `capacity` = rows of the outputs. */
int dr_patch_similarity_f32(int P, int Ki, int Kc, int C, const float* img_feats, const int64_t* img_knn_indices, const float* pcd_feats,
                            const int64_t* pcd_knn_indices, long long pcd_rows, float* out, void* stream);
size_t dr_unique_pairs_workspace_bytes(int n);
int dr_unique_pairs_i64(int n, const int64_t* first, const int64_t* second, long long multiplier, int64_t* unique_keys, int32_t* count,
                        void* workspace, size_t workspace_bytes, void* stream);
int dr_corr_gather_f32(int capacity, const int32_t* count, const int64_t* unique_keys, long long num_points_f, int C, const float* img_points_f,
                       const float* img_pixels_f, const float* pcd_points_f, const float* pcd_pixels_f, const float* img_feats_f, const float* pcd_feats_f,
                       int64_t* img_corr_indices, int64_t* pcd_corr_indices, float* img_corr_points, float* img_corr_pixels, float* pcd_corr_points,
                       float* pcd_corr_pixels, float* corr_scores, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 0.4.0: the patch partition and the ground-truth patch overlaps of the 2D-3D model (EXP/model.py:395-540, between the backbones and the
 * coarse matching, every pair in eval and in training) and the training-only ground-truth search (model.py:565-600).  csrc/partition2d3d.hip.
 * Nothing synchronises.  Bool tensors are uint8 (0 / 1).  Every list is written in the reference's order by a sort or a count / scan / write
 * compaction; distances are sums of squared differences in float32 (the reference's x^2 + y^2 - 2xy form differs from it in the last bits:
 * the tests compare wherever a float64 restatement decides the comparison).
 *
 * dr_point_to_node_partition_f32: point_to_node_partition(points, nodes, point_limit, return_count=True, gather_points=True)
 *   (vision3d/ops/point_cloud_partition.py:41-104).  points [Nf,3], nodes [Nc,3]; point_to_node [Nf]: the nearest node (equal distances: the
 *   lower index); node_sizes [Nc]; node_masks [Nc] = size > 0; node_knn_indices [Nc, point_limit]: the node's own points nearest first (equal
 *   distances: lower index first), padded with Nf, node_knn_masks = not padding.  max_points_per_node (device int32) = the largest node size:
 *   the reference's output is min(that, point_limit) columns wide, the caller slices.  point_limit <= 128 (DR_ENOSUP beyond).  The (Nc x Nf)
 *   distance matrix is never formed: nearest-node pass, one (node, distance, index) sort, one wave per node.
 *   workspace: dr_point_to_node_partition_workspace_bytes(Nf).
 * dr_patchify_f32: patchify (EXP/utils.py:28-56) for an (H_f x W_f) image cut into (H_c x W_c) blocks, every stride-th row / column of a
 *   block: Ki = ceil(H_f / H_c / stride) * ceil(W_f / W_c / stride).  img_points, img_points_da [H_f W_f, 3], img_pixels [H_f W_f, 2],
 *   img_masks, img_masks_da [H_f W_f] -> knn_points, knn_points_da [M, Ki, 3], knn_pixels [M, Ki, 2], knn_indices int64 [M, Ki], knn_masks,
 *   knn_masks_da [M, Ki], node_masks, node_masks_da [M] = any over the block (M = H_c W_c).  One launch.
 * dr_node_correspondences_2d3d_f32: get_2d3d_node_correspondences (EXP/utils.py:59-175) without its mutual-NN list (the next entry): the point
 *   patches moved by transform (16 floats, device, row-major 4 x 4; apply_transform, vision3d/ops/se3.py:46-53), the three masked means (eps
 *   1e-6, vision3d/ops/masked_ops.py:23-41) -> pcd_centers [N,3], img_centers, img_centers_da [M,3]; enclosing radii and the candidate test
 *   over (M x N) (:107-117), candidates compacted in row-major order; per candidate both nearest-neighbour passes over the whole other patch
 *   (k = 1; vision3d/ops/knn.py:10-27), the 3D radius, the 2D radius and the mask tests, the two overlap ratios (:130-163); the pairs with both
 *   ratios > 0 in candidate order (:165-171) -> img_corr_indices, pcd_corr_indices int64, img_corr_overlaps, pcd_corr_overlaps, each of
 *   `capacity` rows.  counts int32 [3]: [0] = pairs written, [1] = candidates kept, [2] = candidates found: [2] > capacity means that the
 *   candidate list was cut at `capacity` and the result must not be used (never a silent truncation: the caller reads counts).
 *   Ki <= 256, Kc <= 128 (DR_ENOSUP beyond).  workspace: dr_node_correspondences_2d3d_workspace_bytes(M, N, Kc, capacity).
 * dr_mutual_nn_radius_f32: multual_nn_correspondence(src, tgt, search_radius, knn = 1) (EXP/utils.py:234-252): the sources whose nearest
 *   target has them as its nearest source and lies closer than radius, ascending: out_src, out_tgt int64 [ns], count (device int32).
 *   workspace: dr_mutual_nn_radius_workspace_bytes(ns, nt).
 * dr_radius_pairs_f32: all (i, j) with |T src_i - tgt_j| < radius in ascending (i, j) order: what get_correspondences / KDTree_corr compute
 *   (EXP/utils.py:426-446; there per query in KD-tree order, which nothing downstream reads: model.py:574-577, 603-604 scatter ones).
 *   transform: 16 floats on the device or NULL (identity).  counts int32 [2]: [0] = pairs written, [1] = pairs found (> capacity: cut).
 *   PARITY UNPINNED against Open3D (not part of the reference tree), pinned against the definition in float64.
 *   workspace: dr_radius_pairs_workspace_bytes(ns, nt). */
size_t dr_point_to_node_partition_workspace_bytes(int Nf);
int dr_point_to_node_partition_f32(int Nf, int Nc, int point_limit, const float* points, const float* nodes, int64_t* point_to_node, int64_t* node_sizes,
                                   uint8_t* node_masks, int64_t* node_knn_indices, uint8_t* node_knn_masks, int32_t* max_points_per_node, void* workspace,
                                   size_t workspace_bytes, void* stream);
int dr_patchify_f32(int H_f, int W_f, int H_c, int W_c, int stride, const float* img_points, const float* img_points_da, const float* img_pixels,
                    const uint8_t* img_masks, const uint8_t* img_masks_da, float* knn_points, float* knn_points_da, float* knn_pixels, int64_t* knn_indices,
                    uint8_t* knn_masks, uint8_t* knn_masks_da, uint8_t* node_masks, uint8_t* node_masks_da, void* stream);
size_t dr_node_correspondences_2d3d_workspace_bytes(int M, int N, int Kc, long long capacity);
int dr_node_correspondences_2d3d_f32(int M, int Ki, int N, int Kc, const uint8_t* img_masks, const float* img_knn_points, const float* img_knn_points_da,
                                     const float* img_knn_pixels, const uint8_t* img_knn_masks, const uint8_t* img_knn_masks_da, const uint8_t* pcd_masks,
                                     const float* pcd_knn_points, const float* pcd_knn_pixels, const uint8_t* pcd_knn_masks, const float* transform,
                                     float pos_radius_2d, float pos_radius_3d, long long capacity, int64_t* img_corr_indices, int64_t* pcd_corr_indices,
                                     float* img_corr_overlaps, float* pcd_corr_overlaps, int32_t* counts, float* pcd_centers, float* img_centers,
                                     float* img_centers_da, void* workspace, size_t workspace_bytes, void* stream);
size_t dr_mutual_nn_radius_workspace_bytes(int ns, int nt);
int dr_mutual_nn_radius_f32(int ns, int nt, const float* src, const float* tgt, float radius, int64_t* out_src, int64_t* out_tgt, int32_t* count,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t dr_radius_pairs_workspace_bytes(int ns, int nt);
int dr_radius_pairs_f32(int ns, int nt, const float* src, const float* tgt, const float* transform, float radius, long long capacity, int64_t* out_src,
                        int64_t* out_tgt, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 0.5.0: the 2D-3D model's point backbone (PointBackbone, EXP/point_backbone.py:8-95, called at EXP/model.py:366-368; vision3d's KPConv FPN).
 * csrc/backbone2d3d.hip.  KPConv's gather half is dr_kpconv_gather_f32 / its backward, its product dr_linear_ex_f32 with the bias in the epilogue,
 * the strided max-pool dr_gather_pool_f32 / its backward; these entries add what the KPFCN backbone does not have.  Nothing synchronises, nothing
 * allocates.  Rows are [N, C] float32 with leading dimensions.
 *
 * dr_group_norm_stats_f32: GroupNormPackMode = nn.GroupNorm(G, C, eps, affine) over the transposed [1, C, N] rows (vision3d/layers/basic_layers/
 *   norm.py:53-65): mean / rstd [G] over all N rows x C/G channels, biased variance, float64 partials over a fixed grid of row slabs (no atomics).
 *   C % G == 0.  workspace: dr_group_norm_workspace_bytes(N, C).
 * dr_group_norm_apply_f32: out = act( gamma_a xhat_a + beta_a + [ gamma_b xhat_b + beta_b  |  b  |  0 ] ), act = LeakyReLU(leaky_slope) or none:
 *   UnaryBlockPackMode's Linear -> GroupNorm -> LeakyReLU (vision3d/layers/unary_block.py:26-30), KPConvBlock's (kpconv.py:203-207) and the tail of
 *   KPResidualBlock (kpconv.py:266-280: the shortcut through its own Linear + GroupNorm when mean_b is given, the identity shortcut added raw when only
 *   b is).  Both operands share C and G.
 * dr_group_norm_backward_f32: the apply step backwards with `out` its result (the LeakyReLU's derivative is read off its sign) -> grad_a, d gamma_a,
 *   d beta_a and, when b took part, grad_b (and, when b was normalised, d gamma_b, d beta_b).  Any output may be NULL.  Float64 column reductions
 *   over a fixed grid.  workspace: dr_group_norm_backward_workspace_bytes(N, C, G).
 * dr_knn_interpolate_f32: knn_interpolate_pack_mode(q, s, x, neighb_inds, k = None) (vision3d/ops/knn_interpolate.py:43-77): out[q] = sum_h w_h x[i_h]
 *   with w = mask / (d^2 + 1e-8) / (sum + 1e-8), the shadow index Ns masked (an all-shadow row gives zeros).  neighb_inds [Nq, H] int64; out has
 *   leading dimension ldo, so it may be a column slice of the decoder's concatenation buffer (EXP/point_backbone.py:81-88).  H <= 64 (DR_ENOSUP beyond).
 * dr_knn_interpolate_backward_f32: grad_x [Ns, C] (zeroed here, then fp32 atomics) from grad_out [Nq, ldg].  H <= 64.
 * dr_kpconv_neighbor_count_f32: the neighbour count of KPConv's normalisation (vision3d/layers/kpconv.py:137-139: neighbours whose feature sum is
 *   > 0) exactly as dr_kpconv_gather_f32 sums it -> counts int32 [Nq] (before the floor at 1).  For tests: the count is a discrete decision. */
size_t dr_group_norm_workspace_bytes(int N, int C);
int dr_group_norm_stats_f32(int N, int C, int G, const float* x, int ldx, float eps, float* mean, float* rstd, void* workspace, size_t workspace_bytes,
                            void* stream);
int dr_group_norm_apply_f32(int N, int C, int G, const float* a, int lda, const float* mean_a, const float* rstd_a, const float* gamma_a, const float* beta_a,
                            const float* b, int ldb, const float* mean_b, const float* rstd_b, const float* gamma_b, const float* beta_b, float leaky_slope,
                            int activate, float* out, int ldo, void* stream);
size_t dr_group_norm_backward_workspace_bytes(int N, int C, int G);
int dr_group_norm_backward_f32(int N, int C, int G, const float* grad_out, int ldg, const float* out, int ldo, const float* a, int lda, const float* mean_a,
                               const float* rstd_a, const float* gamma_a, const float* b, int ldb, const float* mean_b, const float* rstd_b,
                               const float* gamma_b, float leaky_slope, int activate, float* grad_a, int ldga, float* grad_gamma_a, float* grad_beta_a,
                               float* grad_b, int ldgb, float* grad_gamma_b, float* grad_beta_b, void* workspace, size_t workspace_bytes, void* stream);
int dr_knn_interpolate_f32(int Nq, int Ns, int H, int C, const float* q_pts, const float* s_pts, const int64_t* neighb_inds, const float* x, float* out,
                           int ldo, void* stream);
int dr_knn_interpolate_backward_f32(int Nq, int Ns, int H, int C, const float* q_pts, const float* s_pts, const int64_t* neighb_inds, const float* grad_out,
                                    int ldg, float* grad_x, void* stream);
int dr_kpconv_neighbor_count_f32(int Nq, int Ns, int H, int Cin, const int64_t* neighb_inds, const float* x, int32_t* counts, void* stream);

/* PnP-RANSAC registration of the fine correspondences (EXP/eval.py:174-182 -> vision3d/utils/opencv.py:10-63 = cv2.solvePnPRansac with
 * iterationsCount = 50000, reprojectionError = 8.0, flags = SOLVEPNP_P3P).  OpenCV is not part of the reference tree: the published algorithm of
 * that call -- RANSAC over 4-point samples, P3P on three + disambiguation by the fourth, inliers under the reprojection tolerance, refit on the
 * inliers -- restated in oracle/pnp_oracle.py (every hypothesis is scored; counter-based sampling; Grunert's quartic; Gauss-Newton refit on the
 * reprojection error).  PARITY UNPINNED against OpenCV, pinned against the oracle.
 *   points [n,3], pixels [n,2] float32 device ((h, w) rows when transposed != 0, opencv.py:42-43), intrinsics: 9 doubles on the HOST (row-major K),
 *   transform: 16 doubles (device, row-major 4 x 4, 3D -> camera), n_inlier / best_iter: device ints.  n >= 4. */
size_t dr_pnp_ransac_workspace_bytes(int n, int iters);
int dr_pnp_ransac_f64(int n, const float* points, const float* pixels, int transposed, const double* intrinsics_host, int iters, double distance_tolerance,
                      uint64_t seed, double* transform, int32_t* n_inlier, int32_t* best_iter, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 2D-3D variant (Diff-Reg-2d3d): the reverse sampling of MATR2D3D.forward
 * (EXP/model.py:637-694, 830-846; EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1)
 * with CrossModalFusionModule (EXP/fusion_module.py:61-107, vision3d/layers/transformer.py:58-301)
 * as the denoiser and the position-free Matching head (EXP/matching.py:91-147).
 * src = N point-cloud nodes, tgt = M image patches.
 */
typedef struct {        /* one vision3d TransformerLayer: weights [out,in] row-major, biases [out] */
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b;     /* attention.attention.{q,k,v}_token_layer   */
    const float *lin_w, *lin_b, *norm1_w, *norm1_b;     /* attention.linear, attention.norm          */
    const float *expand_w, *expand_b, *squeeze_w, *squeeze_b, *norm2_w, *norm2_b; /* output.*        */
} dr_fusion_layer_weights;

typedef struct {
    const dr_fusion_layer_weights* layers;   /* HOST array [n_layers] */
    const float *img_emb_w, *img_emb_b;      /* img_emb_proj: weight zero-padded to [C, 44] (K = 42 -> 44)  */
    const float *pcd_emb_w, *pcd_emb_b;      /* pcd_emb_proj: weight zero-padded to [C, 64] (K = 63 -> 64)  */
    const float *img_in_w, *img_in_b;        /* img_in_proj      [C, img_dim]                               */
    const float *dino_w, *dino_b;            /* img_in_proj_dino [C, dino_dim]                              */
    const float *all_w, *all_b;              /* img_in_proj_all  [C, 2C]                                    */
    const float *pcd_in_w, *pcd_in_b;        /* pcd_in_proj      [C, pcd_dim]                               */
    const float *out_w, *out_b;              /* out_proj         [C, C]                                     */
    const float* src_proj;                   /* denoising_coarse_matching.src_proj.weight [C,C] (Q1)        */
    const float* bin_score;
    const void* prepacked;                   /* dr_loop2d3d_prepack image of THESE weights (device, 256-byte aligned) or NULL: calls that
                                              * take the plane path then pack them into the workspace EVERY time -- 7 pack launches, 3 copies
                                              * and 6 bound kernels per layer, also inside a captured graph (every replay repeats them): pass a
                                              * prepacked image unless the weights really change between calls.  The image must be complete on
                                              * the stream of the call: synchronise (or order with an event) after dr_loop2d3d_prepack when the
                                              * loop runs on another stream                                                            */
} dr_fusion_weights;

typedef struct {
    int C, H, n_layers;          /* hidden/output dim (256), heads (4), blocks (self, cross, ...)   */
    int img_dim, dino_dim, pcd_dim;
    int steps, sk_iters;
    float sample_rate, max_condition_num;
    int flags;                   /* DR_LOOP_*                                                     */
    const double* h_alphas_cumprod;
    const int32_t* h_times;
} dr_loop2d3d_config;

/* Calls of at least 4096 token rows (P (N + M); cfg5: two pairs or more) run the layer's nn.Linears and its attention on fp16 hi / lo
 * plane images like dr_denoise_loop does ("Plane images" above; biases, the post-add LayerNorms and the ReLU feed-forward of the vision3d
 * layer are epilogue modes of the same GEMM); DR_LOOP_PLANES_FORCE / DR_LOOP_PLANES_OFF in cfg->flags take the decision away from the size
 * rule.  The packed weights: once per engine with dr_loop2d3d_prepack (0 bytes = this configuration has no plane path). */
size_t dr_loop2d3d_prepack_bytes(const dr_loop2d3d_config* cfg);
int dr_loop2d3d_prepack(const dr_loop2d3d_config* cfg, const dr_fusion_weights* w, void* packed, size_t packed_bytes, void* stream);
size_t dr_denoise_loop_2d3d_workspace_bytes(const dr_loop2d3d_config* cfg, int P, int N, int M);

/* inputs : img_feats [P,M,img_dim], img_dino [P,M,dino_dim], img_pixels [P,M,2], pcd_feats [P,N,pcd_dim],
 *          s_pcd [P,N,3] (point nodes), t_pcd_da [P,M,3] (depth-back-projected patch centres),
 *          src_mask [P,N], tgt_mask [P,M], tgt_mask_da [P,M] uint8 (all three or none), x_T [P,N,M]
 * outputs: conf [P,N,M] float64; matches [P,N+M,3] int64 + match_count [P] (optional); x_final (optional);
 *          trace as in dr_denoise_loop; steps == 0 runs ONE fusion + matching evaluation on s_pcd as given
 *          and writes x_start into conf as float64 (used by the component tests) */
int dr_denoise_loop_2d3d(const dr_loop2d3d_config* cfg, const dr_fusion_weights* w, int P, int N, int M,
                         const float* img_feats, const float* img_dino, const float* img_pixels,
                         const float* pcd_feats, const float* s_pcd, const float* t_pcd_da, const uint8_t* src_mask,
                         const uint8_t* tgt_mask, const uint8_t* tgt_mask_da, const float* x_T, double* conf,
                         double* x_final, int64_t* matches, int32_t* match_count, float* img_out, float* pcd_out,
                         const dr_loop_trace* trace, void* workspace, size_t workspace_bytes, void* stream);

/* The same vision3d TransformerLayer for TRAINING (the 2D-3D training branch, EXP/model.py:386-392 and :615-621; the layer is
 * vision3d/layers/transformer.py:58-301: biased q / k / v, attention, linear, LayerNorm(x + .), expand, ReLU, squeeze, LayerNorm(z + .)): the forward
 * that keeps what its backward needs, and the whole backward, one call each, as dr_attention_layer_train_forward_f32 / dr_attention_layer_backward_f32
 * do for the 3D layer.  x [B*L, C] (queries), y [B*S, C] (keys / values; y == x for a self-attention call) contiguous; y_mask uint8 [B*S] or NULL:
 * 1 = a valid key (the reference's k_masks is the complement: True = ignored).  C % H == 0, (C / H) % 4 == 0, C / H <= 160, C <= 1024.
 *   forward : out [B*L, C]; `saved` = caller memory of dr_fusion_layer_train_saved_bytes(B, L, S, C): q | k | v | heads' output | LN1 input | z |
 *             ReLU activation | LN2 input | (mean, rstd) of both LayerNorms -- opaque, handed to the backward
 *   backward: grad_out [B*L, C] -> grad_x [B*L, C], grad_y [B*S, C] (separate buffers also when x == y: the caller adds them) and the 16 parameter
 *             gradients (dr_fusion_layer_grads: the layout of dr_fusion_layer_weights; overwritten, not accumulated).  Every sum in a fixed order
 *             (bias / LayerNorm gradients: column partials per block of 16 rows, added in block order; no atomics): bit-reproducible between
 *             launches.  workspace: dr_fusion_layer_backward_workspace_bytes(B, H, L, S, C). */
typedef struct {
    float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b;
    float *lin_w, *lin_b, *norm1_w, *norm1_b;
    float *expand_w, *expand_b, *squeeze_w, *squeeze_b, *norm2_w, *norm2_b;
} dr_fusion_layer_grads;
size_t dr_fusion_layer_train_saved_bytes(int B, int L, int S, int C);
int dr_fusion_layer_train_forward_f32(const dr_fusion_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                      const uint8_t* y_mask, float* out, void* saved, size_t saved_bytes, void* stream);
size_t dr_fusion_layer_backward_workspace_bytes(int B, int H, int L, int S, int C);
int dr_fusion_layer_backward_f32(const dr_fusion_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                 const uint8_t* y_mask, const void* saved, const float* grad_out, float* grad_x, float* grad_y,
                                 const dr_fusion_layer_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* The coarse loss of the 2D-3D training branch (EXP/loss.py:30-75, CoarseMatchingLoss; its circle terms):
 * dr_l2_normalize_f32: F.normalize(x, p = 2, dim = 1, eps) on rows [rows, C] (EXP/model.py:552-553, 630-631); norms [rows] = |x| per row, kept for
 *   dr_l2_normalize_backward_f32 (grad_x = (g - y (g . y)) / |x| where |x| >= eps, g / eps below).
 * dr_circle_loss_f32: the weighted circle loss (vision3d/loss/circle_loss.py:11-52) of feat_dists = sqrt(clamp(2 - 2 img pcd^T, 0) + 1e-8)
 *   (vision3d/ops/pairwise_distance.py:38-56): img [M, C] (rows) and pcd [N, C] (columns), both already normalised; the node correspondences as
 *   K duplicate-free entries (img_idx, pcd_idx int64, min_overlaps, max_overlaps float; entries outside the matrix are skipped -- the reference
 *   raises); positives where the min overlap > pos_overlap with scale sqrt(min overlap), negatives where the max overlap < neg_overlap (0 off the
 *   list).  CoarseMatchingLoss reads its max overlaps from the MIN list (EXP/loss.py:36): its caller passes that list twice.  *loss (device
 *   float): an empty anchor set gives NaN, as the reference's mean of an empty selection.  Row / column log-sum-exps and the means in double,
 *   each in one fixed order.  workspace: dr_circle_loss_workspace_bytes(M, N, C).
 * dr_circle_loss_backward_f32: grad_img [M, C], grad_pcd [N, C] = d loss / d features, scaled by *grad_loss (device float; NULL = 1); the weights
 *   are constants (the reference detaches them); zero where the clamp is active (2 - 2 x y < 0); an empty anchor set contributes no gradient, as
 *   torch's.  It recomputes the forward (loss: optional device float). */
typedef struct {
    float pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale;   /* cfg.loss.coarse_loss.* */
    float pos_overlap, neg_overlap;                                      /* positive_overlap, negative_overlap */
} dr_circle_loss_params;
int dr_l2_normalize_f32(int rows, int C, const float* x, float eps, float* y, float* norms, void* stream);
int dr_l2_normalize_backward_f32(int rows, int C, const float* y, const float* norms, float eps, const float* grad_y, float* grad_x, void* stream);
size_t dr_circle_loss_workspace_bytes(int M, int N, int C);
int dr_circle_loss_f32(int M, int N, int C, const float* img, const float* pcd, int K, const int64_t* img_idx, const int64_t* pcd_idx,
                       const float* min_overlaps, const float* max_overlaps, const dr_circle_loss_params* params, float* loss, void* workspace,
                       size_t workspace_bytes, void* stream);
int dr_circle_loss_backward_f32(int M, int N, int C, const float* img, const float* pcd, int K, const int64_t* img_idx, const int64_t* pcd_idx,
                                const float* min_overlaps, const float* max_overlaps, const dr_circle_loss_params* params, const float* grad_loss,
                                float* loss, float* grad_img, float* grad_pcd, void* workspace, size_t workspace_bytes, void* stream);

/* The fine loss of the 2D-3D training step (EXP/loss.py:157-215, FineMatchingLoss.forward behind its random_choice; ABI 0.6.0):
 * dr_fine_loss_f32 replaces loss.py:175, 186-213 and get_recall (:146-155): img_points [HW,3], img_feats [HW,C], pcd_points [N,3], pcd_pixels [N,2],
 *   pcd_feats [N,C], transform [4,4] (row-major; applied to the M selected points only), img_sel_pixels [M,2] int64 (v, u: the dense row is
 *   v * image_w + u), pcd_sel_indices [M] int64.  dist3d / dist2d are float32 norms of differences (pairwise_distance(strict=True)), positives lie
 *   under both positive radii, negatives above either negative radius, fdist = clamp(x^2 - 2 x y + y^2, 0) (squared, normalized=False), the
 *   circle loss is the unweighted one of vision3d/loss/circle_loss.py:11-52 (an entry outside a mask keeps the logit 0 and counts in the
 *   log-sum-exp).  loss_recall (2 device floats): [0] the loss (NaN for an empty anchor set on either side, torch's mean of an empty selection),
 *   [1] the recall (rows whose arg-min of fdist -- first minimum -- is a positive / (rows holding a positive + 1e-12)).  `saved`: caller memory
 *   of dr_fine_loss_saved_bytes(M), opaque (row / column log-sum-exps, anchor flags, gradient coefficients), handed to the backward.  Dot
 *   products, logits, log-sum-exps and means in double, every sum in one fixed order -- on purpose NOT dr_circle_loss_f32's choice of float32
 *   logits: the float32 rounding of fdist times log_scale is the size of the bar the gradients are held to (csrc/fine_loss.hip).  A selection outside its tensor (v or u negative, u >= image_w, row >= HW; index outside [0, N)) reads a zero row and
 *   receives no gradient (the reference raises).  M <= 1024, C <= 256: DR_ENOSUP beyond.
 * dr_fine_loss_backward_f32: the same inputs and `saved` -> grad_img_feats [HW,C], grad_pcd_feats [N,C] = d loss / d features * *grad_loss
 *   (device float; NULL = 1), DENSE: zero-filled, then the <= M touched rows; selections of one pixel / point accumulate (in selection order), as
 *   torch's index backward; zero where the clamp is active; all zero for an empty anchor set.  No atomics: two runs are bit-identical.
 *   workspace: dr_fine_loss_backward_workspace_bytes(M, C). */
typedef struct {
    float pos_radius_3d, neg_radius_3d, pos_radius_2d, neg_radius_2d;    /* cfg.loss.fine_loss.*_radius_* */
    float pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale;   /* cfg.loss.fine_loss.* */
} dr_fine_loss_params;
size_t dr_fine_loss_saved_bytes(int M);
int dr_fine_loss_f32(int HW, int N, int M, int C, const float* img_points, const float* img_feats, const float* pcd_points, const float* pcd_pixels,
                     const float* pcd_feats, const float* transform, const int64_t* img_sel_pixels, const int64_t* pcd_sel_indices, int image_w,
                     const dr_fine_loss_params* params, float* loss_recall, void* saved, size_t saved_bytes, void* stream);
size_t dr_fine_loss_backward_workspace_bytes(int M, int C);
int dr_fine_loss_backward_f32(int HW, int N, int M, int C, const float* img_points, const float* img_feats, const float* pcd_points,
                              const float* pcd_pixels, const float* pcd_feats, const float* transform, const int64_t* img_sel_pixels,
                              const int64_t* pcd_sel_indices, int image_w, const dr_fine_loss_params* params, const void* saved, size_t saved_bytes,
                              const float* grad_loss, float* grad_img_feats, float* grad_pcd_feats, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 0.7.0: the evaluation metrics of the 2D-3D model (csrc/eval2d3d.hip): the two consumers of MATR2D3D.forward's output dict,
 * EvalFunction (EXP/loss.py:241-301, after every training and test step) and the offline evaluator (EXP/eval.py:121-200 on
 * vision3d/array_ops/registration_utils.py:151-225 and array_ops/metrics.py:25-166).  One pair per call; pairs queue on the stream.  Nothing
 * synchronises or reads back; results go to device memory of the caller.  Double arithmetic on the float32 inputs; no float atomics (integer
 * atomics on bitmaps and counters only); every sum of reals is a set of per-workgroup double partials added in one fixed order: two runs are
 * bit-identical.  Transforms are 16 doubles on the device, row-major 4 x 4, last row (0, 0, 0, 1) (not read).
 *
 * dr_sparse_corr_eval_i64: K predicted node pairs (img_node_corr_indices, pcd_node_corr_indices) against G ground-truth pairs over an
 *   img_num_nodes x pcd_num_nodes grid.  gt_node_corr_min_overlaps (float32 [G], or NULL = every GT pair counts): a GT pair counts only where its
 *   overlap is > acceptance_overlap (torch.gt, loss.py:258).  out (4 doubles): [0] LIST precision = mean over the K listed predictions of GT
 *   membership (EvalFunction.evaluate_coarse_matching: duplicates count each time; K = 0 -> NaN, torch.mean of nothing); [1] SET precision,
 *   [2] recall, [3] hit_ratio of evaluate_sparse_correspondences (duplicates count once; denominators + 1e-12; hit_ratio from the row / column
 *   "any" counts).  counts (4 int32): unique predictions, unique GT, unique positives, listed positives.  No dense float matrix: two bit
 *   matrices in the workspace (dr_sparse_corr_eval_workspace_bytes; zeroed by the call).  Supported: img_num_nodes * round_up(pcd_num_nodes, 32)
 *   <= 2^26 (1 530 x 4 096 is 6.3e6; two bit matrices of 8 MiB at the limit) -- DR_ENOSUP beyond.  An index outside [0, img_num_nodes) /
 *   [0, pcd_num_nodes) (negative ones included: no wrap) is skipped -- it marks nothing and is no listed positive, K stays the list's
 *   denominator -- and sets bit 1 of the device status word (dr_device_status -> DR_EINVAL).
 * dr_corr_eval_f32: n fine correspondences (pcd_corr_points, img_corr_points float32 [n,3]), the ground-truth transform (cloud -> camera) and
 *   positive_radius.  sel_indices (int64 [n_sel], or NULL with n_sel = 0 = all n in order): the correspondences that take part (the wrapper's
 *   top-num_corr by score, eval.py:121-127); m = n_sel or n of them.  out (4 doubles): [0] inlier ratio (registration_inlier_ratio), [1] mean
 *   residual (registration_corr_distance), [2] overlap (point_cloud_overlap: for every IMAGE point the distance to the nearest TRANSFORMED CLOUD
 *   point among the m, mean of < radius -- knn(tgt, src)), [3] EvalFunction.evaluate_fine_matching's IR: with depth_mask != 0 over the
 *   correspondences whose image point has z > 0, 0 when none remain (nan_to_num_); with depth_mask == 0 over all m.  m = 0 writes eval.py's
 *   {0, 0, 0} (and [3] = 0).  counts (4 int32): inliers, overlapping image points, correspondences kept by the mask (m without it), inliers among those.
 *   Brute-force nearest neighbour over LDS tiles: m <= 16 384 (DR_ENOSUP beyond).  A selection outside [0, n) is skipped (no numerator, nobody's
 *   neighbour; m stays the denominator) and sets the status bit.  workspace: dr_corr_eval_workspace_bytes(m).
 * dr_registration_eval_f64: pcd_points float32 [N,3], the ground-truth and the estimated transform.  out (4 doubles): [0] eval.py's RMSE
 *   sqrt(mean |T_gt p - T_est p|^2) (registration_rmse), [1] EvalFunction.evaluate_registration's "rmse" mean |inv(T_gt) T_est p - p| (a true
 *   inverse of the 3 x 3 block, as torch.linalg.inv), [2] RRE in degrees (acos of (trace(R_est^T R_gt) - 1) / 2 clipped to [-1, 1]), [3] RTE.
 *   recall (2 int32): out[0] < rmse_threshold, out[1] < rmse_threshold.  N = 0: both means NaN, both flags 0, RRE and RTE as usual.
 *   Grid-stride double partials (at most 256 workgroups), one-workgroup final.  workspace: dr_registration_eval_workspace_bytes(N). */
size_t dr_sparse_corr_eval_workspace_bytes(int img_num_nodes, int pcd_num_nodes);
int dr_sparse_corr_eval_i64(int img_num_nodes, int pcd_num_nodes, int K, const int64_t* img_node_corr_indices,
                            const int64_t* pcd_node_corr_indices, int G, const int64_t* gt_img_node_corr_indices,
                            const int64_t* gt_pcd_node_corr_indices, const float* gt_node_corr_min_overlaps, float acceptance_overlap,
                            double* out, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
size_t dr_corr_eval_workspace_bytes(int m);
int dr_corr_eval_f32(int n, const float* pcd_corr_points, const float* img_corr_points, const double* transform, double positive_radius,
                     int n_sel, const int64_t* sel_indices, int depth_mask, double* out, int32_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t dr_registration_eval_workspace_bytes(int N);
int dr_registration_eval_f64(int N, const float* pcd_points, const double* gt_transform, const double* est_transform, double rmse_threshold,
                             double* out, int32_t* recall, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 0.7.0, second set: the geometry head and the feature-layout glue of MATR2D3D.forward (csrc/front2d3d.hip).  One image per call, queued on
 * the stream; nothing synchronises or reads back.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.
 *
 * dr_back_project_f32: depth [H,W], intrinsics [3,3] (device, row-major) -> points [H*W,3], mask [H*W] (uint8: z > 0) and, when pixels is not
 *   NULL, pixels [H*W,2] = (row, column) as float32 -- create_meshgrid(H, W).float() (vision3d/ops/meshgrid.py:4-37; EXP/model.py:310).
 *   mode 0 = vision3d.ops.back_project (ops/back_project.py:29-53; EXP/model.py:306): z = depth / a (a true division).
 *   mode 1 = MATR2D3D.back_project_depth (EXP/model.py:875-899; :349): z = depth * a + b, a product and a sum (no FMA); a_dev / b_dev (device,
 *   one float each) replace a / b where not NULL -- depth_coffa and depth_coffb are device tensors.  Both: has_limit != 0: z > depth_limit -> 0;
 *   x = (u - cx) * z / fx, y = (v - cy) * z / fy in that order in float32.  One launch, one pass, four pixels per thread (16-byte loads and
 *   stores when every pointer is 16-byte aligned -- the mask 4 --, scalar ones otherwise).  H * W < 2^31 - 4 (DR_ENOSUP beyond).
 * dr_render_f32: points [N,3], intrinsics [3,3], extrinsics [4,4] or NULL (row-major, last row not read) -> pixels [N,2] = (h, w) =
 *   (fy * y / max(z, eps) + cy, fx * x / max(z, eps) + cx) without rounding, after p <- R p + t in float32 (vision3d/ops/render.py:34-52,
 *   ops/se3.py:49-52; EXP/model.py:335); depth [N] (or NULL) receives the unclamped z (return_depth).
 * dr_resize_tokens_f32: in [C,Hs,Ws] -> out [Hd*Wd, C]: F.interpolate(mode="bilinear", align_corners=True) written as token rows
 *   (EXP/model.py:374-375: interpolate + view + transpose) in one launch.  Source index = d * (in - 1) / (out - 1), scale 0 when out == 1, as
 *   ATen; the arithmetic is double on the float32 texels, rounded once.  Hs * Ws, Hd * Wd <= 2^24, C <= 2^20 (DR_ENOSUP beyond); an empty source
 *   with a non-empty destination is DR_EINVAL.
 * dr_resize_tokens_backward_f32: grad_out [Hd*Wd, C] -> grad_in [C,Hs,Ws] (every element written).  A GATHER: each source texel sums, in
 *   ascending destination order and in double, the at most ceil(Hd / Hs + 1) x ceil(Wd / Ws + 1) destinations whose footprint holds it -- no
 *   atomics, two runs are bit-identical.
 * dr_rows_normalize_chw_f32: in [C,P] (CHW, P = H * W) -> out [P,C], each row divided by max(|row|_2, 1e-12) (EXP/model.py:536-538:
 *   view + transpose + contiguous + F.normalize) through an LDS tile: every element is read once and written once.  The sum of squares is
 *   double.  C <= 256 (DR_ENOSUP beyond), P < 2^31 - 64.
 * dr_rows_normalize_chw_backward_f32: in [C,P], grad_out [P,C] -> grad_in [C,P] = (g - y <g, y>) / max(|x|, 1e-12), y recomputed from in.
 * dr_rows_normalize_chw_backward_rows_f32: the same for a gradient that is zero outside K rows: rows int64 [K] (repeats allowed: their
 *   gradient rows are summed in list order), grad_rows [K,C].  grad_in [C,P] is zero-filled by the call and only the touched columns are
 *   written.  A row outside [0, P) is skipped and sets bit 1 of the device status word (dr_device_status -> DR_EINVAL). */
int dr_back_project_f32(int H, int W, const float* depth, const float* intrinsics, int mode, float a, float b, const float* a_dev,
                        const float* b_dev, int has_limit, float depth_limit, float* points, uint8_t* mask, float* pixels, void* stream);
int dr_render_f32(int N, const float* points, const float* intrinsics, const float* extrinsics, float eps, float* pixels, float* depth,
                  void* stream);
int dr_resize_tokens_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* in, float* out, void* stream);
int dr_resize_tokens_backward_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* grad_out, float* grad_in, void* stream);
int dr_rows_normalize_chw_f32(int C, int64_t P, const float* in, float* out, void* stream);
int dr_rows_normalize_chw_backward_f32(int C, int64_t P, const float* in, const float* grad_out, float* grad_in, void* stream);
int dr_rows_normalize_chw_backward_rows_f32(int C, int64_t P, int K, const float* in, const int64_t* rows, const float* grad_rows,
                                            float* grad_in, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Forward half of the training branch: the pieces of Pipeline.forward's
 * `if self.training:` block (3D/models/pipeline.py:182-216) and of MatchMotionLoss.ge_coarse_loss
 * (3D/models/loss.py:80-170) that are not already kernels of the loop.  Values only: no backward.
 * `workspace`: dr_train_workspace_bytes(P, N, M) bytes, any content.
 */
#define DR_MATCH_SINKHORN 0
#define DR_MATCH_DUAL_SOFTMAX 1
size_t dr_train_workspace_bytes(int P, int N, int M);

/* match_2_conf_matrix (loss.py:316-320) and matrix_gt (pipeline.py:203-206): out [P,N,M] = 0, then 1 at the rows (b, i, j) of
 * matches [K,3] int64 (duplicates set the same entry; rows outside the matrix are skipped -- the reference raises) */
int dr_match_matrix_f32(int P, int N, int M, int K, const int64_t* matches, float* out, void* stream);

/* pipeline.py:209-214: noise = (|r| % 1) * (|r| / r) * 1.5 of randn [P,N,M] (float32 arithmetic), q_sample(x_start = matrix_gt, t,
 * noise) = sqrt(ac_t) matrix_gt + sqrt(1 - ac_t) noise in float64 (pipeline.py:84-95: the schedule is float64 and promotes),
 * nan_to_num(nan = 0), minus the minimum over the WHOLE [P,N,M] tensor (not per pair).  Bit-exact against the reference. */
int dr_gt_noising_f64(int P, int N, int M, const float* matrix_gt, const float* randn, double sqrt_ac, double sqrt_one_minus_ac, double* out,
                      void* workspace, void* stream);

/* MatchMotionLoss.compute_correspondence_loss (loss.py:273-314): focal loss of conf [P,N,M] against conf_gt (entries 1 / 0) ->
 * *loss (device float).  DR_MATCH_SINKHORN: pos_w mean_pos(-alpha (1-c)^gamma log c) + neg_w mean_neg(-alpha c^gamma log(1-c));
 * DR_MATCH_DUAL_SOFTMAX: pos_w mean_pos(... weight).  c clamped to [1e-6, 1-1e-6]; a class without entries contributes 0 (the
 * reference's stand-in entry with weight 0).  Terms in float32 in the reference's operation order, summed in float64. */
int dr_focal_loss_f32(int P, int N, int M, const float* conf, const float* conf_gt, const float* weight, float alpha, float gamma, float pos_w,
                      float neg_w, int match_type, float* loss, void* workspace, void* stream);

/* MatchMotionLoss.compute_match_recall (loss.py:323-345): match_pred [K,3] int64 rows (b, i, j) -> recall_precision[0] = TP / sum(conf_gt),
 * [1] = TP / max(K, 1), TP = ground-truth entries among the (distinct) predicted ones */
int dr_match_recall_f32(int P, int N, int M, const float* conf_gt, int K, const int64_t* match_pred, float* recall_precision, void* workspace,
                        void* stream);

/* the L1 motion term (loss.py:108-128): mean over the rows with overlap_mask [P,N] set of |(R_pred s + t_pred) - (R_gt (s + flow) + t_gt)|_1;
 * s_pcd [P,N,3], flow [P,N,3] or NULL (3DMatch), R [P,3,3], t [P,3] float32 */
int dr_motion_l1_f32(int P, int N, const float* s_pcd, const float* flow, const float* R_pred, const float* t_pred, const float* R_gt,
                     const float* t_gt, const uint8_t* overlap_mask, float* loss, void* workspace, void* stream);

/* First backward kernels of the training branch: the matching head's loss.
 * dr_focal_loss_backward_f32: d loss / d conf of compute_correspondence_loss in its sinkhorn form (loss.py:311-314; torch.clamp passes no
 *   gradient outside [1e-6, 1 - 1e-6]); workspace: dr_train_workspace_bytes(P, N, M).
 * dr_sinkhorn_backward_f32: backward of log_optimal_transport + exp + [:, :-1, :-1] (matching.py:61-93, 207-216): scores [P,N,M] as the forward
 *   saw them (masked entries -inf), the masks (both or none), bin_score, iters, grad_conf = d loss / d conf [P,N,M] ->
 *   grad_scores [P,N,M] (0 at masked entries) and grad_bin_score [P] (one partial per pair: the caller sums them).  float32 in and out; the
 *   dual variables, the plans' exponents and every sum are kept in double (at logits in the thousands Z + u + v cancels: a float32
 *   exponent cost 2.7e-3 of the gradient's maximum); every reduction in a fixed order.  workspace: dr_sinkhorn_backward_workspace_bytes(P, N, M, iters). */
/* d loss / d (R_pred [P,3,3], t_pred [P,3]) of dr_motion_l1_f32 (loss.py:108-128; 4DMatch trains with motion_weight 0.1) */
int dr_motion_l1_backward_f32(int P, int N, const float* s_pcd, const float* flow, const float* R_pred, const float* t_pred, const float* R_gt,
                              const float* t_gt, const uint8_t* overlap_mask, float* grad_R, float* grad_t, void* workspace, void* stream);

/* The non-GEMM pieces of the GeometryAttentionLayer backward (transformero.py:43-96; composed with dr_linear_f32 by diffreg_hip/autograd.py):
 * nn.LayerNorm forward with saved statistics (mean_rstd [rows,2]) and its backward (grad_x, grad_gamma, grad_beta; workspace:
 * dr_layernorm_backward_workspace_bytes(C)); the masked softmax of an explicit attention matrix scores [B,H,L,S] over S (a key j is -inf
 * for a valid query: q_mask[b][l] && !k_mask[b][j], transformero.py:78-79; then / sqrt(d) = `scale`) and its backward
 * dS = scale P (dP - sum_j dP_j P_j); ReLU backward. */
int dr_layernorm_f32(int rows, int C, const float* x, const float* gamma, const float* beta, float eps, float* y, float* mean_rstd, void* stream);
size_t dr_layernorm_backward_workspace_bytes(int C);
int dr_layernorm_backward_f32(int rows, int C, const float* x, const float* gamma, const float* mean_rstd, const float* grad_y, float* grad_x,
                              float* grad_gamma, float* grad_beta, void* workspace, void* stream);
/* softmax(q k^T scale) v per head, fused (no [B,H,L,S] matrix): forward on the inference kernels, and its backward (3D/models/transformero.py:79-85
 * under autograd).  Token layout: q / out / grad_o [B L, ld], k / v [B S, ld], head h in columns [h d, (h + 1) d); masks [B L] / [B S] uint8 (both
 * or none): key j is dead for query l when q_mask[l] && !k_mask[j], as the training forward applies them.  The backward is three launches on the
 * f32-input MFMA (per-query log-sum-exp and delta; dQ by query blocks; dK | dV by key blocks), fixed summation orders (bit-reproducible);
 * workspace: dr_attention_backward_workspace_bytes(B, H, L).  d % 4 == 0, d <= 160 (both ways).  The backward's workgroup is 4 waves up to d = 124,
 * 3 at d = 128 .. 156 and 2 at d = 160 (the waves' K / V tiles have to fit 160 KiB of LDS); the forward runs 136 < d <= 160 on its 32-query kernel only
 * (no plane-image operands).  Neither path beyond d = 136 has been timed. */
int dr_attention_f32(int B, int H, int L, int S, int d, const float* q, const float* k, const float* v, int ld, const uint8_t* q_mask,
                     const uint8_t* k_mask, float scale, float* out, void* stream);
size_t dr_attention_backward_workspace_bytes(int B, int H, int L);
int dr_attention_backward_f32(int B, int H, int L, int S, int d, const float* q, const float* k, const float* v, const float* o, const float* grad_o,
                              int ld, const uint8_t* q_mask, const uint8_t* k_mask, float scale, float* grad_q, float* grad_k, float* grad_v,
                              void* workspace, size_t workspace_bytes, void* stream);
int dr_softmax_rows_f32(int B, int H, int L, int S, const float* scores, float scale, const uint8_t* q_mask, const uint8_t* k_mask, float* P, void* stream);
int dr_softmax_backward_f32(int rows, int cols, const float* P, const float* grad_P, float scale, float* grad_scores, void* stream);
/* The dual-softmax read-out of Matching.forward (3D/models/matching.py:193-205; match_type 'dual_softmax'):
 *   conf[p][i][j] = softmax_i(sim[p][.][j] / temperature over the valid source rows) * softmax_j(sim[p][i][.] / temperature over the valid target columns),
 *   0 where either mask is 0; masks uint8 [P,N] / [P,M] or both NULL (the reference's mask-free branch).  col_stats: caller scratch of 2 P M floats. */
int dr_dual_softmax_f32(int P, int N, int M, const float* sim, float temperature, const uint8_t* src_mask, const uint8_t* tgt_mask, float* conf,
                        float* col_stats, void* stream);
/* its backward (ABI 0.2.1): grad_sim = d loss / d sim given grad_conf = d loss / d conf -- the two softmax adjoints; entries under a mask receive 0, as
 * the reference's masked_fill_ lets nothing through.  workspace: dr_dual_softmax_backward_workspace_bytes (column / row statistics and sums). */
size_t dr_dual_softmax_backward_workspace_bytes(int P, int N, int M);
int dr_dual_softmax_backward_f32(int P, int N, int M, const float* sim, float temperature, const uint8_t* src_mask, const uint8_t* tgt_mask,
                                 const float* grad_conf, float* grad_sim, void* workspace, size_t workspace_bytes, void* stream);
int dr_relu_backward_f32(long long n, const float* y, const float* grad_y, float* grad_x, void* stream);

/* embed_rotary (position_encoding.py:25-35) on contiguous rows [rows, C]: out = R(theta) x * scale with cos / sin [rows, C/2]; inverse != 0:
 * R(-theta), the transpose = the backward of the embedding */
int dr_rotary_f32(int rows, int C, const float* x, const float* cos_t, const float* sin_t, int inverse, float scale, float* out, void* stream);
int dr_focal_loss_backward_f32(int P, int N, int M, const float* conf, const float* conf_gt, float alpha, float gamma, float pos_w, float neg_w,
                               float* grad_conf, void* workspace, void* stream);
size_t dr_sinkhorn_backward_workspace_bytes(int P, int N, int M, int iters);
int dr_sinkhorn_backward_f32(int P, int N, int M, const float* scores, const uint8_t* src_mask, const uint8_t* tgt_mask, const float* bin_score,
                             int iters, const float* grad_conf, float* grad_scores, float* grad_bin_score, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 0.7.0, fourth set: the 2D-3D image backbone's inference forward (ImageBackbone.forward, EXP/image_backbone.py:254-289, called at
 * EXP/model.py:358-361) on token rows.  csrc/conv2d.hip, index arithmetic in csrc/conv_index.h.  Every activation is [H W, C] float32 (NHWC)
 * with a leading dimension -- the rows dr_group_norm_stats_f32 / dr_group_norm_apply_f32 take, so nn.GroupNorm(G, C) over [1, C, H, W] is
 * dr_group_norm_stats_f32(N = H W, C, G).  Nothing synchronises, nothing allocates, no atomics: two runs are bit-equal.
 *
 * dr_conv2d_rows_f32: nn.Conv2d(Cin, Cout, k, stride, padding, dilation, groups = 1, padding_mode = "zeros") (vision3d/layers/conv_block.py:118-119;
 *   every conv of EXP/image_backbone.py:21-57 and :81-252): x [Hi Wi, ldx] -> out [Ho Wo, ldo], Ho = (Hi + 2 padding - dilation (k - 1) - 1) / stride
 *   + 1.  weight is PACKED [Cout, k k Cin], tap-major and ci-minor (the module's [Cout, Cin, k, k] permuted to [Cout, k, k, Cin]).  bias [Cout]
 *   or NULL; addend [Ho Wo, lda] or NULL is added last (the sums of EXP/image_backbone.py:272, :277, :280).  Cin % 4 == 0: implicit GEMM on the
 *   f32-input MFMA, A gathered per (output pixel, tap) with 16-byte loads, no im2col buffer, a tap in the padding loads nothing (scalar loads when
 *   x or weight is not 16-byte aligned or ldx % 4 != 0); other Cin: a direct kernel.  Pointers must be 4-byte aligned, Ho, Wo >= 1 (DR_EINVAL);
 *   Hi Wi, Ho Wo <= 2^24, Cin, Cout <= 2^16, k k Cin <= 2^20, k <= 31, stride, dilation <= 64, padding <= 1024, leading dimensions <= 2^20
 *   (DR_ENOSUP beyond).
 * dr_resize_rows_f32: F.interpolate(mode = "bilinear", align_corners = True) from rows to rows (EXP/image_backbone.py:264, :270, :275, :281):
 *   in [Hs Ws, ldi] -> out [Hd Wd, ldo] = addend + resample(in), addend [Hd Wd, lda] or NULL (the sums of :267, :272, :277).  Source index and
 *   weights as dr_resize_tokens_f32 computes them (one shared statement: the two agree bit for bit).  Limits as dr_resize_tokens_f32; every
 *   extent >= 1. */
int dr_conv2d_rows_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* x, int ldx,
                       const float* weight, const float* bias, const float* addend, int lda, float* out, int ldo, void* stream);
int dr_resize_rows_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* in, int ldi, const float* addend, int lda, float* out, int ldo,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 0.7.0, fifth set: the backward of the fourth set's two entries (csrc/conv2d.hip, csrc/conv_index.h, csrc/resize_index.h).
 * The forward's rules hold: token rows [H W, C] float32 with leading dimensions, nothing synchronises, nothing allocates, no atomics (two runs
 * are bit-equal), DR_EINVAL / DR_ENOSUP before any launch for the forward entry's domain (and k k Cout <= 2^20), and EVERY element of every
 * output is written -- zeros where no gradient arrives.
 *
 * dr_conv2d_rows_backward_data_f32: grad_out [Ho Wo, ldg] -> grad_x [Hi Wi, ldgx] (+ addend [Hi Wi, lda] or NULL, added last).  weight_t is
 *   PACKED [Cin, k k Cout], tap-major and co-minor (the module's [Cout, Cin, k, k] permuted to [Cin, k, k, Cout]).  Cout % 4 == 0: the forward's
 *   implicit GEMM with the roles turned (m = input pixel, N = Cin, kk = (tap, co)); a slot whose tap has no output pixel -- the padding, or a
 *   position the stride skips -- loads nothing and is zero.  Other Cout: a direct kernel, double accumulation in a fixed order.
 * dr_conv2d_rows_backward_weight_f32: x [Hi Wi, ldx], grad_out [Ho Wo, ldg] -> grad_w PACKED [Cout, k k Cin] as the forward's weight, and
 *   grad_bias [Cout]; either may be NULL.  The Ho Wo output pixels are reduced in S slabs of L pixels, S and L functions of Ho Wo alone
 *   (S0 = min(64, ceil(M / 2048)), L = ceil(M / S0) rounded up to 32, S = ceil(M / L)): float32 partial sums per slab in the workspace, added in
 *   ascending slab order in double and rounded once.  Cin % 4 == 0: an MFMA kernel; other Cin: a direct kernel over the same slabs.  The
 *   workspace holds dr_conv2d_rows_backward_weight_workspace_bytes(...) bytes (0 for arguments outside the domain: a pure host call) and is
 *   16-byte aligned.
 * dr_resize_rows_backward_f32: grad_out [Hd Wd, ldg] -> grad_in [Hs Ws, ldgi], the backward of dr_resize_rows_f32 with respect to `in` (the
 *   addend's gradient is grad_out itself).  A gather: every source texel sums its destination pixels in a fixed order, through the statement
 *   dr_resize_tokens_backward_f32 uses -- the two agree bit for bit. */
int dr_conv2d_rows_backward_data_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* grad_out, int ldg,
                                     const float* weight_t, const float* addend, int lda, float* grad_x, int ldgx, void* stream);
size_t dr_conv2d_rows_backward_weight_workspace_bytes(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation);
int dr_conv2d_rows_backward_weight_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* x, int ldx,
                                       const float* grad_out, int ldg, float* grad_w, float* grad_bias, void* workspace, size_t workspace_bytes,
                                       void* stream);
int dr_resize_rows_backward_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* grad_out, int ldg, float* grad_in, int ldgi, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, sixth set (detected by symbol like the fourth and fifth sets): the frozen DINOv2 ViT encoder of the 2D-3D model in the
 * reference's own fp16 arithmetic (csrc/vit.hip, index arithmetic in csrc/vit_index.h).  fp16 operands, ONE fp16 MFMA product per MAC,
 * fp32 accumulation; the residual stream is fp32.  Nothing synchronises, nothing allocates, no atomics and no split-k: two runs are bit-equal.
 * Every pointer below is device memory unless said otherwise; "fp16 rows" are IEEE half rows with a leading dimension in elements.
 *
 * dr_pack_weight_f16: an nn.Linear weight [N, K] fp16 (row stride ldw) -> the image dr_gemm_rows_f16 streams, K padded with zeros to
 *   Kp = round_up(K, 32) (the patch embedding's flattened Conv2d weight: 588 -> 608); dr_pack_weight_f16_bytes(N, K) bytes, 16-byte aligned.
 *   N % 16 == 0 (else DR_EINVAL / 0 bytes).
 * dr_gemm_rows_f16: out = A W^T (+ bias), A [M, K] fp16 rows (lda >= K, lda % 8 == 0, 16-byte aligned), W packed with Kp == K.  nn.Linear of
 *   layers/attention.py:52, :60 and layers/mlp.py:35-39, the Conv2d of layers/patch_embed.py:75.  M is ragged: rows past M are never read and
 *   never stored.  K % 32 == 0 and N % 16 == 0, anything else is DR_EINVAL before any access.  bias fp32 [N] or NULL.  mode:
 *     DR_GEMM_ROWS_F16             (acc + bias) * colscale for columns < colscale_cols (a multiple of 16; the q third of qkv takes d^-0.5,
 *                                  layers/attention.py:54), rounded once to fp16 rows
 *     DR_GEMM_ROWS_GELU_F16        exact erf GELU (nn.GELU() default) of acc + bias, rounded once to fp16 rows
 *     DR_GEMM_ROWS_SCALE_RESID_F32 out[row] += gamma[col] * (acc + bias) on fp32 rows in place (gamma fp32 [N], NULL = 1): LayerScale and the
 *                                  residual of layers/block.py:83-87
 *     DR_GEMM_ROWS_F32             acc + bias (+ addend rows fp32 [M, ld_addend], or NULL) as fp32 rows
 *   out, bias, gamma, addend 16-byte aligned, ldo and ld_addend multiples of 4.
 * dr_layernorm_rows_f16: nn.LayerNorm(C, eps) over fp32 rows (layers/block.py:83, :86; dinov2.py:232): statistics in fp32, two passes;
 *   out_f32 = 0: fp16 rows, 1: fp32 rows.  gamma / beta fp32 [C] or NULL.
 * dr_attention_rows_f16: softmax(q k^T) v without a mask over packed qkv rows [L, 3 H d] fp16 in the layout of qkv.reshape(N, 3, H, d)
 *   (layers/attention.py:49-62), q already scaled; out fp16 rows [L, H d].  Flash form, fp32 online softmax, P rounded to fp16 once.  d == 64 only
 *   (else DR_EINVAL); ldqkv % 8 == 0, ldo % 4 == 0, qkv 16-byte and out 8-byte aligned.  Not a form of dr_attention_f32's dispatcher.
 * dr_patch_rows_f16: the p x p patches of a [3, H, W] image (fp16, or fp32 with img_f32 = 1) as fp16 rows [(H / p)(W / p), ldo >= Kp], k in the
 *   order of the flattened Conv2d weight, Kp = round_up(3 p p, 32), pad columns zero (layers/patch_embed.py:69-82).  H % p == W % p == 0.
 * dr_vit_forward_f16: DinoVisionTransformer.forward_features of one image (dinov2.py:166-237): prepare_tokens_with_masks without masks, every
 *   block (layers/block.py:82-107 in eval mode), the final norm.  Writes x_prenorm fp32 [L, D] (L = 1 + patches; it IS the residual stream),
 *   x_norm fp16 [L, D], and the stream after block take[i] into take_out[i] (fp32 [L, D]) for get_intermediate_layers.  `blocks`, `take` and
 *   `take_out` are HOST arrays read during the call; pos is the position rows [L, D] fp32 for this (H, W).  heads * 64 == D, Dh % 32 == 0.
 *   The workspace holds dr_vit_workspace_bytes(H, W, p, D, Dh) bytes (0 outside the domain), 256-byte aligned; less is DR_EINVAL.  The size query
 *   and the entry share one carve function.  It can be captured in a graph. */
#define DR_GEMM_ROWS_F16 0
#define DR_GEMM_ROWS_GELU_F16 1
#define DR_GEMM_ROWS_SCALE_RESID_F32 2
#define DR_GEMM_ROWS_F32 3
typedef struct dr_gemm_rows_f16_args {
    const void* a;                 /* [M, lda] fp16                                                                      */
    const void* w_packed;          /* dr_pack_weight_f16 image of [N, K]                                                 */
    const float* bias;             /* [N] or NULL                                                                        */
    const float* gamma;            /* SCALE_RESID_F32: [N] or NULL                                                       */
    const float* addend;           /* F32: [M, ld_addend] or NULL                                                        */
    void* out;                     /* fp16 or fp32 rows [M, ldo]                                                         */
    int M, K, N, lda, ldo, ld_addend;
    int mode;                      /* DR_GEMM_ROWS_*                                                                     */
    int colscale_cols;             /* F16: columns [0, colscale_cols) are multiplied by colscale                         */
    float colscale;
} dr_gemm_rows_f16_args;
typedef struct dr_vit_block_f16 {
    const float *norm1_g, *norm1_b;
    const void* qkv_w;             /* packed [3 D, D]   */
    const float* qkv_b;
    const void* proj_w;            /* packed [D, D]     */
    const float* proj_b;
    const float* ls1;              /* LayerScale gamma [D] or NULL */
    const float *norm2_g, *norm2_b;
    const void* fc1_w;             /* packed [Dh, D]    */
    const float* fc1_b;
    const void* fc2_w;             /* packed [D, Dh]    */
    const float* fc2_b;
    const float* ls2;
} dr_vit_block_f16;
typedef struct dr_vit_config_f16 {
    int H, W, p, D, heads, Dh, depth;
    float eps;
    const void* img;               /* [3, H, W] fp16, or fp32 with img_f32 = 1 */
    int img_f32;
    const void* patch_w;           /* packed [D, 3 p p] */
    const float* patch_b;
    const float* cls;              /* [D]               */
    const float* pos;              /* [L, D]            */
    const dr_vit_block_f16* blocks;/* HOST array [depth] */
    const float *norm_g, *norm_b;
    float* x_prenorm;              /* out fp32 [L, D]   */
    void* x_norm;                  /* out fp16 [L, D]   */
    int n_take;
    const int* take;               /* HOST [n_take] block indices */
    float* const* take_out;        /* HOST [n_take] device pointers, fp32 [L, D] each */
    void* workspace;
    size_t workspace_bytes;
} dr_vit_config_f16;
size_t dr_pack_weight_f16_bytes(int N, int K);
int dr_pack_weight_f16(int N, int K, const void* w, int ldw, void* packed, void* stream);
int dr_gemm_rows_f16(const dr_gemm_rows_f16_args* args, void* stream);
int dr_layernorm_rows_f16(int rows, int C, const float* x, int ldx, const float* gamma, const float* beta, float eps, int out_f32, void* out, int ldo,
                          void* stream);
int dr_attention_rows_f16(int L, int H, int d, const void* qkv, int ldqkv, void* out, int ldo, void* stream);
int dr_patch_rows_f16(int H, int W, int p, const void* img, int img_f32, void* out, int ldo, void* stream);
size_t dr_vit_workspace_bytes(int H, int W, int p, int D, int Dh);
int dr_vit_forward_f16(const dr_vit_config_f16* cfg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, seventh set (detected by symbol like the fourth to sixth sets): the float32 convolutional decoder of Depth-Anything,
 * DPTHead.forward (depth_anything/dpt.py:103-136, depth_anything/blocks.py:37-153; called through EXP/model.py:343-351).  csrc/conv2d.hip, index
 * arithmetic in csrc/conv_index.h; DESIGN 5q.  The fourth set's rules hold: token rows [H W, C] float32 with leading dimensions, exact fp32
 * products on the f32-input MFMA, no atomics and no split-k, one fixed accumulation order (two runs are bit-equal), nothing synchronises,
 * nothing allocates, DR_EINVAL / DR_ENOSUP before any launch, and dr_conv2d_rows_f32's limits unless said otherwise.  `out` sharing an element
 * with any input is DR_EINVAL.
 *
 * dr_conv2d_rows_act_f32: dr_conv2d_rows_f32 with a flags word and a second addend:
 *     out = relu_out?(conv(relu_in?(x)) + bias) + addend + addend2
 *   DR_CONV_RELU_IN: max(x, 0) on the input as it is fetched (the pre-activation of ResidualConvUnit.forward, blocks.py:79, :84; nn.ReLU(False),
 *   so x itself is untouched and can be the residual).  DR_CONV_RELU_OUT: ReLU after the bias and BEFORE the addends.  addend2 [Ho Wo, lda2] or
 *   NULL is added after addend (blocks.py:92 then :136).  One entry is conv1 of a unit (RELU_IN | RELU_OUT), conv2 of a unit (addend = the unit's
 *   input, addend2 = xs[0] in a fusion block), layerN_rn (blocks.py:20-32), out_conv (:117), projects[i] (dpt.py:29-37, :113-115: the ViT's token
 *   rows are the conv's rows as they are), resize_layers[3] (dpt.py:53-58) and output_conv1 (dpt.py:93).  With flags = 0 and addend2 = NULL the
 *   result is bit-equal to dr_conv2d_rows_f32.  Flags and addend2 exist on the MFMA arm only: either with Cin % 4 != 0 is DR_ENOSUP.  Unknown flag
 *   bits are DR_EINVAL.
 * dr_conv_transpose2d_rows_f32: nn.ConvTranspose2d(Cin, Cout, kernel = s, stride = s, padding 0, output_padding 0, dilation 1, groups 1)
 *   (dpt.py:40-51): x [H W, ldx] -> out [H s W s, ldo], out[(y s + i)(W s) + x s + j][co] = bias[co] + sum_ci x[y W + x][ci] w[ci][co][i][j].  No two
 *   taps meet, so it is one GEMM whose store is a pixel shuffle.  weight is PACKED [s s Cout, Cin] ((i, j) major, co minor: the module's
 *   [Cin, Cout, s, s] permuted to [s, s, Cout, Cin]).  bias [Cout] or NULL.  Every output element is written.  Domain: Cin % 4 == 0, 1 <= s <= 8,
 *   (H s)(W s) <= 2^24, s s Cout <= 2^16, Cin <= 2^16, leading dimensions <= 2^20; s < 1 is DR_EINVAL, everything else outside is DR_ENOSUP.
 * dr_conv2d_rows_project_f32: the head's tail (dpt.py:95-99) in one launch: out[m] = relu_out?(b2 + sum_c w2[c] relu(conv(x)[m][c] + b1[c])),
 *   conv k x k from Cin to Cmid channels (w1 PACKED [Cmid, k k Cin] as dr_conv2d_rows_f32's weight, b1 [Cmid] or NULL), w2 [Cmid], b2 a DEVICE
 *   pointer to one float or NULL; out [Ho Wo] with the leading dimension ldo >= 1 (one value per pixel).  The hidden [Ho Wo, Cmid] is never
 *   written: the products relu(.) w2 are formed and added in double in a fixed order (across the 32 lanes of a row, then across the wave pair)
 *   and rounded once.  Cmid <= 64 and Cin % 4 == 0, else DR_ENOSUP. */
#define DR_CONV_RELU_IN 1
#define DR_CONV_RELU_OUT 2
int dr_conv2d_rows_act_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* x, int ldx,
                           const float* weight, const float* bias, int flags, const float* addend, int lda, const float* addend2, int lda2,
                           float* out, int ldo, void* stream);
int dr_conv_transpose2d_rows_f32(int H, int W, int Cin, int Cout, int s, const float* x, int ldx, const float* weight, const float* bias, float* out,
                                 int ldo, void* stream);
int dr_conv2d_rows_project_f32(int Hi, int Wi, int Cin, int Cmid, int k, int stride, int padding, int dilation, const float* x, int ldx,
                               const float* w1, const float* b1, const float* w2, const float* b2, int relu_out, float* out, int ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, eighth set (detected by symbol like the fourth to seventh sets): the float32 ViT-L/14 encoder of Depth-Anything,
 * DPT_DINOv2.forward's self.pretrained.get_intermediate_layers(x, 4, return_class_token=True) (depth_anything/dpt.py:155-166; the class is
 * torchhub/facebookresearch_dinov2_main/vision_transformer.py, called once per pair through EXP/model.py:339-345).  csrc/vit_f32.hip, index
 * arithmetic in csrc/vit_f32_index.h; DESIGN 5r.  float32 operands, exact fp32 products on the f32-input MFMA, fp32 accumulation in one fixed k
 * order; no atomics and no split-k across workgroups: two runs are bit-equal.  Nothing synchronises, nothing allocates; every entry can be
 * captured in a graph.  Every pointer below is device memory unless said otherwise.  The sixth set (fp16) is untouched.
 *
 * dr_gemm_rows_f32: out = A W^T (+ bias), A [M, K] float32 rows (lda >= K, lda % 4 == 0, 16-byte aligned), W the nn.Linear weight [N, K] as it is
 *   (row stride ldw >= K, ldw % 4 == 0, 16-byte aligned; there is no packed image).  nn.Linear of dinov2/layers/attention.py:52, :60 and
 *   dinov2/layers/mlp.py:35-39, the Conv2d of dinov2/layers/patch_embed.py:75.  M is ragged: rows past M are never read and never stored.
 *   K % 32 == 0 and N % 16 == 0 (K >= 32, N >= 16), anything else is DR_EINVAL before any access.  bias [N] or NULL.  mode:
 *     DR_GEMM_ROWS32_COLSCALE     (acc + bias) * colscale for columns < colscale_cols (a multiple of 16; the q third of qkv takes d^-0.5,
 *                                 layers/attention.py:54); the other columns acc + bias
 *     DR_GEMM_ROWS32_GELU         exact erf GELU (nn.GELU() default) of acc + bias
 *     DR_GEMM_ROWS32_SCALE_RESID  out[row] += gamma[col] * (acc + bias) in place (gamma [N], NULL = 1): LayerScale and the residual of
 *                                 layers/block.py:83-87
 *     DR_GEMM_ROWS32_ADDEND       acc + bias (+ addend rows [M, ld_addend >= N], or NULL): the patch embedding plus the position rows
 *   gamma outside SCALE_RESID, addend outside ADDEND and colscale_cols != 0 outside COLSCALE are DR_EINVAL.  out [M, ldo >= N] sharing an element
 *   with A, W, bias, gamma or addend is DR_EINVAL (in SCALE_RESID out itself is the one input it has to be).  M lda, M ldo, N ldw < 2^31, else
 *   DR_ENOSUP.  The workgroup tile follows from (M, K, N) alone (dr_debug_gemm_rows_f32_tile forces one).
 * dr_patch_rows_f32: the p x p patches of a [3, H, W] float32 image as float32 rows [(H / p)(W / p), ldo >= Kp], k in the order of the flattened
 *   Conv2d weight, Kp = round_up(3 p p, 32), pad columns zero (layers/patch_embed.py:69-82).  H % p == W % p == 0.
 * dr_vit_forward_f32: DinoVisionTransformer.forward_features and get_intermediate_layers of one image (vision_transformer.py:212-231, :253-321):
 *   prepare_tokens_with_masks without masks or register tokens, every block (layers/block.py in eval mode, Attention.forward of
 *   layers/attention.py:49-62), the final norm.  Writes x_prenorm [L, D] (L = 1 + patches; it IS the residual stream), x_norm [L, D], and for
 *   each i < n_take the stream after block take[i] into take_out[i] ([L, D]) -- through the final norm when norm_take = 1
 *   (get_intermediate_layers(..., norm=True), :309-310), as it is when norm_take = 0.  `blocks`, `take` and `take_out` are HOST arrays read
 *   during the call; pos is the position rows [L, D] for this (H, W).  Weights are the modules' own [N, K] matrices, contiguous; patch_w is
 *   [D, Kp] with its pad columns zero.  heads * 64 == D, Dh % 32 == 0.  The workspace holds dr_vit_workspace_bytes_f32(H, W, p, D, Dh) bytes (0
 *   outside the domain), 256-byte aligned; less is DR_EINVAL.  The size query and the entry share one carve function. */
#define DR_GEMM_ROWS32_COLSCALE 0
#define DR_GEMM_ROWS32_GELU 1
#define DR_GEMM_ROWS32_SCALE_RESID 2
#define DR_GEMM_ROWS32_ADDEND 3
typedef struct dr_gemm_rows_f32_args {
    const float* a;                /* [M, lda]                                                                           */
    const float* w;                /* [N, ldw]                                                                           */
    const float* bias;             /* [N] or NULL                                                                        */
    const float* gamma;            /* SCALE_RESID: [N] or NULL                                                           */
    const float* addend;           /* ADDEND: [M, ld_addend] or NULL                                                     */
    float* out;                    /* [M, ldo]                                                                           */
    int M, K, N, lda, ldw, ldo, ld_addend;
    int mode;                      /* DR_GEMM_ROWS32_*                                                                   */
    int colscale_cols;             /* COLSCALE: columns [0, colscale_cols) are multiplied by colscale                    */
    float colscale;
} dr_gemm_rows_f32_args;
typedef struct dr_vit_block_f32 {
    const float *norm1_g, *norm1_b;
    const float *qkv_w, *qkv_b;    /* [3 D, D], [3 D]   */
    const float *proj_w, *proj_b;  /* [D, D], [D]       */
    const float* ls1;              /* LayerScale gamma [D] or NULL */
    const float *norm2_g, *norm2_b;
    const float *fc1_w, *fc1_b;    /* [Dh, D], [Dh]     */
    const float *fc2_w, *fc2_b;    /* [D, Dh], [D]      */
    const float* ls2;
} dr_vit_block_f32;
typedef struct dr_vit_config_f32 {
    int H, W, p, D, heads, Dh, depth;
    float eps;
    const float* img;              /* [3, H, W]         */
    const float* patch_w;          /* [D, Kp]           */
    const float* patch_b;
    const float* cls;              /* [D]               */
    const float* pos;              /* [L, D]            */
    const dr_vit_block_f32* blocks;/* HOST array [depth] */
    const float *norm_g, *norm_b;
    float* x_prenorm;              /* out [L, D]        */
    float* x_norm;                 /* out [L, D]        */
    int n_take;
    int norm_take;                 /* 1: take_out[i] = norm(stream after block take[i]) */
    const int* take;               /* HOST [n_take] block indices */
    float* const* take_out;        /* HOST [n_take] device pointers, [L, D] each */
    void* workspace;
    size_t workspace_bytes;
} dr_vit_config_f32;
int dr_gemm_rows_f32(const dr_gemm_rows_f32_args* args, void* stream);
int dr_patch_rows_f32(int H, int W, int p, const float* img, float* out, int ldo, void* stream);
size_t dr_vit_workspace_bytes_f32(int H, int W, int p, int D, int Dh);
int dr_vit_forward_f32(const dr_vit_config_f32* cfg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, ninth set (detected by symbol like the fourth to eighth sets): the collate-time native code of the 2D-3D loader
 * (GraphPyramid2D3DRegistrationCollateFn, vision3d/utils/collate.py:265-310 -> vision3d/array_ops/graph_pyramid.py:9-70 -> the two functions of
 * vision3d/csrc/cpu/) and the calibration of its neighbour limits (calibrate_neighbors_pack_mode, vision3d/utils/dataloader.py:42-67).
 * csrc/collate.hip; DESIGN 5s.  Lengths are int32 [nb] on the device as for the other collate entries; `status` has their meaning; nothing
 * synchronises, nothing allocates, every entry can be captured in a graph.
 *
 * vision3d's two functions against the KPConv forms the older entries restate, expression by expression:
 *   grid_subsampling.cpp:32   origin = floor(min_corner / voxel_size) * voxel_size     DIFFERS: KPConv multiplies by the float reciprocal,
 *                             floor(min * (1 / dl)) * dl, which names another origin when min / voxel_size lies within a rounding of an
 *                             integer -- hence dr_grid_subsample_vision3d_f32
 *   grid_subsampling.cpp:39-41  floor((p - origin) / voxel_size) per axis               same
 *   grid_subsampling.h:23-26  count += 1; point += p, in input order (cloud.h:50-55)    same
 *   grid_subsampling.cpp:52   point * (1.0 / count): the double reciprocal narrowed to float by operator*(Point, const float) (cloud.h:76)   same
 *   radius_neighbors.cpp:24-60  radius2 = radius * radius in float; nanoflann 1.3.0 L2_Simple_Adaptor (result += diff * diff per axis),
 *                             RadiusResultSet::addPoint keeps dist < radius (strict), search_params.sorted = true   same
 *   radius_neighbors.cpp:82-84  cloud-local index + the cloud's first support row; padding = the total number of supports   same
 * so dr_radius_neighbors_f32 serves vision3d's radius_neighbors(...)[:, :limit] as it is (limits above 64 stay DR_EINVAL).
 *
 * dr_grid_subsample_vision3d_f32: dr_grid_subsample_f32 with vision3d's origin; same arguments, same output order (per cloud ascending
 *   (iz, iy, ix); the reference emits std::unordered_map order), same workspace (dr_grid_subsample_workspace_bytes).  A cloud of length 0
 *   yields length 0.
 * dr_radius_count_hist_f32: per query the NUMBER of supports of its own cloud with d^2 < radius^2 -- the float32 expression and the sweep of
 *   dr_radius_neighbors_f32, with a counter in place of the list: the count has no upper limit.  hist [hist_n] int32 is ACCUMULATED:
 *   hist[count] += 1 when count < hist_n; counts >= hist_n are not recorded (np.bincount(c, minlength=hist_n)[:hist_n] of a matrix cut at
 *   hist_n columns, dataloader.py:56-58).  The caller zeroes hist before the first call.  counts [nq] int32 or NULL receives every count.
 *   1 <= hist_n <= 4096 (the bins of a workgroup live in LDS), else DR_EINVAL; ns = 0 records nq counts of 0.  Integer atomics only: two runs
 *   are bit-equal.  Workspace: dr_radius_count_hist_workspace_bytes(nq, ns, nb), DR_EWORKSPACE when smaller. */
int dr_grid_subsample_vision3d_f32(int n, int nb, const float* points, const int32_t* lengths, float voxel_size, float* out_points,
                                   int32_t* out_lengths, int32_t* out_total, int32_t* status, void* workspace, size_t workspace_bytes,
                                   void* stream);
size_t dr_radius_count_hist_workspace_bytes(int nq, int ns, int nb);
int dr_radius_count_hist_f32(int nq, int ns, int nb, const float* queries, const float* supports, const int32_t* q_lengths,
                             const int32_t* s_lengths, float radius, int hist_n, int32_t* hist, int32_t* counts, int32_t* status,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, tenth set (detected by symbol like the fourth to ninth sets): the input transform in front of Depth-Anything,
 * depth_anything/util/transform.py:168-178, 219-222, 232-234 (Resize.__call__ with cv2.INTER_CUBIC, NormalizeImage.__call__,
 * PrepareForNet.__call__), which EXP/model.py:339-342 runs on the host on every forward.  csrc/image_transform.hip; DESIGN 5t.
 *
 * dr_image_cubic_chw_f32: src_hwc [Hs, Ws, 3] float32 with ld_src >= 3 Ws floats per source row -> out_chw [3, Hd, Wd] float32, contiguous.
 *   The resample is OpenCV's INTER_CUBIC for CV_32F as csrc/cubic_index.h states it: per axis scale = (double)in / out; for destination d,
 *   f = (float)((d + 0.5) scale - 0.5), s = floor(f), t = f - s in float; the Keys weights with A = -0.75 in float, the fourth as
 *   1 - c0 - c1 - c2; taps s-1 .. s+2 clamped to [0, in-1]; no antialiasing; the 16-term blend columns first, then rows, in double on the
 *   float32 texels, rounded once to float32 (OpenCV's float32 output).  With `normalize` non-zero each channel c then becomes
 *   (float)(((double)v - mean[c]) / std[c]): numpy's float64 arithmetic narrowed by PrepareForNet's astype(float32).  `norm` is a HOST struct,
 *   read when the call is enqueued and passed as kernel arguments (a captured graph keeps the values of the capture); NULL is allowed when
 *   `normalize` is 0.  `stream` is a hipStream_t.
 *   One launch; no workspace, no atomics, no scratch; two runs are bit-equal; nothing synchronises, so the call can be captured in a graph.
 *   DR_EINVAL, with the output untouched: Hs, Ws, Hd or Wd < 1; ld_src < 3 Ws; a NULL src_hwc or out_chw; `normalize` with a NULL norm or a
 *   std[c] == 0. */
typedef struct {
    double mean[3];
    double std[3];
} dr_image_norm;
int dr_image_cubic_chw_f32(int Hs, int Ws, int ld_src, const float* src_hwc, int Hd, int Wd, int normalize, const dr_image_norm* norm,
                           float* out_chw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, eleventh set (detected by symbol like the fourth to tenth sets): the ground-truth half of the 3D / 4D training
 * collate, 3D/datasets/dataloader.py:236-259, 495-523 with 3D/datasets/utils.py:23-80, which the reference runs per pair on its loader's CPU
 * workers.  csrc/collate_gt.hip, indices in csrc/collate_gt_index.h; DESIGN 5u.
 *
 * Both entries are ragged over P pairs in one call: pair p's rows of a stacked [n, 3] float32 array are [offsets[p], offsets[p + 1]) of an int32
 * DEVICE array of P + 1 entries.  They are asynchronous on `stream` (a hipStream_t), read nothing back to the host, allocate nothing and use no
 * atomics: two runs are bit-equal, and a call can be captured in a graph.  All float32 arithmetic is unfused, operation by operation as numpy
 * performs it; d^2 = ((dx dx + dy dy) + dz dz) with d = reference - query; sqrtf and the divisions are correctly rounded.
 * status [P] int32 receives per pair 0, or bit 0 (1): too few points, where the reference's np.argpartition raises; bit 1 (2): the pair's offsets
 * are not 0 <= lo <= hi <= n.  A pair with a non-zero status is neither read nor computed.  P = 0 is a no-op; a negative size or a NULL pointer
 * that a non-empty array needs is DR_EINVAL; n * 3 or the grid beyond 2^31 - 1 is DR_ENOSUP.
 *
 * dr_blend_flow_knn3_f32: blend_scene_flow(query, reference, reference_flow, knn=3) of utils.py:43-59.  Per query the three references of its
 *   pair with the smallest d^2, in ascending d^2; EQUAL d^2 go to the LOWEST index (the reference's np.argpartition leaves the order of equal
 *   distances unspecified).  dist = max(sqrtf(d^2), 1e-10f), w = 1 / dist, w_k /= (w0 + w1) + w2, out_flow = (f0 w0 + f1 w1) + f2 w2 per
 *   component.  A pair with fewer than 4 references gets status bit 0 and its rows of out_flow stay untouched (np.argpartition(kth=3) raises).
 * dr_coarse_gt_matches_f32: the `get match at coarse level` block.  src [ns, 3] / tgt [nt, 3]: the pairs' coarse source / target clouds, stacked
 *   each on its own; src_flow [ns, 3] or NULL (4DMatch: p' = p + flow first); rot [P, 3, 3], trn [P, 3]: w = ((r0 x + r1 y) + r2 z) + t per row
 *   (the reference's matmul may round differently by an ulp where a BLAS fuses; this entry does not imitate that).  Then
 *   multual_nn_correspondence(w, tgt, radius, knn=1): nearest target j of every source i and nearest source of every target, equal d^2 to the
 *   lowest index; i is kept when the nearest source of j is i and sqrtf(d^2) < radius.  Pair p's kept (i, j), pair-local, in ascending i, are
 *   written to out_src / out_tgt [ns] int64 from row s_offsets[p]; counts [P] int32 receives their number.  Rows behind a pair's count are not
 *   written.  A pair whose source or target cloud has fewer than 2 points gets count 0 and status bit 0 (np.argpartition(kth=1) raises).
 *   Workspace: dr_coarse_gt_matches_workspace_bytes(ns, nt), 4-byte aligned; DR_EWORKSPACE when missing or smaller.  The size query and the entry
 *   share one carve function. */
int dr_blend_flow_knn3_f32(int P, int nq, int nr, const float* query, const int32_t* q_offsets, const float* reference,
                           const float* reference_flow, const int32_t* r_offsets, float* out_flow, int32_t* status, void* stream);
size_t dr_coarse_gt_matches_workspace_bytes(int ns, int nt);
int dr_coarse_gt_matches_f32(int P, int ns, int nt, const float* src, const int32_t* s_offsets, const float* tgt, const int32_t* t_offsets,
                             const float* src_flow, const float* rot, const float* trn, float radius, int64_t* out_src, int64_t* out_tgt,
                             int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, twelfth set (detected by symbol like the fourth to eleventh sets): the closing leg of a training iteration -- the
 * gradient gate and the SGD / Adam / AdamW update.  csrc/optim.hip, indices in csrc/optim_index.h; DESIGN 5v.
 *
 * A parameter set is a HOST array of `count` descriptors; every pointer in a descriptor is a DEVICE pointer to contiguous float32 values that
 * needs only 4-byte alignment, and the pointers of one tensor may sit at different offsets from a 16-byte boundary.  The entries copy the
 * descriptors by value into the argument blocks of their launches (64 tensors per launch, as many launches as the set needs): the host array
 * is not read after the call returns.  They are asynchronous on `stream` (a hipStream_t), never synchronise the host, read nothing back,
 * allocate nothing, use no scratch and no atomic other than the integer OR into the status word: two runs are bit-equal and the sequence
 * finite -> step (per group) -> finish can be captured on one stream.  A descriptor with numel == 0 is skipped (its pointers are not looked
 * at); a 0-d tensor is numel == 1.  A NULL or misaligned pointer that a non-empty tensor needs, or an option outside torch's own argument
 * checks, is DR_EINVAL, reported before the first launch.
 *
 * status word: one int32 on the device, owned by the caller, zero before the first sweep.  step counter / skipped counter: one int32 each.
 *
 * dr_grads_finite_multi_f32: validate_gradient(model), 3D/lib/utils.py:96-106 (one isnan().any() and one isinf().any() with a host read each,
 *   per parameter tensor, called at lib/trainer.py:195), and check_gradients, 2D-3D vision3d/engine/base_trainer.py:311-325.  Sweeps `grad`
 *   of every descriptor (the other pointers are not looked at) and ORs DR_GRAD_NAN / DR_GRAD_POS_INF / DR_GRAD_NEG_INF into *status_word.  The
 *   word is NOT reset: the sweeps of several parameter groups accumulate into one.
 * dr_sgd_step_multi_f32: optimizer.step() of torch.optim.SGD (3D/main.py:90-96 builds it; lib/trainer.py:197-199 steps it and zeroes the
 *   gradients), per element in float32, in the order of torch's single-tensor statement; fma(a, b, c) = a b + c with one rounding, where
 *   torch's own elementwise kernel for `self + alpha * other` has one, and nothing else fused:
 *     g = maximize ? -g : g;  if (weight_decay != 0) g = fma(wd, p, g);
 *     if (momentum != 0) { buf = (*step_counter == 0) ? g : fma(1 - dampening, g, buf momentum);  g = nesterov ? fma(momentum, buf, g) : buf; }
 *     p = fma(-lr, g, p)
 *   state0 = momentum_buffer; with momentum == 0 state0 is not looked at and may be NULL.  state1 is not looked at.  The scalars are rounded to
 *   float32 once, (1 - dampening) in double first, as torch's kernels receive them.
 * dr_adam_step_multi_f32: optimizer.step() of torch.optim.Adam / AdamW (3D/main.py:97-103; 2D-3D vision3d/utils/optimizer.py:134-141, stepped
 *   at vision3d/engine/base_trainer.py:253-254); amsgrad is not provided.  state0 = exp_avg, state1 = exp_avg_sq.  With t = *step_counter + 1:
 *     g = maximize ? -g : g;  if (weight_decay != 0) { decoupled ? p = p (1 - lr wd) : g = fma(wd, p, g); }
 *     m = lerp(m, g, 1 - beta1) = fma(w, g - m, m) for w < 0.5;  v = fma(1 - beta2, g g, v beta2);
 *     p = fma(-(lr / (1 - beta1^t)), m / (sqrtf(v) r + eps), p) with r = 1.f / (float)sqrt(1 - beta2^t)
 *   The bias corrections are computed in the kernel, in double, from the device counter (the host does not know whether a gated step was
 *   taken) and rounded to float32 where torch rounds them.
 *   Both updates are gated: when *status_word != 0 no parameter and no state is written.  zero_grads != 0: the same pass writes 0 into every
 *   gradient (zero_grad(set_to_none=False)), also when gated off, as the reference zeroes them either way.
 * dr_optim_finish: one workgroup.  *status_word == 0: ++*step_counter; otherwise ++*skipped_counter (may be NULL).  Then *status_word = 0, and
 *   the new step count is written as float32 into step_mirror[0 .. n_mirror) (torch's per-parameter Adam `step` entries; may be NULL / 0). */
#define DR_GRAD_NAN 0x1
#define DR_GRAD_POS_INF 0x2
#define DR_GRAD_NEG_INF 0x4
typedef struct dr_optim_tensor {
    void* param;
    void* grad;
    void* state0;
    void* state1;
    size_t numel;
} dr_optim_tensor;
typedef struct dr_sgd_options {
    double lr, weight_decay, momentum, dampening;
    int nesterov, maximize, zero_grads;
} dr_sgd_options;
typedef struct dr_adam_options {
    double lr, beta1, beta2, eps, weight_decay;
    int decoupled, maximize, zero_grads;
} dr_adam_options;
int dr_grads_finite_multi_f32(const dr_optim_tensor* tensors, size_t count, int32_t* status_word, void* stream);
int dr_sgd_step_multi_f32(const dr_optim_tensor* tensors, size_t count, const dr_sgd_options* options, const int32_t* status_word,
                          const int32_t* step_counter, void* stream);
int dr_adam_step_multi_f32(const dr_optim_tensor* tensors, size_t count, const dr_adam_options* options, const int32_t* status_word,
                           const int32_t* step_counter, void* stream);
int dr_optim_finish(int32_t* status_word, int32_t* step_counter, int32_t* skipped_counter, float* step_mirror, size_t n_mirror, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, thirteenth set (detected by symbol like the fourth to twelfth sets): the pixel-point ground truth of a 2D-3D dataset
 * item, which the reference builds per item on a loader worker with two cKDTrees: get_2d3d_correspondences_mutual / _radius, 2D-3D
 * vision3d/array_ops/registration_utils.py:30-60, 63-89, with back_project and render (array_ops/depth_image.py:9-65, 68-99), apply_transform
 * (array_ops/se3.py:7-17) and mutual_select (array_ops/mutual_select.py:7-35); the np.unique lists of return_overlap_indices
 * (datasets/registration/sevenscenes/sevenscenes_hard.py:184-196).  csrc/item2d3d.hip, indices in csrc/item2d3d_index.h; DESIGN 5w.
 *
 * Common to the three entries.  depth [H, W] float32 in raw units; intrinsics [9] and transform [16] float64 row-major, DEVICE pointers; points
 * [N, 3] float32 (points_f64 == 0) or float64.  All arithmetic is float64 and unfused.  Image point of pixel (h, w): z = depth / scaling_factor,
 * z > depth_limit -> 0 (pass +inf for the reference's depth_limit=None), kept when z > 0; x = (w - cx) z / fx; y = (v - cy) z / fy with
 * v = (h W + w) / W, back_project's TRUE division -- v keeps the fraction w / W.  The reference's image-point index is the rank of the pixel
 * among the kept ones in row-major order; the entries return pixels, so they order by h W + w, which is the same order.  Cloud point:
 * q = ((x r0 + y r1) + z r2) + t per row of transform (apply_transform; a BLAS may round the reference's matmul differently by an ulp, which
 * this entry does not imitate).  d^2 = ((dx dx + dy dy) + dz dz), 3D test sqrt(d^2) < radius_3d.  render(q) = (trunc(fy qy / qz + cy),
 * trunc(fx qx / qz + cx)): array_ops.render TRUNCATES with .astype(int), unlike the vision3d.ops version dr_render_f32 restates.  2D test:
 * sqrt(dh dh + dw dw) < radius_2d between the integer pixel and render(q); a render value that is not finite or reaches 2^30 passes no 2D test
 * (numpy's cast is undefined there).
 * The entries are asynchronous on `stream`, read nothing back, allocate nothing and use no atomics: two runs are bit-equal.  counts [2] int32
 * receives (rows written = min(found, cap), rows found, saturated at 2^31 - 1); found > cap is never a silent cut: the caller reads counts.
 * Rows behind counts[0] are not written.  H W <= 2^30 and N <= 2^28, else DR_ENOSUP.  Workspace: the entry's size query, 32-byte aligned;
 * DR_EWORKSPACE when missing or smaller.  The three size queries share one carve function with the entries.
 *
 * dr_corr_2d3d_mutual_f64: pairs (pixel i, point j) with j the nearest cloud point of i, i the nearest image point of j, and both tests
 *   passed; EQUAL d^2 go to the LOWEST index on either side (the reference's cKDTree leaves ties unspecified).  Ascending i (mutual_select's
 *   order).  img_corr_pixels [cap, 2] int64 (h, w), pcd_corr_indices [cap] int64; cap = min(H W, N) always suffices.  Only pairs closer than
 *   radius_3d survive, so a point's nearest pixel is searched inside the pixel window its radius_3d ball projects to (the whole image when
 *   qz <= radius_3d, no pixel when qz <= -radius_3d), and the reverse check runs for those at most N pixels against the whole cloud.
 * dr_corr_2d3d_radius_f64: all pairs that pass both tests, in ascending (i, j) (the reference's inner order is its KD-tree's).
 * dr_overlap_2d3d_f64: np.unique of the radius variant's pixel indices h W + w and of its point indices, without building the pair list:
 *   img_overlap_indices [cap_img] int64, pcd_overlap_indices [cap_pcd] int64, both ascending; counts [4] = (written, found) of either.
 * dr_column_mean_seq_f32: out [3] = x.mean(axis=0) of a float32 [n, 3] array as numpy performs it (sevenscenes_hard.py:140, the centre of the
 *   augmentation): the rows are added one after the other in float32 -- numpy's pairwise blocks apply to the inner axis only -- and the sum is
 *   divided by (float)n.  A parallel sum rounds differently, and the difference would show in the item's float32 transform.  n >= 1. */
int dr_column_mean_seq_f32(int n, const float* x, float* out, void* stream);
size_t dr_corr_2d3d_mutual_workspace_bytes(int H, int W, int N);
int dr_corr_2d3d_mutual_f64(int H, int W, int N, const float* depth, double scaling_factor, double depth_limit, const double* intrinsics,
                            const void* points, int points_f64, const double* transform, double radius_2d, double radius_3d, long long cap,
                            int64_t* img_corr_pixels, int64_t* pcd_corr_indices, int32_t* counts, void* workspace, size_t workspace_bytes,
                            void* stream);
size_t dr_corr_2d3d_radius_workspace_bytes(int H, int W, int N);
int dr_corr_2d3d_radius_f64(int H, int W, int N, const float* depth, double scaling_factor, double depth_limit, const double* intrinsics,
                            const void* points, int points_f64, const double* transform, double radius_2d, double radius_3d, long long cap,
                            int64_t* img_corr_pixels, int64_t* pcd_corr_indices, int32_t* counts, void* workspace, size_t workspace_bytes,
                            void* stream);
size_t dr_overlap_2d3d_workspace_bytes(int H, int W, int N);
int dr_overlap_2d3d_f64(int H, int W, int N, const float* depth, double scaling_factor, double depth_limit, const double* intrinsics,
                        const void* points, int points_f64, const double* transform, double radius_2d, double radius_3d, long long cap_img,
                        long long cap_pcd, int64_t* img_overlap_indices, int64_t* pcd_overlap_indices, int32_t* counts, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, fourteenth set (detected by symbol like the fourth to thirteenth sets): non-rigid ICP on an embedded deformation graph,
 * the step from a 4DMatch match list to a deformation field.  2D-3D vision3d/ops/deformation_graph.py:26-103, vision3d/ops/
 * embedded_deformation.py:31-66, vision3d/ops/nonrigid_icp_adam.py:9-131.  csrc/nonrigid.hip, indices in csrc/nonrigid_index.h; DESIGN 5x.
 *
 * All entries are ragged over P pairs: pair p's rows of a stacked array are [offsets[p], offsets[p + 1]) of an int32 DEVICE array of P + 1 entries
 * (p_offsets: points, m_offsets: nodes, c_offsets: correspondences, e_offsets: edges).  Node indices (anchors, edge endpoints) are PAIR-LOCAL
 * int64.  The entries are asynchronous on `stream` (a hipStream_t), allocate nothing, read nothing back to the host and use no floating-point
 * atomic: two runs are bit-equal and every entry can be captured in a graph (dr_init sets the solver's LDS attribute, outside any capture).
 * status [P] int32 receives per pair 0 or a sum of: 1, the pair has points but no node (dr_ed_graph_f32) or more nodes than max_nodes;
 * 2, the pair's offsets are not 0 <= lo <= hi <= total; 4, an anchor outside [-1, M) or an edge endpoint outside [0, M) was met and treated as
 * absent; 8 (dr_ed_graph_f32), a NaN or Inf coordinate of a point or a node left a point with fewer than min(K, M) anchors; 16
 * (dr_nicp_adam_f32), a negative resumed step count was taken as 0; 32 is the sixteenth set's (a failed pivot); 64 and 128 are the seventeenth
 * set's (dr_fps_nodes_f32: sample_cap reached before the stop rule; point 0 of the cloud is not finite), the only two bits of that set's status
 * which NonRigidRegistration ORs into the same word (its 1, 2 and 8 mean other things there and are masked off); 256 and 512 are the
 * eighteenth set's (dr_geo_graph_f32: a duplicate node index; a point with more neighbours than max_degree).  A pair with bit 1 or 2 is neither read nor computed: its rows of the
 * outputs are not written.  max_nodes is an upper bound of every pair's node count known to the HOST.  1 <= K <= 8.  P = 0 is a no-op; a negative size, a K out of range or a NULL pointer that a non-empty array needs is DR_EINVAL, a
 * product of sizes beyond 2^31 - 1 DR_ENOSUP, a missing or short workspace DR_EWORKSPACE (16-byte aligned, else DR_EINVAL): all reported before
 * the first launch, with every output untouched.
 *
 * dr_ed_graph_f32: build_euclidean_deformation_graph (deformation_graph.py:26-103).  Anchors: the min(K, M) nearest nodes of each point by brute
 *   force in float64 on the float32 coordinates, d^2 = (dx dx + dy dy) + dz dz, ascending by d^2 and by the LOWEST index on equal d^2 (KeOps'
 *   Kmin_argKmin leaves ties unspecified); columns from min(K, M) on receive index -1, weight 0, distance 0.  Only a FINITE d^2 makes an
 *   anchor: a point or node with a NaN or Inf coordinate anchors nothing, the point's remaining columns are -1 / 0 / 0, its weights are
 *   normalised over the anchors it has, no bit of the map is touched for the missing ones, and the pair gets status bit 8.  anchor_distances (or NULL) =
 *   sqrt(d^2); anchor_weights = exp(-d^2 / (2 c^2)) divided by the row's sum (:22, :70-71), each rounded once to float32.  Two nodes are adjacent
 *   when they anchor the same point (self edges included, :80-83): an M x M bit map in the workspace, filled with integer OR.  The edge list is
 *   torch.nonzero's (:95): row-major ascending.  edge_distances (or NULL) = sqrt(max(|a|^2 - 2 a.b + |b|^2, 0) + 1e-8), pairwise_distance's
 *   non-strict form (pairwise_distance.py:51-58; a self edge is 1e-4, not 0); edge_weights = its skinning weight over max(row sum, eps) (:85-87).
 *   TWO calls: with e_offsets == NULL the entry writes the anchors, fills the bit map and writes edge_counts [P]; the caller turns the counts into
 *   e_offsets [P + 1] (the one host read of a batch, or a device cumsum) and calls again with e_offsets != NULL and the SAME workspace, which
 *   writes pair p's edges from row e_offsets[p]; rows at or behind min(e_offsets[p + 1], edge_cap) are not written.  node_coverage > 0.
 *   Workspace: dr_ed_graph_workspace_bytes(n_nodes, max_nodes): n_nodes rows of ceil(max_nodes / 32) words, plus 12 bytes per node.
 *   0 <= max_nodes <= n_nodes, else DR_EINVAL.
 * dr_ed_warp_f32: apply_deformation (embedded_deformation.py:31-66) for any point set: out = sum_k w_k (R_k (p - g_k) + t_k + g_k) over the
 *   anchors k != -1, w_k = anchor_weights_k / (sum over ALL K columns + eps) (:53), in float64, rounded once.  A point whose anchors are all -1
 *   warps to zero (:63-65).  One thread per point.  transforms [n_nodes, 4, 4] row-major.
 * dr_nicp_node_capacity: the largest node count of one pair the two solver entries accept: rotations, translations and both Adam moments of a
 *   pair live in the LDS of one compute unit (csrc/nonrigid_index.h states the carve); at least 512.  There is no global-memory path above it.
 * dr_nicp_cost_grad_f32: compute_cost_function (nonrigid_icp_adam.py:9-73) at the given rotations [n_nodes, 3, 3] / translations [n_nodes, 3]:
 *   cost [P, 3] = (landmark: mean over the pair's N correspondences, :18; ARAP: mean over ALL its E edges, self edges counted, :36; orthogonality:
 *   mean over its M nodes, :50-51), and grad_rot / grad_trn = the gradient of w_landmark landmark + w_arap arap + w_ortho ortho.  An empty mean is
 *   NaN, as torch's.  Gradients reach a node by gather through node-major lists built in the workspace, each summed in float64 in a fixed order
 *   and rounded once.  problem->max_nodes: an upper bound of every pair's node count known to the HOST, <= dr_nicp_node_capacity(), else
 *   DR_EINVAL; it sizes the LDS of the launch.
 * dr_nicp_adam_f32: non_rigid_icp_adam (nonrigid_icp_adam.py:76-131): options->num_iterations iterations of (cost, backward, Adam step,
 *   ExponentialLR step) in ONE launch, one workgroup per pair.  Adam is torch's single-tensor statement as dr_adam_step_multi_f32 restates it
 *   (no weight decay, no amsgrad), evaluated in float64 on the float32 state with each of parameter, exp_avg and exp_avg_sq rounded once per
 *   iteration; the bias corrections are float64 from the step count; lr is multiplied by gamma once per iteration in float64,
 *   step times before the first iteration when resuming (a negative step is taken as 0: status bit 16).  state: NULL, or a struct of DEVICE pointers (each may be NULL): with resume != 0 the run
 *   starts from them (a NULL moment is zero, a NULL step 0; rotations / translations are required), otherwise from identity rotations, zero
 *   translations and moments, step 0; non-NULL members receive the final state either way (step [P] += num_iterations).  transforms
 *   [n_nodes, 4, 4] and cost [P, 3] (the three terms at the FINAL state; may be NULL) are always written; num_iterations == 0 returns the
 *   starting state.  trace (or NULL) [P, num_iterations, 3] receives the three terms each iteration's backward started from.
 *   Workspace of both: dr_nicp_workspace_bytes(P, n_corr, n_nodes, n_edges, K); the size query and the entries share one carve. */
typedef struct dr_nicp_problem {
    int P, n_corr, n_nodes, n_edges, K, max_nodes;
    const float* nodes;               /* [n_nodes, 3] */
    const int32_t* m_offsets;
    const float* src_corr;            /* [n_corr, 3] */
    const float* tgt_corr;            /* [n_corr, 3] */
    const int32_t* c_offsets;
    const int64_t* anchor_indices;    /* [n_corr, K] */
    const float* anchor_weights;      /* [n_corr, K] */
    const int64_t* edges;             /* [n_edges, 2] */
    const float* edge_weights;        /* [n_edges] */
    const int32_t* e_offsets;
} dr_nicp_problem;
typedef struct dr_nicp_options {
    int num_iterations;                                   /* 500 */
    double lr, gamma, beta1, beta2, eps;                  /* 0.5, 0.999, 0.9, 0.999, 1e-8 */
    double w_landmark, w_arap, w_ortho;                   /* 1.0, 0.1, 0.1 */
} dr_nicp_options;
typedef struct dr_nicp_state {
    float* rotations;                 /* [n_nodes, 3, 3] */
    float* translations;              /* [n_nodes, 3] */
    float* exp_avg_rot;
    float* exp_avg_trn;
    float* exp_avg_sq_rot;
    float* exp_avg_sq_trn;
    int32_t* step;                    /* [P] */
} dr_nicp_state;
int dr_nicp_node_capacity(void);
size_t dr_ed_graph_workspace_bytes(int n_nodes, int max_nodes);
int dr_ed_graph_f32(int P, int n_points, int n_nodes, int max_nodes, int K, const float* points, const int32_t* p_offsets, const float* nodes,
                    const int32_t* m_offsets, double node_coverage, double eps, int64_t* anchor_indices, float* anchor_weights,
                    float* anchor_distances, int32_t* edge_counts, const int32_t* e_offsets, long long edge_cap, int64_t* edge_indices,
                    float* edge_weights, float* edge_distances, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int dr_ed_warp_f32(int P, int n_points, int n_nodes, int K, const float* points, const int32_t* p_offsets, const float* nodes,
                   const int32_t* m_offsets, const float* transforms, const int64_t* anchor_indices, const float* anchor_weights, double eps,
                   float* out, int32_t* status, void* stream);
size_t dr_nicp_workspace_bytes(int P, int n_corr, int n_nodes, int n_edges, int K);
int dr_nicp_cost_grad_f32(const dr_nicp_problem* problem, const float* rotations, const float* translations, double w_landmark, double w_arap,
                          double w_ortho, float* cost, float* grad_rot, float* grad_trn, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);
int dr_nicp_adam_f32(const dr_nicp_problem* problem, const dr_nicp_options* options, const dr_nicp_state* state, int resume,
                     float* transforms, float* cost, float* trace, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, fifteenth set (detected by symbol like the fourth to fourteenth sets): the 3D / 4D dataset item, what
 * _3DMatch.__getitem__ (3D/datasets/_3dmatch.py:55-135) and _4DMatch.__getitem__ (3D/datasets/_4dmatch.py:58-146) compute behind their file
 * reads.  csrc/item3d.hip, indices in csrc/item3d_index.h; DESIGN 5y.
 *
 * Both entries are ragged over P pairs: pair p's rows of a stacked array are [offsets[p], offsets[p + 1]) of an int32 DEVICE array of P + 1
 * entries.  They are asynchronous on `stream` (a hipStream_t), allocate nothing, read nothing back to the host and use no floating-point atomic
 * (the status words take integer ORs): two runs are bit-equal and both can be captured on one stream.  status [P] int32 receives per pair 0 or a
 * sum of: 2, the pair's offsets are not 0 <= lo <= hi <= total (the pair is neither read nor written); 4, a selection index outside the pair's
 * raw cloud was met (its output row is zero); 8, the flow is recomputed but the pair's selected and raw source counts differ.  P = 0 is a no-op;
 * Rows of a stacked array that lie in no pair's slice (in front of offsets[0], behind offsets[P], or in a pair with status bit 2) are allowed:
 * dr_item3d_prepare_f32 writes such output rows as zero, dr_radius_pairs_ragged_f32 pairs them with nothing.
 * a negative size or a NULL pointer that a non-empty array needs is DR_EINVAL, P > 256 (every thread scans the offsets: P is a batch size) or more than 2^28 stacked rows DR_ENOSUP, a missing or
 * short workspace DR_EWORKSPACE (16-byte aligned, else DR_EINVAL): all reported before the first launch.
 *
 * dr_item3d_prepare_f32: per pair, in the reference's order --
 *   subsample (_3dmatch.py:71-76, _4dmatch.py:86-91): output row i of a side is raw row src_sel[i] / tgt_sel[i] (PAIR-LOCAL int64, stacked like
 *     the outputs: the first max_points entries of a permutation); a NULL selection is the identity and needs n_src == n_src_raw;
 *   rotate (_3dmatch.py:95-103): rot_ab [P, 3, 3] float64 (Rotation.from_euler('zyx', .)) turns the source when coin[p] > 0.5, else the target:
 *     cloud' = rot_ab cloud; rot' = rot rot_ab^T (source) or rot' = rot_ab rot, trans' = rot_ab trans (target).  NULL: no rotation;
 *   jitter (_3dmatch.py:105-106): cloud' += (u - 0.5) noise with u = src_jitter [n_src, 3] / tgt_jitter [n_tgt, 3] float64 draws in [0, 1);
 *     NULL: no jitter;
 *   flow (_4dmatch.py:77, 115, 124; flow_raw != NULL and recompute_flow != 0): flow' = rot_ab (src + flow) - src', the deformed copy built in
 *     float32 from the loaded arrays, turned with the source when the source is turned, and NOT jittered, minus the jittered source.
 *   The reference computes a turned cloud in float64 (numpy promotes through rot_ab) and adds the jitter to an unturned float32 cloud in place;
 *   the collate casts to float32.  So every output is evaluated in double on the float32 inputs and rounded once; a row that is neither turned
 *   nor jittered is copied.  rot / trans [P, 3, 3] / [P, 3] are float64 inputs; rot_out / trans_out float32; tsfm_out [P, 3, 4] float32 = (rot' |
 *   trans'), the `transforms` of dr_radius_pairs_ragged_f32 (to_tsfm, _3dmatch.py:109).
 *   The 4DMatch subsample indexes src_pcd ONLY: src_pcd_deformed and s2t_flow keep their loaded row count (_4dmatch.py:77, 86-88).  flow_out is
 *   therefore [n_src_raw, 3], stacked by s_raw_offsets: with recompute_flow == 0 it is flow_raw unchanged -- UNSELECTED, whatever src_sel says,
 *   as the reference returns it -- and with recompute_flow != 0 row i of the deformed copy meets row i of the selected source.  The reference
 *   raises there when the selection is shorter than the cloud (`src_pcd_deformed - src_pcd`, shapes differ): flow_raw with recompute_flow and
 *   n_src != n_src_raw is DR_EINVAL (per pair: status bit 8). */
typedef struct dr_item3d_args {
    int P, n_src_raw, n_tgt_raw, n_src, n_tgt;
    const float* src_raw;             /* [n_src_raw, 3] */
    const int32_t* s_raw_offsets;
    const float* tgt_raw;             /* [n_tgt_raw, 3] */
    const int32_t* t_raw_offsets;
    const float* flow_raw;            /* [n_src_raw, 3] or NULL */
    const int64_t* src_sel;           /* [n_src] or NULL */
    const int64_t* tgt_sel;           /* [n_tgt] or NULL */
    const int32_t* s_offsets;         /* [P + 1] rows of the outputs */
    const int32_t* t_offsets;
    const double* rot_ab;             /* [P, 3, 3] or NULL */
    const double* coin;               /* [P]; required with rot_ab */
    const double* src_jitter;         /* [n_src, 3] or NULL */
    const double* tgt_jitter;         /* [n_tgt, 3] or NULL */
    double noise;                     /* augment_noise */
    int recompute_flow;               /* data_augmentation of _4dmatch.py:109 */
    const double* rot;                /* [P, 3, 3] */
    const double* trans;              /* [P, 3] */
    float* src_out;                   /* [n_src, 3] */
    float* tgt_out;                   /* [n_tgt, 3] */
    float* flow_out;                  /* [n_src_raw, 3]; required with flow_raw */
    float* rot_out;                   /* [P, 3, 3] */
    float* trans_out;                 /* [P, 3] */
    float* tsfm_out;                  /* [P, 3, 4] */
    int32_t* status;                  /* [P] */
} dr_item3d_args;
int dr_item3d_prepare_f32(const dr_item3d_args* args, void* stream);

/* dr_radius_pairs_ragged_f32: get_correspondences / KDTree_corr (3D/lib/benchmark_utils.py:166-185, K = None) for P pairs at once: per pair all
 *   (i, j), PAIR-LOCAL, with |T_p src_i - tgt_j| < radius, in ascending (i, j) (Open3D's search_radius_vector_3d returns a row's partners in
 *   ascending distance).  The float32 expressions are dr_radius_pairs_f32's: q = x T0 + y T1 + z T2 + T3 per row of transforms [P, 3, 4] (NULL:
 *   identity), d^2 = dx dx + dy dy + dz dz, d^2 < radius^2.  The targets are sorted by (pair, cell of edge radius (1 + 2^-7) counted from the
 *   pair's min corner) and a row sweeps its 27 cells, so the work follows the number of close points, not ns x nt; a row may have any number of
 *   partners.  Cell coordinates are clamped to [0, 65535]: a source outside the target's grid, or a cloud wider than 65536 cells, only tests more
 *   candidates.  Pair p's list goes to rows [c_offsets[p], min(c_offsets[p + 1], capacity)) of out_src / out_tgt [capacity] (c_offsets: int64
 *   DEVICE array of P + 1 entries); counts [P, 2] int32 = (written, found), found exact and saturated at 2^31 - 1, written = min(found, room);
 *   nothing is written behind a pair's room, and the entries kept are the first in (i, j) order.  capacity == 0 (c_offsets and the outputs may be
 *   NULL) counts only.  radius > 0.  Workspace: dr_radius_pairs_ragged_workspace_bytes(P, ns, nt); the size query and the entry share one carve. */
size_t dr_radius_pairs_ragged_workspace_bytes(int P, int ns, int nt);
int dr_radius_pairs_ragged_f32(int P, int ns, int nt, const float* src, const int32_t* s_offsets, const float* tgt, const int32_t* t_offsets,
                               const float* transforms, float radius, const int64_t* c_offsets, long long capacity, int64_t* out_src,
                               int64_t* out_tgt, int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, sixteenth set (detected by symbol like the fourth to fifteenth sets): Gauss-Newton non-rigid ICP on the embedded
 * deformation graph of the fourteenth set, the solver vision3d wraps as the layer NonRigidICP.  2D-3D vision3d/layers/nonrigid_icp.py:18-154,
 * vision3d/ops/so3.py:107-133 and :389-406, vision3d/ops/numeric.py:7-9.  csrc/nonrigid_gn.hip, indices in csrc/nonrigid_gn_index.h; DESIGN 5z.
 *
 * The entries keep the fourteenth set's conventions: dr_nicp_problem (with edge_weights == NULL allowed here: weight 1, :60-61), ragged over P
 * pairs through int32 DEVICE offset arrays, PAIR-LOCAL int64 node indices, asynchronous on `stream`, nothing allocated, nothing read back, no
 * floating-point atomic: two runs are bit-equal and every entry can be captured on one stream (the launch sequence depends only on
 * problem->max_nodes / n_max and num_iterations).  status [P] int32 receives per pair 0 or a sum of: 1, more nodes than max_nodes; 2, the
 * pair's offsets are not 0 <= lo <= hi <= total (a pair with bit 1 or 2 is neither read nor computed, its output rows are not written); 4, an
 * anchor outside [-1, M) or an edge endpoint outside [0, M) was met and treated as absent; 32, a pivot of the factorisation was not finite or not
 * > 0 (possible with lm_lambda <= 0 and a node that no row constrains).  P = 0 is a no-op; a negative size, a K out of 1 .. 8, max_nodes > 1024,
 * or a NULL pointer that a non-empty array needs is DR_EINVAL, a product of sizes beyond 2^31 - 1 or P > 65535 DR_ENOSUP, a missing or short
 * workspace DR_EWORKSPACE (16-byte aligned, else DR_EINVAL): all reported before the first launch, with every output untouched.
 *
 * The unknowns of a pair of M nodes are ordered as the reference's permute(1, 3, 0, 2, 4) orders its Jacobian's columns (:105): axis-angle
 * increments first (3 n + d), then translation increments (3 M + 3 n + d).  One iteration (:93-150), at rotations R_n and translations t_n:
 *   correspondence rows (:98-112): residual corr_lambda (warp(p_c) - q_c), warp = dr_ed_warp_f32's apply_deformation with its sum + 1e-6
 *     normalisation; blocks -corr_lambda w [R_n (p_c - g_n)]x (rotation) and corr_lambda w I (translation) for the columns with anchor != -1
 *     and anchor weight > 0 (:71), w = the RAW anchor weight, times sqrt(corr_weights[c]) when corr_weights is given (:79) -- which enters the
 *     blocks only, never the residual, as in the reference.  A row that names one node in two such columns keeps the LATER column's block (the
 *     reference's indexed assignment keeps one write, unspecified on a GPU).
 *   ARAP rows (:117-137; none when arap_lambda <= 0): per edge (u, v), u != v (self edges dropped :54; (u, v) and (v, u) are two rows),
 *     s = arap_lambda sqrt(edge_weight): residual s (R_u (g_v - g_u) + t_u + g_u - g_v - t_v); blocks -s [R_u (g_v - g_u)]x and s I at u,
 *     -s I at v's translation.
 *   solve (:140-144): A = J^T J + lm_lambda I, b = -J^T r, A x = b.  J is never built: the workgroup of node n gathers n's 6 x 6 blocks against
 *     each partner node through the node-major lists of the fourteenth set's set-up pass (the same device code) in float64, in list order, and
 *     writes row block n of the dense A [6 M, 6 M] in the workspace (both triangles).  A is factored by a blocked right-looking Cholesky
 *     (64-wide blocks) and solved by forward and back substitution, all float64.
 *   update (:146-150): R_n <- exp(phi_n) R_n by Rodrigues' formula with omega = phi / max(|phi|, 1e-6) (so a zero increment is the identity),
 *     t_n <- t_n + dt_n, in float64 on the float32 state, rounded once.
 *
 * dr_nicp_gn_f32: options->num_iterations iterations.  state: NULL, or the fourteenth set's struct of DEVICE pointers, of which only rotations
 *   and translations are used (each may be NULL): non-NULL members are the state the iterations work on and hold the final state; with
 *   resume != 0 the run starts from them (both required), otherwise from identity rotations and zero translations.  transforms [n_nodes, 4, 4]
 *   is written on every call; num_iterations == 0 returns the starting state.  A pair that gets status bit 32 stops there: its state stays as it
 *   was before the failing iteration, its transforms are written from that state, nothing non-finite is written, and the other pairs are not
 *   affected.  max_nodes <= 1024: the capacity is bounded by the workspace, P (6 max_nodes)^2 doubles dominate it (75 MB per pair at 512).
 * dr_nicp_gn_normal_f32: A [P, 6 max_nodes, 6 max_nodes] and b [P, 6 max_nodes] float64 (row-major, pair p's system in the leading 6 M_p
 *   rows / columns of its slot, the rest zero) of ONE iteration at the given rotations [n_nodes, 3, 3] / translations [n_nodes, 3], lm_lambda
 *   added; num_iterations is ignored.
 *   Workspace of both: dr_nicp_gn_workspace_bytes(P, n_corr, n_nodes, n_edges, K, max_nodes); the size query and the entries share one carve.
 * dr_spd_solve_f64: P symmetric positive definite systems in one call, torch.linalg.solve's role at :144.  System p is the leading n[p] x n[p]
 *   corner of slot p of A [P, n_max, n_max] (row-major; only the LOWER triangle is read) and the first n[p] entries of bx [P, n_max]; n is an
 *   int32 DEVICE array.  The lower triangle receives the Cholesky factor L (A = L L^T), bx the solution; the strict upper triangle and
 *   everything outside the leading corner are neither read nor written.  0 <= n_max <= 6144.  status [P]: 0; 2, n[p] outside [0, n_max]
 *   (nothing is touched); 32, a pivot was not finite or not > 0 (the slot's lower triangle is partly overwritten, bx is untouched).  No
 *   workspace. */
typedef struct dr_nicp_gn_options {
    int num_iterations;                                   /* 5 */
    double corr_lambda, arap_lambda, lm_lambda;           /* 1.0, 0.1, 0.1 (the function); 1.0, 1.0, 0.01 (the layer) */
} dr_nicp_gn_options;
size_t dr_nicp_gn_workspace_bytes(int P, int n_corr, int n_nodes, int n_edges, int K, int max_nodes);
int dr_nicp_gn_f32(const dr_nicp_problem* problem, const dr_nicp_gn_options* options, const float* corr_weights, const dr_nicp_state* state,
                   int resume, float* transforms, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int dr_nicp_gn_normal_f32(const dr_nicp_problem* problem, const dr_nicp_gn_options* options, const float* corr_weights, const float* rotations,
                          const float* translations, double* A, double* b, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream);
int dr_spd_solve_f64(int P, int n_max, const int32_t* n, double* A, double* bx, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, seventeenth set (detected by symbol like the fourth to sixteenth sets): furthest-point sampling, where the nodes of
 * the fourteenth set's deformation graph come from in the reference.  2D-3D vision3d/csrc/cpu/node_sampling/node_sampling.cpp:10-78 and its
 * numpy restatement vision3d/array_ops/furthest_point_sample.py:22-66 (node form); vision3d/csrc/cuda/furthest_point_sample/
 * furthest_point_sample_cuda.cuh:29-88 behind vision3d/ops/furthest_point_sample.py:12-49 (batch form).  csrc/fps.hip, indices in
 * csrc/fps_index.h; DESIGN 5za.
 *
 * Conventions of the fourteenth set: ragged over P clouds through an int32 DEVICE array of P + 1 offsets (node form), asynchronous on `stream`
 * (a hipStream_t), nothing allocated, nothing read back, NO atomic of any kind: two runs are bit-equal and both entries can be captured on one
 * stream.  One workgroup owns one cloud for all its iterations and clouds run side by side; no workgroup waits for another.  A cloud of at most
 * dr_fps_onchip_capacity() points keeps its coordinates and running distances in registers; a larger one takes the streaming instantiation of
 * the same kernel (running distances in the workspace, coordinates re-read each iteration), whose result is the same entry for entry.  P = 0 is
 * a no-op; a negative size, max_points > n_points, sample_cap < 1 or a NULL pointer that a non-empty array needs is DR_EINVAL, more than
 * 65 535 clouds or 2^31 / 3 stacked points DR_ENOSUP, a missing or short workspace DR_EWORKSPACE (16-byte aligned, else DR_EINVAL): all reported
 * before the first launch, with every output untouched.
 *
 * Arithmetic: float32, operation by operation in the reference's order, never contracted into an FMA.  Every selection takes the candidate with
 * the largest running distance; among EQUAL distances the LOWEST index wins, whatever lane, wave or instantiation holds it.  (Stated
 * difference: the reference resolves a tie by the scan order of its swap-popped candidate array (C++), of its shrinking list (numpy), or by
 * thread stride and tree order (CUDA).  The fixture is screened so that no selection of it is a tie.)  A point with a NaN or Inf coordinate
 * is never selected and never enters the stop test: its distance key is -inf.
 *
 * dr_fps_nodes_f32: the node form.  d = sqrtf((dx dx + dy dy) + dz dz) with sq_norm's order (cloud.h:46) and a correctly rounded square root;
 *   the running minimum starts at +inf; node 0 is point 0; each further node is the candidate with the largest running minimum that is
 *   strictly > 0; the loop stops when num_samples > 0 nodes are taken (tested BEFORE the scan, node_sampling.cpp:44), when that maximum is
 *   < min_distance (:67), or when no candidate is left -- every remaining running minimum is 0: the cloud is used up, e.g. num_samples >= the
 *   number of distinct points (the reference indexes out of range there when min_distance <= 0).  min_distance <= 0 (or NaN) together with
 *   num_samples <= 0 is therefore DR_EINVAL: neither rule could stop the reference.  "None" of the reference is min_distance = -1 /
 *   num_samples = -1 (array_ops/furthest_point_sample.py:14-17).  The reference drops a point closer than min_distance to a node from its
 *   candidate list (:60-61); such a point could win only a selection at which the loop stops, so this changes nothing but the reference's tie
 *   order, and the device keeps no list.
 *   max_points: an upper bound of every cloud's point count known to the HOST; it decides whether the streaming instantiation is launched.
 *   out_indices [P, sample_cap] int64, CLOUD-LOCAL, -1 beyond the count; out_points (or NULL) [P, sample_cap, 3] = the nodes' coordinates, bit
 *   for bit, 0 beyond the count; out_distances (or NULL) [P, sample_cap] = the running-minimum distance at which node k was taken (0 for node
 *   0; non-increasing in k), 0 beyond the count: one sampling can be cut at any coarser min_distance without running again.  out_counts [P].
 *   status [P] int32 receives per cloud 0 or a sum of: 1, the cloud has more points than max_points; 2, its offsets are not 0 <= lo <= hi <=
 *   n_points (with 1 or 2 nothing is read, the count is 0 and the row is -1 / 0); 8, a point with a NaN or Inf coordinate was met and left out;
 *   64, sample_cap nodes were taken and the next candidate did not meet the stop rule (the loop was cut by sample_cap, not by num_samples or
 *   min_distance); 128, point 0 is not finite: the cloud yields 0 nodes.  An empty cloud yields count 0 and status 0.
 *   Workspace: dr_fps_workspace_bytes(P, n_points, max_points): 0 when max_points <= dr_fps_onchip_capacity(), else one float per stacked point.
 * dr_fps_batch_f32: the batch form on points [B, N, 3].  d = (dx dx + dy dy) + dz dz (.cuh:64); the running minimum starts at 1e10
 *   (ops/furthest_point_sample.py:34); index 0 first, then num_samples - 1 times the candidate with the largest running minimum strictly > -1
 *   (:55-70), and index 0 when there is none; there is no stop and no status.  num_samples > N repeats indices as the reference's kernel does:
 *   once every running minimum is 0 the lowest index wins each time.  A non-finite point 0 is still index 0 (it updates no distance).
 *   out_indices [B, num_samples] int64.  N == 0 with num_samples > 0 is DR_EINVAL (the reference reads point 0).  Workspace:
 *   dr_fps_workspace_bytes(B, B N, N). */
int dr_fps_onchip_capacity(void);
size_t dr_fps_workspace_bytes(int P, int n_points, int max_points);
int dr_fps_nodes_f32(int P, int n_points, int max_points, const float* points, const int32_t* p_offsets, float min_distance, int num_samples,
                     int sample_cap, int64_t* out_indices, float* out_points, float* out_distances, int32_t* out_counts, int32_t* status,
                     void* workspace, size_t workspace_bytes, void* stream);
int dr_fps_batch_f32(int B, int N, int num_samples, const float* points, int64_t* out_indices, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, eighteenth set (detected by symbol like the fourth to seventeenth sets): the geodesic deformation graph of a point
 * cloud, the reference's second graph builder.  2D-3D vision3d/csrc/cpu/deformation_graph/deformation_graph.cpp:13-180 behind
 * vision3d/array_ops/deformation.py:443-490.  csrc/geo_graph.hip, indices in csrc/geo_graph_index.h; DESIGN 5zb.
 *
 * Conventions of the fourteenth set: ragged over P clouds through int32 DEVICE arrays of P + 1 offsets (p_offsets: points, n_offsets: nodes),
 * asynchronous on `stream` (a hipStream_t), nothing allocated, nothing read back, no floating-point atomic and no atomic that decides an order:
 * two runs are bit-equal and both entries can be captured in a graph (dr_init sets the relaxation's LDS attribute, outside any capture).
 * node_indices [n_nodes] int64 are CLOUD-LOCAL point indices, as dr_fps_nodes_f32 returns them; the node numbers in the outputs are
 * cloud-local too.  P = 0 is a no-op; a negative size, max_points > n_points, max_nodes > n_nodes, num_neighbors or num_anchors outside
 * 1 .. 8, max_degree < 1, a max_distance or node_coverage that is not finite and > 0, or a NULL pointer that a non-empty array needs is
 * DR_EINVAL; more than 65 535 clouds, 2^31 / 3 stacked points, max_nodes > 2 048 or max_degree > 1 024 DR_ENOSUP; a missing or short workspace
 * DR_EWORKSPACE (16-byte aligned, else DR_EINVAL): all reported before the first launch, with every output untouched.
 *
 * dr_geo_graph_f32 computes, for every cloud, exactly this:
 *   Edges: points i != k are joined iff d(i, k) < max_distance, d = sqrtf((dx dx + dy dy) + dz dz) in float32, operation by operation, never
 *     contracted (cloud.h:46, .cpp:62).  (The reference's voxel hash only finds these pairs.)  A point with a NaN or Inf coordinate has no edge.
 *   Path length: g_i(x) = the smallest left-to-right float32 sum of edge lengths over the paths from node i's point to x; x is reached iff
 *     g_i(x) <= 2.0 * node_coverage, compared in double (.cpp:137); the node's own point is reached at 0.  The device relaxes
 *     g(y) = min(g(y), fl(g(x) + d(x, y))) to its least fixed point, which is the reference's Dijkstra result bit for bit.
 *   neighbor_* [n_nodes, num_neighbors]: of the NODES node i reaches, the first num_neighbors by (g ascending, point index DESCENDING) -- the
 *     pop order of the reference's max-heap of (-g, point); the node itself comes first.  Rows are padded with -1 / 0 / 0.
 *   anchor_* [n_points, num_anchors]: of the nodes that reach point x, the first num_anchors by (g ascending, node index ascending) (.cpp:151);
 *     padded with -1 / 0 / 0; an unreached point has a whole row of padding.
 *   Weights: exp(-(g g) / (2. c c)) with g g in float32 and the rest in double, rounded once (.cpp:9-11).  Anchor weights are then divided by
 *     their float32 sum taken in list order; a sum of 0 gives each 1 / count (.cpp:163-176).  Neighbour weights are not normalised.
 *   Parity with the reference is claimed where no comparison above is a tie or within rounding of its bound (the fixture is screened so).
 *   max_points / max_nodes: upper bounds of every cloud's point / node count known to the HOST.  options->max_degree: the slots of a point's
 *   adjacency row in the workspace; options->onchip_cap_override: 0, or a smaller on-chip capacity than dr_geo_graph_onchip_capacity() (a
 *   test drives the streamed form with it).  A cloud of at most that many points keeps its distances in LDS; a larger one relaxes in the
 *   workspace, with the same result entry for entry.
 *   status [P] int32 receives per cloud 0 or a sum of: 1, more points than max_points or more nodes than max_nodes; 2, the offsets up to this
 *   cloud do not ascend inside [0, total] (nothing of the cloud is written: its rows stay as the caller left them); 4, a node index outside
 *   [0, n) was treated as an absent node (it reaches nothing and nobody's neighbour); 8, a point with a NaN or Inf coordinate was met; 256,
 *   two nodes name one point (the cloud's results are then only guaranteed to be in range); 512, a point has more than max_degree points
 *   closer than max_distance.  A cloud with bit 1 or 512 gets rows of padding only: nothing is cut silently.
 *   Workspace: dr_geo_graph_workspace_bytes(P, n_points, n_nodes, max_points, max_degree): 8 (1 + max_degree) bytes per point and
 *   4 max_points bytes per node (the reach table the anchors are read from).
 * dr_geo_graph_onchip_capacity: the largest cloud whose distances stay in LDS.
 * dr_geo_graph_edges: the neighbour table as dr_nicp_problem's edge list: edge (i, j) for every neighbour 0 <= j < M, j != i of node i, in
 *   row-major order, with the neighbour's weight.  TWO calls, as dr_ed_graph_f32: with e_offsets == NULL it writes edge_counts [P]; with
 *   e_offsets [P + 1] it writes cloud p's edges from row e_offsets[p]; rows at or behind min(e_offsets[p + 1], edge_cap) are not written.
 *   edge_weights may be NULL.  n_nodes * num_neighbors is an upper bound of the total, so a caller that must not read back can size by it. */
typedef struct dr_geo_graph_options {
    int num_neighbors, num_anchors;                       /* Kn, Ka: 1 .. 8 */
    float max_distance, node_coverage;
    int max_degree;                                       /* slots of a point's adjacency row */
    int onchip_cap_override;                              /* 0 = the default capacity */
} dr_geo_graph_options;
int dr_geo_graph_onchip_capacity(void);
size_t dr_geo_graph_workspace_bytes(int P, int n_points, int n_nodes, int max_points, int max_degree);
int dr_geo_graph_f32(int P, int n_points, int n_nodes, int max_points, int max_nodes, const float* points, const int32_t* p_offsets,
                     const int64_t* node_indices, const int32_t* n_offsets, const dr_geo_graph_options* options, int64_t* neighbor_indices,
                     float* neighbor_distances, float* neighbor_weights, int64_t* anchor_indices, float* anchor_distances, float* anchor_weights,
                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int dr_geo_graph_edges(int P, int n_nodes, int num_neighbors, const int64_t* neighbor_indices, const float* neighbor_weights,
                       const int32_t* n_offsets, int32_t* edge_counts, const int32_t* e_offsets, long long edge_cap, int64_t* edge_indices,
                       float* edge_weights, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, nineteenth set (detected by symbol like the fourth to eighteenth sets): what measures the output of the non-rigid
 * chain.  2D-3D vision3d/ops/knn.py:10-107 (knn over keops_knn), vision3d/ops/knn_interpolate.py:10-40 (its k = 3 consumer) and the six
 * non-rigid metrics of vision3d/ops/metrics.py:258-372.  csrc/knn_points.hip, indices in csrc/knn_index.h; DESIGN 5zc.
 *
 * Conventions of the fourteenth set: ragged over P pairs through int32 DEVICE arrays of P + 1 offsets, asynchronous on `stream` (a
 * hipStream_t), nothing allocated, nothing read back, NO atomic of any kind: two runs are bit-equal and every entry can be captured.  Each
 * offset array may be given a second time as a HOST mirror (host_*_offsets, or NULL): a mirror that does not start at >= 0, ascend and end at
 * <= the row count is DR_EINVAL before any launch.  The device arrays are checked by the kernels: a pair whose offsets do not describe slices
 * sets status bit 4 and is skipped (its rows are not written; its sums are 0).  P = 0 is a no-op; a negative size, k outside
 * 1 .. dr_knn_points_max_k() or a NULL pointer that a non-empty array needs is DR_EINVAL, more than 65 535 pairs or 2^31 / 3 stacked rows
 * DR_ENOSUP, a missing or short workspace DR_EWORKSPACE (16-byte aligned, else DR_EINVAL): all reported before the first launch.
 *
 * dr_knn_points_f32: for every query of pair p its k nearest supports of pair p (knn.py:22-27, dij = (xi - xj).norm2(), Kmin_argKmin).
 *   THE RULE: d2 = (dx dx + dy dy) + dz dz in float32, operation by operation, never contracted into an FMA; a row's k slots ascend by
 *   (d2, support index), so among equal d2 the LOWER index comes first, whatever lane, wave or tile met it; out_distances = sqrtf(d2),
 *   correctly rounded.  KeOps' own tie order is not claimed.  (Ordering by (distance, index) differs only where two distinct d2 round to one
 *   sqrtf; the fixture's screen excludes that.)  out_distances [n_queries, k] float32 and out_indices [n_queries, k] int64 (PAIR-LOCAL support
 *   rows); either may be NULL.  Slots that cannot be filled -- fewer than k supports, an empty support cloud -- hold +inf and -1 (stated
 *   difference: the reference returns min(k, S) columns, knn.py:75).  A support with a NaN or Inf coordinate, and one whose d2 overflows
 *   float32, is never selected.  A query with a NaN or Inf coordinate gets an all +inf / -1 row and sets status bit 8 (the bit's meaning
 *   in the fourteenth set).  status [P] int32: 0 or a sum of 4 and 8.  No workspace.
 *   dr_knn_points_max_k() = 16; dr_knn_points_block() = the queries of one workgroup, dr_knn_points_tile() = the supports of one LDS tile
 *   (exported so that tests can place shapes on both sides of them).
 * dr_nn_stats_f32: the k = 1 search with its reduction fused, no distance array: out [P, 4] double = the number of queries that have a
 *   nearest support (a query without a finite support, and a non-finite query, is not counted and contributes nothing), sum dist,
 *   sum dist^2 (dist promoted to double, then squared), the count of dist < distance_limit (float32 compare).  compute_chamfer_distance
 *   (metrics.py:365-372) is two calls, compute_corr_coverage (:359-362) one.  The order is fixed: the 64 queries of a block by the tree
 *   lane l += lane l + off, off = 32 .. 1; the blocks of a pair in ascending order, in double.  Workspace: dr_nn_stats_workspace_bytes(P,
 *   n_queries).
 * dr_flow_metrics_f32: the per-point predicates of compute_scene_flow_accuracy (:323-337), compute_scene_flow_outlier_ratio (:340-356),
 *   compute_nonrigid_inlier_ratio (:258-284) and the last two lines of compute_nonrigid_feature_matching_recall (:318-319) in one pass over
 *   pred / target [n_points, 3]: with rot [P, 9] / trn [P, 3] (both or neither) pred is first replaced by R pred + t of its pair (the
 *   reference's `transform`); |e| = sqrtf of the float32 d2 above of (pred, target); rel = |e| / (|target| + eps); strict / relaxed =
 *   |e| < abs || rel < rel_thr; outlier = |e| > abs || rel > rel_thr, where a NEGATIVE threshold is the reference's None; within = |e| <
 *   strict_abs alone (the NIR / NFMR predicate).  mask (uint8 [n_points] or NULL): a point with mask 0 is left out of everything.
 *   out [P, 6] double = n, sum |e|, n_strict, n_relaxed, n_outlier, n_within; counts are integers held in double; sums go lanes -> wave
 *   (the tree above) -> the four waves in order -> the blocks of a pair in ascending order.  status [P]: 0 or 4.  Workspace:
 *   dr_flow_metrics_workspace_bytes(P, n_points). */
int dr_knn_points_max_k(void);
int dr_knn_points_tile(void);
int dr_knn_points_block(void);
int dr_knn_points_f32(int P, int n_queries, const float* queries, const int32_t* q_offsets, int n_supports, const float* supports,
                      const int32_t* s_offsets, const int32_t* host_q_offsets, const int32_t* host_s_offsets, int k, float* out_distances,
                      int64_t* out_indices, int32_t* status, void* stream);
size_t dr_nn_stats_workspace_bytes(int P, int n_queries);
int dr_nn_stats_f32(int P, int n_queries, const float* queries, const int32_t* q_offsets, int n_supports, const float* supports,
                    const int32_t* s_offsets, const int32_t* host_q_offsets, const int32_t* host_s_offsets, float distance_limit, double* out,
                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
size_t dr_flow_metrics_workspace_bytes(int P, int n_points);
int dr_flow_metrics_f32(int P, int n_points, const float* pred, const float* target, const int32_t* offsets, const int32_t* host_offsets,
                        const uint8_t* mask, const float* rot, const float* trn, float strict_abs, float strict_rel, float relaxed_abs,
                        float relaxed_rel, float outlier_abs, float outlier_rel, float eps, double* out, int32_t* status, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, twentieth set (detected by symbol like the fourth to nineteenth sets): the rigid counterpart of the non-rigid
 * chain, vision3d's RANSAC-free estimators.  2D-3D vision3d/ops/weighted_procrustes.py:10-71, vision3d/models/geotransformer/
 * local_global_registration.py:104-161, vision3d/ops/spatial_consistency.py:7-54, vision3d/ops/eigenvector.py:21-31 and
 * vision3d/models/geotransformer/spatial_consistency_filtering.py:15-19.  csrc/lgr.hip, indices in csrc/lgr_index.h; DESIGN 5zd.
 *
 * Conventions of the fourteenth set: ragged over P problems (G groups) through int32 DEVICE arrays of P + 1 offsets, asynchronous on `stream`
 * (a hipStream_t), nothing allocated, nothing read back, no floating-point atomic: two runs are bit-equal and every entry can be captured on
 * one stream.  Each offset array may be given a second time as a HOST mirror (host_*_offsets, or NULL): a mirror that does not start at >= 0,
 * ascend and end at <= the row count is DR_EINVAL before any launch.  The device arrays are checked by the kernels: a problem whose offsets
 * do not describe slices sets status bit 4, one that holds a NaN or Inf coordinate, weight or score sets status bit 8; either way the problem
 * is SKIPPED: none of its outputs but the status word is written.  P = 0 is a no-op; a negative size or a NULL pointer that a non-empty
 * array needs is DR_EINVAL, more than 65 535 problems or 2^31 / 3 stacked rows DR_ENOSUP, a missing or short workspace DR_EWORKSPACE
 * (16-byte aligned, else DR_EINVAL; transform arrays are 16-byte aligned as well): all reported before the first launch.
 *
 * dr_weighted_procrustes_f32 (RULE 1): for group g, rows [offsets[g], offsets[g + 1]) of src / tgt [n, 3] and weights [n] (NULL: ones):
 *   w = (w < weight_threshold) ? 0 : w;  W = sum w;  pc = (sum w p) / (W + eps), qc = (sum w q) / (W + eps);
 *   H = sum (w / (W + eps)) (p - pc)(q - qc)^T;  H = U S V^T by the library's double one-sided Jacobi (svd3_jacobi);
 *   R = V diag(1, 1, sign det(V U^T)) U^T;  t = qc - R pc.  Every sum runs in double on the float32 inputs in ONE order: element i belongs
 *   to slot (i / 64 % 4, i % 64); a slot adds its elements ascending, the 64 slots of a virtual wave meet in the tree lane l += lane l + off
 *   (off = 32 .. 1), the four virtual waves are added ascending.  R and t are rounded once to float32: transforms [G, 16], row-major 4 x 4.
 *   A group of at most wave_limit rows is fitted by one wave, a longer one by a workgroup (wave_limit < 0: dr_lgr_wave_limit(); 0 sends
 *   every group to the workgroup path, INT_MAX every group to the wave path): the two paths add the same doubles in the same order and are
 *   bit-equal.  A group with no positive weight, or an all-zero H, has R = identity and status bit 16 (torch.svd of a zero matrix gives
 *   U = V = identity as well); t follows the rule (0 when W = 0).  A group of one or two rows has a rank-1 H (eps keeps it from zero): R is
 *   a proper rotation that maps the fitted direction, its turn about that direction is the Jacobi SVD's completion of the basis, not
 *   LAPACK's.  status [G]: 0, 4, 8 or 16.  No workspace.
 * dr_lgr_f32: local_to_global_registration for P problems in one call, five launches whatever P.  Per problem its correspondences in
 *   torch.nonzero order -- src_points / tgt_points [n_corr, 3], scores [n_corr], patch_ids [n_corr] int32, NON-DESCENDING inside a problem
 *   (a violation sets status bit 4) -- and its verification set v_* under offsets of its own (the same arrays, or the caller's top
 *   max_global_correspondences).  (a) chunks = the runs of equal patch id of at least min_local_correspondences rows, found by a count pass
 *   and a scan; (b) one fit per chunk by rule 1 with the scores as weights; (c) per chunk the INTEGER count of verification correspondences
 *   inside acceptance_radius, one wave per hypothesis; the best chunk has the largest count, the LOWEST chunk index among equals;
 *   (d), (e) num_refinement_steps times: cur = v_scores * inlier(current transform), then a fit by rule 1 on the verification set with cur;
 *   the first round's transform is the best chunk's.  A problem without a chunk first fits the whole verification set with v_scores (the
 *   reference's degenerate branch, :147-151).  All rounds of a problem run in one launch by one workgroup.
 *   THE RESIDUAL RULE: with the transform already rounded to float32, x' = ((R00 x + R01 y) + R02 z) + t0 and likewise y', z', in float32,
 *   never contracted; d2 = (dx dx + dy dy) + dz dz of (tgt - x'); inlier iff sqrtf(d2) < acceptance_radius, a float32 compare.
 *   Outputs: transform [P, 16]; optional best_chunk [P] (-1 in the degenerate branch), final_scores [n_verify] (the cur of the last fit),
 *   chunk_transforms [n_corr, 16] / chunk_counts [n_corr] (hypothesis chunk_offsets[p] + j is chunk j of problem p; capacity n_corr rows) and
 *   chunk_offsets [P + 1]; status [P]: bit 32 = a problem with no correspondence (transform = identity; the reference raises), bit 16 = the
 *   last fit was degenerate.  Workspace: dr_lgr_workspace_bytes(P, n_corr).  1 <= num_refinement_steps <= 64, min_local >= 1.
 * dr_spatial_consistency_f32: the dense [Nq_p, Ns_p] matrix of problem p at element mat_offsets[p] of out (int64 DEVICE offsets, P + 1).
 *   RULE, float32, never contracted: d = sqrtf(d2) of the two source points and of the two target points, d2 = (dx dx + dy dy) + dz dz;
 *   delta = |ds - dt|; sc = max(1 - (delta * delta) / (sigma * sigma), 0).  Stated difference: the reference's pairwise_distance expands
 *   |x|^2 - 2xy + |y|^2 and clamps; this entry takes the difference first.  status [P]: 0, 4 or 8.  No workspace.
 * dr_sc_row_sums_f32: out[i] = sum_j sc(i, j) * multiplier[j] (NULL: 1) over the supports of query i's problem, without the matrix.  A
 *   workgroup owns dr_sc_block() queries, a lane one query; the supports pass through LDS in tiles of dr_sc_tile(); the sum runs in double,
 *   supports ascending, and is rounded once to float32.  out [n_queries].  No workspace.
 * dr_sc_leading_eigenvector_f32: power iteration on the spatial-consistency matrix of src_points / tgt_points [n, 3] (matrix-free), or, with
 *   mat != NULL (points NULL), on the caller's dense [N_p, N_p] matrices at mat_offsets.  v0 = 1; per iteration y = float32(M v) (double
 *   sums; dense form: lane l adds columns l, l + 64, ... ascending, then the tree), v = y / max(float32(sqrt(sum y^2 in double, rule 1's
 *   order)), 1e-12); the problem stops when |v - v_last| <= 1e-8 + 1e-5 |v_last| holds for every entry in float32 -- a DEVICE flag: the
 *   remaining iterations leave that problem's vector untouched.  out [n]; iterations [P] = the iterations that ran.  Two launches per
 *   iteration and one before the first.  Workspace: dr_sc_leading_eigenvector_workspace_bytes(P, n). */
int dr_lgr_wave_limit(void);
int dr_sc_block(void);
int dr_sc_tile(void);
int dr_weighted_procrustes_f32(int G, int n, const float* src, const float* tgt, const float* weights, const int32_t* offsets,
                               const int32_t* host_offsets, float weight_threshold, float eps, int wave_limit, float* transforms,
                               int32_t* status, void* stream);
size_t dr_lgr_workspace_bytes(int P, int n_corr);
int dr_lgr_f32(int P, int n_corr, const float* src_points, const float* tgt_points, const float* scores, const int32_t* patch_ids,
               const int32_t* corr_offsets, int n_verify, const float* v_src_points, const float* v_tgt_points, const float* v_scores,
               const int32_t* verify_offsets, const int32_t* host_corr_offsets, const int32_t* host_verify_offsets, float acceptance_radius,
               int min_local_correspondences, int num_refinement_steps, float weight_threshold, float eps, float* transform,
               int32_t* best_chunk, float* final_scores, float* chunk_transforms, int32_t* chunk_counts, int32_t* chunk_offsets,
               int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int dr_spatial_consistency_f32(int P, int n_queries, const float* q_src_points, const float* q_tgt_points, const int32_t* q_offsets,
                               int n_supports, const float* s_src_points, const float* s_tgt_points, const int32_t* s_offsets,
                               const int32_t* host_q_offsets, const int32_t* host_s_offsets, float sigma, const int64_t* mat_offsets, float* out,
                               int32_t* status, void* stream);
int dr_sc_row_sums_f32(int P, int n_queries, const float* q_src_points, const float* q_tgt_points, const int32_t* q_offsets, int n_supports,
                       const float* s_src_points, const float* s_tgt_points, const int32_t* s_offsets, const int32_t* host_q_offsets,
                       const int32_t* host_s_offsets, float sigma, const float* multiplier, float* out, int32_t* status, void* stream);
size_t dr_sc_leading_eigenvector_workspace_bytes(int P, int n);
int dr_sc_leading_eigenvector_f32(int P, int n, const float* src_points, const float* tgt_points, const int32_t* offsets,
                                  const int32_t* host_offsets, float sigma, const float* mat, const int64_t* mat_offsets, int num_iterations,
                                  float* out, int32_t* iterations, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Added after ABI 0.7.0, twenty-first set (detected by symbol like the fourth to twentieth sets): the refinement every registration user
 * runs after the coarse pose, multi_scale_icp of 2D-3D vision3d/utils/open3d.py:378-396 -- per scale a voxel down-sample of both clouds and
 * Open3D's registration_icp with TransformationEstimationPointToPoint(False).  csrc/icp.hip, indices in csrc/icp_index.h; the down-sample
 * in csrc/collate.hip; DESIGN 5ze.  Open3D is not part of this project's environment: PARITY WITH OPEN3D ITSELF IS NOT CLAIMED.  The
 * published loop is stated below and the kernels are held to that statement (tests/icp_ref.py).
 *
 * Conventions of the fourteenth and twentieth sets: ragged over P pairs through int32 DEVICE arrays of P + 1 offsets with optional HOST
 * mirrors (a mirror that does not start at >= 0, ascend and end at <= the row count is DR_EINVAL), asynchronous on `stream`, nothing
 * allocated, nothing read back, no floating-point atomic: two runs are bit-equal and the call can be captured on one stream.  status [P]:
 * bit 4 = the pair's source or target offsets do not ascend from entry 0 inside [0, rows]; bit 8 = a NaN / Inf coordinate of the pair, or
 * a NaN / Inf in the first three rows of its initial transform.  A pair with bit 4 or 8 is SKIPPED: none of its outputs but the status word
 * is written.  P = 0 is a no-op; a negative size, a NULL pointer that a non-empty array needs, max_correspondence_distance that is not
 * positive and finite, max_iteration outside [0, 4096] or a negative / NaN relative_* is DR_EINVAL; more than 65 535 pairs or 2^31 / 3
 * stacked rows DR_ENOSUP (P is meant to be a BATCH size: the kernels map rows and workgroups to pairs by walking the offsets, O(P)
 * reads per target row, per workgroup of the sweep and per pair of the set-up; the limit is what the 16 pair bits of the grid key hold, not a
 * size at which the call is fast); a missing or short workspace DR_EWORKSPACE (16-byte aligned, else DR_EINVAL; transforms and init_transforms are
 * 16-byte aligned as well): all reported before the first launch.
 *
 * dr_icp_p2p_f32, THE RULE.  With r = max_correspondence_distance and T a float32 [R | t]:
 *   Evaluate(T): every source row of the pair is moved by THE RESIDUAL RULE of dr_lgr_f32, x' = ((R00 x + R01 y) + R02 z) + t0 and
 *     likewise y', z', float32, never contracted; d2 = (dx dx + dy dy) + dz dz of (x' - target).  The partner of a row is the target of its
 *     OWN pair with the smallest (d2, pair-local target index) among those with d2 < r * r (float32 compares; r * r rounded once); none: -1.
 *     n_corr = rows with a partner; fitness = float32(n_corr / n_src) (0 for an empty source); inlier_rmse = float32(sqrt(sum d2 /
 *     n_corr)), the sum of the float32 d2 in double; 0 when n_corr = 0.
 *   Loop: res = Evaluate(init) (init_transforms NULL: identity; only the first three rows are read, the fourth is written as 0 0 0 1).
 *     Then at most max_iteration times: (1) update = the fit of RULE 1 with unit weights and eps = 0 on (moved source, partner) over the
 *     current correspondences -- pc, qc the means, H = (sum p q^T - (sum p)(sum q)^T / n) / n from the moments in double, taken about
 *     the min corner of the pair's targets (a target coordinate that equals the min corner's over all partners then gives an exactly
 *     zero column of H; any other rank-deficient set of partners gives an H that is rank-deficient only up to rounding of the moments, about
 *     1e-16 relative, and is detected only when its second singular value still falls under the 1e-12 below), svd3_jacobi,
 *     R = V diag(1, 1, sign det(V U^T)) U^T, t = qc - R pc; (2) T = update * T, in double on the float32 T, rounded once to float32;
 *     (3) new = Evaluate(T); (4) new becomes the result, and the pair stops when both |res.fitness - new.fitness| < relative_fitness and
 *     |res.rmse - new.rmse| < relative_rmse hold (float32 subtractions and compares).  iterations [P] = the fits that ran.
 *     max_iteration = 0 is evaluation only.  A pair whose evaluation has no correspondence stops there with status bit 32 and keeps its
 *     transform.  A fit whose H has rank <= 1 (second singular value <= 1e-12 of the first: one or two correspondences, collinear
 *     targets) follows rule 1 -- R is the proper rotation with the Jacobi SVD's completion of the basis, not LAPACK's -- and sets status
 *     bit 16; an all-zero H (one correspondence) gives R = identity, t = qc - pc, and bit 16 as well.  The loop goes on after bit 16.
 *   The sums: a workgroup of the sweep owns 64 consecutive source rows of one pair; wave w adds rows w, w + 4, ... of them ascending; the
 *     four waves are added ascending into the workgroup's partial; the finish adds a pair's partials ascending.  The order depends on the
 *     shapes alone.
 *   Outputs: transforms [P, 16] row-major 4 x 4; fitness, inlier_rmse [P] of the last evaluation; iterations [P]; correspondence [ns] or
 *     NULL: per stacked source row the pair-local partner (or -1) of the last evaluation; status [P]: 0 or bits 4, 8, 16, 32.
 *   Launches: 1 (status) + the target grid (origin, key, bitonic sort, gather: cells of edge r (1 + 2^-7), the grid of
 *     dr_radius_pairs_ragged_f32, built once because targets never move) + 2 for the evaluation of init, then 2 per iteration (the sweep and
 *     the finish), whatever P.  A pair that has stopped sets a DEVICE flag: later launches leave it untouched.  No scratch; LDS: 544 bytes
 *     (4 waves x 17 doubles) in the sweep, 136 bytes in the finish.  Workspace: dr_icp_p2p_workspace_bytes(P, ns, nt).
 * dr_grid_subsample_open3d_f32: dr_grid_subsample_vision3d_f32 with the origin of Open3D's PointCloud::VoxelDownSample, origin = min_corner -
 *   0.5 * voxel_size in float32; voxel = floor((p - origin) / voxel_size) per axis; the barycentre as in the other two entries (float32 sum
 *   in input order, times the float reciprocal of the count; Open3D sums in double).  Same arguments, same workspace
 *   (dr_grid_subsample_workspace_bytes).  The output order is this library's voxel-key order, per cloud ascending (iz, iy, ix): Open3D emits
 *   the order of a std::unordered_map, which is unspecified. */
size_t dr_icp_p2p_workspace_bytes(int P, int ns, int nt);
int dr_icp_p2p_f32(int P, int ns, const float* src, const int32_t* s_offsets, int nt, const float* tgt, const int32_t* t_offsets,
                   const int32_t* host_s_offsets, const int32_t* host_t_offsets, const float* init_transforms,
                   float max_correspondence_distance, int max_iteration, float relative_fitness, float relative_rmse, float* transforms,
                   float* fitness, float* inlier_rmse, int32_t* iterations, int32_t* correspondence, int32_t* status, void* workspace,
                   size_t workspace_bytes, void* stream);
int dr_grid_subsample_open3d_f32(int n, int nb, const float* points, const int32_t* lengths, float voxel_size, float* out_points,
                                 int32_t* out_lengths, int32_t* out_total, int32_t* status, void* workspace, size_t workspace_bytes,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFREG_HIP_H */
