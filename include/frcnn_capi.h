/*
 * frcnn_capi.h -- C-ABI of the MI355X-native region-proposal + RoI hot path.
 *
 * This is the drop-in boundary.  Every entry point:
 *   - is extern "C", takes plain pointers / sizes, no torch types;
 *   - takes caller-owned DEVICE buffers (unless a parameter says "host");
 *   - is stream-ordered and asynchronous on `stream` (a hipStream_t, passed
 *     as void*; NULL = the default stream), never synchronises, never
 *     allocates (workspace comes from the caller, sized by the matching
 *     *_workspace_size() query), so a sequence of calls can be captured in a
 *     hipGraph;
 *   - returns 0 on success or a negative FRCNN_E* code, never throws across
 *     the ABI; frcnn_last_error() returns a message for the calling thread.
 *
 * Each function cites the reference interface it replaces (file:line in
 * juniorliu95/replication_faster_rcnn, or the torchvision op the reference
 * calls at that line).  Numerics: see DESIGN.md "Parity contract".
 */
#ifndef FRCNN_CAPI_H_
#define FRCNN_CAPI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_OK 0
#define FRCNN_EINVAL (-1)     /* bad shape / argument */
#define FRCNN_EHIP (-2)       /* HIP runtime error (launch failure) */
#define FRCNN_EWORKSPACE (-3) /* workspace too small */

const char* frcnn_version(void);
const char* frcnn_last_error(void);

/* Runtime helpers (no reference counterpart: the reference runs one image at
 * a time on the host).  CU count of the current device (sizes the grids). */
int frcnn_device_cu_count(int* out);

/* Streams on a CU subset (hipExtStreamCreateWithCUMask: bit i of word i/32 =
 * CU i; words = 0 -> an ordinary non-blocking stream).  The proposal chain is
 * latency bound on a few workgroups while the RoIPool forward holds every CU's
 * LDS for its whole run; giving each its own CUs lets them overlap.  The
 * RoIPool forward sizes its RoI shares to the CUs of the stream it is launched on.
 * frcnn_stream_cu_count: CUs a launch on `stream` may use.
 * frcnn_probe_hw_ids: diagnostic -- out[2b] = HW_ID, out[2b+1] = XCC_ID of
 * workgroup b of an nblocks launch (spin: s_sleep rounds that keep it resident). */
int frcnn_stream_create(const uint32_t* cu_mask, int words, void** out);
int frcnn_stream_destroy(void* stream);
int frcnn_stream_cu_count(void* stream, int* out);
int frcnn_probe_hw_ids(uint32_t* out, int nblocks, int spin, void* stream);

/* Kernel-path selection, process-global (tests and A/B tools; the default
 * "auto" is what every caller should use).  op / path:
 *   "roi_pool_fwd"   : "auto" | "wave" (plane-major image tile in LDS, compare-and-select scan,
 *                      one wave per RoI; RoIs grouped by image; the auto choice) | "dense" (image
 *                      tile, bins packed 64 per wave; any RoI order) | "generic" (one
 *                      workgroup per RoI)
 *   "roi_pool_bwd"   : "auto" (leader-gather plane owner for 7-wide outputs, else ring) | "ring" (latency-hidden plane owner) | "plain"
 *   "propose"        : "auto" | "hybrid" | "lazy" (fused per image) | "wide" (chip-wide bitmask)
 *   "roi_pool_split" : "auto" | "1".."64" (RoI shares per image and channel group)
 *   "roi_pool_cg"    : "auto" | "4" | "8" | "16" (channels per RoIPool forward workgroup)
 *   "roi_pool_fwd_store": "auto" = "temporal" | "nt" (the wave forward's output stores
 *                      non-temporal: better beside concurrent kernels at cfg2, worse alone)
 *   "sampler"        : "auto" = "chip" (the stream cut into 1024-word segments, each one's
 *                      map of entering to leaving step count tabulated chip-wide and
 *                      chained; the walk below runs instead when a step count leaves
 *                      its planned range, or for > 128 images) | "walk" (one workgroup
 *                      walks the MT19937 stream) | "chip_only" (no walk behind it) |
 *                      "chip_tight" (zero-margin ranges: exercises the walk behind it);
 *                      the target creators' _draw / _sample entry points
 *   "rpn_epilogue_strip": "auto" = "64" | "128" (pixels per workgroup strip of the 16-bit
 *                      frcnn_rpn_head_epilogue_t; the fp32 kernel always takes 64)
 * All paths give bit-identical results.  Not thread-safe against calls in
 * flight on other threads; set it before launching. */
int frcnn_set_path(const char* op, const char* path);

/* ---------------------------------------------------------------- anchors */

/* utils/anchors.py:5 generate_anchor_base(base_size, ratios, anchor_scales).
 * ratios / scales are HOST arrays (n_ratios*n_scales <= 64).  out_base: device
 * fp32 [n_ratios*n_scales, 4], row r*n_scales+s. */
int frcnn_anchor_base(const double* ratios, int n_ratios, const double* scales, int n_scales,
                      double base_size, float* out_base, void* stream);

/* utils/anchors.py:33 generate_anchors(anchor_base, feat_stride, width, height).
 * anchor_base fp32 [K,4]; out fp32 [height*width*K, 4]. */
int frcnn_generate_anchors(const float* anchor_base, int K, int feat_stride, int width,
                           int height, float* out, void* stream);

/* utils/utils.py:47 reg2bbox(anchors, reg): fp32 [n,4] x [n,4] -> [n,4]. */
int frcnn_reg2bbox(const float* anchors, const float* reg, int64_t n, float* out, void* stream);

/* nets/rpn.py:117-124 RPN head epilogue, one launch instead of the reference's
 * permute/contiguous/softmax/slice chain:
 *   cls fp32 [N, 2K, H, W] (self.cls conv output), reg fp32 [N, 4K, H, W]
 *   -> cls_nhwc fp32 [N, A, 2]  = cls.permute(0,2,3,1).contiguous().view(N,-1,2)  (:117-118)
 *      fg       fp32 [N, A]     = F.softmax(cls_nhwc, -1)[:, :, 1]              (:119)
 *      reg_nhwc fp32 [N, A, 4]  = reg.permute(0,2,3,1).contiguous().view(N,-1,4)  (:123-124)
 * A = H*W*K, 1 <= K <= 32.  fg feeds frcnn_propose's scores, reg_nhwc its deltas. */
int frcnn_rpn_head_epilogue(const float* cls, const float* reg, int N, int K, int feat_h,
                            int feat_w, float* cls_nhwc, float* fg, float* reg_nhwc,
                            void* stream);

/* ------------------------------------------------------------- proposals */

/* Parameters of the batched proposal layer (nets/rpn.py:22-45 kwargs). */
typedef struct frcnn_propose_params {
    int N;            /* images in the batch */
    int A;            /* anchors per image */
    int K;            /* anchors per location (used when anchors == NULL) */
    int feat_h;       /* feature map height   (used when anchors == NULL) */
    int feat_w;       /* feature map width    (used when anchors == NULL) */
    int feat_stride;  /* 16                   (used when anchors == NULL) */
    float img_h;      /* clamp bound of box columns 0,2 (nets/rpn.py:62) */
    float img_w;      /* clamp bound of box columns 1,3 (nets/rpn.py:63) */
    float min_size;   /* nets/rpn.py:27,65 */
    int pre_nms;      /* nets/rpn.py:39-43 */
    int post_nms;     /* nets/rpn.py:40-43 */
    double iou_threshold; /* nets/rpn.py:44 */
} frcnn_propose_params;

size_t frcnn_propose_workspace_size(const frcnn_propose_params* p);

/* nets/rpn.py:47-79 region_proposal.__call__, batched over N images
 * (replaces the per-image loop nets/rpn.py:131-136).
 *   scores  fp32 [N, A]     fg softmax (nets/rpn.py:119)
 *   deltas  fp32 [N, A, 4]  RPN reg    (nets/rpn.py:124)
 *   anchors fp32 [A, 4] or NULL; if NULL, anchors are generated in-kernel from
 *           anchor_base fp32 [K,4] on the feat_h x feat_w grid (A = feat_h*feat_w*K)
 * Outputs (padded to post_nms):
 *   out_rois  fp32 [N, post_nms, 4]   rows >= out_count[n] are zero
 *   out_idx   int32 [N, post_nms]     anchor index of each roi, -1 padding
 *   out_count int32 [N]               min(post_nms, #kept by NMS) */
int frcnn_propose(const frcnn_propose_params* p, const float* scores, const float* deltas,
                  const float* anchors, const float* anchor_base, float* out_rois,
                  int32_t* out_idx, int32_t* out_count, void* workspace, size_t ws_bytes,
                  void* stream);

/* torchvision.ops.nms(boxes, scores, iou_threshold) as called at nets/rpn.py:75.
 *   boxes fp32 [n,4] (x1,y1,x2,y2), scores fp32 [n]
 *   keep int64 [n]: kept indices in descending-score order; *count (device
 *   int32) = number kept. */
size_t frcnn_nms_workspace_size(int64_t n);
int frcnn_nms(const float* boxes, const float* scores, int64_t n, double iou_threshold,
              int64_t* keep, int32_t* count, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- RoIPool */

/* nets/heads.py:42-47: image-space rois fp32 [R,4] + roi_inds fp32 [R] ->
 * boxes fp32 [R,5] = [idx, r0/img_h*feat_h, r1/img_w*feat_w, r2/img_h*feat_h,
 * r3/img_w*feat_w]. */
int frcnn_roi_transform(const float* rois, const float* roi_inds, int64_t R, float img_h,
                        float img_w, int feat_h, int feat_w, float* boxes, void* stream);

/* torchvision.ops.roi_pool forward (nets/heads.py:48):
 *   x fp32 [N,C,H,W], rois fp32 [R,5] -> out fp32 [R,C,PH,PW],
 *   argmax int32 [R,C,PH,PW] (h*W+w within the plane, -1 for empty bins).
 * RoIs whose batch index is outside [0,N) produce 0 / -1.
 * rois_sorted != 0 PROMISES the RoIs are grouped by non-decreasing batch
 * index (true for proposals and for train.py's sample_rois_ind): one launch,
 * each workgroup finds its image's RoI range itself.  rois_sorted == 0 works
 * for any order (a list kernel groups them first).
 * The workspace (frcnn_roi_pool_fwd_workspace_size bytes) is always required. */
size_t frcnn_roi_pool_fwd_workspace_size(int64_t R, int N, int C);
int frcnn_roi_pool_fwd(const float* x, const float* rois, int64_t R, int N, int C, int H, int W,
                       int PH, int PW, float spatial_scale, int rois_sorted, float* out,
                       int32_t* argmax, void* workspace, size_t ws_bytes, void* stream);

/* ResnetHead.forward's RoI transform + pack + roi_pool (nets/heads.py:42-48)
 * in one call: rois fp32 [R,4] in image pixels (RPN output / sample_rois),
 * roi_inds fp32 [R] -> boxes fp32 [R,5] exactly as frcnn_roi_transform, and
 * out / argmax exactly as frcnn_roi_pool_fwd on those boxes.  With
 * rois_sorted != 0 (same promise as above) the transform runs inside the pool
 * kernel (one launch); otherwise the two calls run back to back.  boxes is
 * always written (the backward needs it).  Workspace: frcnn_roi_pool_fwd_
 * workspace_size(R, N, C). */
int frcnn_roi_pool_fwd_head(const float* x, const float* rois, const float* roi_inds, int64_t R,
                            int N, int C, int H, int W, int PH, int PW, float img_h, float img_w,
                            float spatial_scale, int rois_sorted, float* boxes, float* out,
                            int32_t* argmax, void* workspace, size_t ws_bytes, void* stream);

/* The kernel frcnn_roi_pool_fwd_head (head == 1: 16-B aligned rois; head == 2:
 * an unaligned rois pointer, which the head entry point handles as transform +
 * the plain forward) or frcnn_roi_pool_fwd (head == 0) launches for this shape on
 * `stream` under the current frcnn_set_path choices, as its template name (e.g.
 * "roi_pool_fwd_wave_kernel<1024, 16, 7, true, false, 38400>"), NUL-terminated in name[len]:
 * the label bench.py and the rocprofv3 records key the dominant kernel on. */
int frcnn_roi_pool_fwd_kernel(int64_t R, int N, int C, int H, int W, int PH, int PW, int rois_sorted,
                              int head, void* stream, char* name, size_t len);

/* torchvision _roi_pool_backward (autograd of nets/heads.py:48, reached from
 * train.py:126):  grad_in fp32 [N,C,H,W] = 0, then for n, c, ph, pw in order
 * grad_in[b(n), c, argmax] += grad[n, c, ph, pw].  Deterministic, atomic-free,
 * same summation order as the CPU kernel. */
size_t frcnn_roi_pool_bwd_workspace_size(int64_t R, int N, int PH, int PW);
int frcnn_roi_pool_bwd(const float* grad, const float* rois, const int32_t* argmax, int64_t R,
                       int N, int C, int H, int W, int PH, int PW, float spatial_scale,
                       float* grad_in, void* workspace, size_t ws_bytes, void* stream);
/* The RoIPool backward kernel frcnn_roi_pool_bwd launches for this shape under
 * the current frcnn_set_path choice (e.g. "roi_pool_bwd_lead_kernel<4, 7, 7>"),
 * NUL-terminated in name[len] (bench.py's label for it; the per-image lists
 * launch before it is not named). */
int frcnn_roi_pool_bwd_kernel(int64_t R, int N, int C, int H, int W, int PH, int PW, char* name, size_t len);

/* RoIPool in 16-bit types.  `dtype` is the element type of x / out
 * (forward) and grad / grad_in (backward); rois, roi_inds and boxes stay fp32 and
 * argmax int32.  FRCNN_F32 does exactly what the untyped function does.  For
 * FRCNN_F16 / FRCNN_BF16 every comparison and sum is fp32 on the widened values:
 * argmax is the fp32 forward's on x widened, out is that forward's output
 * rounded to nearest even (exact wherever something was selected; a non-empty
 * bin in which nothing passes the strict '>' gives -inf, the rounded -FLT_MAX),
 * and grad_in is the fp32 backward's sums in the same order, rounded once at
 * the write-out.  Same workspaces, launches and frcnn_set_path overrides as the
 * untyped functions; the one exception is a backward whose planes do not fit
 * LDS ("roi_pool_bwd_kernel_h<T, false>"), which takes an [N,C,H,W] fp32 scratch
 * from the stream-ordered allocator for the duration of the kernel.  Any other
 * dtype code: FRCNN_EINVAL before any HIP call. */
enum { FRCNN_F32 = 0, FRCNN_F16 = 1, FRCNN_BF16 = 2 };
int frcnn_roi_pool_fwd_t(int dtype, const void* x, const float* rois, int64_t R, int N, int C, int H, int W,
                         int PH, int PW, float spatial_scale, int rois_sorted, void* out, int32_t* argmax,
                         void* workspace, size_t ws_bytes, void* stream);
int frcnn_roi_pool_fwd_head_t(int dtype, const void* x, const float* rois, const float* roi_inds, int64_t R,
                              int N, int C, int H, int W, int PH, int PW, float img_h, float img_w,
                              float spatial_scale, int rois_sorted, float* boxes, void* out, int32_t* argmax,
                              void* workspace, size_t ws_bytes, void* stream);
int frcnn_roi_pool_bwd_t(int dtype, const void* grad, const float* rois, const int32_t* argmax, int64_t R,
                         int N, int C, int H, int W, int PH, int PW, float spatial_scale, void* grad_in,
                         void* workspace, size_t ws_bytes, void* stream);
/* The name queries for a dtype: FRCNN_F32 gives the untyped answer, the 16-bit
 * types name the `_h` sibling with its element type first (e.g.
 * "roi_pool_fwd_wave_kernel_h<__half, 1024, 16, 7, true, false, 38400>",
 * "roi_pool_bwd_lead_kernel_h<__hip_bfloat16, 4, 7, 7>"). */
int frcnn_roi_pool_fwd_kernel_t(int dtype, int64_t R, int N, int C, int H, int W, int PH, int PW,
                                int rois_sorted, int head, void* stream, char* name, size_t len);
int frcnn_roi_pool_bwd_kernel_t(int dtype, int64_t R, int N, int C, int H, int W, int PH, int PW, char* name,
                                size_t len);

/* --------------------------------------------------------------- RoIAlign */

/* torchvision.ops.roi_align(input, boxes, output_size, spatial_scale,
 * sampling_ratio, aligned), forward and backward, with the semantics and the
 * summation order of torchvision's CPU kernel (DESIGN.md §3 "RoIAlign").  No
 * reference counterpart: the reference pools with roi_pool (nets/heads.py:48).
 *   x, out, grad, grad_in: `dtype` (FRCNN_F32 / FRCNN_F16 / FRCNN_BF16), one per
 *   call; x [N,C,H,W], out / grad [R,C,PH,PW], grad_in [N,C,H,W]
 *   rois fp32 [R,5] = (b, x1, y1, x2, y2), any order
 * Every operation is fp32 and separately rounded.  Per RoI:
 *   off = aligned ? 0.5f : 0;  sw = x1*scale - off, sh = y1*scale - off,
 *   ew = x2*scale - off, eh = y2*scale - off;  rw = ew - sw, rh = eh - sh, each
 *   raised to 1.f when !aligned;  bh = rh / PH, bw = rw / PW;
 *   gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / PH), gw likewise;
 *   count = (float)max((int64)gh * gw, 1);
 *   sample (ph, iy): y = (sh + ph*bh) + (((iy + .5f) * bh) / gh); x likewise from
 *   sw, pw, bw, ix, gw.
 * A sample with y < -1 || y > H || x < -1 || x > W is outside: it contributes
 * nothing (forward) and adds nothing (backward).  Otherwise, per axis:
 *   if (y <= 0) y = 0;  yl = (int)y;  if (yl >= H-1) { yh = yl = H-1; y = yl; }
 *   else yh = yl + 1;  ly = y - yl, hy = 1 - ly
 * and w1 = hy*hx, w2 = hy*lx, w3 = ly*hx, w4 = ly*lx.
 * Forward: acc = +0; for iy, then ix, ascending:
 *   acc += ((w1*v(yl,xl) + w2*v(yl,xh)) + w3*v(yh,xl)) + w4*v(yh,xh);
 *   out[n,c,ph,pw] = acc / count.
 * Backward: grad_in = +0; for n, ph, pw, iy, ix ascending and g = grad[n,c,ph,pw],
 *   four additions in this order, all four even where a weight is zero:
 *   gi[b,c,yl,xl] += (g*w1)/count; gi[b,c,yl,xh] += (g*w2)/count;
 *   gi[b,c,yh,xl] += (g*w3)/count; gi[b,c,yh,xh] += (g*w4)/count
 *   into fp32 sums in exactly this order: no atomics, the same bits on every call.
 * Guards (torchvision's behaviour is undefined there): a RoI whose batch index
 * b is not in (-1, N) (truncated toward zero otherwise), or one of whose four
 * scaled coordinates x1*scale .. y2*scale is not finite or above 2^20 in
 * magnitude, gives an all-zero output and no gradient; nothing is read or
 * written out of bounds.
 * sampling_ratio <= 0 is adaptive, 1..16 fixed, above 16 FRCNN_EINVAL.  Work per
 * bin is bounded by the map, not by the box: samples outside the map (forward)
 * or off the workgroup's pixels (backward) are skipped without being visited.
 * 16-bit types: widened exactly at the load, the fp32 arithmetic above, rounded
 * to nearest even once at the store (float16 overflow: +-inf); the backward
 * never sums in 16 bits.
 * Argument errors (FRCNN_EINVAL before any HIP call, the message names the
 * argument): a dtype code other than the three, PH or PW < 1, sampling_ratio >
 * 16, a null pointer with R > 0.  R == 0 succeeds; the backward then stores an
 * all-zero grad_in.  The backward stores every grad_in element exactly once (no
 * memset); one launch each.  Nothing is kept between launches: the workspace
 * sizes are a nominal 256 and the buffers are not touched (NULL is accepted). */
size_t frcnn_roi_align_fwd_workspace_size(int64_t R, int N, int C);
int frcnn_roi_align_fwd_t(int dtype, const void* x, const float* rois, int64_t R, int N, int C, int H, int W,
                          int PH, int PW, float spatial_scale, int sampling_ratio, int aligned, void* out,
                          void* workspace, size_t ws_bytes, void* stream);
size_t frcnn_roi_align_bwd_workspace_size(int64_t R, int N, int PH, int PW);
int frcnn_roi_align_bwd_t(int dtype, const void* grad, const float* rois, int64_t R, int N, int C, int H, int W,
                          int PH, int PW, float spatial_scale, int sampling_ratio, int aligned, void* grad_in,
                          void* workspace, size_t ws_bytes, void* stream);
/* The kernels the two calls launch for this dtype and shape, as their template
 * names ("roi_align_fwd_kernel<ElemF16>", "roi_align_bwd_tile_kernel<ElemF32, 8>"),
 * NUL-terminated in name[len].  Same argument checks as the calls. */
int frcnn_roi_align_fwd_kernel(int dtype, int64_t R, int N, int C, int H, int W, int PH, int PW,
                               int sampling_ratio, char* name, size_t len);
int frcnn_roi_align_bwd_kernel(int dtype, int64_t R, int N, int C, int H, int W, int PH, int PW,
                               int sampling_ratio, char* name, size_t len);
/* The launch plan of the two calls for this shape (host only, no HIP call; the
 * launches read the same functions), and the constants behind it:
 *   plan = { run (channels per forward thread, 8), tile (backward tile edge, 8),
 *            stride (LDS words per pixel row, 65), waves (tiles per workgroup, 5),
 *            stage_bins (a RoI's gradients are staged in LDS up to PH*PW = 49),
 *            scan (sampling grids up to 16 points per axis are walked whole),
 *            lane_samples (up to 64 samples per axis go one per lane),
 *            fwd_threads, fwd_grid (workgroups of 256; both 0 where the forward
 *            only clears `out`: N, H or W == 0),
 *            tiles_x, tiles_y, cgroups (groups of 64 channels), units (tiles_x *
 *            tiles_y * cgroups * N), blocks, idle (waves of the last workgroup
 *            without a unit), lds_bytes, staged (PH*PW <= stage_bins) }.
 * Same shape checks as the calls, the backward's "map too large" included. */
int frcnn_roi_align_plan(int64_t R, int N, int C, int H, int W, int PH, int PW, int64_t plan[17]);
/* The pyramid backward's: plan = { first[0..8] (level l owns the units [first[l],
 * first[l + 1]); first[8] = units), cgroups, units, blocks, idle, staged }.  H, W:
 * host arrays of n_levels entries. */
int frcnn_roi_align_multi_plan(int n_levels, const int* H, const int* W, int N, int C, int PH, int PW,
                               int64_t plan[14]);

/* Multi-scale RoIAlign over a feature pyramid (torchvision.ops.MultiScaleRoIAlign's
 * pooling; DESIGN.md §3 "Multi-scale RoIAlign"): every RoI is pooled from the level
 * that matches its size, one launch forward and one backward, no host sync.
 *   n_levels L in [1, 8]; x[l] / grad_in[l] `dtype` [N,C,H[l],W[l]], fine to coarse,
 *   all of one N, C and dtype; spatial_scales[l] fp32; rois fp32 [R,5] in image
 *   coordinates, any order; out / grad `dtype` [R,C,PH,PW]; levels int32 [R] or NULL.
 *   x, grad_in, H, W, spatial_scales and thresholds are HOST arrays of L (thresholds:
 *   L - 1, may be NULL for L == 1) entries, read during the call; the pointers in x
 *   and grad_in are device pointers.
 * Level of a RoI, every operation fp32:
 *   s = sqrtf((x2 - x1) * (y2 - y1))   (two subtractions, one product, a correctly
 *   rounded root);  level = #{k : s >= thresholds[k]}.
 * A NaN s (a NaN coordinate, a negative area) compares false everywhere: level 0.
 * No logarithm is evaluated on the device.  The caller derives the thresholds from
 * torchvision's LevelMapper, floor(lvl0 + log2(s / s0) + 1e-6) clamped to [k_min,
 * k_max] minus k_min: thresholds[k - 1] is the smallest non-negative fp32 s at which
 * that formula, in fp32 on the host, yields at least k (ops.level_thresholds).
 * Pooling: a RoI of level l is pooled from x[l] with spatial_scales[l] exactly as
 * frcnn_roi_align_fwd_t pools it -- the same guards (batch index, scaled coordinates
 * beyond 2^20 under that level's scale), sampling_ratio limit, clipping of adaptive
 * grids, separately rounded fp32 operations and one rounding of 16-bit types.  A
 * level with H[l] == 0 or W[l] == 0 gives zeros for its RoIs.
 *   out[n] is stored exactly once, in RoI order (no zero fill, no scatter);
 *   levels[n], if asked for, once.
 *   grad_in[l] sums the RoIs of level l only, in ascending RoI index and the order of
 *   bins and samples above; every element of every level is stored exactly once,
 *   +0 where no RoI of the level reaches (levels no RoI maps to included).  No atomics.
 * So with idx_l the ascending indices of level l, bit for bit:
 *   out[idx_l]  = roi_align_fwd(x[l], rois[idx_l], spatial_scales[l])
 *   grad_in[l]  = roi_align_bwd(grad[idx_l], rois[idx_l], spatial_scales[l]).
 * Argument errors (FRCNN_EINVAL before any HIP call): n_levels outside [1, 8], a NaN
 * threshold or one below its predecessor (equal neighbours are accepted: a level no
 * size reaches), and everything the single-map calls refuse, per level.  No device
 * allocation, no synchronisation; the workspace is not touched (NULL is accepted). */
int frcnn_roi_align_multi_fwd_t(int dtype, int n_levels, const void* const* x, const int* H, const int* W,
                                const float* spatial_scales, const float* thresholds, const float* rois, int64_t R,
                                int N, int C, int PH, int PW, int sampling_ratio, int aligned, void* out,
                                int* levels, void* workspace, size_t ws_bytes, void* stream);
int frcnn_roi_align_multi_bwd_t(int dtype, int n_levels, const void* grad, const int* H, const int* W,
                                const float* spatial_scales, const float* thresholds, const float* rois, int64_t R,
                                int N, int C, int PH, int PW, int sampling_ratio, int aligned, void* const* grad_in,
                                void* workspace, size_t ws_bytes, void* stream);
/* The kernels the two calls launch, as their template names
 * ("roi_align_multi_fwd_kernel<ElemF32>", "roi_align_multi_bwd_tile_kernel<ElemBF16, 8>"). */
int frcnn_roi_align_multi_fwd_kernel(int dtype, int n_levels, int64_t R, int N, int C, int PH, int PW,
                                     int sampling_ratio, char* name, size_t len);
int frcnn_roi_align_multi_bwd_kernel(int dtype, int n_levels, int64_t R, int N, int C, int PH, int PW,
                                     int sampling_ratio, char* name, size_t len);

/* FPN proposal layer: torchvision's RegionProposalNetwork.filter_proposals with
 * BoxCoder(weights=(1, 1, 1, 1)) over a feature pyramid (DESIGN.md §3 "FPN proposals"):
 * per-level top-k, decode, clip, filters, level-wise NMS and the merge, four launches,
 * no host sync, no device allocation.
 *   n_levels L in [1, 8]; objectness[l] `dtype` [N,K,H[l],W[l]]; deltas[l] `dtype`
 *   [N,4K,H[l],W[l]], channel 4k + c -- the RPN head's conv outputs, contiguous, read in
 *   place (no permute, no cast; a 16-bit value is widened exactly at the load, so every
 *   output is bit-identical to the call on the fp32 copies); anchor_bases[l] fp32 [K,4]
 *   (x1, y1, x2, y2), 16-byte aligned; image_sizes fp32 [N,2] of (h, w), a device pointer.
 *   objectness, deltas, anchor_bases, H, W, stride_h and stride_w are HOST arrays of L
 *   entries, read during the call; the pointers in the first three are device pointers.
 * Per image and level, A = K*H*W anchors, anchor a = (y*W + x)*K + k = base[k] + (x*stride_w,
 * y*stride_h, x*stride_w, y*stride_h), one fp32 addition per coordinate, formed in registers:
 *   1. selection: the first min(pre_nms, A) anchors in the stable descending order of the
 *      raw logit -- every NaN first, -0.0 == +0.0, ties by ascending a -- before any filter;
 *   2. decode of those, fp32, every operation rounded separately: w = x2 - x1, cx = x1 + 0.5*w;
 *      dw, dh clamped from above at float(log(1000/16)) (a NaN stays); pcx = dx*w + cx;
 *      pw = exp(dw)*w with a correctly rounded exp; box = pcx -+ 0.5*pw (the same in y);
 *   3. clip x to [0, w_n], y to [0, h_n] (a NaN stays); keep a box iff x2 - x1 >= min_size and
 *      y2 - y1 >= min_size and logit >= logit_thresh (a NaN fails each; -inf keeps every
 *      non-NaN logit).  logit_thresh is the caller's score threshold as a logit
 *      (ops.logit_threshold); no sigmoid is evaluated on the device;
 *   4. greedy NMS in the selection order, per image and level on its own, with
 *      torchvision's test (double)(inter / union) > nms_thresh, stopped at post_nms kept;
 *   5. merge: the kept boxes of an image by (logit descending, level ascending, a ascending);
 *      the first post_nms are written, count[n] is how many.
 * Outputs, every element stored exactly once per call: boxes fp32 [N,post,4] (padding 0),
 * logits fp32 [N,post] (-inf), levels / anchor_idx int32 [N,post] (-1), count int32 [N],
 * rois fp32 [N*post,5] rows (n, x1, y1, x2, y2), a padding row (-1, 0, 0, 0, 0).
 * Limits (FRCNN_EINVAL with a message, before any launch, like NULLs, misaligned pointers
 * and a short workspace): 1 <= L <= 8, 1 <= N <= 1024, 1 <= K <= 32, H, W >= 1,
 * K*H*W < 2^24, (H-1)*stride_h and (W-1)*stride_w < 2^24, strides >= 1,
 * 1 <= pre_nms <= 2048, 1 <= post_nms <= 4096.  The workspace is stream-ordered scratch,
 * 256-byte aligned; nothing in it needs to be initialised. */
size_t frcnn_propose_multi_workspace_size(int n_levels, int N, int K, const int* H, const int* W, int pre_nms,
                                          int post_nms);
int frcnn_propose_multi_t(int dtype, int n_levels, const void* const* objectness, const void* const* deltas,
                          const float* const* anchor_bases, const int* H, const int* W, const int* stride_h,
                          const int* stride_w, int N, int K, const float* image_sizes, int pre_nms, int post_nms,
                          double nms_thresh, float logit_thresh, float min_size, float* boxes, float* logits,
                          int32_t* levels, int32_t* anchor_idx, int32_t* count, float* rois, void* workspace,
                          size_t ws_bytes, void* stream);
/* The kernels a call of this shape launches, in order; the selection kernel lists the branch
 * each level takes: "sort" (K*H*W <= 2048, the level is sorted whole) or "select" (radix select):
 * "fpn_select_decode_kernel<ElemF16>[select,sort] fpn_nms_mask_kernel fpn_sweep_kernel fpn_merge_kernel". */
int frcnn_propose_multi_kernel(int dtype, int n_levels, int N, int K, const int* H, const int* W, int pre_nms,
                               int post_nms, char* name, size_t len);

/* Pyramid RPN training targets: torchvision's assign_targets_to_anchors (box_iou + Matcher
 * with set_low_quality_matches_), BalancedPositiveNegativeSampler and BoxCoder.encode with
 * weights (1, 1, 1, 1) for a whole batch and pyramid (DESIGN.md §3 "Pyramid RPN training"):
 * five launches, no host sync, no device allocation, no floating-point atomics; the same
 * inputs (rng included) give the same bits on every call.
 *   anchor_bases, H, W, stride_h, stride_w: HOST arrays of L entries as frcnn_propose_multi_t
 *   takes them; anchor_bases[l] is a device pointer, fp32 [K,4], 16-byte aligned.  The global
 *   anchor index is off_l + (y*W_l + x)*K + k, levels in the order given; A is the total.
 *   gt_boxes fp32 [N,G,4] (x1, y1, x2, y2), 16-byte aligned; gt_count int32 [N], clamped to
 *   [0, G]; rng int64 [2] = (seed, calls): device pointers.  rng is read on the device and the
 *   last launch stores calls + 1.
 * Matching, fp32, every operation rounded separately: area = (x2-x1)*(y2-y1), inter = the
 * product of max(min(x2,x2') - max(x1,x1'), 0) and the same in y, iou = inter / ((area_gt +
 * area_anchor) - inter), IEEE divide; inter == 0 gives 0 and a NaN quotient counts as 0.  A gt
 * row below gt_count that is not finite or has x2 <= x1 or y2 <= y1 is absent (its index still
 * counts).  Per anchor the largest IoU over the present rows, the lowest index on a tie;
 * iou < (float)bg -> -1, iou < (float)fg -> -2, else the index.  With allow_low_quality_matches
 * every anchor whose IoU with some present gt g equals the largest IoU any anchor has with g
 * (compared as fp32; 0 == 0 counts) gets its own argmax back.  No present row: -1 everywhere.
 * Sampling: positives are matches >= 0, negatives matches == -1; num_pos = min(P, (int)(B *
 * positive_fraction)) (the double product truncated), num_neg = min(Ng, B - num_pos); chosen
 * are those with the smallest (key, anchor index), key = word 0 of Philox4x32-10 with counter
 * (anchor index, n, calls & 0xFFFFFFFF, calls >> 32) and key (seed & 0xFFFFFFFF, seed >> 32),
 * all but its top key_bits bits cleared (32: the whole key; 0: every key ties; a test knob).
 * Outputs, every element stored exactly once per call:
 *   matches int32 [N,A]; sampled int32 [N,A] (1 sampled positive, 0 sampled negative, -1);
 *   samples int32 [N,B]: the sampled positives in ascending index, then the negatives in
 *   ascending index, then -1; n_pos, n_neg int32 [N]; reg_targets fp32 [N,B,4], 16-byte
 *   aligned: for the positive rows w = x2-x1, cx = x1 + 0.5*w of anchor and matched gt,
 *   (dx, dy, dw, dh) = ((gcx-cx)/w, (gcy-cy)/h, log(gw/w), log(gh/h)) with a correctly
 *   rounded log; every other row is zero.
 * Limits (FRCNN_EINVAL with a message before any launch, like NULLs, misaligned pointers and
 * a short workspace): 1 <= L <= 8, 1 <= N <= 1024, 1 <= K <= 32, 1 <= G <= 256, H, W >= 1,
 * K*H*W < 2^24 per level, (H-1)*stride_h and (W-1)*stride_w < 2^24, strides >= 1, A < 2^31,
 * 1 <= batch_size_per_image <= 1024, positive_fraction in [0, 1], bg_iou_thresh <=
 * fg_iou_thresh, key_bits in [0, 32].  The workspace is stream-ordered scratch, 256-byte
 * aligned (about 4*N*A bytes: it keeps every anchor's key between the launches); nothing in it
 * needs to be initialised. */
size_t frcnn_rpn_targets_multi_workspace_size(int n_levels, int N, int K, const int* H, const int* W, int G,
                                              int batch_size_per_image);
int frcnn_rpn_targets_multi(int n_levels, const float* const* anchor_bases, const int* H, const int* W,
                            const int* stride_h, const int* stride_w, int N, int K, const float* gt_boxes,
                            const int32_t* gt_count, int G, int64_t* rng, int batch_size_per_image,
                            double positive_fraction, double fg_iou_thresh, double bg_iou_thresh,
                            int allow_low_quality_matches, int key_bits, int32_t* matches, int32_t* sampled,
                            int32_t* samples, int32_t* n_pos, int32_t* n_neg, float* reg_targets, void* workspace,
                            size_t ws_bytes, void* stream);
/* The kernels a call of this shape launches, in order, with what of the plan the shape fixes:
 * the workgroups per image of the chip-wide kernels (1024 anchors each) and the anchors of the
 * last one; for the select kernel the number of boundary-bucket keys it sorts in LDS (lds=), the
 * digits of the key its radix passes refine when a boundary bucket holds more than that (radix=8 |
 * 8+12 | 8+12+12 by key_bits <= 8 | <= 20 | above; which of the two happens depends on the data) and
 * the 4096-anchor steps of one of its sweeps over an image:
 * "rpnt_init_kernel rpnt_gtmax_kernel[chunks=88,tail=1002] rpnt_label_kernel
 *  rpnt_select_kernel[lds=4096,radix=8+12+12,steps=22] rpnt_finish_kernel". */
int frcnn_rpn_targets_multi_kernel(int n_levels, int N, int K, const int* H, const int* W, int G,
                                   int batch_size_per_image, int key_bits, char* name, size_t len);

/* Pyramid RPN losses: torchvision's RegionProposalNetwork.compute_loss on the targets above,
 * forward and backward.  objectness[l] `dtype` [N,K,H[l],W[l]], deltas[l] `dtype`
 * [N,4K,H[l],W[l]] (channel 4k + c), read in place as frcnn_propose_multi_t reads them.
 * Forward, over the S = sum(n_pos + n_neg) sample slots: per-element fp32, (max(x,0) - x*t) +
 * log1p(exp(-|x|)) with correctly rounded exp / log1p against t = 1 (slot < n_pos) or 0, and
 * for the positives' four coordinates z = |x - target|, z < (float)beta ? 0.5*z*z/beta :
 * z - 0.5*beta; the terms are added in fp64 in a fixed order; loss[0] = objectness sum / S,
 * loss[1] = box sum / S, each rounded once (S == 0: NaN); stats[0] = S, stats[1] = 0.
 * Backward: dobjectness[l] / ddeltas[l] in `dtype`, every element stored exactly once: +0
 * where sampled < 0 (and in ddeltas where sampled == 0), else (sigmoid(x) - t) * (*g_obj / S)
 * and (z < beta ? (x - target)/beta : sign(x - target)) * (*g_box / S), fp32, rounded once at
 * the store.  g_obj / g_box are device pointers; NULL gives zeros and that input is not read.
 * S == 0 gives zeros.  Limits as above plus beta finite and >= 0.  The forward's workspace is
 * stream-ordered scratch of frcnn_rpn_losses_multi_workspace_size bytes, 256-byte aligned. */
size_t frcnn_rpn_losses_multi_workspace_size(int N, int batch_size_per_image);
int frcnn_rpn_losses_multi_fwd_t(int dtype, int n_levels, const void* const* objectness, const void* const* deltas,
                                 const int* H, const int* W, int N, int K, int batch_size_per_image,
                                 const int32_t* samples, const int32_t* n_pos, const int32_t* n_neg,
                                 const float* reg_targets, double beta, float* loss, int32_t* stats, void* workspace,
                                 size_t ws_bytes, void* stream);
int frcnn_rpn_losses_multi_bwd_t(int dtype, int n_levels, const void* const* objectness, const void* const* deltas,
                                 const int* H, const int* W, int N, int K, int batch_size_per_image,
                                 const int32_t* sampled, const int32_t* samples, const int32_t* n_pos,
                                 const float* reg_targets, double beta, const int32_t* stats, const float* g_obj,
                                 const float* g_box, void* const* dobjectness, void* const* ddeltas, void* stream);

/* Pyramid box-head training targets: torchvision's RoIHeads.select_training_samples
 * (add_gt_proposals, box_iou + Matcher(fg, bg, allow_low_quality_matches=False),
 * assign_targets_to_proposals, BalancedPositiveNegativeSampler, BoxCoder.encode with weights) for
 * a whole batch (DESIGN.md §3 "Pyramid box-head training" is the contract).  Two launches
 * on `stream`, no host synchronisation, no floating-point atomics; fp32 with every operation
 * rounded separately; the same bits on every call.
 *   proposals fp32 [N,R,4] (x1,y1,x2,y2), prop_count int32 [N] (clamped to [0,R]): what
 *   frcnn_propose_multi_t wrote as boxes / count; gt_boxes fp32 [N,G,4], gt_labels int32 [N,G],
 *   gt_count int32 [N] (clamped to [0,G]); rng int64 [2] = (seed, calls) on the device, read by
 *   the first launch; the last one stores calls + 1 and nothing reads rng behind that store.
 * Candidates of an image, M = R + G: index c < R is proposal c, present iff c < prop_count;
 * index R + g is gt row g, present iff add_gt and the row is present (g < gt_count, finite,
 * x2 > x1, y2 > y1: the rule of frcnn_rpn_targets_multi).  IoU as there (no intersection is 0, a
 * NaN quotient is 0); the largest over the present gt rows, lowest index on a tie;
 * matches[n,c] = -1 below (float)bg, -2 in [bg, fg), else the gt index; -3 for an absent
 * candidate; an image without a present gt row has -1 for every present candidate.  label =
 * gt_labels[match], 0 for -1, -1 for -2; positive iff label >= 1, negative iff label == 0.
 * num_pos = min(P, (int)(B * positive_fraction)), num_neg = min(Ng, B - num_pos); chosen are
 * the candidates of each class with the smallest (key, index), key = word 0 of Philox4x32-10
 * with counter (index, n, calls lo, calls hi) and key (seed lo, seed hi), its low 32 - key_bits
 * bits cleared (key_bits = 32 outside tests).
 * Outputs, B slots per image, the chosen candidates in ascending index order (positives and
 * negatives interleaved), then padding; every element is stored on every call:
 *   rois fp32 [N*B,5] (n, x1, y1, x2, y2) with the candidate's bits, padding (-1,0,0,0,0): the
 *   RoI rows of frcnn_roi_align_multi_fwd_t; labels int32 [N,B], padding -1; matched int32
 *   [N,B]: the gt index of a positive, 0 of a negative, padding -1; reg_targets fp32 [N,B,4]:
 *   for a positive w = x2 - x1, cx = x1 + 0.5*w of proposal and gt, ((float)wx * (gcx - cx)) / w
 *   and (float)ww * log(gw / w) with a correctly rounded log, else 0; samples int32 [N,B]: the
 *   candidate index, padding -1; n_pos, n_neg int32 [N]; matches int32 [N,M].
 * Limits: N in [1,1024], R in [1,4096], G in [1,256], batch_size_per_image in [1,1024],
 * positive_fraction in [0,1], bg <= fg, weights finite and positive, key_bits in [0,32].
 * proposals, gt_boxes, reg_targets 16-byte aligned, rng 8-byte.  The workspace is stream-ordered
 * scratch, 256-byte aligned; its contents on entry do not matter. */
size_t frcnn_box_head_targets_workspace_size(int N, int R, int G, int batch_size_per_image);
int frcnn_box_head_targets(const float* proposals, const int32_t* prop_count, int N, int R, const float* gt_boxes,
                           const int32_t* gt_labels, const int32_t* gt_count, int G, int64_t* rng,
                           int batch_size_per_image, double positive_fraction, double fg_iou_thresh,
                           double bg_iou_thresh, double wx, double wy, double ww, double wh, int add_gt, int key_bits,
                           float* rois, int32_t* labels, int32_t* matched, float* reg_targets, int32_t* samples,
                           int32_t* n_pos, int32_t* n_neg, int32_t* matches, void* workspace, size_t ws_bytes,
                           void* stream);
/* Host only: the kernels a call of this shape launches with what the shape fixes of the plan:
 * M, the match kernel's workgroups per image and the candidates of the last one, the candidates
 * per thread of the sample kernel's slot scan, and the 12-bit digits its exact selection may
 * walk (how many it does walk depends on the data: none for a class taken whole):
 * "bht_match_kernel[M=1032,blocks=5,tail=8] bht_sample_kernel[per=2,digits=4x12]". */
int frcnn_box_head_targets_kernel(int N, int R, int G, int batch_size_per_image, int key_bits, char* name, size_t len);

/* Pyramid box-head losses: torchvision's fastrcnn_loss on the targets above, forward and
 * backward.  class_logits `dtype` [N*B,C], box_regression `dtype` [N*B,4C] (column 4c + j),
 * widened exactly at the load.  Slot j of image n is valid iff j < n_pos[n] + n_neg[n] (clamped
 * to B) and its label is >= 0; a valid slot whose label is >= C is skipped and counted in
 * stats[2], never used as an index.  S = the valid slots that are not skipped.
 * Forward: per row, one wave: m = max x, e_c = exp(x_c - m) correctly rounded, their sum with
 * each lane adding classes (lane, lane + 64) in that order and then a butterfly from 32 down to
 * 1, the term log(sum) - (x_label - m) with a correctly rounded log; for a positive (label >= 1)
 * the four columns 4*label + j: z = |x - target|, z < (float)beta ? 0.5*z*z/beta : z - 0.5*beta.
 * The terms are added in fp64 in a fixed order; loss[0] = class sum / S, loss[1] = box sum / S,
 * each rounded once (S == 0: NaN); stats = (S, positives, skipped, 0).
 * Backward: every element of dclass_logits / dbox_regression stored exactly once in `dtype`:
 * (e_c / sum - (c == label)) * (*g_cls / S) on a valid row, (z < beta ? (x - target)/beta :
 * sign(x - target)) * (*g_box / S) on a positive's four label columns, +0 elsewhere; fp32,
 * rounded once at the store.  g_cls / g_box are device pointers; NULL gives zeros and that
 * input is not read.  S == 0 gives zeros.  No atomics.  Limits: N, B as above, C in [2,128],
 * beta finite and >= 0.  The forward's workspace is stream-ordered scratch, 256-byte aligned. */
size_t frcnn_box_head_losses_workspace_size(int N, int batch_size_per_image);
int frcnn_box_head_losses_fwd_t(int dtype, const void* class_logits, const void* box_regression, int N,
                                int batch_size_per_image, int C, const int32_t* labels, const float* reg_targets,
                                const int32_t* n_pos, const int32_t* n_neg, double beta, float* loss, int32_t* stats,
                                void* workspace, size_t ws_bytes, void* stream);
int frcnn_box_head_losses_bwd_t(int dtype, const void* class_logits, const void* box_regression, int N,
                                int batch_size_per_image, int C, const int32_t* labels, const float* reg_targets,
                                const int32_t* n_pos, const int32_t* n_neg, double beta, const int32_t* stats,
                                const float* g_cls, const float* g_box, void* dclass_logits, void* dbox_regression,
                                void* stream);

/* Pyramid box-head inference: torchvision's RoIHeads.postprocess_detections (F.softmax,
 * BoxCoder(weights).decode, box_ops.clip_boxes_to_image, the score_thresh test,
 * box_ops.remove_small_boxes, box_ops.batched_nms in its _batched_nms_vanilla form, the first
 * detections_per_img by score) and GeneralizedRCNNTransform.postprocess's resize_boxes, for a
 * whole batch (DESIGN.md §3 "Pyramid box-head inference" is the contract).  Three launches on
 * `stream`, no host synchronisation, no floating-point atomics; fp32 with every operation
 * rounded separately; the same bits on every call.
 *   class_logits `dtype` [N*R,C], box_regression `dtype` [N*R,4C] (column 4c + j), widened
 *   exactly at the load; row n*R + r is proposal r of image n.  proposals fp32 [N,R,4]
 *   (x1,y1,x2,y2), prop_count int32 [N] (clamped to [0,R]; rows past it are never read): what
 *   frcnn_propose_multi_t wrote as boxes / count.  image_sizes fp32 [N,2] of (h,w);
 *   original_sizes fp32 [N,2] of (h,w) or NULL.
 * Row r < prop_count: m = max x, e_c = exp(x_c - m) correctly rounded, s = their sum in
 * ascending class order, p_c = e_c * (1 / s) (frcnn_detect's rule).  (r, c), c >= 1, is a
 * candidate iff p_c > score_thresh (a NaN never is).  Its box: w = x2 - x1, cx = x1 + 0.5*w,
 * dx = reg[4c] / wx with a correctly rounded division, dw = min(reg[4c+2] / ww,
 * (float)log(1000/16)) as torch.clamp(max=) (a NaN stays), pcx = dx*w + cx, pw = exp(dw)*w,
 * x1' = pcx - 0.5*pw, x2' = pcx + 0.5*pw, the same in y; x clamped to [0, w_n], y to [0, h_n]
 * as torch.clamp; kept iff x2' - x1' >= min_size and y2' - y1' >= min_size (a NaN fails).
 * Greedy NMS per (image, class) in the order (p descending, r ascending), the test of
 * frcnn_nms; classes never meet.  An image's kept boxes in the order (p descending, flat index
 * r*(C-1) + (c-1) ascending): total[n] of them, the first count[n] = min(total[n],
 * detections_per_img) written.  With original_sizes, x is multiplied by orig_w / w_n and y by
 * orig_h / h_n (correctly rounded quotients) last of all.
 * Outputs, every element stored exactly once per call: boxes fp32 [N,D,4] (padding 0), labels
 * int32 [N,D] (-1), scores fp32 [N,D] (0), roi int32 [N,D] (the row r; -1), count, total int32 [N].
 * Limits: N in [1,1024], R in [1,4096], C in [2,128], detections_per_img in [1,1024], weights
 * finite and positive; boxes 16-byte aligned.  The workspace is stream-ordered scratch,
 * 256-byte aligned, 4*N*R*C + 2*N*R*(C-1) + 4*N*(C-1) bytes with each of the three parts
 * rounded up to 256; its contents on entry do not matter. */
size_t frcnn_box_detections_workspace_size(int N, int R, int C);
int frcnn_box_detections_t(int dtype, int N, int R, int C, const void* class_logits, const void* box_regression,
                           const float* proposals, const int32_t* prop_count, const float* image_sizes,
                           const float* original_sizes, float score_thresh, double nms_thresh, int detections_per_img,
                           float min_size, float wx, float wy, float ww, float wh, float* boxes, int32_t* labels,
                           float* scores, int32_t* roi, int32_t* count, int32_t* total, void* workspace,
                           size_t ws_bytes, void* stream);
/* Host only: the kernels a call of this shape launches, with the branch of the launch plan
 * ("rows": R <= 1024, one thread per row; "strided": 1,024 threads, four rows each):
 * "bd_score_kernel<ElemF32> bd_class_nms_kernel<ElemF32,1>[rows] bd_merge_kernel<ElemF32>". */
int frcnn_box_detections_kernel(int dtype, int R, int C, int detections_per_img, char* name, size_t len);

/* Pyramid mask head (DESIGN.md §3 "Pyramid mask head" is the contract): torchvision's
 * project_masks_on_boxes, maskrcnn_loss, and maskrcnn_inference + paste_masks_in_image for a
 * whole batch.  No host synchronisation, no floating-point atomics, every output element stored
 * exactly once per call, the same bits on every call; fp32 with every operation rounded
 * separately, '/' and exp correctly rounded.
 *
 * frcnn_mask_targets: two launches.  bt_rois fp32 [N*B,5], bt_labels / bt_matched int32 [N,B]:
 *   rois, labels, matched of frcnn_box_head_targets; gt_masks uint8 [N,G,Hm,Wm], a byte v read
 *   as the fp32 value v.  An image's positives (label >= 1) go in slot order to rows 0..count-1
 *   of its P rows, count[n] = min(positives, P): rois fp32 [N*P,5] = (n, box), labels, matched,
 *   slot (the source slot) int32 [N,P]; the rows behind them are (-1,0,0,0,0) and -1.
 *   targets fp32 [N*P,M,M]: row = RoIAlign of plane (n, matched) over the box with
 *   spatial_scale 1, sampling_ratio -1, aligned = false, in frcnn_roi_align_fwd_t's order of
 *   operations (iy outer, ix inner, w1*v1 + w2*v2 + w3*v3 + w4*v4 left to right, one division
 *   by the sample count); +0 for a padding row, a matched outside [0,G), or a coordinate that
 *   is NaN or beyond 2^20 in magnitude.
 *   Limits: N in [1,1024], B and P in [1,1024], G in [1,256], Hm, Wm in [1,4096], M in [1,56].
 * frcnn_mask_losses_fwd_t / _bwd_t: mask_logits `dtype` [N*P,C,M,M], read in place; targets,
 *   labels, count as frcnn_mask_targets wrote them.  A row below its image's count contributes
 *   channel labels[row] only: l = (max(x,0) - x*t) + log1p(exp(-|x|)) in fp32 per element (exp
 *   and log1p correctly rounded), summed in fp64 in a fixed order; loss[0] = sum / (S*M*M)
 *   rounded once, S = the sum of the counts (+0 for S == 0); a row whose label is outside
 *   [0,C) is skipped and counted; stats = (S, skipped, 0, 0).
 *   Backward: every element of dlogits stored once in `dtype` with 16-byte stores:
 *   (1/(1+exp(-x)) - t) * (*g_loss / (float)(S*M*M)) on the labelled channel of such a row, +0
 *   elsewhere; g_loss is a device pointer, NULL gives zeros.  dlogits 16-byte aligned.
 *   Limits: C in [2,128]; the workspace is stream-ordered scratch, 256-byte aligned.
 * frcnn_mask_paste_t: one launch.  mask_logits `dtype` [N*D,C,M,M]; boxes fp32 [N,D,4], labels
 *   int32 [N,D], count int32 [N] of frcnn_box_detections_t; image_sizes / original_sizes fp32
 *   [N,2] of (h,w) or NULL (image_sizes needs original_sizes: the boxes are then multiplied by
 *   orig / image as frcnn_box_detections_t does it; original_sizes alone only clips).  Per
 *   detection: p = 1/(1+exp(-x)) of channel label, zero-padded by `padding` to S = M + 2*padding;
 *   expand_boxes with the fp32 scale S/M; truncation toward zero; w = max(x2-x1+1, 1), h alike;
 *   ATen's bilinear formula (align_corners = false): scale = (float)S/(float)w, src = scale*(d+0.5)
 *   - 0.5 clamped below at 0, i0 = (int)src, i1 = i0 + (i0 < S-1), l1 = src - i0, l0 = 1 - l1,
 *   value = l0y*(l0x*a + l1x*b) + l1y*(l0x*c + l1x*d); written inside [0,im_w) x [0,im_h), zeros
 *   elsewhere.  masks uint8 [N,D,Hc,Wc] of (value > threshold) when `binary`, else fp32 values.
 *   All zeros: a row at or beyond count, a label outside [1,C), an inverted box, a coordinate
 *   (before or after the expansion) that is NaN or beyond 2^20 in magnitude.
 *   Limits: D in [1,1024], padding in [0,4], Hc, Wc in [1,4096], M in [1,56].
 * The *_kernel queries are host only and name the kernels and the plan branch a call reaches. */
int frcnn_mask_targets(int N, int B, int P, int G, int Hm, int Wm, int M, const float* bt_rois,
                       const int32_t* bt_labels, const int32_t* bt_matched, const uint8_t* gt_masks, float* rois,
                       int32_t* labels, int32_t* matched, int32_t* slot, int32_t* count, float* targets, void* stream);
int frcnn_mask_targets_kernel(int B, int P, int M, char* name, size_t len);
size_t frcnn_mask_losses_workspace_size(int N, int P);
int frcnn_mask_losses_fwd_t(int dtype, int N, int P, int C, int M, const void* mask_logits, const float* targets,
                            const int32_t* labels, const int32_t* count, float* loss, int32_t* stats, void* workspace,
                            size_t ws_bytes, void* stream);
int frcnn_mask_losses_bwd_t(int dtype, int N, int P, int C, int M, const void* mask_logits, const float* targets,
                            const int32_t* labels, const int32_t* count, const int32_t* stats, const float* g_loss,
                            void* dlogits, void* stream);
int frcnn_mask_losses_kernel(int dtype, int C, int M, char* name, size_t len);
int frcnn_mask_paste_t(int dtype, int N, int D, int C, int M, const void* mask_logits, const float* boxes,
                       const int32_t* labels, const int32_t* count, const float* image_sizes,
                       const float* original_sizes, int padding, float threshold, int binary, int Hc, int Wc,
                       void* masks, void* stream);
int frcnn_mask_paste_kernel(int dtype, int M, int padding, int Wc, int binary, char* name, size_t len);

/* --------------------------------------------------------- target creators */

/* utils/utils.py:102 bbox_iou(bbox_a, bbox_b) -> [na, nb], with numpy's dtype
 * promotion: a, b each fp32 or fp64 (flag); out fp32 if both fp32, else fp64. */
int frcnn_bbox_iou(const void* a, int a_is_f64, int64_t na, const void* b, int b_is_f64,
                   int64_t nb, void* out, void* stream);

/* utils/utils.py:75 bbox2reg(anchors, bbox) -> fp64 [n, 4] (anchor statistics in
 * the anchors' dtype, box statistics in the boxes' dtype, as numpy does). */
int frcnn_bbox2reg(const void* anchors, int a_is_f64, const void* bbox, int b_is_f64, int64_t n,
                   double* out, void* stream);

/* utils/utils.py:122-204 AnchorTargetCreator.__call__, batched over N images in
 * the order of train.py:71-79.
 *   anchors fp32 [A,4]; boxes fp64 [N,G,4] + labels fp64 [N,G] (rows with label
 *   -1 are padding, train.py:74-76; G <= 256)
 *   rng_state u32 [625] = numpy legacy MT19937 key[624] + pos, updated in place
 *   exactly as the reference's np.random.choice calls would; NULL = no sampling
 *   (labels before the disable step, no RNG use)
 * Outputs: reg fp64 [N,A,4] (zeros for an image without gt), label int32 [N,A],
 * optional argmax int32 [N,A] (after the gt override, utils/utils.py:171-172) and
 * max_iou fp64 [N,A]. */
size_t frcnn_anchor_target_workspace_size(int N, int A, int G);
int frcnn_anchor_target(int N, int A, int G, const float* anchors, const double* boxes,
                        const double* labels, int n_sample, double pos_iou_thresh,
                        double neg_iou_thresh, double pos_ratio, uint32_t* rng_state,
                        double* reg, int32_t* label, int32_t* argmax, double* max_iou,
                        void* workspace, size_t ws_bytes, void* stream);

/* frcnn_anchor_target in two halves on one workspace (frcnn_anchor_target =
 * prepare + sample on the same stream):
 *   prepare: gt compaction, anchor x gt IoU, labels and the ordered positive /
 *            negative lists (utils/utils.py:146-188) -- no RNG, so a training
 *            loop can run it ahead, on another stream, beside the previous
 *            step's draws;
 *   sample:  the np.random.choice draws on rng_state (utils/utils.py:190-202)
 *            and the regression targets; runs after prepare on the same
 *            workspace (order the streams with an event). */
int frcnn_anchor_target_prepare(int N, int A, int G, const float* anchors, const double* boxes,
                                const double* labels, double pos_iou_thresh, double neg_iou_thresh,
                                void* workspace, size_t ws_bytes, void* stream);
int frcnn_anchor_target_sample(int N, int A, int G, const float* anchors, int n_sample, double pos_ratio,
                               uint32_t* rng_state, double* reg, int32_t* label, int32_t* argmax,
                               double* max_iou, void* workspace, size_t ws_bytes, void* stream);
/* frcnn_anchor_target_sample in two steps on the same workspace (same arguments):
 * _draw the np.random.choice calls of utils/utils.py:190-202 (the RNG stream's only
 * kernel), _finish the final labels and bbox2reg targets of utils/utils.py:146-150,
 * 203-204 (any stream, after _draw: order the streams with an event). */
int frcnn_anchor_target_draw(int N, int A, int G, int n_sample, double pos_ratio, uint32_t* rng_state,
                             void* workspace, size_t ws_bytes, void* stream);
int frcnn_anchor_target_finish(int N, int A, int G, const float* anchors, double* reg, int32_t* label,
                               int32_t* argmax, double* max_iou, void* workspace, size_t ws_bytes,
                               void* stream);
/* The chip-wide draws' plan of the last _draw on this workspace (synchronous; a
 * diagnostic, no reference counterpart): out[9] = fail (0: the segment tables held;
 * 1: plan over the workspace's capacity; 2: a step count left its planned range --
 * the walk did the draws), calls with >= 1 step, steps, segments, groups, state
 * blocks, start pos, widest range, missed group (-1).  Returns 1 when the
 * workspace has no chip-wide part (> 128 images: the walk only). */
int frcnn_anchor_target_draw_status(int N, int A, int G, const void* workspace, size_t ws_bytes, int* out);

/* utils/utils.py:207-276 ProposalTargetCreator.__call__, batched over N images in
 * the order of train.py:91-104.
 *   rois fp32 [N,Rp,4] with rcount int32 [N] valid rows per image; boxes/labels as
 *   for frcnn_anchor_target; reg_mean / reg_std: HOST fp64 [4] (the fp32 values of
 *   utils/utils.py:272 widened); rng_state as above (required).
 * Outputs (padded to n_sample): sample_roi fp64 [N,n_sample,4], gt_roi_reg fp64
 * [N,n_sample,4], gt_roi_label fp64 [N,n_sample], sample_count int32 [N]. */
size_t frcnn_proposal_target_workspace_size(int N, int Rp, int G, int n_sample);
int frcnn_proposal_target(int N, int Rp, const float* rois, const int32_t* rcount, int G,
                          const double* boxes, const double* labels, int n_sample,
                          double pos_ratio, double pos_iou_thresh, double neg_iou_thresh_high,
                          double neg_iou_thresh_low, const double* reg_mean,
                          const double* reg_std, uint32_t* rng_state, double* sample_roi,
                          double* gt_roi_reg, double* gt_roi_label, int32_t* sample_count,
                          void* workspace, size_t ws_bytes, void* stream);
/* frcnn_proposal_target in two halves on one workspace (same arguments):
 *   _prepare: utils/utils.py:221-246 (gt concat, IoU, argmax, fg / bg lists) --
 *             no RNG, so it can run on the proposals' stream, off the draws' stream;
 *   _sample:  utils/utils.py:248-276 (the np.random.choice draws on rng_state,
 *             sample order, regression targets); runs after prepare on the same
 *             workspace (order the streams with an event). */
int frcnn_proposal_target_prepare(int N, int Rp, const float* rois, const int32_t* rcount, int G,
                                  const double* boxes, const double* labels, int n_sample,
                                  double pos_iou_thresh, double neg_iou_thresh_high,
                                  double neg_iou_thresh_low, void* workspace, size_t ws_bytes,
                                  void* stream);
int frcnn_proposal_target_sample(int N, int Rp, int G, int n_sample, double pos_ratio,
                                 const double* reg_mean, const double* reg_std, uint32_t* rng_state,
                                 double* sample_roi, double* gt_roi_reg, double* gt_roi_label,
                                 int32_t* sample_count, void* workspace, size_t ws_bytes, void* stream);
/* frcnn_proposal_target_sample in two steps on the same workspace: _draw the
 * np.random.choice calls of utils/utils.py:248-258 (sample order, sample_count),
 * _finish sample_roi / gt_roi_reg / gt_roi_label of utils/utils.py:260-276 (any
 * stream, after _draw). */
int frcnn_proposal_target_draw(int N, int Rp, int G, int n_sample, double pos_ratio, uint32_t* rng_state,
                               int32_t* sample_count, void* workspace, size_t ws_bytes, void* stream);
int frcnn_proposal_target_finish(int N, int Rp, int G, int n_sample, const double* reg_mean,
                                 const double* reg_std, const int32_t* sample_count, double* sample_roi,
                                 double* gt_roi_reg, double* gt_roi_label, void* workspace, size_t ws_bytes,
                                 void* stream);
/* frcnn_anchor_target_draw then frcnn_proposal_target_draw on one RNG stream, as
 * one pass (the order of train.py:71 / :91: every AnchorTarget draw, then every
 * ProposalTarget draw, for the same N images): both prepares must have run on
 * their workspaces (same arguments as the two _draw calls; the pass uses the
 * anchor workspace's chip-wide part, frcnn_anchor_target_draw_status reads it).
 * Bit-identical to the two calls in sequence. */
int frcnn_target_draws(int N, int A, int G_at, int n_sample_at, double pos_ratio_at, void* at_workspace,
                       size_t at_bytes, int Rp, int G_pt, int n_sample_pt, double pos_ratio_pt, void* pt_workspace,
                       size_t pt_bytes, int32_t* sample_count, uint32_t* rng_state, void* stream);
/* As frcnn_anchor_target_draw_status, for the last frcnn_proposal_target_draw. */
int frcnn_proposal_target_draw_status(int N, int Rp, int G, int n_sample, const void* workspace, size_t ws_bytes,
                                      int* out);

/* -------------------------------------------------------------- detections */

/* Head outputs -> detections, batched over N images: softmax, per-class box
 * decode, score threshold, per-class NMS.  No reference counterpart: the
 * reference stops at the head (nets/faster_rcnn.py:32, an empty test_eval.py).
 * The contract is the py-faster-rcnn / chainer predict + _suppress convention
 * the reference replicates, in this project's arithmetic (DESIGN.md
 * "Detections"); class 0 is background and yields no detection.
 *   rois   fp32 [N,R,4] [ymin,xmin,ymax,xmax] with rcount int32 [N] valid rows
 *          per image (frcnn_propose's out_rois / out_count as they are; rcount
 *          is clamped to [0,R], rows past it are ignored whatever they hold)
 *   cls    fp32 [N,R,C] head logits (nets/heads.py:50 returns the [N,C,R] view)
 *   reg    fp32 [N,R,4C], class c in columns 4c..4c+3
 *   reg_mean / reg_std: HOST fp32 [4] (utils/utils.py:272)
 *   1 <= R <= 1024, 2 <= C <= 128, max_det >= 1
 * Per image and class c >= 1: p = softmax(cls) (ATen's last-dim order, exp
 * correctly rounded); candidates p[r,c] > score_thresh; box = reg2bbox(rois[r],
 * reg[r,4c:4c+4] * reg_std + reg_mean) clamped to the image as nets/rpn.py:62-63;
 * NMS as frcnn_nms (ties by ascending r).  Non-finite boxes are outside the
 * contract.  Outputs, class ascending then NMS keep order, padded to max_det:
 *   det_boxes  fp32 [N,max_det,4]   padding 0
 *   det_labels int32 [N,max_det]    class id 1..C-1, padding -1
 *   det_scores fp32 [N,max_det]     padding 0
 *   det_roi    int32 [N,max_det]    source row r, padding -1
 *   det_count  int32 [N]            min(det_total, max_det)
 *   det_total  int32 [N]            kept over all classes (<= R*(C-1)) */
size_t frcnn_detect_workspace_size(int N, int R, int C);
int frcnn_detect(int N, int R, int C, const float* rois, const int32_t* rcount, const float* cls,
                 const float* reg, const float* reg_mean, const float* reg_std, float img_h,
                 float img_w, float score_thresh, double nms_thresh, int max_det, float* det_boxes,
                 int32_t* det_labels, float* det_scores, int32_t* det_roi, int32_t* det_count,
                 int32_t* det_total, void* workspace, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------- evaluation */

/* One batch of detections scored against its ground truth and appended to a
 * device-resident accumulator.  No reference counterpart: the reference's
 * test_eval.py is an empty file.  The contract is the VOC devkit's voc_eval in
 * this project's arithmetic (DESIGN.md "Evaluation").
 *   det_boxes fp32 [N,M,4], det_labels int32 [N,M], det_scores fp32 [N,M],
 *   det_count int32 [N]: frcnn_detect's outputs as they are (det_count is
 *   clamped to [0,M]; slots past it are ignored whatever they hold)
 *   gt_boxes fp64 [N,G,4] [ymin,xmin,ymax,xmax]; gt_labels int32 [N,G], a row is
 *   valid when its label is in 1..C-1; gt_difficult uint8 [N,G] or NULL (none)
 *   1 <= N <= 1024, 1 <= M <= 2^20, 0 <= G <= 256, 2 <= C <= 128, 1 <= cap <= 2^24
 * Every slot below the clamped count becomes one record, in (image, slot)
 * order.  A detection's gt is the first maximum of bbox_iou (utils/utils.py:
 * 102-119, fp64; with plus_one, 1.0 added to columns 2, 3 of both boxes) over the
 * valid gt of its class; it is matched when that IoU > iou_thresh.  Flag: 0 not
 * matched (FP), -1 matched to a difficult gt or label outside 1..C-1 (ignored),
 * else 1 (TP) for the gt's first claimant in (descending score, ascending slot)
 * order and 0 for the others.  State (caller-owned, all zero = empty):
 *   hdr       int64 [4+C]   n_records, n_images, batches dropped, 0, npos[0..C)
 *   rec_key   uint64 [cap]  class << 56 | desc_score_key(score) << 24 | record index
 *   rec_flag  int8 [cap]
 *   rec_image int32 [cap]   n_images before the batch + n
 * A batch that does not fit in cap writes nothing and adds one to hdr[2]; that
 * is not an error (nothing is read back). */
int frcnn_eval_update(int N, int M, int G, int C, int64_t cap, const float* det_boxes,
                      const int32_t* det_labels, const float* det_scores, const int32_t* det_count,
                      const double* gt_boxes, const int32_t* gt_labels, const uint8_t* gt_difficult,
                      double iou_thresh, int plus_one, int64_t* hdr, uint64_t* rec_key, int8_t* rec_flag,
                      int32_t* rec_image, void* stream);

/* Per-class AP and mAP of an accumulator (once per dataset; the empty
 * test_eval.py again, DESIGN.md "Evaluation" "Result").  n_records is hdr[0],
 * read back by the caller.  The first n_records keys are sorted ascending
 * (class, descending score, insertion order) inside the library; per class
 * c >= 1 integer running TP / FP sums, rec = tp / npos[c], prec = tp / max(tp +
 * fp, 1), then the 11-point AP (use_07_metric != 0) or the area under the
 * precision envelope.  ap[c] = NaN for c = 0 and where npos[c] == 0; map = mean
 * of the non-NaN entries.
 *   ap double [C], map double [1]: device
 *   sorted_key uint64 [n_records] (device) or NULL: the sorted keys
 * Workspace: frcnn_eval_ap_workspace_size(C, cap) bytes serve every n_records
 * <= cap (0 for a C or cap outside frcnn_eval_update's limits). */
size_t frcnn_eval_ap_workspace_size(int C, int64_t cap);
int frcnn_eval_ap(int C, int64_t n_records, const int64_t* hdr, const uint64_t* rec_key,
                  const int8_t* rec_flag, int use_07_metric, double* ap, double* map,
                  uint64_t* sorted_key, void* ws, size_t ws_bytes, void* stream);

/* The launch shape of the two entry points above for a batch of N images of M
 * slots and a closing step over n_records records, from the constants and host
 * functions the launches themselves use.  Host only: no HIP call is made.
 *   plan[0] images per step of the per-workgroup count sums, plan[1] steps for N
 *   plan[2] slots per match chunk, plan[3] match chunks for M
 *   plan[4] keys per sort tile, plan[5] sort tiles for n_records, plan[6] sort passes
 *   plan[7] histogram words one scan covers, plan[8] the scan's share per thread
 *   plan[9] records per chunk of the precision / recall walk
 * N and M within frcnn_eval_update's limits, 0 <= n_records <= 2^24. */
int frcnn_eval_plan(int N, int M, int64_t n_records, int64_t plan[10]);

/* COCO-style evaluation (DESIGN.md "COCO-style evaluation" is the contract:
 * pycocotools.cocoeval with iouType "bbox", restated; no reference counterpart).
 * One batch is matched at the ten IoU thresholds and the four area ranges and
 * appended to a device-resident accumulator.  Inputs and limits are those of
 * frcnn_eval_update, with gt_crowd uint8 [N,G] or NULL (none) as the one gt flag
 * (pycocotools' iscrowd; a caller who wants VOC's difficult objects treated as
 * ignore regions passes them here).
 *   tables    double [119], device: the IoU thresholds T[10], the recall
 *             thresholds R[101], the area ranges A[4][2] (lo, hi; both ends
 *             inclusive) in the order all, small, medium, large.  They are read,
 *             never recomputed.
 * State (caller-owned, hdr all zero = empty):
 *   hdr       int64 [4+4C]   n_records, n_images, batches dropped, 0, npig[C][4]
 *   rec_key   uint64 [cap]   class << 56 | desc_score_key(score) << 24 | record index
 *   rec_bits  uint64 [cap][2], 16-byte aligned (as det_boxes is: both are read 16 bytes at a time)
 *             word 0: bits 20a..20a+9 the matched mask (bit = threshold) and bits
 *             20a+10..20a+19 the ignored mask of area range a = 0, 1, 2
 *             word 1: bits 0..9 / 10..19 those masks of area range 3; bits 32..38
 *             the rank within (image, class) by (descending score, slot), 127 for
 *             a rank >= 100 and for class 0 records
 * Every slot below the clamped count becomes one record in (image, slot) order;
 * a batch that does not fit in cap writes nothing and adds one to hdr[2]. */
int frcnn_coco_eval_update(int N, int M, int G, int C, int64_t cap, const float* det_boxes,
                           const int32_t* det_labels, const float* det_scores, const int32_t* det_count,
                           const double* gt_boxes, const int32_t* gt_labels, const uint8_t* gt_crowd,
                           const double* tables, int64_t* hdr, uint64_t* rec_key, uint64_t* rec_bits,
                           void* stream);

/* pycocotools' accumulate() and summarize() of an accumulator (once per
 * dataset).  n_records is hdr[0], read back by the caller; the keys are sorted
 * inside the library (frcnn_eval_ap's sort).  Outputs, device, C-contiguous:
 *   precision double [10,101,C,4,3], recall double [10,C,4,3]  (-1: no gt)
 *   stats double [12]: AP AP50 AP75 APs APm APl AR1 AR10 AR100 ARs ARm ARl
 *   ap_per_class double [C]: AP of one class over all areas at maxDet 100
 * Workspace: frcnn_coco_eval_workspace_size(C, cap) bytes serve every n_records
 * <= cap (0 for a C or cap outside the limits). */
size_t frcnn_coco_eval_workspace_size(int C, int64_t cap);
int frcnn_coco_eval_accumulate(int C, int64_t n_records, const int64_t* hdr, const uint64_t* rec_key,
                               const uint64_t* rec_bits, const double* tables, double* precision,
                               double* recall, double* stats, double* ap_per_class, void* ws,
                               size_t ws_bytes, void* stream);

/* Mask overlap counts (DESIGN.md "COCO segm evaluation"; no reference
 * counterpart): what iouType "segm" needs of a batch of pasted masks.
 *   det_masks uint8 [N,D,H,W], gt_masks uint8 [N,G,H,W]: one canvas, device,
 *             16-byte aligned; a pixel is set iff its byte is non-zero
 *   det_count int32 [N] or NULL (every row is a detection), clamped to [0, D]
 *   det_labels int32 [N,D] and gt_labels int32 [N,G], or both NULL
 *   inter     int32 [N,D,G]: pixels set in both masks of a considered pair, 0
 *             for every other pair.  With labels a pair is considered iff
 *             d < det_count[n] and det_labels[n,d] == gt_labels[n,g] and that
 *             label is in [1, C); without, iff d < det_count[n].
 *   det_area  int32 [N,D]: pixels set, 0 for d >= det_count[n] (not read)
 *   gt_area   int32 [N,G]: pixels set
 * Limits: 1 <= N <= 1024, 1 <= D <= 1024, 0 <= G <= 256, 1 <= H, W <= 4096 with
 * H*W <= 2^24, 2 <= C <= 128 (read with labels only).  Every output element is
 * stored exactly once; integers only, so two calls give the same bits.
 * Workspace: frcnn_mask_overlap_workspace_size bytes (0 outside the limits): the
 * masks as bits, one 64-bit word per 64 pixels of a row, and per mask its pixel
 * count and its window of non-empty rows and word columns. */
size_t frcnn_mask_overlap_workspace_size(int N, int D, int G, int H, int W);
int frcnn_mask_overlap(int N, int D, int G, int H, int W, int C, const uint8_t* det_masks,
                       const uint8_t* gt_masks, const int32_t* det_labels, const int32_t* det_count,
                       const int32_t* gt_labels, int32_t* inter, int32_t* det_area, int32_t* gt_area,
                       void* ws, size_t ws_bytes, void* stream);

/* The launch shape of frcnn_mask_overlap.  Host only: no HIP call is made.
 *   plan[0] 64-bit words per row, plan[1] the pack branch: 0 whole 16-byte
 *   vectors (W % 16 == 0), 1 rows with an unaligned head and a tail
 *   plan[2] pack workgroups (one per mask), plan[3] pair workgroups (one per
 *   (image, detection)), plan[4] workspace bytes
 *   plan[5] 16-bit patterns per row, plan[6] rows per band, plan[7] bands per mask */
int frcnn_mask_overlap_plan(int N, int D, int G, int H, int W, int64_t plan[8]);

/* The kernels of a frcnn_mask_overlap call on an H x W canvas and the pack branch,
 * "mo_pack_kernel[vec16]+mo_pair_kernel" or "...[vec16+edges]...".  Host only. */
int frcnn_mask_overlap_kernel(int H, int W, char* name, size_t len);

/* frcnn_coco_eval_update with iouType "segm" (DESIGN.md "COCO segm evaluation"):
 * the same records, appended to the same state, from the counts of
 * frcnn_mask_overlap's labelled form instead of boxes.
 *   inter int32 [N,M,G], det_pixels int32 [N,M], gt_pixels int32 [N,G]
 *   gt_area double [N,G] or NULL: the annotation's area, which the size ranges
 *         and the ignore rule see instead of the pixel count
 * IoU of a pair: 0 when inter == 0; inter / det_pixels for a crowd gt; else
 * inter / (det_pixels + gt_pixels - inter): exact integers, one fp64 division.
 * A detection's area is det_pixels.  Everything else is frcnn_coco_eval_update's. */
int frcnn_coco_segm_eval_update(int N, int M, int G, int C, int64_t cap, const int32_t* det_labels,
                                const float* det_scores, const int32_t* det_count, const int32_t* inter,
                                const int32_t* det_pixels, const int32_t* gt_pixels,
                                const int32_t* gt_labels, const uint8_t* gt_crowd, const double* gt_area,
                                const double* tables, int64_t* hdr, uint64_t* rec_key, uint64_t* rec_bits,
                                void* stream);

/* The kernels of an update: "coco_match_kernel<boxes>+coco_advance_kernel" (segm == 0,
 * frcnn_coco_eval_update) or "coco_match_kernel<counts>+..." (segm == 1).  Host only. */
int frcnn_coco_eval_kernel(int segm, char* name, size_t len);

/* ------------------------------------------------------------------ losses */

/* The training losses of one stage, train.py:29-57 with :81-83 (RPN) or
 * :112-121 (head), forward and backward (DESIGN.md "Losses" is the contract).
 *   rows = N*L rows (anchors or sampled RoIs of the whole batch), 0 <= rows < 2^31
 *   cls    fp32 [rows, C]   logits, 2 <= C <= 128
 *   reg    fp32 [rows, 4P]  P = 1 (RPN: one box per row) or P = C (head: a row
 *          with label c uses columns 4c..4c+3, the gather of train.py:112-117)
 *   reg_t  fp64 [rows, 4]   the target creators' regression targets as emitted
 *   labels int32 [rows] (labels_f64 == 0, frcnn_anchor_target's) or fp64 [rows]
 *          (labels_f64 != 0, frcnn_proposal_target's gt_roi_label; truncated
 *          toward zero as .type(LongTensor)).  -1 = unlabelled; a label outside
 *          -1..C-1 (NaN included) is skipped by both terms, never used as an
 *          index, and counted
 *   sigma  > 0, finite; 1/sigma^2, 0.5*sigma^2 and 0.5/sigma^2 are formed in
 *          double and rounded to fp32, as torch's scalar promotion does
 * All fp32, every operation separately rounded:
 *   cls_loss = mean over rows with a label in 0..C-1 of log(sum_c exp(x_c - max x))
 *              - (x_label - max x); exp and log correctly rounded, the sum in
 *              ascending class order; no such row -> NaN (0/0, as torch)
 *   reg_loss = sum over rows with label > 0 and their four columns of
 *              d < 1/sigma^2 ? (0.5*sigma^2)*(d*d) : d - 0.5/sigma^2, d = |x - (float)t|,
 *              divided by max(n_pos, 1)
 * The rows' terms are added in fp64, in an order that depends on rows alone:
 * the same inputs give the same bits on every call (no atomics).  Only labelled
 * rows are read: values of cls / reg / reg_t in other rows, NaN included,
 * influence nothing.
 * Outputs: loss fp32 [2] = (cls_loss, reg_loss); stats int32 [4] = (n_valid,
 * n_pos, n_skipped, 0).  rows == 0 gives (NaN, 0) and zero counts; cls, reg,
 * reg_t and labels may then be NULL.
 * Workspace: frcnn_losses_workspace_size(rows, C) bytes (0 for arguments
 * outside the limits).  Two launches. */
size_t frcnn_losses_workspace_size(int64_t rows, int C);
int frcnn_losses_fwd(int64_t rows, int C, int P, const float* cls, const float* reg, const double* reg_t,
                     const void* labels, int labels_f64, double sigma, float* loss, int32_t* stats,
                     void* workspace, size_t ws_bytes, void* stream);

/* Gradients of the two losses above with respect to cls and reg (the autograd
 * of train.py:126 through :81-83 / :112-121).  Inputs as frcnn_losses_fwd, plus
 * its stats and the upstream gradients g_cls / g_reg: DEVICE pointers to one
 * fp32 each (NULL = 0: that output is all zero and its inputs are not read);
 * nothing is read back to the host.  Outputs, dense, every element stored
 * exactly once by one launch (16-byte stores when dcls and dreg are 16-byte
 * aligned; no memset):
 *   dcls fp32 [rows, C]  = (softmax(x) - onehot(label)) * (g_cls / n_valid) on
 *        rows with a label in 0..C-1, 0 elsewhere
 *   dreg fp32 [rows, 4P] = (d < 1/sigma^2 ? sigma^2*(x - t) : sign(x - t)) *
 *        (g_reg / max(n_pos, 1)) on the label's four columns of rows with label
 *        > 0, 0 elsewhere
 * A NaN logit in an unlabelled row yields a zero gradient here; torch's dense
 * log-softmax backward would give NaN.  Finite inputs are the contract. */
int frcnn_losses_bwd(int64_t rows, int C, int P, const float* cls, const float* reg, const double* reg_t,
                     const void* labels, int labels_f64, double sigma, const int32_t* stats,
                     const float* g_cls, const float* g_reg, float* dcls, float* dreg, void* stream);

/* ------------------------------------------- predictions in 16-bit types */

/* The ops that read the network's predictions, for float16 / bfloat16
 * predictions (a network under autocast; DESIGN.md §3 "Predictions in 16-bit
 * types").  `dtype` (FRCNN_F32 / FRCNN_F16 / FRCNN_BF16) is the element type of
 * every `void*` prediction argument of the call; all of them share it.
 * FRCNN_F32 does exactly what the untyped function does (same launches).  For
 * the 16-bit types each value is widened exactly at the load and the fp32
 * function's arithmetic runs unchanged, so every fp32 / int32 output is
 * bit-identical to the untyped function's on the widened inputs; outputs in
 * the 16-bit type are either copies of input bits or fp32 results rounded once
 * to nearest even at the store (float16 overflow gives +-inf).  Targets, labels,
 * RoIs, losses, statistics and workspaces are those of the untyped functions.
 * Any other dtype code: FRCNN_EINVAL before any HIP call.  A pointer must be
 * aligned to its element type; wider loads and stores are used where the
 * addresses allow them.
 *
 * frcnn_rpn_head_epilogue_t: cls [N,2K,H,W], reg [N,4K,H,W] of `dtype` ->
 *   cls_nhwc [N,A,2], reg_nhwc [N,A,4] of `dtype` (the inputs' bit patterns,
 *   permuted), fg fp32 [N,A], and for the 16-bit types deltas fp32 [N,A,4] =
 *   reg_nhwc widened, which is what frcnn_propose reads.  With FRCNN_F32 deltas
 *   is not written and may be NULL (reg_nhwc is the proposal layer's input). */
int frcnn_rpn_head_epilogue_t(int dtype, const void* cls, const void* reg, int N, int K, int feat_h, int feat_w,
                              void* cls_nhwc, float* fg, void* reg_nhwc, float* deltas, void* stream);
/* frcnn_losses_fwd_t / frcnn_losses_bwd_t: cls, reg (and dcls, dreg) of `dtype`.
 *   loss and stats as frcnn_losses_fwd on the widened inputs; dcls / dreg are
 *   frcnn_losses_bwd's fp32 values rounded once at the store, never scaled or
 *   accumulated in 16 bits; every element is stored exactly once (16-byte stores,
 *   eight elements, where dcls and dreg are 16-byte aligned). */
int frcnn_losses_fwd_t(int dtype, int64_t rows, int C, int P, const void* cls, const void* reg, const double* reg_t,
                       const void* labels, int labels_f64, double sigma, float* loss, int32_t* stats,
                       void* workspace, size_t ws_bytes, void* stream);
int frcnn_losses_bwd_t(int dtype, int64_t rows, int C, int P, const void* cls, const void* reg, const double* reg_t,
                       const void* labels, int labels_f64, double sigma, const int32_t* stats, const float* g_cls,
                       const float* g_reg, void* dcls, void* dreg, void* stream);
/* frcnn_detect_t: cls [N,R,C] and reg [N,R,4C] of `dtype`; everything else, the
 *   workspace included, as frcnn_detect. */
int frcnn_detect_t(int dtype, int N, int R, int C, const float* rois, const int32_t* rcount, const void* cls,
                   const void* reg, const float* reg_mean, const float* reg_std, float img_h, float img_w,
                   float score_thresh, double nms_thresh, int max_det, float* det_boxes, int32_t* det_labels,
                   float* det_scores, int32_t* det_roi, int32_t* det_count, int32_t* det_total, void* workspace,
                   size_t ws_bytes, void* stream);

/* ----------------------------------------------------------- preprocessing */

/* The image half of voc_data.__getitem__ (utils/data_loader.py:38,61-75) for a
 * batch: uint8 HWC RGB images of differing sizes -> fp32 [N,3,out_h,out_w],
 * resized as skimage.transform.resize does with its defaults and normalised
 * (DESIGN.md "Preprocessing" is the contract).
 *   pixels  uint8 [pixels_bytes] (device): image n is h*w*3 bytes, HWC, at
 *           offset[n]; gaps between images and any order of offsets are allowed
 *   offset  int64 [N] (device); hw int32 [N,2] = (h, w) per image (device)
 *   max_h, max_w  host bounds of the batch's sizes: they size the launch and
 *           its LDS, no size is read back.  1 <= max_h, max_w <= 16384
 *   1 <= N <= 1024, 1 <= out_h, out_w <= 4096
 *   mean, std  HOST fp32 [3], finite, std > 0
 * Anything outside these limits returns FRCNN_EINVAL before any HIP call.
 * Per channel r = Wh p Ww^T with p = uint8 / 255 and, per axis n_in -> n_out,
 * W = bilinear x Gaussian:
 *   bilinear row d: position ((2d+1) n_in - n_out) / (2 n_out) in exact integer
 *     arithmetic, floor i0 and fraction f; weights 1-f on i0, f on i0+1
 *   Gaussian (anti-aliasing, only where n_in > n_out): s = (n_in/n_out - 1)/2,
 *     radius r = int(4s + 0.5), weights exp(-0.5 k^2 / s^2) / sum on i-r..i+r
 *   indices outside 0..n-1 fold by mirror without edge repeat (period 2(n-1):
 *     -1 -> 1, n -> n-2; n == 1 -> 0)
 * and out = (r - mean[c]) / std[c].  The weights are formed in fp64 and rounded
 * to fp32 once; the sums are fp32 in ascending tap order.  The same image gives
 * the same bits on every call, alone or in any batch (no atomics).
 * Outputs, every element stored exactly once (no memset):
 *   out     fp32 [N,3,out_h,out_w]
 *   status  int32 [N]: 0 ok; 1 = h or w outside 1..max_h / 1..max_w, or an axis
 *           with in > 5*out (at 5: s = 2, r = 8, 18 taps); 2 = offset[n] < 0
 *           or offset[n] + 3*h*w > pixels_bytes.  An image with a nonzero
 *           status is never read and its three planes are zeros.
 * Stream-ordered, asynchronous, no allocation, capturable; one launch.
 * Workspace: frcnn_preprocess_workspace_size(...) bytes (0 for arguments
 * outside the limits).  This version keeps nothing between launches: the size
 * is a nominal 256 and the buffer is not touched. */
size_t frcnn_preprocess_workspace_size(int N, int max_h, int max_w, int out_h, int out_w);
int frcnn_preprocess(int N, const uint8_t* pixels, int64_t pixels_bytes, const int64_t* offset,
                     const int32_t* hw, int max_h, int max_w, int out_h, int out_w,
                     const float* mean, const float* std, float* out, int32_t* status,
                     void* workspace, size_t ws_bytes, void* stream);
/* The launch plan frcnn_preprocess takes for these host bounds (host only, no
 * HIP call; the launch reads the same function): plan = { TH (tile height; the
 * tile is TH x 64 outputs), lds_rows, lds_cols (the staged source footprint's
 * bound), max_taps (2 + 2r of the wider axis), lds_bytes, grid_x, grid_y,
 * grid_z }.  Same argument checks as frcnn_preprocess. */
int frcnn_preprocess_plan(int N, int max_h, int max_w, int out_h, int out_w, int32_t plan[8]);

/* The boxes' rescale that goes with it (utils/data_loader.py:66-69), fp64:
 * boxes [N,G,4] as [ymin, xmin, ymax, xmax]; columns 0, 2 are b / h * out_h,
 * columns 1, 3 are b / w * out_w (divide, then multiply, each rounded); every
 * negative result becomes -1; an image with h < 1 or w < 1 gets all -1.
 * Bit-exact with the numpy expression.  1 <= N <= 1024, 0 <= G <= 65536.
 *   boxes, out double [N,G,4]; hw int32 [N,2]: device.  One launch. */
int frcnn_rescale_boxes(int N, int G, const double* boxes, const int32_t* hw, int out_h, int out_w,
                        double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FRCNN_CAPI_H_ */
