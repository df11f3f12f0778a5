// Detections: head outputs -> per-class boxes, score threshold, per-class NMS.
//
// The reference has no counterpart (nets/faster_rcnn.py stops at the head, its
// test_eval.py is empty); the contract is the py-faster-rcnn / chainer
// predict + _suppress convention, written out in DESIGN.md "Detections".
// A batch is N x (C-1) independent box sets of 0..R boxes each, so the work is
// cut per (image, class), not per image as in proposal.hip:
//   det_softmax_kernel   : eight RoI rows per workgroup, one thread per logit;
//                          probabilities p [N, C, R] (class-major, so a class
//                          reads its column coalesced).  The fp64-backed exp_cr
//                          runs once per logit here.
//   det_class_nms_kernel : one workgroup per (image, class): compact the rows
//                          over the score threshold (ballot + wave prefix +
//                          cross-wave counts), rank-sort the (score desc, row
//                          asc) keys in LDS, decode the candidates only, greedy
//                          NMS in 64-candidate blocks (each block first against
//                          the kept list, all waves; then its own 64x64 mask,
//                          resolved by one wave).  LDS is linear in the
//                          candidate count.  The kept (row, score, box) list and
//                          its length go to the (image, class) slot of the
//                          workspace.
//   det_emit_kernel      : one workgroup per image and 1,024 output slots:
//                          exclusive scan of the C-1 counts, copy into the padded
//                          outputs, padding, counts.
// Every workspace word a kernel reads was written by an earlier kernel of the
// same call, and nothing is accumulated with atomics: no state carries over,
// and results are bit-identical from run to run.
//
// float16 / bfloat16 head outputs (frcnn_detect_t; DESIGN.md §3 "Predictions in
// 16-bit types"): det_softmax_kernel is a template on the element type of cls
// and det_class_nms_kernel on that of reg, the only two sites that read them;
// each value is widened at its load and everything behind it is the fp32 code.
#include "common.h"
#include "elem16.h"
#include "nms_iou.h"

namespace frcnn {

constexpr int kDetMaxR = 1024;  // RoI slots per image: one thread per row in det_class_nms_kernel
constexpr int kDetMaxC = 128;

struct DetWs {
    float* prob;      // [N, C, R]
    int32_t* krow;    // [N, C-1, R] kept source rows, NMS keep order
    float* kscore;    // [N, C-1, R]
    float4* kbox;     // [N, C-1, R]
    int32_t* kcnt;    // [N, C-1]
    size_t bytes;
};

static DetWs carve_det(void* ws, int N, int R, int C) {
    Carver c(ws);
    DetWs w{};
    const size_t rows = static_cast<size_t>(N) * R;
    const size_t slots = rows * (C - 1);
    w.prob = c.take<float>(rows * C);
    w.krow = c.take<int32_t>(slots);
    w.kscore = c.take<float>(slots);
    w.kbox = c.take<float4>(slots);
    w.kcnt = c.take<int32_t>(static_cast<size_t>(N) * (C - 1));
    w.bytes = c.used();
    return w;
}

static bool det_shape_ok(int N, int R, int C) {
    return N >= 1 && N <= 65535 && R >= 1 && R <= kDetMaxR && C >= 2 && C <= kDetMaxC;
}

__device__ __forceinline__ int det_valid_rows(const int32_t* rcount, int n, int R) {
    const int k = rcount[n];
    return k < 0 ? 0 : (k > R ? R : k);
}

// p_c = e_c * (1 / s), e_c = exp_cr(x_c - max x), s summed in ascending class
// order: ATen's last-dim CPU softmax, as rpn_head_epilogue_kernel for two classes.
// A workgroup takes kSmRows consecutive rows: one thread per logit for the
// fp64-backed exp (the cost), one thread per row for the max and the ordered sum.
constexpr int kSmRows = 8;

template <class E>
__global__ __launch_bounds__(256) void det_softmax_kernel(const typename E::raw* __restrict__ cls,
                                                          const int32_t* __restrict__ rcount, int N, int R,
                                                          int C, float* __restrict__ prob) {
    __shared__ float xs[kSmRows * kDetMaxC];
    __shared__ float rm[kSmRows];  // the row's max, then 1 / its sum
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kSmRows;
    const int nrow = min(kSmRows, N * R - row0);
    const int ne = nrow * C;
    const typename E::raw* x = cls + static_cast<size_t>(row0) * C;
    for (int i = tid; i < ne; i += 256) xs[i] = E::widen(x[i]);
    __syncthreads();
    if (tid < nrow) {
        const float* v = xs + tid * C;
        float m = v[0];
        for (int c = 1; c < C; ++c) m = v[c] > m ? v[c] : m;  // a NaN logit leaves m or makes e NaN: the row is NaN either way
        rm[tid] = m;
    }
    __syncthreads();
    for (int i = tid; i < ne; i += 256) xs[i] = exp_cr(xs[i] - rm[i / C]);
    __syncthreads();
    if (tid < nrow) {
        const float* v = xs + tid * C;
        float s = v[0];
        for (int c = 1; c < C; ++c) s = s + v[c];
        rm[tid] = 1.0f / s;
    }
    __syncthreads();
    for (int i = tid; i < ne; i += 256) {
        const int row = i / C, c = i - row * C;
        const int n = (row0 + row) / R, r = row0 + row - n * R;
        if (r < det_valid_rows(rcount, n, R)) prob[(static_cast<size_t>(n) * C + c) * R + r] = xs[i] * rm[row];
    }
}

struct DetParams {
    int R, C;
    float img_h, img_w, score_thresh;
    float mean[4], std[4];
};

// blockDim.x = R rounded up to whole waves (<= 1024): thread r owns row r.
template <class E>
__global__ __launch_bounds__(1024) void det_class_nms_kernel(DetParams P, const float* __restrict__ rois,
                                                             const int32_t* __restrict__ rcount,
                                                             const typename E::raw* __restrict__ reg, NmsThr thr,
                                                             DetWs w) {
    __shared__ uint64_t ckey[kDetMaxR];
    __shared__ float4 cbox[kDetMaxR];
    __shared__ float carea[kDetMaxR];
    __shared__ int klist[kDetMaxR];  // kept candidates (positions in cbox), keep order
    __shared__ uint64_t diag[64];    // the block's own mask: bit j of row i = "i suppresses j", j > i
    __shared__ uint64_t red[16];
    __shared__ int wcnt[16];
    __shared__ int s_kcount;

    const int c = blockIdx.x + 1, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
    const int R = P.R, C = P.C;
    const int k = det_valid_rows(rcount, n, R);
    const float* pc = w.prob + (static_cast<size_t>(n) * C + c) * R;
    const size_t obase = (static_cast<size_t>(n) * (C - 1) + (c - 1)) * R;

    // ---- candidates, compacted in ascending row order (NaN > thresh is false)
    float p = 0.0f;
    bool cand = false;
    if (tid < k) {
        p = pc[tid];
        cand = p > P.score_thresh;
    }
    const uint64_t bal = __ballot(cand);
    if (lane == 0) wcnt[wid] = __popcll(bal);
    __syncthreads();
    int base = 0, cc = 0;
    for (int v = 0; v < nw; ++v) {
        const int q = wcnt[v];
        base += v < wid ? q : 0;
        cc += q;
    }
    if (cand)
        ckey[base + __popcll(bal & lanemask_lt())] =
            (static_cast<uint64_t>(desc_score_key(p)) << 32) | static_cast<uint32_t>(tid);
    __syncthreads();

    // ---- rank sort: keys are distinct, a key's place is the number of keys below it
    const uint64_t my = tid < cc ? ckey[tid] : 0ull;
    int rank = 0;
    if (tid < cc)
        for (int j = 0; j < cc; ++j) rank += ckey[j] < my ? 1 : 0;
    __syncthreads();
    if (tid < cc) ckey[rank] = my;
    __syncthreads();

    // ---- decode the candidates: loc = reg * std + mean, reg2bbox, clamp
    if (tid < cc) {
        const int r = static_cast<int>(static_cast<uint32_t>(ckey[tid]));  // < k <= R
        const float* a = rois + (static_cast<size_t>(n) * R + r) * 4;
        const typename E::raw* d = reg + (static_cast<size_t>(n) * R + r) * 4 * C + 4 * c;
        float4 loc;
        loc.x = E::widen(d[0]) * P.std[0];
        loc.x = loc.x + P.mean[0];
        loc.y = E::widen(d[1]) * P.std[1];
        loc.y = loc.y + P.mean[1];
        loc.z = E::widen(d[2]) * P.std[2];
        loc.z = loc.z + P.mean[2];
        loc.w = E::widen(d[3]) * P.std[3];
        loc.w = loc.w + P.mean[3];
        float4 b = decode_box(make_float4(a[0], a[1], a[2], a[3]), loc);
        b.x = clamp_nan(b.x, 0.0f, P.img_h);
        b.z = clamp_nan(b.z, 0.0f, P.img_h);
        b.y = clamp_nan(b.y, 0.0f, P.img_w);
        b.w = clamp_nan(b.w, 0.0f, P.img_w);
        cbox[tid] = b;
        carea[tid] = box_area(b);
    }
    __syncthreads();

    // ---- greedy NMS over 64-candidate blocks, in score order
    int kcount = 0;
    const int nb = (cc + 63) >> 6;
#pragma unroll 1
    for (int blk = 0; blk < nb; ++blk) {
        const int j = blk * 64 + lane;
        const bool jv = j < cc;
        float4 bj = make_float4(0.f, 0.f, 0.f, 0.f);
        float aj = 0.f;
        if (jv) {
            bj = cbox[j];
            aj = carea[j];
        }
        bool sup = false;  // by a box kept in an earlier block
        if (jv && !thr.never)
            for (int i = wid; i < kcount; i += nw) {
                const int ki = klist[i];
                if (iou_over(cbox[ki], carea[ki], bj, aj, thr)) {
                    sup = true;
                    break;
                }
            }
        const uint64_t supm = __ballot(sup);
        if (lane == 0) red[wid] = supm;
        for (int r = wid; r < 64; r += nw) {
            const int ia = blk * 64 + r;
            bool bit = false;
            if (jv && lane > r && ia < cc && !thr.never) bit = iou_over(cbox[ia], carea[ia], bj, aj, thr);
            const uint64_t D = __ballot(bit);
            if (lane == 0) diag[r] = D;
        }
        __syncthreads();
        if (wid == 0) {
            uint64_t removed = 0;
            for (int v = 0; v < nw; ++v) removed |= red[v];
            const int rows = cc - blk * 64;
            if (rows < 64) removed |= ~0ull << rows;
            uint64_t alive = ~removed, K = 0;
            const uint64_t Dl = diag[lane];
            while (alive) {  // the lowest live candidate is kept and removes what it suppresses
                const int i = __ffsll(static_cast<unsigned long long>(alive)) - 1;
                K |= 1ull << i;
                alive &= ~(1ull << i) & ~__shfl(Dl, i, 64);
            }
            if ((K >> lane) & 1ull) {
                const int slot = kcount + __popcll(K & lanemask_lt());  // < cc <= R
                klist[slot] = j;
                const int r = static_cast<int>(static_cast<uint32_t>(ckey[j]));
                w.krow[obase + slot] = r;
                w.kscore[obase + slot] = pc[r];
                w.kbox[obase + slot] = bj;
            }
            if (lane == 0) s_kcount = kcount + __popcll(K);
        }
        __syncthreads();
        kcount = s_kcount;
    }
    if (tid == 0) w.kcnt[static_cast<size_t>(n) * (C - 1) + (c - 1)] = kcount;
}

// Workgroup (x, n): output slots [x * kEmitSlots, (x+1) * kEmitSlots) of image n.
constexpr int kEmitSlots = 1024;

__global__ __launch_bounds__(256) void det_emit_kernel(int R, int C, int max_det, DetWs w,
                                                       float* __restrict__ det_boxes,
                                                       int32_t* __restrict__ det_labels,
                                                       float* __restrict__ det_scores,
                                                       int32_t* __restrict__ det_roi,
                                                       int32_t* __restrict__ det_count,
                                                       int32_t* __restrict__ det_total) {
    __shared__ int kc[kDetMaxC];    // kc[i]: kept of class i+1
    __shared__ int offs[kDetMaxC];  // offs[i]: detections of classes 1..i; offs[C-1]: all
    const int n = blockIdx.y, tid = threadIdx.x;
    if (tid < C - 1) {
        const int q = w.kcnt[static_cast<size_t>(n) * (C - 1) + tid];
        kc[tid] = q < 0 ? 0 : (q > R ? R : q);
    }
    __syncthreads();
    if (tid < C) {
        int acc = 0;
        for (int i = 0; i < tid; ++i) acc += kc[i];
        offs[tid] = acc;
    }
    __syncthreads();
    const int total = offs[C - 1];
    const int cnt = total < max_det ? total : max_det;
    const int s0 = blockIdx.x * kEmitSlots;
    const int s1 = max_det - s0 < kEmitSlots ? max_det : s0 + kEmitSlots;
    for (int s = s0 + tid; s < s1; s += 256) {
        const size_t o = static_cast<size_t>(n) * max_det + s;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.f;
        int label = -1, row = -1;
        if (s < cnt) {
            int lo = 0, hi = C - 1;  // offs[lo] <= s < offs[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (offs[mid] <= s) lo = mid; else hi = mid;
            }
            const size_t src = (static_cast<size_t>(n) * (C - 1) + lo) * R + (s - offs[lo]);
            b = w.kbox[src];
            sc = w.kscore[src];
            row = w.krow[src];
            label = lo + 1;
        }
        det_boxes[o * 4 + 0] = b.x;
        det_boxes[o * 4 + 1] = b.y;
        det_boxes[o * 4 + 2] = b.z;
        det_boxes[o * 4 + 3] = b.w;
        det_labels[o] = label;
        det_scores[o] = sc;
        det_roi[o] = row;
    }
    if (tid == 0 && blockIdx.x == 0) {
        det_count[n] = cnt;
        det_total[n] = total;
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_detect_workspace_size(int N, int R, int C) {
    if (!det_shape_ok(N, R, C)) return 0;
    return carve_det(nullptr, N, R, C).bytes;
}

namespace frcnn {

template <class E>
static int detect_impl(const char* fn, int N, int R, int C, const float* rois, const int32_t* rcount,
                       const void* cls_v, const void* reg_v, const float* reg_mean, const float* reg_std, float img_h,
                       float img_w, float score_thresh, double nms_thresh, int max_det, float* det_boxes,
                       int32_t* det_labels, float* det_scores, int32_t* det_roi, int32_t* det_count,
                       int32_t* det_total, void* workspace, size_t ws_bytes, void* stream) {
    const typename E::raw* cls = static_cast<const typename E::raw*>(cls_v);
    const typename E::raw* reg = static_cast<const typename E::raw*>(reg_v);
    FRCNN_REQUIRE(N >= 1 && N <= 65535, "%s: N=%d must be in [1, 65535]", fn, N);
    FRCNN_REQUIRE(R >= 1 && R <= kDetMaxR, "%s: R=%d must be in [1, %d]", fn, R, kDetMaxR);
    FRCNN_REQUIRE(C >= 2 && C <= kDetMaxC, "%s: C=%d must be in [2, %d]", fn, C, kDetMaxC);
    FRCNN_REQUIRE(max_det >= 1, "%s: max_det=%d must be >= 1", fn, max_det);
    FRCNN_REQUIRE(static_cast<size_t>(N) * max_det <= (size_t{1} << 30), "%s: N*max_det=%zu over 2^30", fn,
                  static_cast<size_t>(N) * max_det);
    FRCNN_REQUIRE(rois && rcount && cls && reg, "%s: null input (rois / rcount / cls / reg)", fn);
    FRCNN_REQUIRE(reg_mean && reg_std, "%s: null reg_mean / reg_std", fn);
    FRCNN_REQUIRE(aligned_to(cls, sizeof(typename E::raw)) && aligned_to(reg, sizeof(typename E::raw)),
                  "%s: cls / reg not aligned to their element type", fn);
    FRCNN_REQUIRE(det_boxes && det_labels && det_scores && det_roi && det_count && det_total,
                  "%s: null output (det_boxes / det_labels / det_scores / det_roi / det_count / "
                  "det_total)", fn);
    const DetWs w = carve_det(workspace, N, R, C);
    if (!workspace || ws_bytes < w.bytes) {
        set_error("%s: workspace %zu < %zu", fn, workspace ? ws_bytes : size_t{0}, w.bytes);
        return FRCNN_EWORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    DetParams P{};
    P.R = R;
    P.C = C;
    P.img_h = img_h;
    P.img_w = img_w;
    P.score_thresh = score_thresh;
    for (int i = 0; i < 4; ++i) {
        P.mean[i] = reg_mean[i];
        P.std[i] = reg_std[i];
    }
    det_softmax_kernel<E><<<(N * R + kSmRows - 1) / kSmRows, 256, 0, st>>>(cls, rcount, N, R, C, w.prob);
    FRCNN_LAUNCH_CHECK("det_softmax_kernel");
    const int threads = (R + 63) / 64 * 64;
    det_class_nms_kernel<E><<<dim3(C - 1, N), threads, 0, st>>>(P, rois, rcount, reg, make_thr(nms_thresh), w);
    FRCNN_LAUNCH_CHECK("det_class_nms_kernel");
    det_emit_kernel<<<dim3((max_det + kEmitSlots - 1) / kEmitSlots, N), 256, 0, st>>>(
        R, C, max_det, w, det_boxes, det_labels, det_scores, det_roi, det_count, det_total);
    FRCNN_LAUNCH_CHECK("det_emit_kernel");
    return FRCNN_OK;
}

}  // namespace frcnn

extern "C" int frcnn_detect(int N, int R, int C, const float* rois, const int32_t* rcount, const float* cls,
                            const float* reg, const float* reg_mean, const float* reg_std, float img_h,
                            float img_w, float score_thresh, double nms_thresh, int max_det, float* det_boxes,
                            int32_t* det_labels, float* det_scores, int32_t* det_roi, int32_t* det_count,
                            int32_t* det_total, void* workspace, size_t ws_bytes, void* stream) {
    return detect_impl<ElemF32>("frcnn_detect", N, R, C, rois, rcount, cls, reg, reg_mean, reg_std, img_h, img_w,
                                score_thresh, nms_thresh, max_det, det_boxes, det_labels, det_scores, det_roi,
                                det_count, det_total, workspace, ws_bytes, stream);
}

extern "C" int frcnn_detect_t(int dtype, int N, int R, int C, const float* rois, const int32_t* rcount,
                              const void* cls, const void* reg, const float* reg_mean, const float* reg_std,
                              float img_h, float img_w, float score_thresh, double nms_thresh, int max_det,
                              float* det_boxes, int32_t* det_labels, float* det_scores, int32_t* det_roi,
                              int32_t* det_count, int32_t* det_total, void* workspace, size_t ws_bytes, void* stream) {
    FRCNN_REQUIRE(dtype_code_ok(dtype), "frcnn_detect_t: dtype code %d is not FRCNN_F32, FRCNN_F16 or FRCNN_BF16",
                  dtype);
    if (dtype == FRCNN_F32)
        return frcnn_detect(N, R, C, rois, rcount, static_cast<const float*>(cls), static_cast<const float*>(reg),
                            reg_mean, reg_std, img_h, img_w, score_thresh, nms_thresh, max_det, det_boxes, det_labels,
                            det_scores, det_roi, det_count, det_total, workspace, ws_bytes, stream);
    if (dtype == FRCNN_F16)
        return detect_impl<ElemF16>("frcnn_detect_t", N, R, C, rois, rcount, cls, reg, reg_mean, reg_std, img_h,
                                    img_w, score_thresh, nms_thresh, max_det, det_boxes, det_labels, det_scores,
                                    det_roi, det_count, det_total, workspace, ws_bytes, stream);
    return detect_impl<ElemBF16>("frcnn_detect_t", N, R, C, rois, rcount, cls, reg, reg_mean, reg_std, img_h, img_w,
                                 score_thresh, nms_thresh, max_det, det_boxes, det_labels, det_scores, det_roi,
                                 det_count, det_total, workspace, ws_bytes, stream);
}
