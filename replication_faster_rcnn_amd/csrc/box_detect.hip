// Pyramid box-head inference on gfx950: torchvision's RoIHeads.postprocess_detections
// (softmax, BoxCoder.decode, clip_boxes_to_image, score_thresh, remove_small_boxes, class-wise
// NMS, the best detections_per_img by score) and GeneralizedRCNNTransform.postprocess's
// resize_boxes for a whole batch (DESIGN.md §3 "Pyramid box-head inference"; include/frcnn_capi.h
// states the contract).  Three launches, no host synchronisation:
//   bd_score_kernel<Elem>      sixteen rows per workgroup, one thread per logit for the
//       fp64-backed exp_cr, one thread per row for the max and the ordered sum (ops.detect's
//       softmax rule); probabilities p [N, C, R], class-major, stored row-fastest.
//   bd_class_nms_kernel<Elem, Q>  one workgroup per (image, class), gone at once when the class
//       has no candidate: ballot / prefix compaction of the rows over the score threshold, an
//       LDS bitonic sort of the distinct (score descending, row) keys, decode + clip + size
//       filter of the candidates only, the greedy sweep in 64-candidate blocks of detect.hip.
//       Q = 1 ("rows": R <= 1,024, thread r owns row r) or 4 ("strided": 1,024 threads, thread
//       t owns rows t, t + 1024, ...).  The kept rows go to the (image, class) list.
//   bd_merge_kernel<Elem>      one workgroup per image: exact radix select (radix_select.h) of
//       the D-th (score key, flat index) over the kept lists, an LDS sort of at most D keys,
//       then the gather: the box of a winner is decoded again (the same function, the same
//       bits), rescaled if asked, and every output element is stored once, padding included.
// The workspace holds p and the kept rows (16 bits each) only.  Every workspace word a kernel
// reads was written by an earlier kernel of the same call; the only atomics are integer ones
// on LDS whose results are order-free (histogram counts, slots of keys that are sorted next).
#include <cmath>

#include "common.h"
#include "elem16.h"
#include "nms_iou.h"
#include "radix_select.h"

namespace frcnn {
namespace {

constexpr int kBdMaxN = 1024;
constexpr int kBdMaxR = 4096;
constexpr int kBdMaxC = 128;
constexpr int kBdMaxD = 1024;
constexpr int kBdRowsR = 1024;     // the largest R of the "rows" branch
constexpr int kBdScoreRows = 16;   // rows per workgroup of bd_score_kernel
constexpr int kBdStage = 2048;     // merge: an image's keys are staged in LDS up to this many
constexpr int kBdBins = 4096;
constexpr int kBdThreads = 1024;
constexpr uint32_t kBdBad = 0x80000000u;  // low word of a sorted key: the box failed the size filter

struct BdWs {
    float* prob;      // [N, C, R]
    uint16_t* krow;   // [N, C-1, R] kept rows, sweep order
    int32_t* kcnt;    // [N, C-1]
    size_t bytes;
};

BdWs bd_carve(void* ws, int N, int R, int C) {
    Carver c(ws);
    BdWs w{};
    const size_t rows = static_cast<size_t>(N) * R;
    w.prob = c.take<float>(rows * C);
    w.krow = c.take<uint16_t>(rows * (C - 1));
    w.kcnt = c.take<int32_t>(static_cast<size_t>(N) * (C - 1));
    w.bytes = c.used();
    return w;
}

struct BdParams {
    int R, C, D;
    float score_thresh, min_size, dclip;
    float wx, wy, ww, wh;
};

__device__ __forceinline__ int bd_valid_rows(const int32_t* pcount, int n, int R) {
    const int k = pcount[n];
    return k < 0 ? 0 : (k > R ? R : k);
}

// p_c = e_c * (1 / s), e_c = exp_cr(x_c - max x), s summed in ascending class order: the rule
// of det_softmax_kernel (detect.hip).  Rows are padded to C + 1 words in LDS so that the
// per-row threads do not share a bank.
template <class E>
__global__ __launch_bounds__(256) void bd_score_kernel(const typename E::raw* __restrict__ logits,
                                                       const int32_t* __restrict__ pcount, int N, int R, int C,
                                                       float* __restrict__ prob) {
    __shared__ float xs[kBdScoreRows * (kBdMaxC + 1)];
    __shared__ float rm[kBdScoreRows];  // the row's max, then 1 / its sum
    const int tid = threadIdx.x;
    const int S = C + 1;
    const int row0 = blockIdx.x * kBdScoreRows;
    const int nrow = min(kBdScoreRows, N * R - row0);
    const int ne = nrow * C;
    const typename E::raw* x = logits + static_cast<size_t>(row0) * C;
    for (int i = tid; i < ne; i += 256) {
        const int row = i / C;
        xs[row * S + (i - row * C)] = E::widen(x[i]);
    }
    __syncthreads();
    if (tid < nrow) {
        const float* v = xs + tid * S;
        float m = v[0];
        for (int c = 1; c < C; ++c) m = v[c] > m ? v[c] : m;  // a NaN logit leaves m or makes e NaN: the row is NaN either way
        rm[tid] = m;
    }
    __syncthreads();
    for (int i = tid; i < ne; i += 256) {
        const int row = i / C;
        const int at = row * S + (i - row * C);
        xs[at] = exp_cr(xs[at] - rm[row]);
    }
    __syncthreads();
    if (tid < nrow) {
        const float* v = xs + tid * S;
        float s = v[0];
        for (int c = 1; c < C; ++c) s = s + v[c];
        rm[tid] = 1.0f / s;
    }
    __syncthreads();
    for (int i = tid; i < ne; i += 256) {  // row-fastest: a class's stores are consecutive
        const int c = i / nrow, row = i - c * nrow;
        const int g = row0 + row;
        const int n = g / R, r = g - n * R;
        if (r < bd_valid_rows(pcount, n, R)) prob[(static_cast<size_t>(n) * C + c) * R + r] = xs[row * S + c] * rm[row];
    }
}

// BoxCoder.decode_single for class c of one row, clip_boxes_to_image, remove_small_boxes:
// fp32, every operation rounded separately, '/' correctly rounded.  False: the box is dropped
// (a NaN side fails both comparisons).
template <class E>
__device__ __forceinline__ bool bd_decode(const BdParams& P, const float* __restrict__ a,
                                          const typename E::raw* __restrict__ d, float img_h, float img_w, float4& out) {
    const float x1 = a[0], y1 = a[1], x2 = a[2], y2 = a[3];
    const float w = x2 - x1, h = y2 - y1;
    const float cx = x1 + 0.5f * w, cy = y1 + 0.5f * h;
    const float dx = E::widen(d[0]) / P.wx, dy = E::widen(d[1]) / P.wy;
    float dw = E::widen(d[2]) / P.ww, dh = E::widen(d[3]) / P.wh;
    dw = dw > P.dclip ? P.dclip : dw;  // torch.clamp(max=): NaN stays
    dh = dh > P.dclip ? P.dclip : dh;
    float pcx = dx * w;
    pcx = pcx + cx;
    float pcy = dy * h;
    pcy = pcy + cy;
    const float pw = exp_cr(dw) * w, ph = exp_cr(dh) * h;
    const float hw = 0.5f * pw, hh = 0.5f * ph;
    float4 b = make_float4(pcx - hw, pcy - hh, pcx + hw, pcy + hh);
    b.x = clamp_nan(b.x, 0.0f, img_w);
    b.z = clamp_nan(b.z, 0.0f, img_w);
    b.y = clamp_nan(b.y, 0.0f, img_h);
    b.w = clamp_nan(b.w, 0.0f, img_h);
    out = b;
    return (b.z - b.x >= P.min_size) && (b.w - b.y >= P.min_size);
}

// Q = 1: blockDim.x = R rounded up to whole waves; Q = 4: blockDim.x = 1024.  Thread t owns
// rows t + q * blockDim.x, q < Q.
template <class E, int Q>
__global__ __launch_bounds__(kBdThreads) void bd_class_nms_kernel(BdParams P, const float* __restrict__ proposals,
                                                                   const int32_t* __restrict__ pcount,
                                                                   const typename E::raw* __restrict__ reg,
                                                                   const float* __restrict__ img_sizes, NmsThr thr,
                                                                   BdWs w) {
    constexpr int kCap = Q * 1024;
    __shared__ uint64_t ckey[kCap];   // (desc_score_key << 32) | row, sorted; kBdBad set by the decode
    __shared__ float4 cbox[kCap];     // decoded boxes, sorted order
    __shared__ uint16_t klist[kCap];  // kept candidates (sorted positions), keep order
    __shared__ uint64_t diag[64];     // the block's own mask: bit j of row i = "i suppresses j", j > i
    __shared__ uint64_t red[16];
    __shared__ int wcnt[Q][16];
    __shared__ int s_kcount;

    const int c = blockIdx.x + 1, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nt = blockDim.x, nw = nt >> 6;
    const int R = P.R, C = P.C;
    const int k = bd_valid_rows(pcount, n, R);
    const float* pc = w.prob + (static_cast<size_t>(n) * C + c) * R;
    const size_t obase = (static_cast<size_t>(n) * (C - 1) + (c - 1)) * R;

    // ---- candidates (NaN > thresh is false), compacted per (q, wave, lane)
    float p[Q];
    bool cand[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int r = q * nt + tid;
        p[q] = 0.0f;
        cand[q] = false;
        if (r < k) {
            p[q] = pc[r];
            cand[q] = p[q] > P.score_thresh;
        }
        const uint64_t bal = __ballot(cand[q]);
        if (lane == 0) wcnt[q][wid] = __popcll(bal);
    }
    __syncthreads();
    int cc = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        int off = cc;
        for (int v = 0; v < nw; ++v) {
            const int cnt = wcnt[q][v];
            off += v < wid ? cnt : 0;
            cc += cnt;
        }
        const uint64_t bal = __ballot(cand[q]);
        if (cand[q])  // off + ... < cc <= k <= R <= kCap
            ckey[off + __popcll(bal & lanemask_lt())] =
                (static_cast<uint64_t>(desc_score_key(p[q])) << 32) | static_cast<uint32_t>(q * nt + tid);
    }
    if (cc == 0) {  // uniform: nearly every class of a real head
        if (tid == 0) w.kcnt[static_cast<size_t>(n) * (C - 1) + (c - 1)] = 0;
        return;
    }

    // ---- bitonic sort, ascending: score descending, row ascending (keys are distinct)
    int ns = 64;
    while (ns < cc) ns <<= 1;  // <= kCap
    for (int i = cc + tid; i < ns; i += nt) ckey[i] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= ns; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < ns; i += nt) {
                const int o = i ^ j;
                if (o > i) {
                    const uint64_t a = ckey[i], b = ckey[o];
                    if ((a > b) == ((i & kk) == 0)) {
                        ckey[i] = b;
                        ckey[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- decode the candidates in score order; a dropped box keeps its place, flagged
    const float img_h = img_sizes[2 * n], img_w = img_sizes[2 * n + 1];
    for (int j = tid; j < cc; j += nt) {
        const int r = min(static_cast<int>(static_cast<uint32_t>(ckey[j])), R - 1);
        float4 b;
        const bool ok = bd_decode<E>(P, proposals + (static_cast<size_t>(n) * R + r) * 4,
                                     reg + (static_cast<size_t>(n) * R + r) * 4 * C + 4 * c, img_h, img_w, b);
        cbox[j] = b;
        if (!ok) ckey[j] |= kBdBad;
    }
    __syncthreads();

    // ---- greedy NMS over 64-candidate blocks, in score order (detect.hip's sweep)
    int kcount = 0;
    const int nb = (cc + 63) >> 6;
#pragma unroll 1
    for (int blk = 0; blk < nb; ++blk) {
        const int j = blk * 64 + lane;
        const bool jv = j < cc && !(static_cast<uint32_t>(ckey[j < cc ? j : 0]) & kBdBad);
        float4 bj = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jv) bj = cbox[j];
        const float aj = box_area(bj);
        bool sup = false;  // by a box kept in an earlier block
        if (jv && !thr.never)
            for (int i = wid; i < kcount; i += nw) {
                const float4 bi = cbox[klist[i]];
                if (iou_over(bi, box_area(bi), bj, aj, thr)) {
                    sup = true;
                    break;
                }
            }
        const uint64_t supm = __ballot(sup);
        if (lane == 0) red[wid] = supm;
        for (int r = wid; r < 64; r += nw) {
            const int ia = blk * 64 + r;
            bool bit = false;
            if (jv && lane > r && ia < cc && !thr.never) {
                const float4 bi = cbox[ia];
                bit = iou_over(bi, box_area(bi), bj, aj, thr);
            }
            const uint64_t D = __ballot(bit);
            if (lane == 0) diag[r] = D;
        }
        __syncthreads();
        if (wid == 0) {
            uint64_t removed = 0;
            for (int v = 0; v < nw; ++v) removed |= red[v];
            uint64_t alive = __ballot(jv) & ~removed, K = 0;
            const uint64_t Dl = diag[lane];
            while (alive) {  // the lowest live candidate is kept and removes what it suppresses
                const int i = __ffsll(static_cast<unsigned long long>(alive)) - 1;
                K |= 1ull << i;
                alive &= ~(1ull << i) & ~__shfl(Dl, i, 64);
            }
            if ((K >> lane) & 1ull) {
                const int slot = kcount + __popcll(K & lanemask_lt());  // < cc <= R
                klist[slot] = static_cast<uint16_t>(j);
                w.krow[obase + slot] = static_cast<uint16_t>(static_cast<uint32_t>(ckey[j]));
            }
            if (lane == 0) s_kcount = kcount + __popcll(K);
        }
        __syncthreads();
        kcount = s_kcount;
    }
    if (tid == 0) w.kcnt[static_cast<size_t>(n) * (C - 1) + (c - 1)] = kcount;
}

struct BdMergeShared {
    RadixBin bin;
    unsigned ccount;
    unsigned wsum[16];
};

// Key e of image n's kept boxes, classes concatenated: (desc_score_key(p) << 32) | flat index
// r * (C-1) + (c-1).  offs[i] = kept of classes 1..i.
__device__ __forceinline__ uint64_t bd_kept_key(const BdWs& w, const int* offs, int n, int R, int C, int e) {
    int lo = 0, hi = C - 1;  // offs[lo] <= e < offs[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= e) lo = mid; else hi = mid;
    }
    const int r = min(static_cast<int>(w.krow[(static_cast<size_t>(n) * (C - 1) + lo) * R + (e - offs[lo])]), R - 1);
    const float p = w.prob[(static_cast<size_t>(n) * C + lo + 1) * R + r];
    return (static_cast<uint64_t>(desc_score_key(p)) << 32) | static_cast<uint32_t>(r * (C - 1) + lo);
}

template <class E>
__global__ __launch_bounds__(kBdThreads) void bd_merge_kernel(BdParams P, const float* __restrict__ proposals,
                                                               const typename E::raw* __restrict__ reg,
                                                               const float* __restrict__ img_sizes,
                                                               const float* __restrict__ orig_sizes, BdWs w,
                                                               float4* __restrict__ boxes, int32_t* __restrict__ labels,
                                                               float* __restrict__ scores, int32_t* __restrict__ roi,
                                                               int32_t* __restrict__ count, int32_t* __restrict__ total_out) {
    __shared__ unsigned hist[kBdBins];
    __shared__ uint64_t stage[kBdStage];
    __shared__ uint64_t skey[kBdMaxD];
    __shared__ int kc[kBdMaxC];
    __shared__ int offs[kBdMaxC];
    __shared__ BdMergeShared sh;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int R = P.R, C = P.C, D = P.D;
    if (tid < C - 1) {
        const int q = w.kcnt[static_cast<size_t>(n) * (C - 1) + tid];
        kc[tid] = q < 0 ? 0 : (q > R ? R : q);
    }
    if (tid == 0) sh.ccount = 0;
    __syncthreads();
    if (tid < C) {
        int acc = 0;
        for (int i = 0; i < tid; ++i) acc += kc[i];
        offs[tid] = acc;
    }
    __syncthreads();
    const int total = offs[C - 1];
    const bool staged = total <= kBdStage;
    if (staged) {
        for (int e = tid; e < total; e += kBdThreads) stage[e] = bd_kept_key(w, offs, n, R, C, e);
        __syncthreads();
    }

    // ---- T: the D-th smallest key (digits 12/12/8 of the score, 12/12 of the index)
    uint64_t T = ~0ull;
    if (total > D) {
        uint64_t prefix = 0, hm = 0;
        unsigned need = static_cast<unsigned>(D);
#pragma unroll 1
        for (int pass = 0; pass < 5; ++pass) {
            const int width = pass == 2 ? 8 : 12;
            const int shift = pass == 0 ? 52 : pass == 1 ? 40 : pass == 2 ? 32 : pass == 3 ? 12 : 0;
            const int nbins = 1 << width;
            for (int i = tid; i < nbins; i += kBdThreads) hist[i] = 0;
            __syncthreads();
            for (int e = tid; e < total; e += kBdThreads) {
                const uint64_t key = staged ? stage[e] : bd_kept_key(w, offs, n, R, C, e);
                if ((key & hm) == prefix) atomicAdd(&hist[static_cast<unsigned>(key >> shift) & (nbins - 1)], 1u);
            }
            __syncthreads();
            hist_find(hist, nbins, need, sh.bin, sh.wsum);
            need -= sh.bin.before;
            prefix |= static_cast<uint64_t>(sh.bin.digit) << shift;
            hm = ~0ull << shift;
            T = prefix | ((1ull << shift) - 1ull);
            const bool whole = sh.bin.bucket == need;  // every key of the bucket is selected
            __syncthreads();                           // sh.* consumed before the next pass rewrites them
            if (whole) break;
        }
    }
    const int cnt = total < D ? total : D;
    for (int e = tid; e < total; e += kBdThreads) {
        const uint64_t key = staged ? stage[e] : bd_kept_key(w, offs, n, R, C, e);
        if (key <= T) {
            const unsigned at = atomicAdd(&sh.ccount, 1u);
            if (at < static_cast<unsigned>(kBdMaxD)) skey[at] = key;  // exactly cnt keys: they are distinct
        }
    }
    int ns = 64;
    while (ns < cnt) ns <<= 1;  // <= kBdMaxD
    for (int i = cnt + tid; i < ns; i += kBdThreads) skey[i] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= ns; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (tid < ns) {
                const int o = tid ^ j;
                if (o > tid) {
                    const uint64_t a = skey[tid], b = skey[o];
                    if ((a > b) == ((tid & kk) == 0)) {
                        skey[tid] = b;
                        skey[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- gather, rescale, padding
    const float img_h = img_sizes[2 * n], img_w = img_sizes[2 * n + 1];
    float ratio_h = 1.0f, ratio_w = 1.0f;
    if (orig_sizes) {
        ratio_h = orig_sizes[2 * n] / img_h;
        ratio_w = orig_sizes[2 * n + 1] / img_w;
    }
    if (tid < D) {
        const size_t o = static_cast<size_t>(n) * D + tid;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.f;
        int label = -1, row = -1;
        if (tid < cnt) {
            const uint32_t flat = static_cast<uint32_t>(skey[tid]);
            const int r = min(static_cast<int>(flat / static_cast<uint32_t>(C - 1)), R - 1);
            const int c = static_cast<int>(flat - static_cast<uint32_t>(r) * (C - 1)) + 1;
            bd_decode<E>(P, proposals + (static_cast<size_t>(n) * R + r) * 4,
                         reg + (static_cast<size_t>(n) * R + r) * 4 * C + 4 * c, img_h, img_w, b);
            if (orig_sizes) {
                b.x = b.x * ratio_w;
                b.z = b.z * ratio_w;
                b.y = b.y * ratio_h;
                b.w = b.w * ratio_h;
            }
            sc = w.prob[(static_cast<size_t>(n) * C + c) * R + r];
            label = c;
            row = r;
        }
        boxes[o] = b;
        labels[o] = label;
        scores[o] = sc;
        roi[o] = row;
    }
    if (tid == 0) {
        count[n] = cnt;
        total_out[n] = total;
    }
}

int bd_check_shape(const char* who, int N, int R, int C, int D) {
    FRCNN_REQUIRE(N >= 1 && N <= kBdMaxN, "%s: N must be in [1, %d], got %d", who, kBdMaxN, N);
    FRCNN_REQUIRE(R >= 1 && R <= kBdMaxR, "%s: R must be in [1, %d], got %d", who, kBdMaxR, R);
    FRCNN_REQUIRE(C >= 2 && C <= kBdMaxC, "%s: C must be in [2, %d], got %d", who, kBdMaxC, C);
    FRCNN_REQUIRE(D >= 1 && D <= kBdMaxD, "%s: detections_per_img must be in [1, %d], got %d", who, kBdMaxD, D);
    return FRCNN_OK;
}

const char* bd_elem_name(int dtype) { return dtype == FRCNN_F32 ? "ElemF32" : dtype == FRCNN_F16 ? "ElemF16" : "ElemBF16"; }

template <class E>
int bd_launch(const BdParams& P, int N, const void* logits_v, const void* reg_v, const float* proposals,
              const int32_t* pcount, const float* img_sizes, const float* orig_sizes, double nms_thresh, const BdWs& w,
              float* boxes, int32_t* labels, float* scores, int32_t* roi, int32_t* count, int32_t* total,
              hipStream_t st) {
    using raw = typename E::raw;
    const raw* logits = static_cast<const raw*>(logits_v);
    const raw* reg = static_cast<const raw*>(reg_v);
    const int R = P.R, C = P.C;
    hipLaunchKernelGGL((bd_score_kernel<E>), dim3((N * R + kBdScoreRows - 1) / kBdScoreRows), dim3(256), 0, st, logits,
                       pcount, N, R, C, w.prob);
    FRCNN_LAUNCH_CHECK("bd_score_kernel");
    const NmsThr thr = make_thr(nms_thresh);
    if (R <= kBdRowsR)
        hipLaunchKernelGGL((bd_class_nms_kernel<E, 1>), dim3(C - 1, N), dim3((R + 63) / 64 * 64), 0, st, P, proposals,
                           pcount, reg, img_sizes, thr, w);
    else
        hipLaunchKernelGGL((bd_class_nms_kernel<E, 4>), dim3(C - 1, N), dim3(kBdThreads), 0, st, P, proposals, pcount,
                           reg, img_sizes, thr, w);
    FRCNN_LAUNCH_CHECK("bd_class_nms_kernel");
    hipLaunchKernelGGL((bd_merge_kernel<E>), dim3(N), dim3(kBdThreads), 0, st, P, proposals, reg, img_sizes, orig_sizes,
                       w, reinterpret_cast<float4*>(boxes), labels, scores, roi, count, total);
    FRCNN_LAUNCH_CHECK("bd_merge_kernel");
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_box_detections_workspace_size(int N, int R, int C) {
    if (bd_check_shape("frcnn_box_detections_workspace_size", N, R, C, 1)) return 0;
    return bd_carve(nullptr, N, R, C).bytes;
}

extern "C" int frcnn_box_detections_kernel(int dtype, int R, int C, int detections_per_img, char* name, size_t len) {
    const char* who = "frcnn_box_detections_kernel";
    FRCNN_REQUIRE(name && len > 0, "%s: null name buffer", who);
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int rc = bd_check_shape(who, 1, R, C, detections_per_img);
    if (rc) return rc;
    const char* e = bd_elem_name(dtype);
    std::snprintf(name, len, "bd_score_kernel<%s> bd_class_nms_kernel<%s,%d>[%s] bd_merge_kernel<%s>", e, e,
                  R <= kBdRowsR ? 1 : 4, R <= kBdRowsR ? "rows" : "strided", e);
    return FRCNN_OK;
}

extern "C" int frcnn_box_detections_t(int dtype, int N, int R, int C, const void* class_logits,
                                      const void* box_regression, const float* proposals, const int32_t* prop_count,
                                      const float* image_sizes, const float* original_sizes, float score_thresh,
                                      double nms_thresh, int detections_per_img, float min_size, float wx, float wy,
                                      float ww, float wh, float* boxes, int32_t* labels, float* scores, int32_t* roi,
                                      int32_t* count, int32_t* total, void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "frcnn_box_detections_t";
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int rc = bd_check_shape(who, N, R, C, detections_per_img);
    if (rc) return rc;
    FRCNN_REQUIRE(wx > 0.0f && wx <= FLT_MAX && wy > 0.0f && wy <= FLT_MAX && ww > 0.0f && ww <= FLT_MAX && wh > 0.0f &&
                      wh <= FLT_MAX,
                  "%s: reg_weights must be four finite positive numbers, got (%g, %g, %g, %g)", who, wx, wy, ww, wh);
    FRCNN_REQUIRE(class_logits && box_regression && proposals && prop_count && image_sizes,
                  "%s: null input (class_logits / box_regression / proposals / prop_count / image_sizes)", who);
    const size_t esz = dtype == FRCNN_F32 ? 4 : 2;
    FRCNN_REQUIRE(aligned_to(class_logits, esz) && aligned_to(box_regression, esz),
                  "%s: class_logits / box_regression not aligned to their element type", who);
    FRCNN_REQUIRE(boxes && labels && scores && roi && count && total,
                  "%s: null output (boxes / labels / scores / roi / count / total)", who);
    FRCNN_REQUIRE(aligned_to(boxes, 16), "%s: boxes must be 16-byte aligned", who);
    const BdWs w = bd_carve(workspace, N, R, C);
    if (!workspace || ws_bytes < w.bytes) {
        set_error("%s: workspace %zu < %zu", who, workspace ? ws_bytes : size_t{0}, w.bytes);
        return FRCNN_EWORKSPACE;
    }
    FRCNN_REQUIRE(aligned_to(workspace, 256), "%s: workspace must be 256-byte aligned", who);
    BdParams P{};
    P.R = R;
    P.C = C;
    P.D = detections_per_img;
    P.score_thresh = score_thresh;
    P.min_size = min_size;
    P.dclip = static_cast<float>(std::log(1000.0 / 16.0));  // torchvision's bbox_xform_clip
    P.wx = wx;
    P.wy = wy;
    P.ww = ww;
    P.wh = wh;
    hipStream_t st = as_stream(stream);
    if (dtype == FRCNN_F32)
        return bd_launch<ElemF32>(P, N, class_logits, box_regression, proposals, prop_count, image_sizes, original_sizes,
                                  nms_thresh, w, boxes, labels, scores, roi, count, total, st);
    if (dtype == FRCNN_F16)
        return bd_launch<ElemF16>(P, N, class_logits, box_regression, proposals, prop_count, image_sizes, original_sizes,
                                  nms_thresh, w, boxes, labels, scores, roi, count, total, st);
    return bd_launch<ElemBF16>(P, N, class_logits, box_regression, proposals, prop_count, image_sizes, original_sizes,
                               nms_thresh, w, boxes, labels, scores, roi, count, total, st);
}
