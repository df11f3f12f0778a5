// VOC detection evaluation: detections x ground truth -> TP / FP / ignored
// records, and per-class AP / mAP from the accumulated records.
//
// The reference has no counterpart (its test_eval.py is an empty file); the
// contract is the VOC devkit's voc_eval in this project's arithmetic, written
// out in DESIGN.md "Evaluation".
//   eval_match_kernel   : one workgroup per image.  The image's gt (fp64 boxes
//                         with the pixel convention applied, area, label,
//                         difficult) are staged in LDS; the workgroup walks the
//                         detection slots in chunks of its size, twice.  Pass
//                         one: thread = slot, fp64 IoU against the gt of the
//                         slot's class, 64-bit LDS atomic-min of the claim key
//                         (desc_score_key << 32 | slot) on the best gt.  Pass
//                         two recomputes the best gt (same arithmetic, same
//                         answer), reads the winning claim and writes the three
//                         record arrays, one record per slot, coalesced.  The
//                         records' base is hdr[0] plus the prefix of the clamped
//                         counts, both read by every workgroup.
//   eval_advance_kernel : the header step, in stream order behind every
//                         workgroup of the match kernel: records / images
//                         advance, or the dropped-batch count grows.
//   eval_sort_*_kernel  : stable LSD radix sort of the record keys over bits
//                         24..63 (class and score; the low 24 bits are the
//                         insertion order the input already has), five 8-bit
//                         passes of histogram / scan / scatter.
//   eval_ap_kernel      : one workgroup per class: its segment of the sorted
//                         keys by binary search on the class field, then
//                         ev_pr_walk (eval_common.h: the tp / fp totals and one
//                         pass from the last record to the first with running
//                         tp / fp and the suffix maximum of the precision),
//                         integrating at each record.
//   eval_map_kernel     : mean of the non-NaN APs in ascending class order.
//   frcnn_eval_plan     : host only: the chunk, tile and scan numbers of the launches above for
//                         a shape, from the constants and functions they read (eval_common.h).
// The limits, the header step, the walk and the sort's host entry
// (eval_sort_keys) are shared with the COCO-style evaluation (eval_common.h, eval_coco.hip).
// Integer atomics only (LDS claim minima, npos counts): every result is
// independent of the order workgroups and waves run in.
#include <cmath>

#include "eval_common.h"

namespace frcnn {

// np.maximum / np.minimum (NaN propagates), as bbox_iou uses them.
__device__ __forceinline__ double ev_max(double a, double b) { return (a != a || a >= b) ? a : b; }
__device__ __forceinline__ double ev_min(double a, double b) { return (a != a || a <= b) ? a : b; }

// utils/utils.py:102-119 in fp64, every op separately rounded (targets.hip's iou_np).
__device__ __forceinline__ double ev_iou(const double* a, double area_a, const double* b, double area_b) {
    const double tl0 = ev_max(a[0], b[0]);
    const double tl1 = ev_max(a[1], b[1]);
    const double br0 = ev_min(a[2], b[2]);
    const double br1 = ev_min(a[3], b[3]);
    double inter = (br0 - tl0) * (br1 - tl1);
    inter = inter * ((tl0 < br0 && tl1 < br1) ? 1.0 : 0.0);
    double uni = area_a + area_b;
    uni = uni - inter;
    return inter / uni;
}

struct EvGt {
    double box[kEvMaxG][4];  // columns 2, 3 already carry the pixel convention's +1
    double area[kEvMaxG];
    int label[kEvMaxG];  // 0 for a row that is not a valid gt
    unsigned char difficult[kEvMaxG];
};

// The gt a detection is matched to: strict > maximum from -inf over j ascending
// (a NaN IoU never wins, a tie stays with the first gt), matched when the
// maximum is strictly over the threshold.  -1: not matched.
__device__ __forceinline__ int ev_best_gt(const float* db, int label, int G, const EvGt& gt, int plus_one,
                                          double thr) {
    double a[4] = {static_cast<double>(db[0]), static_cast<double>(db[1]), static_cast<double>(db[2]),
                   static_cast<double>(db[3])};
    if (plus_one) {
        a[2] = a[2] + 1.0;
        a[3] = a[3] + 1.0;
    }
    const double area_a = (a[2] - a[0]) * (a[3] - a[1]);
    double ovmax = -INFINITY;
    int jmax = -1;
    for (int j = 0; j < G; ++j) {
        if (gt.label[j] != label) continue;
        const double ov = ev_iou(a, area_a, gt.box[j], gt.area[j]);
        if (ov > ovmax) {
            ovmax = ov;
            jmax = j;
        }
    }
    return (ovmax > thr) ? jmax : -1;
}

__global__ __launch_bounds__(kEvThreads) void eval_match_kernel(
    int N, int M, int G, int C, long long cap, const float* __restrict__ det_boxes,
    const int32_t* __restrict__ det_labels, const float* __restrict__ det_scores,
    const int32_t* __restrict__ det_count, const double* __restrict__ gt_boxes,
    const int32_t* __restrict__ gt_labels, const uint8_t* __restrict__ gt_difficult, double thr, int plus_one,
    long long* hdr, uint64_t* __restrict__ rec_key, int8_t* __restrict__ rec_flag,
    int32_t* __restrict__ rec_image) {
    __shared__ EvGt gt;
    __shared__ unsigned long long claim[kEvMaxG];
    __shared__ unsigned int cpos[kEvMaxC];
    __shared__ long long red[2 * kEvWaves];

    const int n = blockIdx.x, tid = threadIdx.x;
    const long long nrec = hdr[0], nimg = hdr[1];
    long long before, total;
    ev_count_sums(det_count, N, M, n, red, &before, &total);
    if (!ev_fits(nrec, total, cap)) return;

    if (tid < kEvMaxC) cpos[tid] = 0;
    if (tid < G) {  // G <= kEvMaxG == kEvThreads
        const size_t g = static_cast<size_t>(n) * G + tid;
        const int l = gt_labels[g];
        const bool valid = l >= 1 && l < C;
        const double* b = gt_boxes + g * 4;
        double b2 = b[2], b3 = b[3];
        if (plus_one) {
            b2 = b2 + 1.0;
            b3 = b3 + 1.0;
        }
        gt.box[tid][0] = b[0];
        gt.box[tid][1] = b[1];
        gt.box[tid][2] = b2;
        gt.box[tid][3] = b3;
        gt.area[tid] = (b2 - b[0]) * (b3 - b[1]);
        gt.label[tid] = valid ? l : 0;
        gt.difficult[tid] = (gt_difficult && gt_difficult[g]) ? 1 : 0;
        claim[tid] = ~0ull;
    }
    __syncthreads();
    if (tid < G && gt.label[tid] && !gt.difficult[tid]) atomicAdd(&cpos[gt.label[tid]], 1u);
    __syncthreads();
    if (tid < C && cpos[tid])
        atomicAdd(reinterpret_cast<unsigned long long*>(hdr + 4 + tid), static_cast<unsigned long long>(cpos[tid]));

    const int k = ev_count(det_count, n, M);
    const size_t row = static_cast<size_t>(n) * M;
    // ---- pass one: every detection claims its gt; the minimum key is the first claimant
    for (int s0 = 0; s0 < k; s0 += kEvThreads) {
        const int s = s0 + tid;
        if (s >= k) continue;
        const int label = det_labels[row + s];
        if (label < 1 || label >= C) continue;
        const int j = ev_best_gt(det_boxes + (row + s) * 4, label, G, gt, plus_one, thr);
        if (j >= 0 && !gt.difficult[j])
            atomicMin(&claim[j], (static_cast<unsigned long long>(desc_score_key(det_scores[row + s])) << 32) |
                                     static_cast<unsigned int>(s));
    }
    __syncthreads();
    // ---- pass two: flags and records
    const long long rbase = nrec + before;  // rbase + k <= nrec + total <= cap
    for (int s0 = 0; s0 < k; s0 += kEvThreads) {
        const int s = s0 + tid;
        if (s >= k) continue;
        const int label = det_labels[row + s];
        const uint32_t skey = desc_score_key(det_scores[row + s]);
        int cls = 0, flag = -1;
        if (label >= 1 && label < C) {
            cls = label;
            const int j = ev_best_gt(det_boxes + (row + s) * 4, label, G, gt, plus_one, thr);
            if (j < 0)
                flag = 0;
            else if (gt.difficult[j])
                flag = -1;
            else
                flag = claim[j] == ((static_cast<unsigned long long>(skey) << 32) | static_cast<unsigned int>(s)) ? 1
                                                                                                                 : 0;
        }
        const long long r = rbase + s;
        rec_key[r] = (static_cast<uint64_t>(cls) << 56) | (static_cast<uint64_t>(skey) << 24) |
                     static_cast<uint64_t>(r);
        rec_flag[r] = static_cast<int8_t>(flag);
        rec_image[r] = static_cast<int32_t>(nimg + n);
    }
}

__global__ __launch_bounds__(kEvThreads) void eval_advance_kernel(int N, int M, long long cap,
                                                                  const int32_t* __restrict__ det_count,
                                                                  long long* hdr) {
    __shared__ long long red[2 * kEvWaves];
    ev_advance(N, M, cap, det_count, hdr, red);
}

// ----------------------------------------------------------------------- sort
// The sort's constants, its tile count (ev_sort_blocks) and the scan's share per thread
// (ev_scan_share) are in eval_common.h.
// hist[d * nblk + b]: keys of workgroup b's tile with digit d.
__global__ __launch_bounds__(kEvThreads) void eval_sort_hist_kernel(const uint64_t* __restrict__ in, int n, int shift,
                                                                    int nblk, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kSortBins];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * kSortTile;
    const int end = min(n, base + kSortTile);
    for (int i = base + tid; i < end; i += kEvThreads) atomicAdd(&h[(in[i] >> shift) & (kSortBins - 1)], 1u);
    __syncthreads();
    hist[static_cast<size_t>(tid) * nblk + blockIdx.x] = h[tid];
}

// In-place exclusive scan of hist[0 .. len): one workgroup, a contiguous share per thread.
__global__ __launch_bounds__(kScanThreads) void eval_sort_scan_kernel(uint32_t* __restrict__ hist, int len) {
    __shared__ uint32_t wsum[kScanThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int per = ev_scan_share(len);
    const int lo = min(len, tid * per), hi = min(len, lo + per);
    uint32_t s = 0;
    for (int i = lo; i < hi; ++i) s += hist[i];
    const uint32_t v = wave_scan_incl(s, op_add{});  // inclusive scan over the threads
    if (lane == 63) wsum[wid] = v;
    __syncthreads();
    uint32_t pre = 0;
    for (int w = 0; w < wid; ++w) pre += wsum[w];
    uint32_t run = pre + v - s;
    for (int i = lo; i < hi; ++i) {
        const uint32_t c = hist[i];
        hist[i] = run;
        run += c;
    }
}

// Stable scatter of one tile: the tile is taken 256 keys at a time in order; a
// key's place is its digit's running offset + the keys of the same digit in
// lower waves + those in lower lanes of its wave.
__global__ __launch_bounds__(kEvThreads) void eval_sort_scatter_kernel(const uint64_t* __restrict__ in,
                                                                       uint64_t* __restrict__ out, int n, int shift,
                                                                       int nblk, const uint32_t* __restrict__ hist) {
    __shared__ uint32_t run[kSortBins];
    __shared__ uint32_t wcnt[kEvWaves][kSortBins];
    const int tid = threadIdx.x, wid = tid >> 6;
    run[tid] = hist[static_cast<size_t>(tid) * nblk + blockIdx.x];
    for (int w = 0; w < kEvWaves; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * kSortTile;
    const int end = min(n, base + kSortTile);
    for (int i0 = base; i0 < end; i0 += kEvThreads) {
        const int i = i0 + tid;
        const bool valid = i < end;
        const uint64_t key = valid ? in[i] : 0ull;
        const int d = static_cast<int>((key >> shift) & (kSortBins - 1));
        uint64_t peers = __ballot(valid);  // lanes of this wave with the same digit
        for (int b = 0; b < kSortBits; ++b) {
            const bool bit = (d >> b) & 1;
            const uint64_t bal = __ballot(valid && bit);
            peers &= bit ? bal : ~bal;
        }
        if (valid && (peers & lanemask_lt()) == 0) wcnt[wid][d] = __popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t o = run[d] + __popcll(peers & lanemask_lt());
            for (int w = 0; w < wid; ++w) o += wcnt[w][d];
            if (o < static_cast<uint32_t>(n)) out[o] = key;
        }
        __syncthreads();
        uint32_t add = 0;
        for (int w = 0; w < kEvWaves; ++w) {
            add += wcnt[w][tid];
            wcnt[w][tid] = 0;
        }
        run[tid] += add;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------- AP
// The flag of a sorted key's record.  A record index is below n by construction;
// a key that is not one (a caller's n over the records held) reads as ignored.
__device__ __forceinline__ int ev_flag(const int8_t* __restrict__ rec_flag, uint64_t key, int n) {
    const uint32_t r = static_cast<uint32_t>(key & 0xFFFFFFull);
    return r < static_cast<uint32_t>(n) ? rec_flag[r] : -1;
}

__device__ __forceinline__ double ev_dmax(double a, double b) { return a > b ? a : b; }

__global__ __launch_bounds__(kEvThreads) void eval_ap_kernel(int C, int n, const long long* __restrict__ hdr,
                                                             const uint64_t* __restrict__ sorted,
                                                             const int8_t* __restrict__ rec_flag, int use_07,
                                                             double* __restrict__ ap) {
    __shared__ unsigned long long wtot[kEvWaves];
    __shared__ double wmax[kEvWaves];
    __shared__ double wred[kEvWaves];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long npos_ll = hdr[4 + c];
    if (c == 0 || npos_ll <= 0) {
        if (tid == 0) ap[c] = NAN;
        return;
    }
    const double npos = static_cast<double>(npos_ll);
    const int lo = count_before(sorted, n, static_cast<uint64_t>(c) << 56);
    const int hi = count_before(sorted, n, static_cast<uint64_t>(c + 1) << 56);
    const int nc = hi - lo;

    // ---- the walk from the last record to the first (ev_pr_walk), then the integration
    const auto flag = [&](int p) { return ev_flag(rec_flag, sorted[lo + p], n); };
    const auto prec_of = [](int, double tp, double all) { return tp / (all < 1.0 ? 1.0 : all); };
    if (use_07) {  // the largest precision at a recall of at least i / 10
        double pm[11];
        for (int i = 0; i < 11; ++i) pm[i] = 0.0;
        ev_pr_walk(nc, wtot, wmax, flag, prec_of, [&](int, double tp, double prec, double) {
            const double rec = tp / npos;
            for (int i = 0; i < 11; ++i)
                if (rec >= static_cast<double>(i) * 0.1) pm[i] = ev_dmax(pm[i], prec);
        });
        double total = 0.0;
        for (int i = 0; i < 11; ++i) {
            double v = wave_reduce(pm[i], op_max{});
            if (lane == 0) wred[wid] = v;
            __syncthreads();
            v = wred[0];
            for (int w = 1; w < kEvWaves; ++w) v = ev_dmax(v, wred[w]);
            __syncthreads();
            total = total + v / 11.0;
        }
        if (tid == 0) ap[c] = total;
    } else {  // the area under the envelope: mrec changes exactly at a TP
        double sum = 0.0;
        ev_pr_walk(nc, wtot, wmax, flag, prec_of, [&](int f, double tp, double, double m) {
            if (f != 1) return;
            const double d = tp / npos - (tp - 1.0) / npos;
            sum = sum + d * m;
        });
        sum = wave_reduce(sum, op_add{});
        if (lane == 0) wred[wid] = sum;
        __syncthreads();
        if (tid == 0) {
            double total = wred[0];
            for (int w = 1; w < kEvWaves; ++w) total = total + wred[w];
            ap[c] = total;
        }
    }
}

__global__ void eval_map_kernel(int C, const double* __restrict__ ap, double* __restrict__ map) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    int k = 0;
    for (int c = 0; c < C; ++c) {
        const double v = ap[c];
        if (v == v) {
            s = s + v;
            ++k;
        }
    }
    map[0] = k ? s / static_cast<double>(k) : NAN;
}

struct EvalWs {
    uint64_t* a;     // [cap]
    uint64_t* b;     // [cap]
    uint32_t* hist;  // [kSortBins * ev_sort_blocks(cap)]
    size_t bytes;
};

static EvalWs carve_eval(void* ws, int64_t cap) {
    Carver c(ws);
    EvalWs w{};
    w.a = c.take<uint64_t>(static_cast<size_t>(cap));
    w.b = c.take<uint64_t>(static_cast<size_t>(cap));
    w.hist = c.take<uint32_t>(static_cast<size_t>(kSortBins) * ev_sort_blocks(cap));
    w.bytes = c.used();
    return w;
}

size_t eval_sort_workspace_size(int64_t cap) { return carve_eval(nullptr, cap).bytes; }

int eval_sort_keys(const uint64_t* rec_key, int64_t n_records, void* ws, size_t ws_bytes, const char* who,
                   hipStream_t st, const uint64_t** sorted) {
    const int n = static_cast<int>(n_records);
    const EvalWs w = carve_eval(ws, n_records);
    if (!ws || ws_bytes < w.bytes) {
        set_error("%s: workspace %zu < %zu", who, ws ? ws_bytes : size_t{0}, w.bytes);
        return FRCNN_EWORKSPACE;
    }
    const int nblk = ev_sort_blocks(n_records);
    const uint64_t* src = rec_key;
    uint64_t* dst = w.a;
    for (int pass = 0; pass < kSortPasses; ++pass) {
        const int shift = kSortFirstBit + pass * kSortBits;
        eval_sort_hist_kernel<<<nblk, kEvThreads, 0, st>>>(src, n, shift, nblk, w.hist);
        FRCNN_LAUNCH_CHECK("eval_sort_hist_kernel");
        eval_sort_scan_kernel<<<1, kScanThreads, 0, st>>>(w.hist, ev_scan_len(nblk));
        FRCNN_LAUNCH_CHECK("eval_sort_scan_kernel");
        eval_sort_scatter_kernel<<<nblk, kEvThreads, 0, st>>>(src, dst, n, shift, nblk, w.hist);
        FRCNN_LAUNCH_CHECK("eval_sort_scatter_kernel");
        src = dst;
        dst = dst == w.a ? w.b : w.a;
    }
    *sorted = src;  // an odd number of passes: w.a
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_eval_update(int N, int M, int G, int C, int64_t cap, const float* det_boxes,
                                 const int32_t* det_labels, const float* det_scores, const int32_t* det_count,
                                 const double* gt_boxes, const int32_t* gt_labels, const uint8_t* gt_difficult,
                                 double iou_thresh, int plus_one, int64_t* hdr, uint64_t* rec_key, int8_t* rec_flag,
                                 int32_t* rec_image, void* stream) {
    FRCNN_REQUIRE(N >= 1 && N <= kEvMaxN, "frcnn_eval_update: N=%d must be in [1, %d]", N, kEvMaxN);
    FRCNN_REQUIRE(M >= 1 && M <= kEvMaxM, "frcnn_eval_update: M=%d must be in [1, %d]", M, kEvMaxM);
    FRCNN_REQUIRE(G >= 0 && G <= kEvMaxG, "frcnn_eval_update: G=%d must be in [0, %d]", G, kEvMaxG);
    FRCNN_REQUIRE(C >= 2 && C <= kEvMaxC, "frcnn_eval_update: C=%d must be in [2, %d]", C, kEvMaxC);
    FRCNN_REQUIRE(cap >= 1 && cap <= kEvMaxCap, "frcnn_eval_update: cap=%lld must be in [1, %lld]",
                  static_cast<long long>(cap), static_cast<long long>(kEvMaxCap));
    FRCNN_REQUIRE(iou_thresh == iou_thresh, "frcnn_eval_update: iou_thresh is NaN");
    FRCNN_REQUIRE(det_boxes && det_labels && det_scores && det_count,
                  "frcnn_eval_update: null input (det_boxes / det_labels / det_scores / det_count)");
    FRCNN_REQUIRE(G == 0 || (gt_boxes && gt_labels), "frcnn_eval_update: null input (gt_boxes / gt_labels)");
    FRCNN_REQUIRE(hdr && rec_key && rec_flag && rec_image,
                  "frcnn_eval_update: null state (hdr / rec_key / rec_flag / rec_image)");
    hipStream_t st = as_stream(stream);
    long long* h = reinterpret_cast<long long*>(hdr);
    eval_match_kernel<<<N, kEvThreads, 0, st>>>(N, M, G, C, static_cast<long long>(cap), det_boxes, det_labels,
                                                det_scores, det_count, gt_boxes, gt_labels, gt_difficult, iou_thresh,
                                                plus_one ? 1 : 0, h, rec_key, rec_flag, rec_image);
    FRCNN_LAUNCH_CHECK("eval_match_kernel");
    eval_advance_kernel<<<1, kEvThreads, 0, st>>>(N, M, static_cast<long long>(cap), det_count, h);
    FRCNN_LAUNCH_CHECK("eval_advance_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_eval_plan(int N, int M, int64_t n_records, int64_t plan[10]) {
    FRCNN_REQUIRE(N >= 1 && N <= kEvMaxN, "frcnn_eval_plan: N=%d must be in [1, %d]", N, kEvMaxN);
    FRCNN_REQUIRE(M >= 1 && M <= kEvMaxM, "frcnn_eval_plan: M=%d must be in [1, %d]", M, kEvMaxM);
    FRCNN_REQUIRE(n_records >= 0 && n_records <= kEvMaxCap, "frcnn_eval_plan: n_records=%lld must be in [0, %lld]",
                  static_cast<long long>(n_records), static_cast<long long>(kEvMaxCap));
    FRCNN_REQUIRE(plan, "frcnn_eval_plan: null plan");
    const int nblk = ev_sort_blocks(n_records);
    const int len = ev_scan_len(nblk);
    plan[0] = kEvThreads;  // images per step of ev_count_sums
    plan[1] = ev_steps(N);
    plan[2] = kEvThreads;  // slots per chunk of eval_match_kernel
    plan[3] = ev_steps(M);
    plan[4] = kSortTile;
    plan[5] = nblk;
    plan[6] = kSortPasses;
    plan[7] = len;
    plan[8] = ev_scan_share(len);
    plan[9] = kEvThreads;  // records per chunk of ev_pr_walk
    return FRCNN_OK;
}

extern "C" size_t frcnn_eval_ap_workspace_size(int C, int64_t cap) {
    if (C < 2 || C > kEvMaxC || cap < 1 || cap > kEvMaxCap) return 0;
    return carve_eval(nullptr, cap).bytes;
}

extern "C" int frcnn_eval_ap(int C, int64_t n_records, const int64_t* hdr, const uint64_t* rec_key,
                             const int8_t* rec_flag, int use_07_metric, double* ap, double* map,
                             uint64_t* sorted_key, void* ws, size_t ws_bytes, void* stream) {
    FRCNN_REQUIRE(C >= 2 && C <= kEvMaxC, "frcnn_eval_ap: C=%d must be in [2, %d]", C, kEvMaxC);
    FRCNN_REQUIRE(n_records >= 0 && n_records <= kEvMaxCap, "frcnn_eval_ap: n_records=%lld must be in [0, %lld]",
                  static_cast<long long>(n_records), static_cast<long long>(kEvMaxCap));
    FRCNN_REQUIRE(hdr && ap && map, "frcnn_eval_ap: null pointer (hdr / ap / map)");
    FRCNN_REQUIRE(n_records == 0 || (rec_key && rec_flag), "frcnn_eval_ap: null state (rec_key / rec_flag)");
    hipStream_t st = as_stream(stream);
    const int n = static_cast<int>(n_records);
    const uint64_t* sorted = nullptr;
    if (n > 0) {
        const int rc = eval_sort_keys(rec_key, n_records, ws, ws_bytes, "frcnn_eval_ap", st, &sorted);
        if (rc) return rc;
        if (sorted_key && hipMemcpyAsync(sorted_key, sorted, sizeof(uint64_t) * static_cast<size_t>(n),
                                         hipMemcpyDeviceToDevice, st) != hipSuccess)
            return check_launch("frcnn_eval_ap: copy of the sorted keys");
    }
    eval_ap_kernel<<<C, kEvThreads, 0, st>>>(C, n, reinterpret_cast<const long long*>(hdr), sorted, rec_flag,
                                             use_07_metric ? 1 : 0, ap);
    FRCNN_LAUNCH_CHECK("eval_ap_kernel");
    eval_map_kernel<<<1, 64, 0, st>>>(C, ap, map);
    FRCNN_LAUNCH_CHECK("eval_map_kernel");
    return FRCNN_OK;
}
