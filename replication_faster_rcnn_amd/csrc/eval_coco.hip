// COCO-style detection evaluation: AP over IoU 0.50:0.05:0.95, AP by object
// size, AR at 1 / 10 / 100 detections per image.  The contract is
// pycocotools.cocoeval with iouType "bbox", restated in DESIGN.md "COCO-style
// evaluation"; the numpy restatement is tests/coco_eval_ref.py.  With iouType
// "segm" (DESIGN.md "COCO segm evaluation", tests/coco_segm_ref.py) only the
// source of a detection's IoU row and of the areas changes: CoBoxes forms them
// from boxes in fp64, CoCounts from the pixel counts of mask_overlap.hip.
//   coco_match_kernel<Src> : one workgroup per image, the gt staged in LDS.
//                            Step one, thread = slot: the slot's rank within
//                            its (image, class) in (descending score, ascending
//                            slot) order, counted against every slot of the
//                            image staged through LDS 256 at a time and given up
//                            at 100; the record's key, zero masks and the rank go
//                            out, and (class, rank) of the first 4,096 slots
//                            stay in LDS.  Step two, wave = class (claimed from an LDS
//                            counter): the class's gt and its first 100
//                            detections by rank (slot and box) are listed in
//                            LDS; per detection the wave forms the fp64 IoU row
//                            (lane = gt) once,
//                            then 40 lanes = (area range, threshold) walk the
//                            row, each with its own 256-bit set of taken gt, in
//                            the two-phase form of the contract; two ballots
//                            make the record's mask words.
//   coco_advance_kernel    : the header step in stream order (ev_advance).
//   eval_sort_*_kernel     : eval.hip's stable radix sort over the same key bits.
//   coco_gather_kernel     : the record words in sorted order.
//   coco_accumulate_kernel : one workgroup per (class, area range, maxDet,
//                            threshold): its class segment by binary search,
//                            then ev_pr_walk (eval_common.h, shared with
//                            eval.hip): the tp / fp totals and one pass from the
//                            last record to the first with running tp / fp and
//                            the suffix maximum of the precision.  The record at
//                            which tp reaches j serves the recall thresholds
//                            (j-1)/npig < R[r] <= j/npig.
//   coco_summary_kernel    : the twelve stats and ap_per_class, one workgroup
//                            each: a strided sum and a fixed tree.
// Integer atomics only (LDS counts, npig); no float atomics: every output is
// bit-identical from run to run.
#include <cstdio>

#include "eval_common.h"

namespace frcnn {

constexpr int kCoT = 10;    // IoU thresholds
constexpr int kCoR = 101;   // recall thresholds
constexpr int kCoA = 4;     // area ranges: all, small, medium, large
constexpr int kCoM = 3;     // maxDets 1, 10, 100
constexpr int kCoKeep = 100;
constexpr int kCoRankOut = 127;
constexpr int kCoSlotTable = 4096;  // slots whose (class, rank) step two finds in LDS; later ones are read back
constexpr int kCoTabT = 0, kCoTabR = kCoT, kCoTabA = kCoT + kCoR;  // tables: T[10], R[101], A[4][2]
constexpr double kCoEps = 0x1p-52;
constexpr double kCoBestCap = 1 - 1e-10;

// Record bits, two words per record:
//   word 0  bits 20a .. 20a+9   matched mask of area range a = 0, 1, 2 (bit = threshold)
//           bits 20a+10 .. 20a+19  ignored mask of area range a
//   word 1  bits 0..9 / 10..19  matched / ignored mask of area range 3
//           bits 32..38         rank within (image, class), 127 = out (>= 100, or class 0)
__device__ __forceinline__ void co_words(uint64_t bal_m, uint64_t bal_i, int rank, uint64_t* w0, uint64_t* w1) {
    uint64_t a = 0;
    for (int r = 0; r < 3; ++r) {
        a |= ((bal_m >> (10 * r)) & 0x3FFull) << (20 * r);
        a |= ((bal_i >> (10 * r)) & 0x3FFull) << (20 * r + 10);
    }
    *w0 = a;
    *w1 = ((bal_m >> 30) & 0x3FFull) | (((bal_i >> 30) & 0x3FFull) << 10) | (static_cast<uint64_t>(rank) << 32);
}

__device__ __forceinline__ void co_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct CoGt {
    double area[kEvMaxG];  // the area the size ranges and the ignore rule see
    int label[kEvMaxG];    // 0 for a row that is not a valid gt
    unsigned char crowd[kEvMaxG];
};

// The row source of the matching: what a gt and a detection are, and the IoU of a pair.
//   Shared               : the source's own LDS
//   load_gt(sh, t, g)    : stage gt row g (of the batch) as the image's gt t; returns its area for the ranges
//   stage(sh, wid, lane, nd, order, drow) : the wave's nd ranked detections, before its walk
//   det(sh, wid, r, row) : the detection of rank r (row of the batch); .area is its area for the ranges
//   iou(sh, d, t, crowd, garea) : fp64 IoU of that detection and the image's gt t
struct CoBoxes {  // iouType "bbox"
    struct Shared {
        double box[kEvMaxG][4];
        float dbox[kEvWaves][kCoKeep][4];  // the boxes of a wave's detections, by rank
    };
    struct Det {
        double d0, d1, d2, d3, area;
    };
    const float* __restrict__ det_boxes;
    const double* __restrict__ gt_boxes;

    __device__ __forceinline__ double load_gt(Shared& sh, int t, size_t g) const {
        const double* b = gt_boxes + g * 4;
        sh.box[t][0] = b[0];
        sh.box[t][1] = b[1];
        sh.box[t][2] = b[2];
        sh.box[t][3] = b[3];
        const double h = b[2] - b[0], w = b[3] - b[1];
        return h * w;
    }
    __device__ __forceinline__ void stage(Shared& sh, int wid, int lane, int nd, const int* order, size_t drow) const {
        for (int r = lane; r < nd; r += kWave) {
            const float4 b = *reinterpret_cast<const float4*>(det_boxes + (drow + order[r]) * 4);
            sh.dbox[wid][r][0] = b.x;
            sh.dbox[wid][r][1] = b.y;
            sh.dbox[wid][r][2] = b.z;
            sh.dbox[wid][r][3] = b.w;
        }
    }
    __device__ __forceinline__ Det det(const Shared& sh, int wid, int r, size_t) const {
        const float* db = sh.dbox[wid][r];
        Det d;
        d.d0 = static_cast<double>(db[0]);
        d.d1 = static_cast<double>(db[1]);
        d.d2 = static_cast<double>(db[2]);
        d.d3 = static_cast<double>(db[3]);
        const double dh = d.d2 - d.d0, dw = d.d3 - d.d1;
        d.area = dh * dw;
        return d;
    }
    __device__ __forceinline__ double iou(const Shared& sh, const Det& d, int g, bool crowd, double garea) const {
        const double ih = (d.d2 < sh.box[g][2] ? d.d2 : sh.box[g][2]) - (d.d0 > sh.box[g][0] ? d.d0 : sh.box[g][0]);
        const double iw = (d.d3 < sh.box[g][3] ? d.d3 : sh.box[g][3]) - (d.d1 > sh.box[g][1] ? d.d1 : sh.box[g][1]);
        double v = 0.0;
        if (!(ih <= 0.0) && !(iw <= 0.0)) {
            const double i = ih * iw;
            if (crowd) {
                v = i / d.area;
            } else {
                double u = d.area + garea;
                u = u - i;
                v = i / u;
            }
        }
        return v;
    }
};

struct CoCounts {  // iouType "segm": maskApi.c's rleIou on the counts of frcnn_mask_overlap
    struct Shared {
        int pix[kEvMaxG];  // the gt's pixel count: the union's term, whatever gt_area says
    };
    struct Det {
        const int32_t* irow;  // inter[n, slot, :]
        int pix;
        double area;
    };
    int G;
    const int32_t* __restrict__ inter;     // [N, M, G]
    const int32_t* __restrict__ det_pix;   // [N, M]
    const int32_t* __restrict__ gt_pix;    // [N, G]
    const double* __restrict__ gt_area;    // [N, G] or null: the annotation's area field

    __device__ __forceinline__ double load_gt(Shared& sh, int t, size_t g) const {
        const int p = gt_pix[g];
        sh.pix[t] = p;
        return gt_area ? gt_area[g] : static_cast<double>(p);
    }
    __device__ __forceinline__ void stage(Shared&, int, int, int, const int*, size_t) const {}
    __device__ __forceinline__ Det det(const Shared&, int, int, size_t row) const {
        Det d;
        d.irow = inter + row * G;
        d.pix = det_pix[row];
        d.area = static_cast<double>(d.pix);
        return d;
    }
    __device__ __forceinline__ double iou(const Shared& sh, const Det& d, int g, bool crowd, double) const {
        const int i = d.irow[g];
        if (i == 0) return 0.0;
        const int u = crowd ? d.pix : d.pix + sh.pix[g] - i;  // both counts <= 2^24
        return static_cast<double>(i) / static_cast<double>(u);
    }
};

template <class Src>
__global__ __launch_bounds__(kEvThreads) void coco_match_kernel(
    int N, int M, int G, int C, long long cap, const Src src, const int32_t* __restrict__ det_labels,
    const float* __restrict__ det_scores, const int32_t* __restrict__ det_count,
    const int32_t* __restrict__ gt_labels, const uint8_t* __restrict__ gt_crowd, const double* __restrict__ tables,
    long long* hdr, uint64_t* __restrict__ rec_key, uint64_t* rec_bits) {
    __shared__ CoGt gt;
    __shared__ typename Src::Shared sh;
    __shared__ unsigned int cpig[kEvMaxC * kCoA];
    __shared__ unsigned int dcnt[kEvMaxC];  // detections of the class with a rank below 100
    __shared__ long long red[2 * kEvWaves];
    __shared__ unsigned long long stage[kEvThreads];  // class << 32 | desc_score_key of a chunk of slots
    __shared__ double row[kEvWaves][kEvMaxG];
    __shared__ int members[kEvWaves][kEvMaxG];
    __shared__ int order[kEvWaves][kCoKeep];
    __shared__ unsigned short slot_info[kCoSlotTable];  // class << 8 | rank of the image's first 4,096 slots
    __shared__ int next_class;

    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long nrec = hdr[0];
    long long before, total;
    ev_count_sums(det_count, N, M, n, red, &before, &total);
    if (!ev_fits(nrec, total, cap)) return;

    for (int i = tid; i < kEvMaxC * kCoA; i += kEvThreads) cpig[i] = 0;
    if (tid < kEvMaxC) dcnt[tid] = 0;
    if (tid == 0) next_class = 1;
    if (tid < G) {  // G <= kEvMaxG == kEvThreads
        const size_t g = static_cast<size_t>(n) * G + tid;
        const int l = gt_labels[g];
        const bool valid = l >= 1 && l < C;
        gt.area[tid] = src.load_gt(sh, tid, g);
        gt.label[tid] = valid ? l : 0;
        gt.crowd[tid] = (gt_crowd && gt_crowd[g]) ? 1 : 0;
    }
    __syncthreads();
    if (tid < G && gt.label[tid] && !gt.crowd[tid]) {
        const double ar = gt.area[tid];
        for (int a = 0; a < kCoA; ++a)
            if (ar >= tables[kCoTabA + 2 * a] && ar <= tables[kCoTabA + 2 * a + 1])
                atomicAdd(&cpig[gt.label[tid] * kCoA + a], 1u);
    }
    __syncthreads();
    for (int i = tid; i < C * kCoA; i += kEvThreads)
        if (cpig[i])
            atomicAdd(reinterpret_cast<unsigned long long*>(hdr + 4 + i), static_cast<unsigned long long>(cpig[i]));

    const int k = ev_count(det_count, n, M);
    const size_t drow = static_cast<size_t>(n) * M;
    const long long rbase = nrec + before;  // rbase + k <= nrec + total <= cap

    // ---- step one: keys and ranks
    for (int s0 = 0; s0 < k; s0 += kEvThreads) {
        const int s = s0 + tid;
        const bool valid = s < k;
        int cls = 0;
        uint32_t skey = 0;
        if (valid) {
            const int label = det_labels[drow + s];
            cls = (label >= 1 && label < C) ? label : 0;
            skey = desc_score_key(det_scores[drow + s]);
        }
        int cnt = 0;
        bool done = !valid || cls == 0;
        for (int c0 = 0; c0 < k; c0 += kEvThreads) {
            const int o = c0 + tid;
            unsigned long long v = ~0ull;
            if (o < k) {
                const int label = det_labels[drow + o];
                const unsigned int oc = (label >= 1 && label < C) ? static_cast<unsigned int>(label) : 0u;
                v = (static_cast<unsigned long long>(oc) << 32) | desc_score_key(det_scores[drow + o]);
            }
            stage[tid] = v;
            __syncthreads();
            if (!done) {
                const int lim = min(kEvThreads, k - c0);
                const unsigned long long mine = (static_cast<unsigned long long>(cls) << 32) | skey;
                for (int j = 0; j < lim; ++j) {
                    const unsigned long long ov = stage[j];
                    // same class (equal high words) and before this slot in (key, slot) order
                    const bool pred = (ov >> 32) == (mine >> 32) && (ov < mine || (ov == mine && c0 + j < s));
                    cnt += pred ? 1 : 0;
                }
                done = cnt >= kCoKeep;
            }
            if (__syncthreads_and(done ? 1 : 0)) break;
        }
        if (valid) {
            const int rank = (cls == 0 || cnt >= kCoKeep) ? kCoRankOut : cnt;
            const long long r = rbase + s;
            rec_key[r] = (static_cast<uint64_t>(cls) << 56) | (static_cast<uint64_t>(skey) << 24) |
                         static_cast<uint64_t>(r);
            rec_bits[2 * r] = 0;
            rec_bits[2 * r + 1] = static_cast<uint64_t>(rank) << 32;
            if (s < kCoSlotTable) slot_info[s] = static_cast<unsigned short>((cls << 8) | rank);
            if (rank != kCoRankOut) atomicAdd(&dcnt[cls], 1u);
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---- step two: a wave per class with detections
    double thr = 0.0, alo = 0.0, ahi = 0.0;
    if (lane < kCoA * kCoT) {
        const double t = tables[kCoTabT + lane % kCoT];
        thr = t < kCoBestCap ? t : kCoBestCap;
        alo = tables[kCoTabA + 2 * (lane / kCoT)];
        ahi = tables[kCoTabA + 2 * (lane / kCoT) + 1];
    }
    for (;;) {
        int c = 0;
        if (lane == 0) c = atomicAdd(&next_class, 1);
        c = __shfl(c, 0, 64);
        if (c >= C) break;
        const int nd = static_cast<int>(dcnt[c]);  // <= 100
        if (nd == 0) continue;
        for (int s0 = 0; s0 < k; s0 += kWave) {
            const int s = s0 + lane;
            if (s >= k) continue;
            int rank = kCoRankOut;
            if (s < kCoSlotTable) {
                const int info = slot_info[s];
                if ((info >> 8) == c) rank = info & 0x7F;
            } else if (det_labels[drow + s] == c) {
                rank = static_cast<int>((rec_bits[2 * (rbase + s) + 1] >> 32) & 0x7F);
            }
            if (rank < kCoKeep) order[wid][rank] = s;
        }
        co_wave_sync();
        src.stage(sh, wid, lane, nd, order[wid], drow);
        int nc = 0;  // the class's gt in slot order
        for (int g0 = 0; g0 < G; g0 += kWave) {
            const int g = g0 + lane;
            const bool is = g < G && gt.label[g] == c;
            const uint64_t bal = __ballot(is);
            if (is) members[wid][nc + __popcll(bal & lanemask_lt())] = g;
            nc += __popcll(bal);
        }
        co_wave_sync();
        uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;  // gt taken at this lane's (range, threshold)
        for (int r = 0; r < nd; ++r) {
            const int s = order[wid][r];
            const typename Src::Det dv = src.det(sh, wid, r, drow + s);
            const double area_d = dv.area;
            for (int j = lane; j < nc; j += kWave) {
                const int g = members[wid][j];
                row[wid][j] = src.iou(sh, dv, g, gt.crowd[g] != 0, gt.area[g]);
            }
            co_wave_sync();
            bool matched = false, ign = false;
            if (lane < kCoA * kCoT) {
                double bn = thr, bi = thr;
                int mn = -1, mi = -1;
                for (int j = 0; j < nc; ++j) {
                    const int g = members[wid][j];
                    const bool crowd = gt.crowd[g] != 0;
                    const uint64_t word = j < 64 ? m0 : (j < 128 ? m1 : (j < 192 ? m2 : m3));
                    if (((word >> (j & 63)) & 1ull) && !crowd) continue;
                    const double ga = gt.area[g];
                    const bool gi = crowd || ga < alo || ga > ahi;
                    const double v = row[wid][j];
                    if (!gi) {
                        if (v >= bn) {
                            bn = v;
                            mn = j;
                        }
                    } else if (v >= bi) {
                        bi = v;
                        mi = j;
                    }
                }
                const int m = mn >= 0 ? mn : mi;
                if (m >= 0) {
                    matched = true;
                    ign = mn < 0;
                    const uint64_t bit = 1ull << (m & 63);
                    if (m < 64) m0 |= bit; else if (m < 128) m1 |= bit; else if (m < 192) m2 |= bit; else m3 |= bit;
                } else {
                    ign = area_d < alo || area_d > ahi;
                }
            }
            const uint64_t bal_m = __ballot(matched), bal_i = __ballot(ign);
            if (lane == 0) {
                uint64_t w0, w1;
                co_words(bal_m, bal_i, r, &w0, &w1);
                rec_bits[2 * (rbase + s)] = w0;
                rec_bits[2 * (rbase + s) + 1] = w1;
            }
            co_wave_sync();
        }
    }
}

__global__ __launch_bounds__(kEvThreads) void coco_advance_kernel(int N, int M, long long cap,
                                                                  const int32_t* __restrict__ det_count,
                                                                  long long* hdr) {
    __shared__ long long red[2 * kEvWaves];
    ev_advance(N, M, cap, det_count, hdr, red);
}

// ----------------------------------------------------------------- accumulate
// The record words in sorted order, so that the 120 passes over a class segment read them in sequence.  A
// record index is below n by construction; a key that is not one (a caller's n over the records held) reads as
// rank "out".
__global__ __launch_bounds__(kEvThreads) void coco_gather_kernel(int n, const uint64_t* __restrict__ sorted,
                                                                 const uint64_t* __restrict__ rec_bits,
                                                                 ulonglong2* __restrict__ sorted_bits) {
    const int p = blockIdx.x * kEvThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = static_cast<uint32_t>(sorted[p] & 0xFFFFFFull);
    ulonglong2 w = make_ulonglong2(0ull, static_cast<unsigned long long>(kCoRankOut) << 32);
    if (r < static_cast<uint32_t>(n)) w = reinterpret_cast<const ulonglong2*>(rec_bits)[r];
    sorted_bits[p] = w;
}

// 1 TP, 0 FP, -1 neither (ignored at this threshold or past maxDet) of the record at sorted position p.
__device__ __forceinline__ int co_flag(const ulonglong2* __restrict__ sorted_bits, int p, int a, int t, int max_det) {
    const ulonglong2 b = sorted_bits[p];
    const uint64_t w1 = b.y;
    if (static_cast<int>((w1 >> 32) & 0x7F) >= max_det) return -1;
    const uint64_t w = a < 3 ? b.x >> (20 * a) : w1;
    if ((w >> (10 + t)) & 1ull) return -1;
    return static_cast<int>((w >> t) & 1ull);
}

__global__ __launch_bounds__(kEvThreads) void coco_accumulate_kernel(int C, int n, const long long* __restrict__ hdr,
                                                                     const uint64_t* __restrict__ sorted,
                                                                     const ulonglong2* __restrict__ sorted_bits,
                                                                     const double* __restrict__ tables,
                                                                     double* __restrict__ precision,
                                                                     double* __restrict__ recall) {
    __shared__ unsigned long long wtot[kEvWaves];
    __shared__ double wmax[kEvWaves];
    __shared__ double pout[kCoR];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int t = b % kCoT;
    b /= kCoT;
    const int m = b % kCoM;
    b /= kCoM;
    const int a = b % kCoA;
    const int c = b / kCoA;
    const int max_det = m == 0 ? 1 : (m == 1 ? 10 : kCoKeep);
    const size_t pstride = static_cast<size_t>(C) * kCoA * kCoM;  // between recall thresholds
    const size_t cam = (static_cast<size_t>(c) * kCoA + a) * kCoM + m;
    double* pbase = precision + static_cast<size_t>(t) * kCoR * pstride + cam;
    double* rout = recall + static_cast<size_t>(t) * pstride + cam;
    const long long npig_ll = hdr[4 + c * kCoA + a];
    if (c == 0 || npig_ll <= 0) {
        if (tid < kCoR) pbase[tid * pstride] = -1.0;
        if (tid == 0) *rout = -1.0;
        return;
    }
    const double npig = static_cast<double>(npig_ll);
    const double* R = tables + kCoTabR;
    if (tid < kCoR) pout[tid] = 0.0;
    const int lo = n > 0 ? count_before(sorted, n, static_cast<uint64_t>(c) << 56) : 0;
    const int hi = n > 0 ? count_before(sorted, n, static_cast<uint64_t>(c + 1) << 56) : 0;
    const int nc = hi - lo;

    // ---- the walk from the last record to the first (ev_pr_walk).  The maximum is always at a TP;
    // the record at which tp reaches tpi serves the recall thresholds in ((tpi-1)/npig, tpi/npig].
    const unsigned long long total = ev_pr_walk(
        nc, wtot, wmax, [&](int p) { return co_flag(sorted_bits, lo + p, a, t, max_det); },
        [](int f, double tp, double all) { return f == 1 ? tp / (all + kCoEps) : 0.0; },
        [&](int f, double tp, double, double mx) {
            if (f != 1) return;
            const long long tpi = static_cast<long long>(tp);
            const double rc = tp / npig;
            const double rp = (tp - 1.0) / npig;
            int r = 0;
            if (tpi > 1) {
                r = static_cast<int>(rp * 100.0) - 1;
                r = r < 0 ? 0 : r;
            }
            for (; r < kCoR && R[r] <= rc; ++r)
                if (tpi == 1 || R[r] > rp) pout[r] = mx;
        });
    if (tid == 0) *rout = static_cast<double>(total >> 32) / npig;
    __syncthreads();
    if (tid < kCoR) pbase[tid * pstride] = pout[tid];
}

// Mean of the entries > -1 among count entries base[(i / inner) * outer_stride + (i % inner) * inner_stride],
// or -1 without any.  One workgroup: a strided sum per thread, then a fixed tree.
__device__ __forceinline__ double co_mean(const double* __restrict__ base, long long count, long long inner,
                                          size_t outer_stride, size_t inner_stride, double* red_s,
                                          unsigned long long* red_k) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double s = 0.0;
    unsigned long long k = 0;
    for (long long i = tid; i < count; i += kEvThreads) {
        const double v = base[static_cast<size_t>(i / inner) * outer_stride + static_cast<size_t>(i % inner) * inner_stride];
        if (v > -1.0) {
            s = s + v;
            ++k;
        }
    }
    s = wave_reduce(s, op_add{});
    k = wave_reduce(k, op_add{});
    if (lane == 0) {
        red_s[wid] = s;
        red_k[wid] = k;
    }
    __syncthreads();
    s = red_s[0];
    k = red_k[0];
    for (int w = 1; w < kEvWaves; ++w) {
        s = s + red_s[w];
        k += red_k[w];
    }
    return k ? s / static_cast<double>(k) : -1.0;
}

__global__ __launch_bounds__(kEvThreads) void coco_summary_kernel(int C, const double* __restrict__ precision,
                                                                  const double* __restrict__ recall,
                                                                  double* __restrict__ stats,
                                                                  double* __restrict__ ap_per_class) {
    __shared__ double red_s[kEvWaves];
    __shared__ unsigned long long red_k[kEvWaves];
    const int b = blockIdx.x;
    const size_t cam = static_cast<size_t>(kCoA) * kCoM;      // between classes
    const size_t pstride = static_cast<size_t>(C) * cam;      // between recall thresholds
    double v;
    if (b < 6) {  // AP, AP50, AP75, APs, APm, APl: precision[:, :, :, a, 100]
        const int a = b < 3 ? 0 : b - 2;
        const int t0 = b == 1 ? 0 : (b == 2 ? 5 : 0);
        const int nt = (b == 1 || b == 2) ? 1 : kCoT;
        // (t, r) rows of C entries; t-major, r, then class: rows are pstride apart
        v = co_mean(precision + static_cast<size_t>(t0) * kCoR * pstride + a * kCoM + 2,
                    static_cast<long long>(nt) * kCoR * C, C, pstride, cam, red_s, red_k);
    } else if (b < 12) {  // AR1, AR10, AR100, ARs, ARm, ARl: recall[:, :, a, m]
        const int a = b < 9 ? 0 : b - 8;
        const int m = b < 9 ? b - 6 : 2;
        v = co_mean(recall + a * kCoM + m, static_cast<long long>(kCoT) * C, C, pstride, cam, red_s, red_k);
    } else {  // ap_per_class: precision[:, :, c, all, 100]
        const int c = b - 12;
        v = co_mean(precision + static_cast<size_t>(c) * cam + 2, static_cast<long long>(kCoT) * kCoR, 1, pstride, 0,
                    red_s, red_k);
    }
    if (threadIdx.x == 0) {
        if (b < 12) stats[b] = v; else ap_per_class[b - 12] = v;
    }
}

struct CocoWs {
    void* sort;               // eval_sort_workspace_size(cap) bytes
    ulonglong2* sorted_bits;  // [cap]
    size_t sort_bytes, bytes;
};

static CocoWs carve_coco(void* ws, int64_t cap) {
    Carver c(ws);
    CocoWs w{};
    w.sort_bytes = eval_sort_workspace_size(cap);
    w.sort = c.take<char>(w.sort_bytes);
    w.sorted_bits = c.take<ulonglong2>(static_cast<size_t>(cap));
    w.bytes = c.used();
    return w;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_coco_eval_update(int N, int M, int G, int C, int64_t cap, const float* det_boxes,
                                      const int32_t* det_labels, const float* det_scores, const int32_t* det_count,
                                      const double* gt_boxes, const int32_t* gt_labels, const uint8_t* gt_crowd,
                                      const double* tables, int64_t* hdr, uint64_t* rec_key, uint64_t* rec_bits,
                                      void* stream) {
    FRCNN_REQUIRE(N >= 1 && N <= kEvMaxN, "frcnn_coco_eval_update: N=%d must be in [1, %d]", N, kEvMaxN);
    FRCNN_REQUIRE(M >= 1 && M <= kEvMaxM, "frcnn_coco_eval_update: M=%d must be in [1, %d]", M, kEvMaxM);
    FRCNN_REQUIRE(G >= 0 && G <= kEvMaxG, "frcnn_coco_eval_update: G=%d must be in [0, %d]", G, kEvMaxG);
    FRCNN_REQUIRE(C >= 2 && C <= kEvMaxC, "frcnn_coco_eval_update: C=%d must be in [2, %d]", C, kEvMaxC);
    FRCNN_REQUIRE(cap >= 1 && cap <= kEvMaxCap, "frcnn_coco_eval_update: cap=%lld must be in [1, %lld]",
                  static_cast<long long>(cap), static_cast<long long>(kEvMaxCap));
    FRCNN_REQUIRE(det_boxes && det_labels && det_scores && det_count,
                  "frcnn_coco_eval_update: null input (det_boxes / det_labels / det_scores / det_count)");
    FRCNN_REQUIRE(G == 0 || (gt_boxes && gt_labels), "frcnn_coco_eval_update: null input (gt_boxes / gt_labels)");
    FRCNN_REQUIRE(tables, "frcnn_coco_eval_update: null tables");
    FRCNN_REQUIRE(hdr && rec_key && rec_bits, "frcnn_coco_eval_update: null state (hdr / rec_key / rec_bits)");
    hipStream_t st = as_stream(stream);
    long long* h = reinterpret_cast<long long*>(hdr);
    coco_match_kernel<CoBoxes><<<N, kEvThreads, 0, st>>>(N, M, G, C, static_cast<long long>(cap),
                                                         CoBoxes{det_boxes, gt_boxes}, det_labels, det_scores,
                                                         det_count, gt_labels, gt_crowd, tables, h, rec_key, rec_bits);
    FRCNN_LAUNCH_CHECK("coco_match_kernel");
    coco_advance_kernel<<<1, kEvThreads, 0, st>>>(N, M, static_cast<long long>(cap), det_count, h);
    FRCNN_LAUNCH_CHECK("coco_advance_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_coco_segm_eval_update(int N, int M, int G, int C, int64_t cap, const int32_t* det_labels,
                                           const float* det_scores, const int32_t* det_count, const int32_t* inter,
                                           const int32_t* det_pixels, const int32_t* gt_pixels,
                                           const int32_t* gt_labels, const uint8_t* gt_crowd, const double* gt_area,
                                           const double* tables, int64_t* hdr, uint64_t* rec_key, uint64_t* rec_bits,
                                           void* stream) {
    const char* who = "frcnn_coco_segm_eval_update";
    FRCNN_REQUIRE(N >= 1 && N <= kEvMaxN, "%s: N=%d must be in [1, %d]", who, N, kEvMaxN);
    FRCNN_REQUIRE(M >= 1 && M <= kEvMaxM, "%s: M=%d must be in [1, %d]", who, M, kEvMaxM);
    FRCNN_REQUIRE(G >= 0 && G <= kEvMaxG, "%s: G=%d must be in [0, %d]", who, G, kEvMaxG);
    FRCNN_REQUIRE(C >= 2 && C <= kEvMaxC, "%s: C=%d must be in [2, %d]", who, C, kEvMaxC);
    FRCNN_REQUIRE(cap >= 1 && cap <= kEvMaxCap, "%s: cap=%lld must be in [1, %lld]", who, static_cast<long long>(cap),
                  static_cast<long long>(kEvMaxCap));
    FRCNN_REQUIRE(det_labels && det_scores && det_count && det_pixels,
                  "%s: null input (det_labels / det_scores / det_count / det_pixels)", who);
    FRCNN_REQUIRE(G == 0 || (inter && gt_pixels && gt_labels), "%s: null input (inter / gt_pixels / gt_labels)", who);
    FRCNN_REQUIRE(tables, "%s: null tables", who);
    FRCNN_REQUIRE(hdr && rec_key && rec_bits, "%s: null state (hdr / rec_key / rec_bits)", who);
    hipStream_t st = as_stream(stream);
    long long* h = reinterpret_cast<long long*>(hdr);
    coco_match_kernel<CoCounts><<<N, kEvThreads, 0, st>>>(N, M, G, C, static_cast<long long>(cap),
                                                          CoCounts{G, inter, det_pixels, gt_pixels, gt_area},
                                                          det_labels, det_scores, det_count, gt_labels, gt_crowd,
                                                          tables, h, rec_key, rec_bits);
    FRCNN_LAUNCH_CHECK("coco_match_kernel");
    coco_advance_kernel<<<1, kEvThreads, 0, st>>>(N, M, static_cast<long long>(cap), det_count, h);
    FRCNN_LAUNCH_CHECK("coco_advance_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_coco_eval_kernel(int segm, char* name, size_t len) {
    FRCNN_REQUIRE(name && len > 0, "frcnn_coco_eval_kernel: null name buffer");
    FRCNN_REQUIRE(segm == 0 || segm == 1, "frcnn_coco_eval_kernel: segm must be 0 (bbox) or 1, got %d", segm);
    std::snprintf(name, len, "coco_match_kernel<%s>+coco_advance_kernel", segm ? "counts" : "boxes");
    return FRCNN_OK;
}

extern "C" size_t frcnn_coco_eval_workspace_size(int C, int64_t cap) {
    if (C < 2 || C > kEvMaxC || cap < 1 || cap > kEvMaxCap) return 0;
    return carve_coco(nullptr, cap).bytes;
}

extern "C" int frcnn_coco_eval_accumulate(int C, int64_t n_records, const int64_t* hdr, const uint64_t* rec_key,
                                          const uint64_t* rec_bits, const double* tables, double* precision,
                                          double* recall, double* stats, double* ap_per_class, void* ws,
                                          size_t ws_bytes, void* stream) {
    FRCNN_REQUIRE(C >= 2 && C <= kEvMaxC, "frcnn_coco_eval_accumulate: C=%d must be in [2, %d]", C, kEvMaxC);
    FRCNN_REQUIRE(n_records >= 0 && n_records <= kEvMaxCap,
                  "frcnn_coco_eval_accumulate: n_records=%lld must be in [0, %lld]",
                  static_cast<long long>(n_records), static_cast<long long>(kEvMaxCap));
    FRCNN_REQUIRE(hdr && tables, "frcnn_coco_eval_accumulate: null pointer (hdr / tables)");
    FRCNN_REQUIRE(precision && recall && stats && ap_per_class,
                  "frcnn_coco_eval_accumulate: null output (precision / recall / stats / ap_per_class)");
    FRCNN_REQUIRE(n_records == 0 || (rec_key && rec_bits),
                  "frcnn_coco_eval_accumulate: null state (rec_key / rec_bits)");
    hipStream_t st = as_stream(stream);
    const int n = static_cast<int>(n_records);
    const uint64_t* sorted = nullptr;
    const ulonglong2* sorted_bits = nullptr;
    if (n > 0) {
        const CocoWs w = carve_coco(ws, n_records);
        if (!ws || ws_bytes < w.bytes) {
            set_error("frcnn_coco_eval_accumulate: workspace %zu < %zu", ws ? ws_bytes : size_t{0}, w.bytes);
            return FRCNN_EWORKSPACE;
        }
        const int rc = eval_sort_keys(rec_key, n_records, w.sort, w.sort_bytes, "frcnn_coco_eval_accumulate", st,
                                      &sorted);
        if (rc) return rc;
        coco_gather_kernel<<<(n + kEvThreads - 1) / kEvThreads, kEvThreads, 0, st>>>(n, sorted, rec_bits,
                                                                                     w.sorted_bits);
        FRCNN_LAUNCH_CHECK("coco_gather_kernel");
        sorted_bits = w.sorted_bits;
    }
    coco_accumulate_kernel<<<C * kCoA * kCoM * kCoT, kEvThreads, 0, st>>>(
        C, n, reinterpret_cast<const long long*>(hdr), sorted, sorted_bits, tables, precision, recall);
    FRCNN_LAUNCH_CHECK("coco_accumulate_kernel");
    coco_summary_kernel<<<12 + C, kEvThreads, 0, st>>>(C, precision, recall, stats, ap_per_class);
    FRCNN_LAUNCH_CHECK("coco_summary_kernel");
    return FRCNN_OK;
}
