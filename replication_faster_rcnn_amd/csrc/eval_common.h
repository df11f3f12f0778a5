// What the two evaluation units share (eval.hip: PASCAL VOC, eval_coco.hip:
// COCO-style): the limits, the accumulator's header step, the precision /
// recall walk over a class segment (ev_pr_walk) and the stable radix sort of
// the record keys, which lives in eval.hip and is reached from eval_coco.hip
// through the host entry below.
#pragma once

#include "common.h"

namespace frcnn {

constexpr int kEvMaxN = 1024;
constexpr int kEvMaxM = 1 << 20;
constexpr int kEvMaxG = 256;
constexpr int kEvMaxC = 128;
constexpr int64_t kEvMaxCap = int64_t{1} << 24;  // the record index is a 24-bit key field
constexpr int kEvThreads = 256;
constexpr int kEvWaves = kEvThreads / kWave;

// The sort's shape (eval.hip): the launches, the scan kernel and frcnn_eval_plan read it from here.
constexpr int kSortTile = 4096;  // keys per workgroup and pass
constexpr int kSortBits = 8;
constexpr int kSortBins = 1 << kSortBits;
constexpr int kSortFirstBit = 24;  // below it: the insertion order, already ascending in the input
constexpr int kSortPasses = 5;     // bits 24..63
constexpr int kScanThreads = 1024;

// Sort tiles (workgroups per histogram / scatter launch) of n keys.
__host__ __device__ inline int ev_sort_blocks(int64_t n) { return static_cast<int>((n + kSortTile - 1) / kSortTile); }
// Histogram words of one pass, and the contiguous share of them each scan thread takes.
__host__ __device__ inline int ev_scan_len(int nblk) { return kSortBins * nblk; }
__host__ __device__ inline int ev_scan_share(int len) { return (len + kScanThreads - 1) / kScanThreads; }
// Steps of a workgroup's stride loop over n items, kEvThreads at a time (ev_count_sums over the
// images, eval_match_kernel over an image's slots, ev_pr_walk over a segment's records).
__host__ __device__ inline int ev_steps(int64_t n) { return static_cast<int>((n + kEvThreads - 1) / kEvThreads); }

__device__ __forceinline__ int ev_count(const int32_t* det_count, int n, int M) {
    const int k = det_count[n];
    return k < 0 ? 0 : (k > M ? M : k);
}

// Sum of the clamped counts of all images (total) and of the images before n.
__device__ __forceinline__ void ev_count_sums(const int32_t* det_count, int N, int M, int n, long long* red,
                                              long long* before, long long* total) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    long long b = 0, t = 0;
    for (int i = tid; i < N; i += kEvThreads) {
        const int k = ev_count(det_count, i, M);
        t += k;
        b += i < n ? k : 0;
    }
    b = wave_reduce(b, op_add{});
    t = wave_reduce(t, op_add{});
    if (lane == 0) {
        red[wid] = b;
        red[kEvWaves + wid] = t;
    }
    __syncthreads();
    b = t = 0;
    for (int w = 0; w < kEvWaves; ++w) {
        b += red[w];
        t += red[kEvWaves + w];
    }
    __syncthreads();
    *before = b;
    *total = t;
}

// A batch that does not fit (or a header that is not a state of this capacity)
// writes nothing.
__device__ __forceinline__ bool ev_fits(long long nrec, long long total, long long cap) {
    return nrec >= 0 && nrec <= cap && total <= cap - nrec;
}

// The header step of one update, by one workgroup of kEvThreads in stream order
// behind the match kernel: records / images advance, or the dropped-batch count grows.
__device__ __forceinline__ void ev_advance(int N, int M, long long cap, const int32_t* det_count, long long* hdr,
                                           long long* red) {
    long long before, total;
    ev_count_sums(det_count, N, M, 0, red, &before, &total);
    if (threadIdx.x == 0) {
        if (ev_fits(hdr[0], total, cap)) {
            hdr[0] += total;
            hdr[1] += N;
        } else {
            hdr[2] += 1;
        }
    }
}

// The precision / recall walk over one class segment of nc records in descending
// score order, by one workgroup of kEvThreads (eval.hip's AP, eval_coco.hip's
// accumulate).  flag(p) is the flag of the segment's record p: 1 TP, 0 FP, -1
// neither.  First the totals, tp in the high word and fp in the low word; then
// from the last record to the first, kEvThreads at a time, thread order =
// descending record order: a reversed inclusive scan gives the running tp and
// tp + fp at each record (integers, exact in a double), prec_of(f, tp, all) its
// precision, and an inclusive maximum carried from chunk to chunk the largest
// precision of the record and every later one.  visit(f, tp, prec, suffix_max)
// is called once per record.  Returns the totals.  wtot, wmax: kEvWaves words of
// LDS each; every thread of the workgroup calls it.
template <class Flag, class Prec, class Visit>
__device__ __forceinline__ unsigned long long ev_pr_walk(int nc, unsigned long long* wtot, double* wmax, Flag flag,
                                                         Prec prec_of, Visit visit) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const auto count_of = [](int f) { return f == 1 ? (1ull << 32) : (f == 0 ? 1ull : 0ull); };
    unsigned long long acc = 0;
    for (int p = tid; p < nc; p += kEvThreads) acc += count_of(flag(p));
    acc = wave_reduce(acc, op_add{});
    if (lane == 0) wtot[wid] = acc;
    __syncthreads();
    unsigned long long total = 0;
    for (int w = 0; w < kEvWaves; ++w) total += wtot[w];
    __syncthreads();

    unsigned long long carry = total;  // tp / fp up to and including the last record not yet walked
    double cmax = 0.0;                 // mpre's closing 0, then the suffix maximum of the records walked
    for (int p0 = 0; p0 < nc; p0 += kEvThreads) {
        const int p = p0 + tid;
        const bool valid = p < nc;
        int f = -1;
        if (valid) f = flag(nc - 1 - p);
        const unsigned long long mine = count_of(f);
        // inclusive scan: this record and the later ones of the chunk
        const unsigned long long v = wave_scan_incl(mine, op_add{});
        if (lane == 63) wtot[wid] = v;
        __syncthreads();
        unsigned long long pre = 0, chunk = 0;
        for (int w = 0; w < kEvWaves; ++w) {
            pre += w < wid ? wtot[w] : 0ull;
            chunk += wtot[w];
        }
        const unsigned long long at = carry - (pre + v - mine);  // running sums at this record
        const double tp = static_cast<double>(at >> 32);
        const double all = static_cast<double>((at >> 32) + (at & 0xFFFFFFFFull));
        const double prec = valid ? prec_of(f, tp, all) : 0.0;
        // inclusive maximum in thread order = suffix maximum in record order
        double m = wave_scan_incl(prec, op_max{});
        if (lane == 63) wmax[wid] = m;
        __syncthreads();
        double pmx = cmax, cm = cmax;
        for (int w = 0; w < kEvWaves; ++w) {
            pmx = w < wid ? op_max{}(pmx, wmax[w]) : pmx;
            cm = op_max{}(cm, wmax[w]);
        }
        m = op_max{}(m, pmx);
        if (valid) visit(f, tp, prec, m);
        carry -= chunk;
        cmax = cm;
        __syncthreads();
    }
    return total;
}

// eval.hip: the stable LSD radix sort of n record keys over bits 24..63 (the low
// 24 bits are the insertion order the input already has).  *sorted points into
// the workspace.  FRCNN_EWORKSPACE (message prefixed with `who`) when ws is null
// or smaller than eval_sort_workspace_size(n).
size_t eval_sort_workspace_size(int64_t cap);
int eval_sort_keys(const uint64_t* rec_key, int64_t n, void* ws, size_t ws_bytes, const char* who, hipStream_t st,
                   const uint64_t** sorted);

}  // namespace frcnn
