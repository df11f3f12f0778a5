// What the two evaluation units share (eval.hip: PASCAL VOC, eval_coco.hip:
// COCO-style): the limits, the accumulator's header step and the stable radix
// sort of the record keys, which lives in eval.hip and is reached from
// eval_coco.hip through the host entry below.
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

__device__ __forceinline__ int ev_count(const int32_t* det_count, int n, int M) {
    const int k = det_count[n];
    return k < 0 ? 0 : (k > M ? M : k);
}

__device__ __forceinline__ long long ev_wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
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
    b = ev_wave_sum(b);
    t = ev_wave_sum(t);
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

__device__ __forceinline__ int ev_lower_bound(const uint64_t* __restrict__ keys, int n, uint64_t v) {
    int lo = 0, hi = n;  // first index with keys[i] >= v
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// eval.hip: the stable LSD radix sort of n record keys over bits 24..63 (the low
// 24 bits are the insertion order the input already has).  *sorted points into
// the workspace.  FRCNN_EWORKSPACE (message prefixed with `who`) when ws is null
// or smaller than eval_sort_workspace_size(n).
size_t eval_sort_workspace_size(int64_t cap);
int eval_sort_keys(const uint64_t* rec_key, int64_t n, void* ws, size_t ws_bytes, const char* who, hipStream_t st,
                   const uint64_t** sorted);

}  // namespace frcnn
